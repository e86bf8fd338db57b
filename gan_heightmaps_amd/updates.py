"""lasagne.updates / theano.shared subset used by experiments.py:116-117 and pix2pix.py:30.
The nine update rules of lasagne.updates (``sgd``, ``momentum``, ``nesterov_momentum``, ``adagrad``, ``rmsprop``,
``adadelta``, ``adam``, ``adamax``, ``amsgrad``) are passed to Pix2Pix as ``opt``; calling one with hyper-parameters
returns the specification the engine turns into one flat multi-tensor optimiser kernel per net (ghm_rmsprop /
ghm_adam / ghm_opt_update).  Only ``learning_rate`` may be a shared scalar."""
import numpy as np


class SharedScalar:
    """theano.shared(floatX(v)) for the learning rate: get_value()/set_value() (pix2pix.py:259).
    The engine mirrors the value into a device scalar read by the optimiser kernels, so a captured
    HIP graph sees set_value() on the next step."""

    def __init__(self, value):
        self._v = np.float32(value)
        self._listeners = []

    def get_value(self):
        return self._v

    def set_value(self, v):
        self._v = np.float32(v)
        for fn in self._listeners:
            fn(self._v)

    def __float__(self):
        return float(self._v)


def shared(value, name=None):
    return SharedScalar(value)


class OptimizerSpec:
    def __init__(self, kind, learning_rate, **hp):
        for k, v in hp.items():
            if hasattr(v, 'get_value'):
                raise NotImplementedError("%s: only learning_rate may be a shared variable (%s is baked into the kernel "
                                          "launch); pass a number" % (kind, k))
        self.kind = kind
        self.learning_rate = learning_rate
        self.hp = hp


def rmsprop(learning_rate=1.0, rho=0.9, epsilon=1e-6):
    """lasagne.updates.rmsprop defaults."""
    return OptimizerSpec('rmsprop', learning_rate, rho=rho, epsilon=epsilon)


def adam(learning_rate=0.001, beta1=0.9, beta2=0.999, epsilon=1e-8):
    """lasagne.updates.adam defaults."""
    return OptimizerSpec('adam', learning_rate, beta1=beta1, beta2=beta2, epsilon=epsilon)


def sgd(learning_rate):
    """lasagne.updates.sgd: p -= lr * g."""
    return OptimizerSpec('sgd', learning_rate)


def momentum(learning_rate, momentum=0.9):
    """lasagne.updates.momentum: v = momentum * v - lr * g; p += v."""
    return OptimizerSpec('momentum', learning_rate, momentum=momentum)


def nesterov_momentum(learning_rate, momentum=0.9):
    """lasagne.updates.nesterov_momentum: v = momentum * v - lr * g; p += momentum * v - lr * g."""
    return OptimizerSpec('nesterov_momentum', learning_rate, momentum=momentum)


def adagrad(learning_rate=1.0, epsilon=1e-6):
    """lasagne.updates.adagrad: a += g^2; p -= lr * g / sqrt(a + epsilon)."""
    return OptimizerSpec('adagrad', learning_rate, epsilon=epsilon)


def adadelta(learning_rate=1.0, rho=0.95, epsilon=1e-6):
    """lasagne.updates.adadelta: a = rho a + (1 - rho) g^2; u = g sqrt(d + epsilon) / sqrt(a + epsilon); p -= lr * u;
    d = rho d + (1 - rho) u^2."""
    return OptimizerSpec('adadelta', learning_rate, rho=rho, epsilon=epsilon)


def adamax(learning_rate=0.002, beta1=0.9, beta2=0.999, epsilon=1e-8):
    """lasagne.updates.adamax: m = beta1 m + (1 - beta1) g; u = max(beta2 u, |g|);
    p -= lr / (1 - beta1^t) * m / (u + epsilon)."""
    return OptimizerSpec('adamax', learning_rate, beta1=beta1, beta2=beta2, epsilon=epsilon)


def amsgrad(learning_rate=0.001, beta1=0.9, beta2=0.999, epsilon=1e-8):
    """lasagne.updates.amsgrad: Adam's m and v, vhat = max(vhat, v);
    p -= lr sqrt(1 - beta2^t) / (1 - beta1^t) * m / (sqrt(vhat) + epsilon)."""
    return OptimizerSpec('amsgrad', learning_rate, beta1=beta1, beta2=beta2, epsilon=epsilon)
