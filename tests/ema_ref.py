"""The exponential moving average of csrc/ema.hip restated in numpy float32:

    ema[i] = fl(fl(decay * ema[i]) + fl(c * w[i])),    c = (float)(1.0 - (double)decay)

with ``decay`` the fp32 value the kernel receives.  Two products and one sum, each rounded to float32 on its own -- numpy's
float32 arithmetic does exactly that, so the device result is compared bit for bit (any NaN matching any NaN: which payload
an invalid operation produces is the hardware's choice).  ``skip``: the step's update was skipped (fp16 overflow flag set),
the average is left alone."""
import numpy as np


def coefficients(decay):
    """-> (decay, c) as the float32 values the kernel multiplies by"""
    d = np.float32(decay)
    return d, np.float32(1.0 - float(d))


def ema_update(ema, w, decay, skip=False):
    ema = np.asarray(ema, np.float32)
    if skip:
        return ema.copy()
    d, c = coefficients(decay)
    with np.errstate(all='ignore'):
        a = (d * ema).astype(np.float32)
        b = (c * np.asarray(w, np.float32)).astype(np.float32)
        return (a + b).astype(np.float32)


def ema_run(w0, snapshots, decay, skipped=()):
    """the average after every step of a run: it starts at ``w0`` and follows ``snapshots`` (the parameters read after each
    step); ``skipped``: indices of steps whose update was skipped"""
    out, e = [], np.asarray(w0, np.float32).copy()
    for i, w in enumerate(snapshots):
        e = ema_update(e, w, decay, skip=i in skipped)
        out.append(e)
    return out


def same_bits(a, b, nan_any=False):
    """uint32 equality of two float32 arrays; ``nan_any``: a NaN matches any NaN"""
    a, b = np.ascontiguousarray(a, np.float32).ravel(), np.ascontiguousarray(b, np.float32).ravel()
    eq = a.view(np.uint32) == b.view(np.uint32)
    if nan_any:
        eq |= np.isnan(a) & np.isnan(b)
    return bool(eq.all())
