"""The lowering corpus (tests/lowering_corpus.py) on the device, every graph in every arithmetic mode, against the float64
layer-graph interpreter (tests/golden/symtheano.py) on the same fp32 inputs, parameters and output seed: the output, every
trainable parameter's gradient, the image-input gradients, the BatchNorm running-statistics update and the deterministic
forward.

Bounds (rel-L2), per mode: output (also the deterministic forward and the running statistics) / gradients.  f32 and bf16x3
keep the fp32 bounds of tests/test_gpu_f4.py (worst seen over the corpus on the MI355X: 1.1e-6 / 5.8e-5).  The other three
were measured once over this corpus on the MI355X and set at no more than 4x the worst value seen:

    mode     worst output   worst gradient   bounds
    bf16x2   1.4e-5         1.3e-3           5e-5 / 2e-3
    f16      8.2e-4         4.4e-2           3e-3 / 1e-1
    bf16     7.3e-3         2.2e-1           2.5e-2 / 4e-1

The f16 and bf16 gradient bounds are above the 1e-2 / 6e-2 that compounding the per-product precision of
tests/test_gpu_lp.py predicts.  The excess comes from the non-smooth layers: where a relu / leaky relu pre-activation or
the two largest values of a max-pool window lie within the forward's rounding error of each other, the device and the
float64 reference take different branches, and the gradient there moves by its full size.  That error grows like the
square root of the forward error, not linearly: the graphs with the largest gradient errors are the ones with relu /
lrelu / max-pool layers (small_maps, convpool_lp_lrelu, unet_skip, gen19), and the modes whose forward is exact to
~1e-6 (f32, bf16x3) show no such excess.
"""
import json
import os

import numpy as np
import pytest

from gan_heightmaps_amd import layers as L
from gan_heightmaps_amd.nonlinearities import LeakyRectify
from tests import lowering_corpus as LC
from tests import canary

pytestmark = pytest.mark.gpu

TOL = {          # mode: (output, gradients)
    'f32': (1e-5, 5e-4),
    'bf16x3': (1e-5, 5e-4),
    'bf16x2': (5e-5, 2e-3),
    'f16': (3e-3, 1e-1),
    'bf16': (2.5e-2, 4e-1),
}


gpu = canary.fixtures()[0]


_graphs, _refs = {}, {}


def _graph_and_reference(name, res):
    """the graph is built once per module (the same parameter objects in every mode); its float64 reference once"""
    if name not in _refs:
        _refs[name] = LC.reference(_graphs[name], res["seed"], res["keys"])
    return _refs[name]


def _run(gpu, name, dtype):
    dev, ops, _ = gpu
    if name not in _graphs:
        _graphs[name] = LC.graph(name)
    g = _graphs[name]
    res = LC.run_on_device(dev, ops, g, dtype)
    ref = _graph_and_reference(name, res)
    det_ref = LC.reference_det(g)            # with the running statistics the device left in the store
    return g, res, ref, det_ref


def _report(name, dtype, e):
    path = os.environ.get("GHM_CORPUS_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"graph": name, "dtype": dtype, **{k: (float(v) if isinstance(v, (float, np.floating)) else v)
                                                                  for k, v in e.items() if k != 'worst'}}) + "\n")


@pytest.mark.parametrize("dtype", LC.MODES)
@pytest.mark.parametrize("name", LC.NAMES)
def test_graph_matches_the_float64_interpreter(gpu, name, dtype):
    g, res, ref, det_ref = _run(gpu, name, dtype)
    e = LC.errors(g, res, ref, det_ref)
    _report(name, dtype, e)
    t_out, t_grad = TOL[dtype]
    assert e["out"] < t_out, (name, dtype, "output", e)
    assert e["checked"] >= 1, (name, dtype)
    assert e["grad"] < t_grad, (name, dtype, "parameter gradient", e["worst"], e)
    assert e["gin"] < t_grad, (name, dtype, "input gradient", e)
    assert e["stats"] < max(t_out, 1e-4), (name, dtype, "running statistics", e)
    assert e["det"] < t_out, (name, dtype, "deterministic forward", e)


@pytest.mark.parametrize("dtype", LC.MODES)
def test_bounds_tell_a_slightly_wrong_graph(gpu, dtype):
    """non-vacuity: the device output of lrelu_probe meets its bound against the true reference and fails it against the
    reference with the first layer's leaky-relu slope 0.19 instead of 0.2"""
    g, res, ref, det_ref = _run(gpu, "lrelu_probe", dtype)
    t_out = TOL[dtype][0]
    assert LC.rel(res["out"].reshape(ref["out"].shape), ref["out"]) < t_out
    conv = [l for l in L.get_all_layers(g.out) if isinstance(l, L.Conv2DLayer) and l.nonlinearity.kind == 'lrelu'][0]
    right = conv.nonlinearity
    conv.nonlinearity = LeakyRectify(0.19)
    try:
        wrong = LC.reference(g, res["seed"], res["keys"])
    finally:
        conv.nonlinearity = right
    assert LC.rel(res["out"].reshape(wrong["out"].shape), wrong["out"]) > t_out
