"""Every graph of the lowering corpus (tests/lowering_corpus.py) lowered in every arithmetic mode on the policy device
(host only: the capability answers of libghm.so, no arithmetic): the forward, deterministic forward and backward programs
(with the image-input gradients) are emitted and executed.

  * A graph that lowers in f32 lowers in all five modes: a rewrite is an optimisation and never shrinks what is served.
  * A refusal is a NotImplementedError from a short allow-list, the same in every mode; anything else fails.
  * Across the corpus every targeted program label and rewrite appears in every mode where it applies, so a change to
    the corpus or the generator cannot quietly stop exercising a rule.
"""
import numpy as np
import pytest

from gan_heightmaps_amd import layers as L
from tests import lowering_corpus as LC
from tests.fake_device import PolicyDevice, PolicyOps

LP_MODES = ('bf16x3', 'bf16x2', 'bf16', 'f16')

# refusals a graph of the corpus may meet (message prefixes); none does today
ALLOWED_REFUSALS = (
    "no lowering for",
    "max pooling other than 2x2",
)


class CorpusOps(PolicyOps):
    """PolicyOps that also answers the fused conv + BatchNorm query like the library: bf16 / fp16 products the
    low-precision kernels serve (never the split modes)"""

    def conv_bn_fused_supported(self, d, dtype):
        return dtype in ('bf16', 'f16') and self.lp_supported(d, 0, dtype)


class CorpusDevice(PolicyDevice):
    ops_class = CorpusOps


def _lower(name, dtype):
    """-> (labels of the three programs, rewrites seen) or the refusal's message"""
    g = LC.graph(name)
    dev = CorpusDevice()
    ops = CorpusOps(dev)
    try:
        plan, store, fwd, bwd, gin, seed = LC.plan_graph(dev, ops, g, dtype)
        det = []
        plan.emit_forward(det, deterministic=True)
    except NotImplementedError as e:
        return str(e)
    for e in fwd + bwd + det:
        e[1]()
    assert set(gin) == set(LC.image_inputs(g))
    for l in LC.image_inputs(g):
        assert gin[l].shape == plan.input_tensor(l).shape
    assert plan.out.shape[0] == g.batch
    labels = {e[0] for e in fwd + bwd + det}
    labels |= {c[0] for c in ops.calls}
    return labels, _rewrites(g, plan)


def _rewrites(g, plan):
    """which of R1 (act over a concat split, with an existing act shared) and R2 (act folded into its producer) fired"""
    live = {id(n) for n in plan.order}
    seen = set()
    for l in L.get_all_layers(g.out):
        if not isinstance(l, L.NonlinearityLayer) or l.nonlinearity.kind == 'linear':
            continue
        if id(plan.node_of_layer[id(l)]) in live:
            continue
        if isinstance(l.input_layer, L.ConcatLayer):
            seen.add('R1')
            cat = [n for n in plan.order if n.op == 'concat' and n.layer is l.input_layer]
            if cat and any(len(i.consumers) > 1 for i in cat[0].inputs):
                seen.add('R1_shared')
        else:
            seen.add('R2')
    return seen


_results = {}


def _result(name, dtype):
    if (name, dtype) not in _results:
        _results[(name, dtype)] = _lower(name, dtype)
    return _results[(name, dtype)]


@pytest.mark.parametrize("name", LC.NAMES)
def test_graph_lowers_in_every_mode(name):
    res = {m: _result(name, m) for m in LC.MODES}
    refused = {m: r for m, r in res.items() if isinstance(r, str)}
    if refused:
        msgs = set(refused.values())
        assert len(refused) == len(LC.MODES) and len(msgs) == 1, (name, refused)
        assert msgs.pop().startswith(ALLOWED_REFUSALS), (name, refused)


def test_corpus_is_deterministic():
    for name in ("unet_skip", "gen00", "gen17"):
        a, b = LC.graph(name), LC.graph(name)
        assert [type(l).__name__ for l in L.get_all_layers(a.out)] == [type(l).__name__ for l in L.get_all_layers(b.out)]
        for pa, pb in zip(L.get_all_params(a.out), L.get_all_params(b.out)):
            assert np.array_equal(pa.get_value(), pb.get_value())
        assert all(np.array_equal(x, y) for x, y in zip(a.feeds, b.feeds))
    assert len(LC.GENERATED) == LC.N_GENERATED >= 30
    # the generated graphs are small and differ from one another
    shapes = set()
    for name in LC.GENERATED:
        g = LC.graph(name)
        assert 1 <= g.batch <= 4
        for l in L.get_all_layers(g.out):
            s = l.output_shape
            assert len(s) != 4 or (s[2] <= 64 and s[3] <= 64), (name, l, s)
        shapes.add(tuple(type(l).__name__ for l in L.get_all_layers(g.out)))
    assert len(shapes) >= 25


def test_repro_graphs_lower_in_the_reduced_modes():
    """the two defects the corpus found: bilinear up-sample -> 3x3 conv with a nonlinearity of its own (on the layer, or
    folded from a NonlinearityLayer) in the split modes, and a concat of 12 + 20 channels read by a low-precision conv"""
    for name in ("blconv_act_lrelu", "blconv_act_tanh", "blconv_act_layer"):
        for m in ('bf16x3', 'bf16x2'):
            labels, _ = _result(name, m)
            assert 'upconv_fwd' not in labels and 'blconv_fwd' not in labels, (name, m)   # the literal form
    labels, _ = _result("blconv_bn", 'bf16x3')
    assert 'blconv_fwd' in labels and 'blconv_frame_fwd' in labels
    for m in ('bf16', 'f16', 'bf16x3'):
        labels, _ = _result("concat_unaligned", m)
        assert 'conv2d_fwd_lp' in labels and 'conv2d_fwd_lp_q' not in labels, m            # reads the fp32 concat
        labels, _ = _result("concat_aligned", m)
        assert 'conv2d_fwd_lp_q' in labels, m


@pytest.mark.parametrize("dtype", LP_MODES)
def test_net_input_inside_a_q_concat_packs_its_slice(dtype):
    """a net input that lives in a channel slice of a concat whose q copy a low-precision conv reads: no kernel produces
    the input, so the forward program must pack its q slice (else the conv reads whatever the buffer held)"""
    g = LC.graph("concat_input_slice")
    dev = CorpusDevice()
    ops = CorpusOps(dev)
    plan, store, fwd, bwd, gin, seed = LC.plan_graph(dev, ops, g, dtype)
    inp = plan.node_of_layer[id(g.inputs[0])]
    cat = [n for n in plan.order if n.op == 'concat'][0]
    assert cat.outq is not None and inp.outq is not None and inp.alias[0] is cat
    for e in fwd:
        e[1]()
    packs = [c for c in ops.calls if c[0] == 'q_pack']
    assert any(c[1][1].ptr == inp.outq.ptr and c[1][1].shape == inp.outq.shape for c in packs)


# what the corpus must exercise, per mode: program labels (and the rewrites) -> the modes where they apply
REQUIRED = {
    'upconv_fwd': LC.MODES,
    'blconv_fwd': ('bf16x3', 'bf16x2'),
    'blconv_frame_fwd': ('bf16x3', 'bf16x2'),
    'convpool_fwd': LC.MODES,
    'conv_bn_fwd': ('bf16', 'f16'),
    'maxpool_mask_bwd': LC.MODES,
    'maxpool_fwd': LC.MODES,                  # (tanh: not fusable)
    'in_fwd': LC.MODES,
    'dropout_fwd': LC.MODES,
    'avgpool_fwd': LC.MODES,
    'deconv_fwd': LC.MODES,
    'q_pack': LP_MODES,
    'bn_apply_det': LC.MODES,
    'conv2d_fwd_lp_q': LP_MODES,              # q operands
    'conv2d_fwd_lp': LP_MODES,                # fp32 operands on the low-precision kernels
    'R1': LC.MODES,
    'R1_shared': LC.MODES,
    'R2': LC.MODES,
}


def test_corpus_covers_every_rule_in_every_mode():
    seen = {m: set() for m in LC.MODES}
    for name in LC.NAMES:
        for m in LC.MODES:
            r = _result(name, m)
            if not isinstance(r, str):
                seen[m] |= r[0] | r[1]
    missing = [(k, m) for k, modes in REQUIRED.items() for m in modes if k not in seen[m]]
    assert not missing, missing
    # and the low-precision labels stay out of f32
    assert not {'q_pack', 'conv2d_fwd_lp_q', 'conv2d_fwd_lp', 'conv_bn_fwd', 'blconv_fwd'} & seen['f32']
