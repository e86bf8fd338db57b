"""step_build.cut_buckets: the sub-buckets of a net's flat gradient range, on plain integers, and against the collectives
of built data-parallel plans (all-reduce and sharded form, worlds 2 and 8)."""
import numpy as np
import pytest

from gan_heightmaps_amd import updates
from gan_heightmaps_amd.architectures import dcgan, p2p
from gan_heightmaps_amd.nonlinearities import linear, tanh
from gan_heightmaps_amd.step import GanStep
from gan_heightmaps_amd.step_build import cut_buckets
from tests.fake_device import FakeDevice


def test_cuts_on_integers():
    offsets, sizes = [0, 10, 30], [10, 20, 70]
    # last layers first; a bucket closes once it holds 50 elements, the first parameter closes the last one
    assert cut_buckets(offsets, sizes, 100, 128, 4 * 50, 1, False) == [(30, 100, {2}), (0, 30, {0, 1})]
    assert cut_buckets(offsets, sizes, 100, 128, 4 * 10, 1, False) == [(30, 100, {2}), (10, 30, {1}), (0, 10, {0})]
    assert cut_buckets(offsets, sizes, 100, 128, 1 << 30, 1, False) == [(0, 100, {0, 1, 2})]
    # sharded: cuts fall on multiples of the unit and cover the padding; a straddling parameter is pending in both neighbours
    assert cut_buckets(offsets, sizes, 100, 128, 4 * 50, 64, True) == [(0, 128, {0, 1, 2})]
    assert cut_buckets([0, 10, 100], [10, 90, 100], 200, 256, 4 * 50, 64, True) == [(64, 256, {1, 2}), (0, 64, {0, 1})]
    assert cut_buckets([], [], 0, 0, 4 * 50, 1, False) == []


class _Comm:
    def __init__(self, world):
        self.dev, self.world, self.rank = FakeDevice(), world, 0


@pytest.mark.parametrize("world", [2, 8])
@pytest.mark.parametrize("mode", ["allreduce", "rs_ag"])
def test_cuts_are_the_collectives_of_a_built_plan(world, mode):
    G = dcgan.default_generator(24, True, nch=16, div=[2, 2, 4])
    Dn = dcgan.default_discriminator(32, True, nch=16, div=[4, 2, 2], nonlinearity=linear)
    U = p2p.g_unet(32, True, False, nf=4, act=tanh, bilinear_upsample=True)
    P = p2p.discriminator(32, True, False, nf=4, act=linear, mul_factor=[1, 2])
    spec = updates.rmsprop(learning_rate=updates.shared(1e-4))
    eng = GanStep(FakeDevice(), G, Dn, U, P, 100, True, 'l1', spec, 'both', comm=_Comm(world), use_graph=False,
                  two_streams=False, bucket_mb=4096 / 2 ** 20, exchange_mode=mode)
    b = eng.built(4)
    sharded, unit = mode == "rs_ag", 64 * world if mode == "rs_ag" else 1
    assert eng.sharded == sharded and eng.shard_unit == unit
    several = 0
    for k, st in eng.stores.items():
        tr = sorted((p for p in st.params if p.index[0] == 'w'), key=lambda p: p.index[1])
        cuts = cut_buckets([p.index[1] for p in tr], [int(np.prod(p.shape)) for p in tr], st.n_train, st.n_pad,
                           eng.bucket_bytes, unit, sharded)
        # one collective per cut (sent when its last gradient is reported, which need not be the order they were cut in)
        assert sorted((lo, hi - lo) for lo, hi, _ in cuts) == sorted((lo, n) for _, kk, lo, n in b.xchg_order if kk == k)
        assert b.net_buckets[k] == [(lo, hi) for lo, hi, _ in cuts]
        assert all(lo % unit == 0 for lo, _, _ in cuts)
        # the cuts tile [0, n_train) (sharded: [0, n_pad)), highest range first, without gap or overlap
        end = st.n_pad if sharded else st.n_train
        assert cuts[0][1] == end and cuts[-1][0] == 0
        assert all(a[0] == c[1] and c[0] < c[1] for a, c in zip(cuts, cuts[1:])) and cuts[0][0] < cuts[0][1]
        # a bucket waits for every parameter whose gradients its range holds
        for i, p in enumerate(tr):
            plo, phi = p.index[1], p.index[1] + int(np.prod(p.shape))
            assert all(i in pend for lo, hi, pend in cuts if plo < hi and phi > lo)
        several += len(cuts) > 1
    assert several >= 2         # (4 KB sub-buckets: the nets do cut into several)
