"""The exponential moving average of the generator weights on the MI355X: ghm_ema_update and ghm_swap_f32 bit
for bit against tests/ema_ref.py inside poisoned buffers, the average a training run keeps against the restatement applied
to the parameters read after every step (eager, recorded, captured graphs; with the default path bit-identical to a run
without the average), the skipped fp16 step, the one-rank RCCL form, inference through ema_weights(), and the files.
Nets: the 32^2 SMALL configuration of tests/test_gpu_resume.py, batch 4."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import ema_ref
from tests.gpu_common import NET_PAIRS as NETS, _iterators, assert_same, batches, build, dev, ops, split_run      # noqa: F401  (dev, ops: the module-scoped fixtures)

pytestmark = pytest.mark.gpu

GENS = ('dcgan_gen', 'p2p_gen')
POISON = 0xDEADBEEF
SIZES = [0, 1, 3, 4, 5, 255, 1024, 1027]
OFFSETS = [4, 64]
DECAYS = [0.0, 0.5, 0.999]


# ---- kernels ----------------------------------------------------------------------------------------------------------
SPECIALS = np.array([0x00000001, 0x80000400, 0x007fffff, 0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc12345,
                     0x7f7fffff, 0xff7fffff, 0x00800000, 0x3f800000], np.uint32)     # denormals, +-0, +-inf, a NaN, extremes


def _values(n, seed, shift):
    """n float32 values as uint32 words: normal draws with the specials at the front, rotated by ``shift`` so that the two
    operands meet in different pairs"""
    v = np.random.RandomState(seed).randn(n).astype(np.float32).view(np.uint32).copy()
    k = min(n, len(SPECIALS))
    v[:k] = np.roll(SPECIALS, shift)[:k]
    return v


class _Buf:
    """a poisoned device buffer with the range under test at element ``off``"""

    def __init__(self, dev, words, off):
        from gan_heightmaps_amd.device import DevTensor
        self.n, self.off = len(words), off
        self.host = np.full(off + len(words) + 64 + 5, POISON, np.uint32)
        self.host[off:off + self.n] = words
        self.dev = dev
        self.t = dev.tensor(self.host.view(np.float32))
        self.view = DevTensor(dev, self.t.ptr + 4 * off, (1, max(self.n, 1), 1, 1))

    def words(self):
        return self.t.numpy().ravel().view(np.uint32)

    def inner(self):
        return self.words()[self.off:self.off + self.n]

    def poison_intact(self):
        w = self.words()
        return bool((w[:self.off] == POISON).all() and (w[self.off + self.n:] == POISON).all())

    def unchanged(self):
        return np.array_equal(self.words(), self.host)

    def free(self):
        self.dev.free(self.t.ptr)


@pytest.mark.parametrize("n", SIZES)
def test_ema_update_kernel_bit_for_bit(dev, ops, n):
    for off in OFFSETS:
        for decay in DECAYS:
            e0, w0 = _values(n, 10 + n, 0), _values(n, 20 + n, 5)
            e, w = _Buf(dev, e0, off), _Buf(dev, w0, off)
            ops.ema_update(e.view, w.view, n, decay)
            dev.sync()
            want = ema_ref.ema_update(e0.view(np.float32), w0.view(np.float32), decay)
            assert ema_ref.same_bits(e.inner().view(np.float32), want, nan_any=True), (n, off, decay)
            assert e.poison_intact() and w.unchanged(), (n, off, decay)
            e.free(), w.free()


@pytest.mark.parametrize("n", SIZES)
def test_swap_kernel_bit_for_bit(dev, ops, n):
    for off in OFFSETS:
        a0, b0 = _values(n, 30 + n, 0), _values(n, 40 + n, 3)
        a, b = _Buf(dev, a0, off), _Buf(dev, b0, off)
        ops.swap_f32(a.view, b.view, n)
        dev.sync()
        assert np.array_equal(a.inner(), b0) and np.array_equal(b.inner(), a0), (n, off)         # NaN payloads, -0 included
        assert a.poison_intact() and b.poison_intact()
        ops.swap_f32(a.view, b.view, n)
        dev.sync()
        assert a.unchanged() and b.unchanged(), (n, off)
        a.free(), b.free()


def test_ema_update_follows_the_loss_scale_flag_and_swap_does_not(dev, ops):
    n = 1027
    e0, w0 = _values(n, 1, 0), _values(n, 2, 5)
    e, w = _Buf(dev, e0, 64), _Buf(dev, w0, 4)
    ls = dev.tensor(np.array([4.0, 0.25, 0, 0, 0, 0, 0, 0], np.float32))
    dev.set_loss_scale_state(ls)
    try:
        ls.set(np.array([4.0, 0.25, 0, 1, 0, 0, 0, 0], np.float32))          # the overflow flag, by a host write
        ops.ema_update(e.view, w.view, n, 0.5)
        dev.sync()
        assert e.unchanged() and w.unchanged()
        ops.swap_f32(e.view, w.view, n)                                     # the exchange does not read the state
        dev.sync()
        assert np.array_equal(e.inner(), w0) and np.array_equal(w.inner(), e0)
        ops.swap_f32(e.view, w.view, n)
        ls.set(np.array([4.0, 0.25, 0, 0, 0, 0, 0, 0], np.float32))
        ops.ema_update(e.view, w.view, n, 0.5)
        dev.sync()
        want = ema_ref.ema_update(e0.view(np.float32), w0.view(np.float32), 0.5)        # (the scale itself plays no part)
        assert ema_ref.same_bits(e.inner().view(np.float32), want, nan_any=True) and not e.unchanged()
        assert e.poison_intact() and w.unchanged()
        assert ls.numpy().ravel().tolist() == [4.0, 0.25, 0, 0, 0, 0, 0, 0]
    finally:
        dev.set_loss_scale_state(None)
    e.free(), w.free(), dev.free(ls.ptr)


def test_refusals_write_nothing(dev, ops):
    from gan_heightmaps_amd._lib import GhmError, call
    from gan_heightmaps_amd.device import DevTensor
    n = 64
    a, b = _Buf(dev, _values(n, 3, 0), 4), _Buf(dev, _values(n, 4, 1), 64)
    vp = lambda t: C.c_void_p(t.ptr if t is not None else 0)
    shifted = lambda v, k: DevTensor(dev, v.ptr + 4 * k, (1, n, 1, 1))
    upd = lambda x, y, m=n, d=0.5: call("ghm_ema_update", dev.h, vp(x), vp(y), m, d)
    swp = lambda x, y, m=n: call("ghm_swap_f32", dev.h, vp(x), vp(y), m)
    bad = [(None, b.view), (a.view, None),                                          # null pointers
           (shifted(a.view, 1), b.view), (a.view, shifted(b.view, 3)),              # not 16-byte aligned
           (a.view, a.view), (a.view, shifted(a.view, 4)), (shifted(a.view, 8), a.view)]       # overlapping ranges
    for fn in (upd, swp):
        for x, y in bad:
            with pytest.raises(GhmError):
                fn(x, y)
        with pytest.raises(GhmError):
            fn(a.view, b.view, -1)
    for d in (1.0, 1.5, -0.25, float('nan'), float('inf'), -float('inf')):
        with pytest.raises(GhmError, match="decay"):
            upd(a.view, b.view, n, d)
    dev.sync()
    assert a.unchanged() and b.unchanged()
    upd(a.view, b.view, 0), swp(a.view, b.view, 0)                                  # n == 0: accepted, nothing done
    dev.sync()
    assert a.unchanged() and b.unchanged()
    # ranges that touch do not overlap: the first and the second half of a's range change places, and back
    half = DevTensor(dev, a.view.ptr + 4 * (n // 2), (1, n // 2, 1, 1))
    swp(a.view, half, n // 2)
    dev.sync()
    assert np.array_equal(a.inner(), np.roll(a.host[a.off:a.off + n], n // 2)) and a.poison_intact()
    swp(a.view, half, n // 2)
    dev.sync()
    assert a.unchanged()
    a.free(), b.free()


# ---- the average of a training run ----------------------------------------------------------------------------------------
def _flat(m, what):
    m.engine.sync()
    return {k: getattr(m.engine.stores[k], what).numpy().ravel()[:m.engine.stores[k].n_train].copy() for k in GENS}


def _everything(m):
    from gan_heightmaps_amd import layers as L
    st = m.engine.training_state()
    return ({n: L.get_all_param_values(getattr(m, n[0])[n[1]]) for n in NETS},
            {k: (v['hyper'], v['slots']) for k, v in st['nets'].items()})


def _run(dev, kind, ema, nsteps=4, **kw):
    """-> (model, losses per step, the generators' parameters before the run and after every step, their averages)"""
    m = build(kind, 7, dev, ema=ema, **kw)
    w0 = _flat(m, 'w')
    losses, snaps, avgs = [], [], []
    for b in batches(nsteps):
        losses.append(list(m.train_fn(*b)))
        snaps.append(_flat(m, 'w'))
        if ema is not None:
            avgs.append(_flat(m, 'ema'))
    return m, losses, w0, snaps, avgs


def _assert_average_is_the_restatement(w0, snaps, avgs, decay, keys=GENS, skipped=()):
    for k in keys:
        want = ema_ref.ema_run(w0[k], [s[k] for s in snaps], decay, skipped)
        for i, (got, ref) in enumerate(zip(avgs, want)):
            assert ema_ref.same_bits(got[k], ref), (k, i)


def _assert_same_run(a, b):
    (ma, la, _, sa, _), (mb, lb, _, sb, _) = a, b
    assert np.array_equal(np.asarray(la), np.asarray(lb))
    assert all(np.array_equal(x[k], y[k]) for x, y in zip(sa, sb) for k in GENS)
    (pa, oa), (pb, ob) = _everything(ma), _everything(mb)
    for n in NETS:
        assert all(np.array_equal(x, y) for x, y in zip(pa[n], pb[n])), n
    for k in oa:
        assert np.array_equal(oa[k][0], ob[k][0]), k
        assert sorted(oa[k][1]) == sorted(ob[k][1])
        assert all(np.array_equal(v, ob[k][1][s]) for s, v in oa[k][1].items()), k


@pytest.mark.parametrize("use_graph", [False, 'recorded', True], ids=["eager", "recorded", "graph"])
def test_average_of_a_run_is_the_restatement_and_the_run_is_untouched(dev, use_graph):
    with_ema = _run(dev, 'adam', 0.9, use_graph=use_graph)
    m, losses, w0, snaps, avgs = with_ema
    labels = [e[0] for lane in m.engine.built(4).update for e in lane]
    assert labels.count('ema_dcgan_gen') == 1 and labels.count('ema_p2p_gen') == 1
    assert all(not np.array_equal(snaps[i][k], snaps[i + 1][k]) for i in range(3) for k in GENS)      # the weights do move
    _assert_average_is_the_restatement(w0, snaps, avgs, 0.9)
    assert all(not np.array_equal(avgs[-1][k], snaps[-1][k]) for k in GENS)
    _assert_same_run(with_ema, _run(dev, 'adam', None, use_graph=use_graph))


@pytest.mark.parametrize("kind", ['rmsprop', 'adamax'])
def test_average_behind_a_rule_without_a_tick_and_one_of_opt_update(dev, kind):
    with_ema = _run(dev, kind, 0.9, use_graph=False)
    _assert_average_is_the_restatement(with_ema[2], with_ema[3], with_ema[4], 0.9)
    _assert_same_run(with_ema, _run(dev, kind, None, use_graph=False))


def test_a_generator_that_is_not_trained_keeps_its_initial_average(dev):
    m, losses, w0, snaps, avgs = _run(dev, 'adam', 0.9, use_graph=False, train_mode='dcgan')
    labels = [e[0] for lane in m.engine.built(4).update for e in lane]
    assert 'ema_dcgan_gen' in labels and 'ema_p2p_gen' not in labels
    _assert_average_is_the_restatement(w0, snaps, avgs, 0.9, keys=('dcgan_gen',))
    assert all(ema_ref.same_bits(a['p2p_gen'], w0['p2p_gen']) and ema_ref.same_bits(s['p2p_gen'], w0['p2p_gen'])
               for a, s in zip(avgs, snaps))


def test_skipped_fp16_step_leaves_parameters_and_averages_alone(dev):
    m = build('adam', 7, dev, dtype='f16', ema=0.9, use_graph='recorded')
    eng = m.engine
    bs = batches(5)
    w0 = _flat(m, 'w')
    snaps, avgs = [], []
    for b in bs[:3]:                                     # eager, record, replay: a healthy scale
        assert np.isfinite(m.train_fn(*b)).all()
        snaps.append(_flat(m, 'w')), avgs.append(_flat(m, 'ema'))
    st = eng.loss_scale_state()
    print("fp16 loss-scale state after 3 steps:", st)
    assert all(s['skipped_steps'] == 0 for s in st), st
    _assert_average_is_the_restatement(w0, snaps, avgs, 0.9)
    all_w = lambda: {k: s.w.numpy().copy() for k, s in eng.stores.items()}
    before = all_w()
    eng.set_loss_scale(2.0 ** 40)                        # the way tests/test_gpu_lp.py pushes a step to overflow
    assert np.isfinite(m.train_fn(*bs[3])).all()
    st = eng.loss_scale_state()
    print("fp16 loss-scale state after the overflowed step:", st)
    assert all(s['skipped_steps'] == 1 for s in st), st
    after = all_w()
    assert all(np.array_equal(before[k], after[k]) for k in before)
    skipped_avg = _flat(m, 'ema')
    assert all(ema_ref.same_bits(skipped_avg[k], avgs[-1][k]) for k in GENS)
    # and the average moves again with the next applied step
    eng.set_loss_scale(32768.0)
    m.train_fn(*bs[4])
    assert all(s['skipped_steps'] == 1 for s in eng.loss_scale_state())
    snaps += [{k: before[k].ravel()[:v.size] for k, v in w0.items()}, _flat(m, 'w')]
    avgs += [skipped_avg, _flat(m, 'ema')]
    _assert_average_is_the_restatement(w0, snaps, avgs, 0.9, skipped={3})
    assert all(not ema_ref.same_bits(avgs[-1][k], skipped_avg[k]) for k in GENS)


def test_one_rank_rccl_allreduce_keeps_the_same_average(dev):
    from gan_heightmaps_amd import device, dist
    from gan_heightmaps_amd._lib import GhmError
    alone = _run(dev, 'adam', 0.9, use_graph='recorded')
    cdev = device.Device(dev.index)
    try:
        try:
            comm = dist.Comm(cdev, 0, 1, channels=(2, 4))
        except GhmError as e:
            if "librccl" in str(e):
                pytest.skip("RCCL cannot be loaded: %s" % e)
            raise
        try:
            ranked = _run(dev, 'adam', 0.9, use_graph='recorded', comm=comm, force_exchange=True, exchange_mode='allreduce',
                          bucket_mb=2048.0 / 2 ** 20)
            assert ranked[0].engine.exchange and not ranked[0].engine.sharded
            _assert_same_run(alone, ranked)
            assert all(ema_ref.same_bits(x[k], y[k]) for x, y in zip(alone[4], ranked[4]) for k in GENS)
            lo, hi = ranked[0].engine.replica_checksums()
            assert lo == hi
        finally:
            comm.close()
    finally:
        cdev.close()


# ---- inference ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trained(dev):
    m = build('adam', 7, dev, ema=0.9, use_graph=False)
    for b in batches(3):
        m.train_fn(*b)
    return m


def _inputs():
    rng = np.random.RandomState(11)
    return rng.rand(4, 24).astype(np.float32), rng.uniform(-1, 1, (4, 1, 32, 32)).astype(np.float32)


def test_forwards_inside_ema_weights_are_those_of_a_model_holding_the_averages(dev, trained):
    from gan_heightmaps_amd import layers as L
    m = trained
    Z, X = _inputs()
    params = lambda: {n: L.get_all_param_values(getattr(m, n[0])[n[1]]) for n in NETS}
    before = (m.z_fn_det(Z), m.gen_fn_det(X), params())
    # a second model whose generators are set from the averages (BatchNorm statistics: the live ones)
    other = build('adam', 99, dev, use_graph=False)
    avg = {'dcgan': m.engine.ema_values('dcgan_gen'), 'p2p': m.engine.ema_values('p2p_gen')}
    for stage in ('dcgan', 'p2p'):
        gen = L.get_all_params(getattr(m, stage)['gen'])
        st = m.engine.stores[stage + '_gen']
        differ = 0
        for p, a, live in zip(gen, avg[stage], before[2][(stage, 'gen')]):       # ema_values is the raw buffer, in lasagne layout
            if p.index[0] == 'w':
                assert np.array_equal(a, st._from_device_layout(p, st._view(st.ema, p).numpy().ravel()))
                differ += not np.array_equal(a, live)       # (a bias in front of a BatchNorm has no gradient: it stays 0)
            else:
                assert np.array_equal(a, live)
        assert differ >= 4
        L.set_all_param_values(getattr(other, stage)['gen'], avg[stage])
    want = (other.z_fn_det(Z), other.gen_fn_det(X))
    v0 = m.engine.param_version
    with m.ema_weights():
        assert m.engine.param_version != v0
        inside = (m.z_fn_det(Z), m.gen_fn_det(X))
        chain = m.engine.generate_chain(Z, True)
        for stage in ('dcgan', 'p2p'):
            for a, got in zip(avg[stage], L.get_all_param_values(getattr(m, stage)['gen'])):
                assert np.array_equal(a, got)
        with pytest.raises(RuntimeError, match="ema_weights"):
            m.train_fn(*batches(1)[0])
        with pytest.raises(RuntimeError, match="ema_weights"):
            m.z_fn(Z)
    assert ema_ref.same_bits(inside[0], want[0]) and ema_ref.same_bits(inside[1], want[1])
    assert ema_ref.same_bits(chain[0], want[0]) and ema_ref.same_bits(chain[1], other.gen_fn_det(want[0]))
    assert not np.array_equal(inside[0], before[0]) and not np.array_equal(inside[1], before[1])
    after = (m.z_fn_det(Z), m.gen_fn_det(X), params())
    assert ema_ref.same_bits(after[0], before[0]) and ema_ref.same_bits(after[1], before[1])
    for n in NETS:
        assert all(ema_ref.same_bits(x, y) for x, y in zip(before[2][n], after[2][n])), n
    # the body raising changes nothing of that
    with pytest.raises(ZeroDivisionError):
        with m.ema_weights():
            1 / 0
    assert ema_ref.same_bits(m.z_fn_det(Z), before[0])
    assert all(ema_ref.same_bits(x, y) for n in NETS for x, y in zip(before[2][n], params()[n]))


def test_texture_and_world_follow_the_swap(dev, trained):
    m = trained
    hm = np.random.RandomState(12).uniform(-1, 1, (1, 50, 70)).astype(np.float32)
    rect = (-20, 7, 70, 45)
    with m.terrain_world(42, chunk_cells=2) as world:
        before = (m.texture_heightmap(hm), world.heightmap(*rect), world.texture(*rect))
        n0 = world.computed
        assert np.array_equal(world.heightmap(*rect), before[1]) and world.computed == n0       # served from the cache
        with m.ema_weights():
            inside = (m.texture_heightmap(hm), world.heightmap(*rect), world.texture(*rect))
            n1 = world.computed
            assert n1 > n0                                                                   # ... which the swap emptied
            terrain = m.generate_terrain(z=np.random.RandomState(13).rand(1, 2, 24).astype(np.float32))
        after = (m.texture_heightmap(hm), world.heightmap(*rect), world.texture(*rect))
        assert world.computed > n1
    for b, i, a in zip(before, inside, after):
        assert np.isfinite(i).all() and not np.array_equal(i, b)
        assert ema_ref.same_bits(a, b)
    assert not np.array_equal(terrain, m.generate_terrain(z=np.random.RandomState(13).rand(1, 2, 24).astype(np.float32)))


# ---- files ------------------------------------------------------------------------------------------------------------
def test_resume_with_an_average_is_bit_identical(dev, tmp_path):
    (la, sa), (lc, sc), b = split_run('adam', dev, tmp_path, dtype='f32', ema=0.9)
    assert np.array_equal(np.asarray(la), np.asarray(lc))
    assert_same(sa, sc)
    assert sa['state']['ema'] == sc['state']['ema'] == 0.9
    for k in GENS:
        x, y = sa['state']['nets'][k]['ema'], sc['state']['nets'][k]['ema']
        assert ema_ref.same_bits(x, y) and x.size == b.engine.stores[k].n_train
        assert not np.array_equal(x, b.engine.stores[k].w.numpy().ravel()[:x.size])
    assert all('ema' not in sa['state']['nets'][k] for k in ('dcgan_disc', 'p2p_disc'))


def test_save_model_ema_is_a_plain_model_file_of_the_averages(dev, trained, tmp_path):
    m = trained
    Z, X = _inputs()
    path = str(tmp_path / "avg.model")
    v = m.engine.param_version
    m.save_model(path, ema=True)
    assert m.engine.param_version == v
    with m.ema_weights():
        want = (m.z_fn_det(Z), m.gen_fn_det(X))
        m.save_model(str(tmp_path / "inside.model"))                 # inside the block a plain save writes the same values
    plain = build('adam', 5, dev, use_graph=False)
    for p in (path, str(tmp_path / "inside.model")):
        plain.load_model(p)
        assert ema_ref.same_bits(plain.z_fn_det(Z), want[0]) and ema_ref.same_bits(plain.gen_fn_det(X), want[1])
    with pytest.raises(ValueError, match="average"):
        plain.save_model(str(tmp_path / "no.model"), ema=True)
    with pytest.raises(ValueError, match="average"):
        plain.ema_weights()
    # loading into a model with an average restarts that average from the loaded weights
    other = build('adam', 6, dev, ema=0.5, use_graph=False)
    other.load_model(path)
    assert all(ema_ref.same_bits(_flat(other, 'ema')[k], _flat(other, 'w')[k]) for k in GENS)


def test_train_writes_the_averaged_model_beside_each_checkpoint(dev, tmp_path):
    out, models = str(tmp_path / "out"), str(tmp_path / "models")
    np.random.seed(5)
    m = build('adam', 7, dev, ema=0.9)
    m.train(*_iterators(dev), batch_size=4, num_epochs=2, out_dir=out, model_dir=models, save_every=1)
    assert sorted(os.listdir(models)) == ['1.ema.model', '1.model', '2.ema.model', '2.model']
    live, avg = m._read_checkpoint(models + "/2.model"), m._read_checkpoint(models + "/2.ema.model")
    for stage, key in (('dcgan', 'dcgan_gen'), ('p2p', 'p2p_gen')):
        assert all(np.array_equal(x, y) for x, y in zip(avg[stage]['gen'], m.engine.ema_values(key)))
        assert any(not np.array_equal(x, y) for x, y in zip(avg[stage]['gen'], live[stage]['gen']))
        assert all(np.array_equal(x, y) for x, y in zip(avg[stage]['disc'], live[stage]['disc']))
    # without the average the loop writes what it always wrote
    plain = build('adam', 7, dev)
    plain.train(*_iterators(dev), batch_size=4, num_epochs=1, out_dir=out, model_dir=str(tmp_path / "plain"), save_every=1)
    assert os.listdir(str(tmp_path / "plain")) == ['1.model']
