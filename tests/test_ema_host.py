"""The exponential moving average of the generator weights on CPU: the float32 restatement against a float64
recurrence, where the ``ema_<net>`` entries stand in the update program, that ema=None leaves the program as it was, the
rs_ag refusal, the checkpoint rules, and the ema_weights() contract.  Engines run on tests/fake_device.py's devices."""
import gzip
import pickle
import warnings

import numpy as np
import pytest

from gan_heightmaps_amd import init, updates
from gan_heightmaps_amd.architectures import dcgan, p2p
from gan_heightmaps_amd.device import DevTensor
from gan_heightmaps_amd.nonlinearities import linear, tanh
from gan_heightmaps_amd.step import EMA_NETS, GanStep
from gan_heightmaps_amd.step_build import LANE_OF
from tests import ema_ref
from tests.fake_device import FakeDevice, host_device_class

KEYS = ['dcgan_gen', 'dcgan_disc', 'p2p_gen', 'p2p_disc']


def _nets(seed=7):
    init.set_rng(np.random.RandomState(seed))
    G = dcgan.default_generator(24, True, nch=16, div=[2, 2, 4])
    D = dcgan.default_discriminator(32, True, nch=16, div=[4, 2, 2], nonlinearity=linear)
    U = p2p.g_unet(32, True, False, nf=4, act=tanh, bilinear_upsample=True, dropout=True)
    P = p2p.discriminator(32, True, False, nf=4, act=linear, mul_factor=[1, 2])
    return G, D, U, P


def _engine(dev, kind='adam', train_mode='both', seed=7, **kw):
    G, D, U, P = _nets(seed)
    spec = getattr(updates, kind)(learning_rate=updates.shared(1e-2))
    kw.setdefault('use_graph', False)
    return GanStep(dev, G, D, U, P, 100, True, 'l1', spec, train_mode, **kw)


# ---- the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decay", [0.5, 0.9])
def test_restatement_follows_the_float64_recurrence(decay):
    """values in [1, 2): one binade, ulp = 2^-23.  A step rounds three times (two products, one sum), each by at most half an
    ulp of a value below 2, and the recurrence damps the error carried over by ``decay``: the error settles below
    1.5 ulp / (1 - decay) -- 3 ulps at 0.5, 15 at 0.9."""
    rng = np.random.RandomState(0)
    d, c = ema_ref.coefficients(decay)
    assert d == np.float32(decay) and c == np.float32(1.0 - float(np.float32(decay))) and c.dtype == np.float32
    e32 = (1.0 + rng.rand(4096)).astype(np.float32)
    e64 = e32.astype(np.float64)
    ulp = 2.0 ** -23
    for _ in range(60):
        w = (1.0 + rng.rand(4096)).astype(np.float32)
        e32 = ema_ref.ema_update(e32, w, decay)
        e64 = float(d) * e64 + float(c) * w.astype(np.float64)
        assert e32.dtype == np.float32
        assert np.abs(e32.astype(np.float64) - e64).max() <= 1.5 * ulp / (1.0 - decay)


def test_restatement_rounds_each_operation_and_skips():
    # fl(fl(d e) + fl(c w)) differs from the single-rounded d e + c w on some inputs: the three roundings are kept apart
    rng = np.random.RandomState(1)
    e, w = rng.randn(1 << 14).astype(np.float32), rng.randn(1 << 14).astype(np.float32)
    d, c = ema_ref.coefficients(0.999)
    got = ema_ref.ema_update(e, w, 0.999)
    want = (np.float32(d * e) + np.float32(c * w)).astype(np.float32)
    assert ema_ref.same_bits(got, want)
    fused = (float(d) * e.astype(np.float64) + float(c) * w.astype(np.float64)).astype(np.float32)
    assert not ema_ref.same_bits(got, fused)
    assert ema_ref.same_bits(ema_ref.ema_update(e, w, 0.999, skip=True), e)
    run = ema_ref.ema_run(e, [w, w, w], 0.5, skipped={1})
    assert ema_ref.same_bits(run[1], run[0]) and not ema_ref.same_bits(run[2], run[1])
    # decay 0 is the weights themselves (0 * e + 1 * w, exact for finite e)
    assert ema_ref.same_bits(ema_ref.ema_update(e, w, 0.0), w + np.float32(0) * e)


# ---- program placement ----------------------------------------------------------------------------------------------
def _labels(b):
    return [[e[0] for e in lane] for lane in b.update]


@pytest.mark.parametrize("dtype", ['f32', 'f16'])
@pytest.mark.parametrize("two_streams", [False, True])
@pytest.mark.parametrize("train_mode", ['both', 'dcgan', 'p2p'])
@pytest.mark.parametrize("kind", ['adam', 'rmsprop'])
def test_ema_entries_follow_their_update_on_its_lane(kind, train_mode, two_streams, dtype):
    eng = _engine(FakeDevice(), kind, train_mode, two_streams=two_streams, dtype=dtype, ema=0.9)
    b = eng.built(4)
    labels = _labels(b)
    updated = [k for k in KEYS if train_mode == 'both' or k.startswith(train_mode)]
    want = ['ema_' + k for k in updated if k in EMA_NETS]
    assert sorted(l for lane in labels for l in lane if l.startswith('ema_')) == sorted(want) and want
    ticks = kind == 'adam'
    for k in EMA_NETS:
        st = eng.stores[k]
        assert st.ema.size == st.n_pad and st.ema.dev is eng.devs[LANE_OF[k]]
        if 'ema_' + k not in want:
            continue
        # the update lists are per stage even on one stream, except in fp16 (one list: check* -> update* -> scale update)
        lane = 0 if (dtype == 'f16' and not two_streams) else LANE_OF[k]
        ll = labels[lane]
        i = ll.index('ema_' + k)
        assert ll[i - 1] == (kind + '_tick_' + k if ticks else kind + '_' + k)
        if ticks:
            assert ll[i - 2] == kind + '_' + k
        if dtype == 'f16':
            assert ll[-1] == 'loss_scale_update' and ll.count('loss_scale_update') == 1 and i < len(ll) - 1
        else:
            assert 'loss_scale_update' not in ll
        # the launch: this net's average and weights, n_train elements, the decay -- on the lane's ops
        before = len(eng.ops[lane].calls)
        b.update[lane][i][1]()
        (name, args, _), = eng.ops[lane].calls[before:]
        assert name == 'ema_update' and args[0] is st.ema and args[1] is st.w and args[2:] == (st.n_train, 0.9)
    for k in ('dcgan_disc', 'p2p_disc'):
        assert not hasattr(eng.stores[k], 'ema')


def _norm(v):
    if isinstance(v, DevTensor):
        return ('T', v.ptr, v.shape, v.nstride)
    if isinstance(v, (list, tuple)):
        return tuple(_norm(x) for x in v)
    if isinstance(v, (int, float, str, bool, type(None), np.integer, np.floating)):
        return v
    if hasattr(v, 'ptr'):
        return (type(v).__name__, int(v.ptr))
    if hasattr(v, '_fields_'):
        return tuple(getattr(v, f) for f, _ in v._fields_)
    return type(v).__name__


def _trace(eng):
    """labels, lanes and recorded op calls of one eagerly issued train step"""
    b = eng.built(4)
    seq = eng._sequence(b, 'train')
    for _, e in seq:
        e[1]()
    calls = [[(n, _norm(a), _norm(sorted(kw.items()))) for n, a, kw in o.calls] for o in eng.ops]
    return [(lane, e[0]) for lane, e in seq], calls


@pytest.mark.parametrize("dtype", ['f32', 'f16'])
@pytest.mark.parametrize("two_streams", [False, True])
@pytest.mark.parametrize("train_mode", ['both', 'dcgan', 'p2p'])
def test_ema_none_is_the_program_without_the_argument(train_mode, two_streams, dtype):
    G, D, U, P = _nets()
    spec = updates.adam(learning_rate=updates.shared(1e-2))
    plain = GanStep(FakeDevice(), G, D, U, P, 100, True, 'l1', spec, train_mode, use_graph=False, two_streams=two_streams,
                    dtype=dtype)
    none = _engine(FakeDevice(), 'adam', train_mode, two_streams=two_streams, dtype=dtype, ema=None)
    assert none.ema is None and not any(hasattr(st, 'ema') for st in none.stores.values())
    assert none.devs[0].bytes_allocated == plain.devs[0].bytes_allocated
    tp, tn = _trace(plain), _trace(none)
    assert tp == tn
    # ... and the average adds its entries and nothing else
    with_ema = _trace(_engine(FakeDevice(), 'adam', train_mode, two_streams=two_streams, dtype=dtype, ema=0.9))
    assert [x for x in with_ema[0] if not x[1].startswith('ema_')] == tp[0]
    assert [[c[0] for c in cs if c[0] != 'ema_update'] for cs in with_ema[1]] == [[c[0] for c in cs] for cs in tp[1]]


def test_decay_outside_the_unit_interval_is_refused():
    for bad in (1.0, -0.1, 1.5, float('nan'), float('inf'), 1.0 - 1e-12):       # (the last rounds to 1 in fp32)
        with pytest.raises(ValueError, match="ema"):
            _engine(FakeDevice(), ema=bad)
    assert _engine(FakeDevice(), ema=0).ema == 0.0


# ---- data-parallel forms --------------------------------------------------------------------------------------------
class _OneRank:
    """the one-rank communicator of the forced-exchange construction path (tests/test_dp_product.py)"""

    def __init__(self, dev):
        self.dev, self.rank, self.world = dev, 0, 1

    def max_scalar(self, v):
        return float(v)


def test_sharded_exchange_with_an_average_is_refused():
    HD = host_device_class()
    with pytest.raises(NotImplementedError, match="ema"):
        _engine(HD(0), 'rmsprop', comm=_OneRank(HD(0)), force_exchange=True, exchange_mode='rs_ag', ema=0.9)
    _engine(HD(0), 'rmsprop', comm=_OneRank(HD(0)), force_exchange=True, exchange_mode='rs_ag')          # (as before without)
    eng = _engine(HD(0), 'rmsprop', comm=_OneRank(HD(0)), force_exchange=True, exchange_mode='allreduce', ema=0.9)
    assert eng.exchange and not eng.sharded
    labels = _labels(eng.built(4))
    assert labels[0][labels[0].index('rmsprop_dcgan_gen') + 1] == 'ema_dcgan_gen'
    assert labels[1][labels[1].index('rmsprop_p2p_gen') + 1] == 'ema_p2p_gen'
    # the replica checksum covers the averages
    c0 = eng.replica_checksums()
    st = eng.stores['p2p_gen']
    st.ema.set(st.ema.numpy() + 1)
    assert eng.replica_checksums() != c0


# ---- buffers, checkpoints ---------------------------------------------------------------------------------------------
def _randomise_ema(eng, seed):
    rng = np.random.RandomState(seed)
    for k in EMA_NETS:
        st = eng.stores[k]
        st.ema.set(rng.randn(st.n_pad).astype(np.float32))


def test_the_average_starts_at_the_weights_and_reset_ema_returns_it_there():
    HD = host_device_class()
    eng = _engine(HD(0), ema=0.9)
    for k in EMA_NETS:
        st = eng.stores[k]
        assert np.array_equal(st.ema.numpy().ravel()[:st.n_train], st.w.numpy().ravel()[:st.n_train])
        assert st.w.numpy().any()
    _randomise_ema(eng, 0)
    eng.reset_ema()
    for k in EMA_NETS:
        st = eng.stores[k]
        assert np.array_equal(st.ema.numpy().ravel()[:st.n_train], st.w.numpy().ravel()[:st.n_train])
    with pytest.raises(ValueError, match="average"):
        _engine(HD(0)).reset_ema()


def test_training_state_keys_with_and_without_an_average():
    HD = host_device_class()
    plain = _engine(HD(0), 'adam').training_state()
    assert set(plain) == {'kind', 'hp', 'dtype', 'train_mode', 'nets', 'rng_counters', 'loss_scale'}
    assert all(set(v) == {'n_train', 'n_state', 'hyper', 'slots'} for v in plain['nets'].values())
    eng = _engine(HD(0), 'adam', ema=0.9)
    _randomise_ema(eng, 1)
    st = eng.training_state()
    assert set(st) == set(plain) | {'ema'} and st['ema'] == 0.9
    for k in KEYS:
        assert set(st['nets'][k]) == {'n_train', 'n_state', 'hyper', 'slots'} | ({'ema'} if k in EMA_NETS else set())
    for k in EMA_NETS:
        s = eng.stores[k]
        assert st['nets'][k]['ema'].shape == (s.n_train,)
        assert np.array_equal(st['nets'][k]['ema'], s.ema.numpy().ravel()[:s.n_train])
    # without the average the state pickles to the bytes of an engine that never heard of it
    G, D, U, P = _nets()
    spec = updates.adam(learning_rate=updates.shared(1e-2))
    bare = GanStep(HD(0), G, D, U, P, 100, True, 'l1', spec, 'both', use_graph=False).training_state()
    assert pickle.dumps(bare, 2) == pickle.dumps(plain, 2)


def _slots(eng):
    return {k: {s: t.numpy().copy() for s, t in eng.stores[k].opt_state.items()} for k in KEYS}


def test_check_training_state_cases():
    HD = host_device_class()
    src = _engine(HD(0), 'adam', ema=0.9)
    _randomise_ema(src, 2)
    for k in KEYS:
        for t in src.stores[k].opt_state.values():
            t.set(np.full(t.size, 3.0, np.float32))
    state = src.training_state()
    # the same decay: accepted, written in place
    dst = _engine(HD(0), 'adam', seed=8, ema=0.9)
    ptrs = {k: dst.stores[k].ema.ptr for k in EMA_NETS}
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        dst.check_training_state(state)
        dst.restore_training_state(state)
    for k in EMA_NETS:
        s = dst.stores[k]
        assert s.ema.ptr == ptrs[k]
        assert np.array_equal(s.ema.numpy().ravel()[:s.n_train], state['nets'][k]['ema'])
        assert not s.ema.numpy().ravel()[s.n_train:].any()
    # another decay, an average the run does not keep, values that do not fit: ValueError naming ema, nothing written
    for eng, st in ((_engine(HD(0), 'adam', seed=8, ema=0.5), state), (_engine(HD(0), 'adam', seed=8), state),
                    (_engine(HD(0), 'adam', seed=8, ema=0.9),
                     dict(state, nets=dict(state['nets'], p2p_gen=dict(state['nets']['p2p_gen'], ema=np.zeros(3, np.float32)))))):
        before = _slots(eng)
        ema_before = {k: eng.stores[k].ema.numpy().copy() for k in EMA_NETS} if eng.ema is not None else {}
        with pytest.raises(ValueError, match="ema"):
            eng.check_training_state(st)
        with pytest.raises(ValueError, match="ema"):
            eng.restore_training_state(st)
        after = _slots(eng)
        assert all(np.array_equal(before[k][s], after[k][s]) for k in KEYS for s in before[k])
        assert all(np.array_equal(v, eng.stores[k].ema.numpy()) for k, v in ema_before.items())
    # a checkpoint without an average into a run with one: accepted with a warning, the average is the loaded weights
    old = _engine(HD(0), 'adam', seed=9).training_state()
    eng = _engine(HD(0), 'adam', seed=8, ema=0.9)
    _randomise_ema(eng, 3)
    with pytest.warns(RuntimeWarning, match="ema"):
        eng.check_training_state(old)
    with pytest.warns(RuntimeWarning, match="ema"):
        eng.restore_training_state(old)
    for k in EMA_NETS:
        s = eng.stores[k]
        assert np.array_equal(s.ema.numpy().ravel()[:s.n_train], s.w.numpy().ravel()[:s.n_train])


# ---- ema_weights() ----------------------------------------------------------------------------------------------------
def _swaps(eng):
    return [(lane, c) for lane, o in enumerate(eng.ops) for c in o.calls if c[0] == 'swap_f32']


def test_ema_weights_moves_param_version_and_refuses_what_moves_state():
    eng = _engine(FakeDevice(), ema=0.9)
    b = eng.built(4)
    Z, X, Y = np.zeros((4, 24), np.float32), np.zeros((4, 1, 32, 32), np.float32), np.zeros((4, 3, 32, 32), np.float32)
    state = eng.training_state()
    v0 = eng.param_version
    with eng.ema_weights() as inside:
        assert inside is eng
        v1 = eng.param_version
        assert v1 != v0
        sw = _swaps(eng)
        assert [lane for lane, _ in sw] == [LANE_OF[k] for k in EMA_NETS]
        for (_, (_, args, _)), k in zip(sw, EMA_NETS):
            st = eng.stores[k]
            assert args[0] is st.w and args[1] is st.ema and args[2] == st.n_train
        for call in (lambda: eng.train(Z, X, Y), lambda: eng.loss(Z, X, Y), lambda: eng.enqueue_train(b),
                     lambda: eng.train_pipelined([(Z, X, Y)]), lambda: eng.train_pipelined_from_iterator(None, None, 1),
                     lambda: eng.run_from_iterator(None, None), lambda: eng.generate('dcgan_gen', Z, False),
                     lambda: eng.generate('p2p_gen', X, False), lambda: eng.generate_chain(Z, False),
                     lambda: eng.restore_training_state(state), lambda: eng.training_state(), eng.reset_ema,
                     eng.ema_weights, lambda: eng.profile_train(4)):
            with pytest.raises(RuntimeError, match="ema_weights"):
                call()
        assert eng.param_version == v1 and len(_swaps(eng)) == 2         # nothing of that was issued
        eng.generate('dcgan_gen', Z, True)                              # the deterministic forwards run
        eng.generate_chain(Z, True)
        assert eng.param_version == v1
    assert eng.param_version not in (v0, v1) and len(_swaps(eng)) == 4
    eng.train(Z, X, Y)                                                  # and outside everything runs again
    with eng.ema_weights():
        pass


def test_ema_weights_swaps_back_when_the_body_raises():
    eng = _engine(FakeDevice(), ema=0.9)
    v0 = eng.param_version
    with pytest.raises(KeyError):
        with eng.ema_weights():
            raise KeyError("body")
    sw = _swaps(eng)
    assert [lane for lane, _ in sw] == [0, 0, 1, 1]         # per lane: the entry swap, then the same again
    assert all(x[1][0] is y[1][0] and x[1][1] is y[1][1] and x[1][2] == y[1][2] for (_, x), (_, y) in (sw[:2], sw[2:]))
    assert eng.param_version == v0 + 2 and not eng._in_ema
    with eng.ema_weights():             # usable again
        pass


def test_ema_weights_without_an_average_is_a_value_error():
    eng = _engine(FakeDevice())
    with pytest.raises(ValueError, match="average"):
        eng.ema_weights()
    with pytest.raises(ValueError, match="average"):
        with eng.ema_weights():
            pass


# ---- Pix2Pix: files -------------------------------------------------------------------------------------------------
def _model(dev, seed, **kw):
    from gan_heightmaps_amd import nonlinearities as NL
    from gan_heightmaps_amd.pix2pix import Pix2Pix
    return Pix2Pix(gen_fn_dcgan=dcgan.default_generator, disc_fn_dcgan=dcgan.default_discriminator,
                   gen_params_dcgan=dict(nch=16, div=[2, 2, 4]),
                   disc_params_dcgan=dict(nch=16, div=[4, 2, 2], nonlinearity=NL.linear),
                   gen_fn_p2p=p2p.g_unet, disc_fn_p2p=p2p.discriminator,
                   gen_params_p2p=dict(nf=4, dropout=True), disc_params_p2p=dict(nf=4, mul_factor=[1, 2]),
                   in_shp=32, latent_dim=24, is_a_grayscale=True, is_b_grayscale=False,
                   opt=updates.adam, opt_args={'learning_rate': updates.shared(np.float32(2e-3))},
                   verbose=False, seed=seed, device=dev, use_graph=False, **kw)


def _read(path):
    with gzip.open(path) as g:
        return pickle.load(g, encoding='latin1')


def test_save_model_ema(tmp_path):
    from gan_heightmaps_amd import layers as L
    HD = host_device_class()
    plain = _model(HD(0), 1)
    with pytest.raises(ValueError, match="average"):
        plain.save_model(str(tmp_path / "x.model"), ema=True)
    with pytest.raises(ValueError, match="average"):
        plain.ema_weights()
    m = _model(HD(0), 2, ema=0.9)
    _randomise_ema(m.engine, 4)
    v = m.engine.param_version
    m.save_model(str(tmp_path / "live.model"))
    m.save_model(str(tmp_path / "ema.model"), ema=True)
    assert m.engine.param_version == v                    # read from the average's buffer: nothing was exchanged
    live, avg = _read(str(tmp_path / "live.model")), _read(str(tmp_path / "ema.model"))
    assert set(avg) == set(live) == {'dcgan', 'p2p'}
    for stage, key in (('dcgan', 'dcgan_gen'), ('p2p', 'p2p_gen')):
        st = m.engine.stores[key]
        params = L.get_all_params(getattr(m, stage)['gen'])
        assert len(avg[stage]['gen']) == len(live[stage]['gen']) == len(params)
        for p, a, l in zip(params, avg[stage]['gen'], live[stage]['gen']):
            assert a.shape == l.shape == p.shape and a.dtype == np.float32
            if p.index[0] == 'w':       # trainable: the average, in lasagne layout; the rest (BatchNorm statistics): live
                want = st._from_device_layout(p, st._view(st.ema, p).numpy().ravel())
                assert np.array_equal(a, want) and not np.array_equal(a, l)
            else:
                assert np.array_equal(a, l)
        for a, l in zip(avg[stage]['disc'], live[stage]['disc']):
            assert np.array_equal(a, l)
    # a plain model file: a model without an average loads it, and then holds the averaged generators
    plain.load_model(str(tmp_path / "ema.model"))
    for stage in ('dcgan', 'p2p'):
        for a, got in zip(avg[stage]['gen'], L.get_all_param_values(getattr(plain, stage)['gen'])):
            assert np.array_equal(a, got)


def test_loaders_set_or_refuse_the_average(tmp_path):
    HD = host_device_class()
    src = _model(HD(0), 3)
    src.save_model(str(tmp_path / "a.model"))
    src.save_checkpoint(str(tmp_path / "a.state"), epoch=0)
    m = _model(HD(0), 4, ema=0.9)
    eng = m.engine
    _randomise_ema(eng, 5)
    kept = eng.stores['p2p_gen'].ema.numpy().copy()
    m.load_model(str(tmp_path / "a.model"), mode='dcgan')          # only the generator it loads
    st = eng.stores['dcgan_gen']
    assert np.array_equal(st.ema.numpy().ravel()[:st.n_train], st.w.numpy().ravel()[:st.n_train])
    assert np.array_equal(st.w.numpy(), src.engine.stores['dcgan_gen'].w.numpy())
    assert np.array_equal(eng.stores['p2p_gen'].ema.numpy(), kept)
    m.load_model(str(tmp_path / "a.model"))
    for k in EMA_NETS:
        st = eng.stores[k]
        assert np.array_equal(st.ema.numpy().ravel()[:st.n_train], st.w.numpy().ravel()[:st.n_train])
    Z, X, Y = np.zeros((4, 24), np.float32), np.zeros((4, 1, 32, 32), np.float32), np.zeros((4, 3, 32, 32), np.float32)
    w = {k: eng.stores[k].w.numpy().copy() for k in KEYS}
    with m.ema_weights():
        for call in (lambda: m.load_model(str(tmp_path / "a.model")), lambda: m.load_checkpoint(str(tmp_path / "a.state")),
                     lambda: m.train_fn(Z, X, Y), lambda: m.loss_fn(Z, X, Y), lambda: m.z_fn(Z), lambda: m.gen_fn(X),
                     lambda: m.train(None, None, 4, 1, str(tmp_path / "out")), m.reset_ema, m.ema_weights,
                     lambda: m.save_checkpoint(str(tmp_path / "b.state"))):
            with pytest.raises(RuntimeError, match="ema_weights"):
                call()
        m.save_model(str(tmp_path / "inside.model"))                # reading is fine
    assert all(np.array_equal(w[k], eng.stores[k].w.numpy()) for k in KEYS)
    # a state checkpoint without an average loads into the run with one, with the warning
    with pytest.warns(RuntimeWarning, match="ema"):
        m.load_checkpoint(str(tmp_path / "a.state"))
    # and one with an average does not load into a run without
    m.save_checkpoint(str(tmp_path / "m.state"), epoch=0)
    with pytest.raises(ValueError, match="ema"):
        src.load_checkpoint(str(tmp_path / "m.state"))


def test_the_ema_experiment_is_the_bilinear_one_with_a_decay():
    from gan_heightmaps_amd import experiments
    kw, base = experiments.experiment_kwargs('test1_nobn_bilin_both_ema'), experiments.experiment_kwargs('test1_nobn_bilin_both')
    assert kw.pop('ema') == 0.999 and 'ema' not in base
    kw.pop('opt_args'), base.pop('opt_args')
    assert kw == base
    assert experiments.test1_nobn_bilin_both_ema.__name__ in experiments.main.__code__.co_names
