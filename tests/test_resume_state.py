"""The training-state checkpoint on CPU: the iterators' get_state / set_state, the file format of
Pix2Pix.save_checkpoint, the ValueError of every engine mismatch, and the sharded (rs_ag) optimiser state of a
two-rank gloo run gathered into one whole-net state that a world-1 engine loads.  Engines run on
tests/fake_device.host_device_class() (host-memory contexts; the exchange and rmsprop do arithmetic)."""
import gzip
import os
import pickle
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ['dcgan_gen', 'dcgan_disc', 'p2p_gen', 'p2p_disc']


def _nets(seed, nf=4):
    from gan_heightmaps_amd import init
    from gan_heightmaps_amd.architectures import dcgan, p2p
    from gan_heightmaps_amd.nonlinearities import linear, tanh
    init.set_rng(np.random.RandomState(seed))
    G = dcgan.default_generator(24, True, nch=16, div=[2, 2, 4])
    D = dcgan.default_discriminator(32, True, nch=16, div=[4, 2, 2], nonlinearity=linear)
    U = p2p.g_unet(32, True, False, nf=nf, act=tanh, bilinear_upsample=True, dropout=True)
    P = p2p.discriminator(32, True, False, nf=4, act=linear, mul_factor=[1, 2])
    return G, D, U, P


def _engine(dev, kind='rmsprop', dtype='f32', train_mode='both', nf=4, seed=7, **hp):
    from gan_heightmaps_amd import updates
    from gan_heightmaps_amd.step import GanStep
    G, D, U, P = _nets(seed, nf)
    spec = getattr(updates, kind)(learning_rate=updates.shared(1e-2), **hp)
    return GanStep(dev, G, D, U, P, 100, True, 'l1', spec, train_mode, use_graph=False, dtype=dtype)


def _model(dev, seed, kind='rmsprop'):
    from gan_heightmaps_amd.architectures import dcgan, p2p
    from gan_heightmaps_amd import nonlinearities as NL, updates
    from gan_heightmaps_amd.pix2pix import Pix2Pix
    return Pix2Pix(gen_fn_dcgan=dcgan.default_generator, disc_fn_dcgan=dcgan.default_discriminator,
                   gen_params_dcgan=dict(nch=16, div=[2, 2, 4]),
                   disc_params_dcgan=dict(nch=16, div=[4, 2, 2], nonlinearity=NL.linear),
                   gen_fn_p2p=p2p.g_unet, disc_fn_p2p=p2p.discriminator,
                   gen_params_p2p=dict(nf=4, dropout=True), disc_params_p2p=dict(nf=4, mul_factor=[1, 2]),
                   in_shp=32, latent_dim=24, is_a_grayscale=True, is_b_grayscale=False,
                   opt=getattr(updates, kind), opt_args={'learning_rate': updates.shared(np.float32(2e-3))},
                   verbose=False, seed=seed, device=dev)


def _fill(eng, seed):
    """non-trivial state in every buffer a training state holds (the host kernels are no-ops: put it there by hand)"""
    rng = np.random.RandomState(seed)
    for k in KEYS:
        st = eng.stores[k]
        for s in eng.opt_rule.slots:
            st.opt_state[s].set(np.concatenate([rng.rand(st.n_train), np.zeros(st.n_pad - st.n_train)]).astype(np.float32))
        eng.hyper[k].set(np.array([rng.rand(), 17.0], np.float32))
    eng.built(4)
    for t in eng._counters().values():
        t.set(np.array([rng.randint(1, 1 << 31)], np.uint32).view(np.float32))


# ---- iterators -------------------------------------------------------------------------------------------------------
def _plans(it, n):
    out = []
    for _ in range(n):
        sl, perm, table = it.plan_next()
        out.append((sl.start, sl.stop, perm.tolist(), table.tolist()))
    return out


@pytest.mark.parametrize("split", [0, 2, 3, 5])
def test_hdf5_iterator_state_round_trip_across_an_epoch_boundary(split):
    from gan_heightmaps_amd.data import Hdf5Iterator, ImageDataGenerator
    X = np.zeros((10, 8, 8, 1), np.uint8)
    Y = np.zeros((10, 8, 8, 3), np.uint8)
    mk = lambda: Hdf5Iterator(X, Y, 4, ImageDataGenerator(horizontal_flip=True, vertical_flip=True, rotation_range=30,
                                                          fill_mode='reflect'), True, False)
    a = mk()
    _plans(a, split)                    # 3 slices per pass (4, 4, 2): splits before, inside and after a boundary
    state = pickle.loads(pickle.dumps(a.get_state(), 2))
    want = _plans(a, 7)
    b = mk()
    _plans(b, 1)                        # a different position, then the saved one
    b.set_state(state)
    assert b.peek_n() == len(range(*slice(want[0][0], want[0][1]).indices(10)))
    assert _plans(b, 7) == want


def test_array_iterator_state_round_trip():
    from gan_heightmaps_amd.experiments import ArrayIterator, synthetic_arrays
    X, Y = synthetic_arrays(6, 8, True, False)
    a = ArrayIterator(X, Y, 4, True, False, seed=3)
    next(a)
    state = a.get_state()
    want = [next(a) for _ in range(5)]
    b = ArrayIterator(X, Y, 4, True, False, seed=99)
    b.set_state(state)
    for (x0, y0), (x1, y1) in zip(want, [next(b) for _ in range(5)]):
        assert np.array_equal(x0, x1) and np.array_equal(y0, y1)


# ---- engine state and file format --------------------------------------------------------------------------------------
def test_engine_state_round_trip_in_place_with_pending_counters():
    from tests.fake_device import host_device_class
    HD = host_device_class()
    src = _engine(HD(0), 'amsgrad')
    _fill(src, 1)
    st = src.training_state()
    assert set(st['rng_counters']) == {('U', 4)}         # (the DCGAN generator has no dropout: no counter)
    dst = _engine(HD(0), 'amsgrad', seed=8)
    ptrs = {k: ({s: t.ptr for s, t in dst.stores[k].opt_state.items()}, dst.hyper[k].ptr) for k in KEYS}
    dst.restore_training_state(st)
    for k in KEYS:
        assert {s: t.ptr for s, t in dst.stores[k].opt_state.items()} == ptrs[k][0]        # the same buffers
        assert dst.hyper[k].ptr == ptrs[k][1]
        for s in ('m', 'v', 'vhat'):
            full = dst.stores[k].opt_state[s].numpy().ravel()
            assert np.array_equal(full[:dst.stores[k].n_train], st['nets'][k]['slots'][s])
            assert not full[dst.stores[k].n_train:].any()
        assert np.array_equal(dst.hyper[k].numpy().ravel(), st['nets'][k]['hyper'])
    # no plan built in dst yet: the counters wait for their plan
    assert dst._counters() == {}
    dst.built(4)
    got = {k: int(t.numpy().ravel().view(np.uint32)[0]) for k, t in dst._counters().items()}
    assert got == {k: v for k, v in st['rng_counters'].items() if k in got} and got
    assert dst.training_state()['rng_counters'] == st['rng_counters']


def test_checkpoint_file_format_and_load_model_compatibility(tmp_path):
    from gan_heightmaps_amd import layers as L
    from tests.fake_device import host_device_class
    HD = host_device_class()
    m = _model(HD(0), seed=5, kind='adam')
    _fill(m.engine, 2)
    path = str(tmp_path / "state.model")
    np.random.seed(11)
    m.save_checkpoint(path, {'train': object()}, epoch=3)
    raw = gzip.open(path).read()
    assert raw[:2] == b'\x80\x02'                                 # pickle protocol 2
    dd = pickle.loads(raw, encoding='latin1')
    assert list(dd) == ['dcgan', 'p2p', 'train_state']
    assert sorted(dd['dcgan']) == ['disc', 'gen'] and sorted(dd['p2p']) == ['disc', 'gen']
    plain = str(tmp_path / "plain.model")
    m.save_model(plain)
    old = pickle.load(gzip.open(plain), encoding='latin1')
    for a in ('dcgan', 'p2p'):
        for b in ('gen', 'disc'):
            assert len(old[a][b]) == len(dd[a][b])
            assert all(np.array_equal(x, y) for x, y in zip(old[a][b], dd[a][b]))
    ts = dd['train_state']
    assert ts['epoch'] == 3 and ts['iterators'] == {} and ts['version'] == 1
    assert ts['engine']['kind'] == 'adam' and np.float32(ts['lr']) == np.float32(2e-3)
    # load_model reads the parameters of a state checkpoint
    m2 = _model(HD(0), seed=6, kind='adam')
    m2.load_model(path)
    for net in ('dcgan', 'p2p'):
        for b in ('gen', 'disc'):
            for x, y in zip(L.get_all_param_values(getattr(m2, net)[b]), dd[net][b]):
                assert np.array_equal(x, y)
    # load_checkpoint restores the rest; an iterator without set_state is reported
    m3 = _model(HD(0), seed=7, kind='adam')
    m3.lr.set_value(1.0)
    np.random.seed(0)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert m3.load_checkpoint(path, {'train': object()}) == 3
    assert any(issubclass(x.category, RuntimeWarning) and 'batch order' in str(x.message) for x in w)
    assert m3.lr.get_value() == np.float32(2e-3)
    got = np.random.rand(4)                                       # numpy's global RNG continues from the save
    np.random.seed(11)
    assert np.array_equal(got, np.random.rand(4))
    m3_state = m3.engine.training_state()
    for k in KEYS:
        for s in ('m', 'v'):
            assert np.array_equal(m3_state['nets'][k]['slots'][s], ts['engine']['nets'][k]['slots'][s])
        # t from the engine state, lr through the shared learning rate (hyper[0] follows it)
        assert m3_state['nets'][k]['hyper'].tolist() == [np.float32(2e-3), ts['engine']['nets'][k]['hyper'][1]]
    # a params-only file has no state to continue from
    with pytest.raises(ValueError, match="no training state"):
        m3.load_checkpoint(plain)


@pytest.mark.parametrize("case", ["kind", "hp", "dtype", "train_mode", "n_train"])
def test_every_mismatch_raises_value_error_naming_the_field(case):
    from tests.fake_device import host_device_class
    HD = host_device_class()
    src = _engine(HD(0), 'adam')
    _fill(src, 3)
    st = src.training_state()
    other = {'kind': dict(kind='amsgrad'), 'hp': dict(kind='adam', beta1=0.5), 'dtype': dict(kind='adam', dtype='bf16x3'),
             'train_mode': dict(kind='adam', train_mode='p2p'), 'n_train': dict(kind='adam', nf=8)}[case]
    dst = _engine(HD(0), **other)
    before = {k: dst.stores[k].opt_state['m'].numpy().copy() for k in KEYS if 'm' in dst.stores[k].opt_state}
    with pytest.raises(ValueError, match=case):
        dst.restore_training_state(st)
    for k, v in before.items():
        assert np.array_equal(dst.stores[k].opt_state['m'].numpy(), v)         # nothing was changed


def test_state_checkpoint_of_a_different_configuration_is_refused_before_loading(tmp_path):
    from gan_heightmaps_amd import layers as L
    from tests.fake_device import host_device_class
    HD = host_device_class()
    m = _model(HD(0), seed=5, kind='adam')
    path = str(tmp_path / "s.model")
    m.save_checkpoint(path)
    m2 = _model(HD(0), seed=6, kind='rmsprop')
    before = L.get_all_param_values(m2.p2p['gen'])
    with pytest.raises(ValueError, match="kind"):
        m2.load_checkpoint(path)
    assert all(np.array_equal(a, b) for a, b in zip(before, L.get_all_param_values(m2.p2p['gen'])))


# ---- sharded optimiser state of two ranks (gloo) ----------------------------------------------------------------------
def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as tdist
    tdist.init_process_group("gloo", rank=rank, world_size=world)
    from gan_heightmaps_amd import updates
    from gan_heightmaps_amd.step import GanStep
    from tests.fake_device import host_device_class

    HostDevice = host_device_class()
    dev, cdev = HostDevice(0), HostDevice(0)

    class GlooComm:
        def __init__(self):
            self.dev, self.rank, self.world = cdev, rank, world

        def max_scalar(self, v):
            t = torch.tensor([float(v)], dtype=torch.float64)
            tdist.all_reduce(t, op=tdist.ReduceOp.MAX)
            return float(t[0])

    G, D, U, P = _nets(seed=7)
    spec = updates.rmsprop(learning_rate=updates.shared(1e-2))
    eng = GanStep(dev, G, D, U, P, 100, True, 'l1', spec, 'both', comm=GlooComm(), use_graph=False,
                  two_streams=True, side_streams=True, bucket_mb=2048.0 / 2 ** 20, exchange_mode='rs_ag')
    eng.broadcast_parameters()
    b = eng.built(4)
    rng = np.random.RandomState(50 + rank)
    for _ in range(2):
        for k in KEYS:
            st = eng.stores[k]
            st.g.set(np.concatenate([rng.randn(st.n_train), np.zeros(st.n_pad - st.n_train)]).astype(np.float32))
        eng.enqueue_train(b)
    eng.sync()
    shards = {k: eng.stores[k].opt_state['acc'].numpy().ravel().copy() for k in KEYS}
    state = eng.training_state()
    out = {"rank": rank, "shards": shards, "state": state, "xchg_order": list(b.xchg_order),
           "n_pad": {k: eng.stores[k].n_pad for k in KEYS},
           "w": {k: eng.stores[k].w.numpy().ravel()[:eng.stores[k].n_train].copy() for k in KEYS}}
    with open(os.path.join(out_dir, "r%d.pkl" % rank), "wb") as f:
        pickle.dump(out, f)
    tdist.destroy_process_group()


def test_sharded_state_is_gathered_whole_and_loads_into_a_world_one_engine(tmp_path):
    pytest.importorskip("torch")
    import torch.multiprocessing as tmp_
    world, port = 2, 39500 + (os.getpid() % 2000)
    tmp_.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    rs = [pickle.load(open(os.path.join(str(tmp_path), "r%d.pkl" % r), "rb")) for r in range(world)]
    s0, s1 = rs[0]["state"], rs[1]["state"]
    for k in KEYS:
        # the same whole-net state on both ranks ...
        assert np.array_equal(s0['nets'][k]['slots']['acc'], s1['nets'][k]['slots']['acc'])
        assert np.array_equal(s0['nets'][k]['hyper'], s1['nets'][k]['hyper'])
        # ... = the concatenation of the ranks' shards: bucket by bucket, rank r's slice of each bucket from rank r
        want = np.zeros(rs[0]["n_pad"][k], np.float32)
        buckets = [(lo, n) for _, kk, lo, n in rs[0]["xchg_order"] if kk == k]
        assert sum(n for _, n in buckets) == rs[0]["n_pad"][k]
        for lo, n in buckets:
            sh = n // world
            for r in range(world):
                want[lo + r * sh:lo + (r + 1) * sh] = rs[r]["shards"][k][lo + r * sh:lo + (r + 1) * sh]
        got = s0['nets'][k]['slots']['acc']
        assert np.array_equal(got, want[:got.size]) and got.any()
        # each rank's own shards were nonzero and the other rank's untouched before the gather
        assert not np.array_equal(rs[0]["shards"][k], rs[1]["shards"][k])
    # it loads into a world-1 engine (different padding: no sharding)
    from tests.fake_device import host_device_class
    HD = host_device_class()
    one = _engine(HD(0), 'rmsprop', dtype='bf16x3')       # (GanStep's default, as in the ranks)
    one.restore_training_state(s0)
    for k in KEYS:
        st = one.stores[k]
        assert st.n_pad == st.n_train
        assert np.array_equal(st.opt_state['acc'].numpy().ravel(), s0['nets'][k]['slots']['acc'])
        assert np.array_equal(one.hyper[k].numpy().ravel(), s0['nets'][k]['hyper'])
