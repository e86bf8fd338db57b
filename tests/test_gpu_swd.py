"""The sliced Wasserstein distance on the MI355X (csrc/swd.hip, gan_heightmaps_amd/swd.py): every kernel at the
smallest shapes where it can go wrong, inside NaN-filled pitches and canary margins that must come back untouched, against
the float64 restatement (tests/swd_ref.py) or numpy bit for bit; then Pix2Pix.swd and train(swd_every=) on the SMALL model."""
import gzip
import io

import numpy as np
import pytest

from oracle import step as ostep
from gan_heightmaps_amd import swd as SW
from gan_heightmaps_amd.device import DevTensor
from tests import swd_ref as R
from tests.gpu_common import build_model, dev, model_params, ops, SMALL      # noqa: F401  (dev, ops: the module-scoped fixtures)

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
MARGIN = 64                     # canary cells on either side of every buffer
FLT_MAX = np.finfo(np.float32).max


class Canary:
    """a device buffer of ``shape`` floats between two margins of NaN; ``fill``: its start value (NaN if None).  get() returns
    the body and checks that both margins are NaN still"""

    def __init__(self, dev, shape, fill=None, dtype=np.float32):
        self.dev, self.shape, self.dtype = dev, tuple(shape), dtype
        self.n = int(np.prod(shape))
        body = np.full(self.n, np.nan, np.float32) if fill is None else np.ascontiguousarray(fill, dtype).ravel().view(np.float32)
        assert body.size == self.n
        host = np.concatenate([np.full(MARGIN, np.nan, np.float32), body, np.full(MARGIN, np.nan, np.float32)])
        self.base = dev.alloc(host.nbytes)
        dev.h2d(self.base, host)
        self.ptr = self.base + 4 * MARGIN

    def get(self):
        self.dev.sync()
        host = np.empty(self.n + 2 * MARGIN, np.float32)
        self.dev.d2h(host, self.base, host.nbytes)
        assert np.isnan(host[:MARGIN]).all() and np.isnan(host[-MARGIN:]).all(), "a canary margin was written"
        return host[MARGIN:-MARGIN].view(self.dtype).reshape(self.shape).copy()

    def free(self):
        self.dev.free(self.base)


def pitched(x, pitch):
    """[..., W] -> [..., pitch] with NaN beyond W"""
    out = np.full(x.shape[:-1] + (pitch,), np.nan, np.float32)
    out[..., :x.shape[-1]] = x
    return out


# ---- 1. pyramid -----------------------------------------------------------------------------------------------------------
def _pyramid_inputs(n, C, H, W):
    rs = np.random.RandomState(H * 100 + W)
    uni = rs.uniform(-1, 1, (n, C, H, W)).astype(np.float32)
    delta = np.zeros((n, C, H, W), np.float32)
    for i, (y, x) in enumerate([(0, 0), (H - 1, W - 1), (H - 2, 1), (H // 2, W // 2 + 1)]):
        delta[i % n, i % C, y, x] = 256.0
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    ramp = np.broadcast_to(0.25 * xx - 3.0 * yy + 5.0, (n, C, H, W)).astype(np.float32)
    return {"uniform": uni, "delta": delta, "ramp": ramp}


@pytest.mark.parametrize("n,C,H,W,pitch", [(1, 1, 16, 16, 16), (2, 3, 32, 48, 48), (3, 1, 64, 64, 71)],
                         ids=["16x16", "32x48_C3", "64x64_pitch71_n3"])
def test_pyramid_level_against_the_float64_restatement(dev, ops, n, C, H, W, pitch):
    np_, lp = W // 2 + (3 if pitch > W else 0), W + (5 if pitch > W else 0)        # the outputs' pitches
    for name, x in _pyramid_inputs(n, C, H, W).items():
        src = Canary(dev, (n, C, H, pitch), pitched(x, pitch))
        nxt, lap = Canary(dev, (n, C, H // 2, np_)), Canary(dev, (n, C, H, lp))
        ops.swd_pyramid_level(DevTensor(dev, src.ptr, (n, C, H, W), C * H * pitch), pitch, nxt.ptr, np_, lap.ptr, lp)
        g1, l0 = nxt.get(), lap.get()
        assert np.array_equal(src.get()[..., :W], x)                                # the source is only read
        assert np.isnan(g1[..., W // 2:]).all() and np.isnan(l0[..., W:]).all()     # nothing beyond a row's width
        want_g, want_l = R.down(x), x.astype(np.float64) - R.up(R.down(x))
        bound = 64 * U * float(np.abs(x).max())                                     # dyadic weights, <= 50 rounded operations
        eg = float(np.abs(g1[..., :W // 2] - want_g).max())
        el = float(np.abs(l0[..., :W] - want_l).max())
        print("pyramid %dx%d %-7s: max |device - f64|: G %.3e, Lap %.3e (bound %.3e)" % (H, W, name, eg, el, bound))
        assert eg <= bound and el <= bound
        if name == "delta":
            assert np.array_equal(g1[..., :W // 2], want_g.astype(np.float32))     # small integers: exact
        # the coarsest level: Lap = G, bit for bit, from the level just made
        top = Canary(dev, (n, C, H // 2, np_))
        ops.swd_pyramid_level(DevTensor(dev, nxt.ptr, (n, C, H // 2, W // 2), C * (H // 2) * np_), np_, None, 0, top.ptr, np_)
        t = top.get()
        assert np.array_equal(t[..., :W // 2], g1[..., :W // 2]) and np.isnan(t[..., W // 2:]).all()
        for c in (src, nxt, lap, top):
            c.free()


def test_constant_image_has_an_exactly_zero_laplacian_on_the_device(dev, ops):
    x = np.full((1, 2, 16, 32), 0.7, np.float32)
    src, nxt, lap = Canary(dev, x.shape, x), Canary(dev, (1, 2, 8, 16)), Canary(dev, x.shape)
    ops.swd_pyramid_level(DevTensor(dev, src.ptr, x.shape), None, nxt.ptr, 16, lap.ptr, 32)
    assert np.array_equal(lap.get(), np.zeros_like(x)) and np.array_equal(nxt.get(), np.full((1, 2, 8, 16), 0.7, np.float32))
    for c in (src, nxt, lap):
        c.free()


# ---- 2. gather ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 3])
def test_gather_is_numpy_slicing_bit_for_bit(dev, ops, C):
    n, H, W, pitch, P, off, extra = 2, 16, 24, 29, 5, 3, 2
    rs = np.random.RandomState(C)
    img = rs.uniform(-1, 1, (n, C, H, W)).astype(np.float32)
    cor = np.array([[(0, 0), (H - 7, W - 7), (0, W - 7), (H - 7, 0), (3, 5)],
                    [(3, 5), (3, 5), (H - 7, W - 7), (1, 0), (0, 1)]], np.int32)         # the four extremes, repeats
    total = off + n * P + extra
    src = Canary(dev, (n, C, H, pitch), pitched(img, pitch))
    tab = Canary(dev, cor.shape, cor, np.int32)
    desc = Canary(dev, (total, 49 * C))
    ops.swd_gather(src.ptr, n, C, H, W, pitch, tab.ptr, P, desc.ptr, off, total)
    got = desc.get()
    assert np.array_equal(got[off:off + n * P], R.gather(img, cor))
    assert np.isnan(got[:off]).all() and np.isnan(got[off + n * P:]).all()             # the other rows are not touched
    assert np.array_equal(tab.get(), cor)
    from gan_heightmaps_amd._lib import GhmError
    with pytest.raises(GhmError):
        ops.swd_gather(src.ptr, n, C, H, W, pitch, tab.ptr, P, desc.ptr, off + extra + 1, total)      # rows past the matrix
    with pytest.raises(GhmError):
        ops.swd_gather(src.ptr, n, 5, H, W, pitch, tab.ptr, P, desc.ptr, 0, total)                    # K beyond the library's
    for c in (src, tab, desc):
        c.free()


# ---- 3. statistics ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,C", [(1000, 3), (1, 1), (70000, 1)])
def test_statistics_against_float64_and_bit_repeatable(dev, ops, N, C):
    rs = np.random.RandomState(N)
    x = (rs.randn(N, C, 49) * np.array([1.0, 0.02, 5.0])[:C, None] + np.array([0.5, -0.1, 30.0])[:C, None]).astype(np.float32)
    desc = Canary(dev, (N, 49 * C), x)
    ws = Canary(dev, (ops.swd_workspace() // 4,))
    runs = []
    for _ in range(2):
        st = Canary(dev, (C, 2))
        ops.swd_stats(desc.ptr, N, C, st.ptr, ws.ptr)
        runs.append(st.get())
        st.free()
    assert np.array_equal(runs[0], runs[1])
    x64 = x.astype(np.float64)
    mean, std = x64.mean(axis=(0, 2)), x64.std(axis=(0, 2))
    rel = max(np.abs(runs[0][:, 0] - mean).max() / np.abs(mean).max(), (np.abs(runs[0][:, 1] - std) / std).max())
    print("stats N=%d C=%d: relative error %.3e" % (N, C, rel))
    assert (np.abs(runs[0][:, 0] - mean) <= 1e-6 * np.abs(mean)).all() and (np.abs(runs[0][:, 1] - std) <= 1e-6 * std).all()
    ws.get()
    desc.free(), ws.free()


def test_a_constant_channel_reports_a_deviation_of_zero(dev, ops):
    x = np.random.RandomState(0).randn(300, 2, 49).astype(np.float32)
    x[:, 1] = 0.3
    desc, ws, st = Canary(dev, (300, 98), x), Canary(dev, (ops.swd_workspace() // 4,)), Canary(dev, (2, 2))
    ops.swd_stats(desc.ptr, 300, 2, st.ptr, ws.ptr)
    got = st.get()
    assert got[1, 1] == 0.0 and got[1, 0] == np.float32(0.3) and got[0, 1] > 0.9
    for c in (desc, ws, st):
        c.free()


# ---- 4. sort ---------------------------------------------------------------------------------------------------------------
def _sort_inputs(N, M, seed):
    rs = np.random.RandomState(seed)
    rnd = rs.randn(M, N).astype(np.float32)
    rnd.ravel()[::7] = FLT_MAX                                   # the padding is +inf, not the largest finite value
    rnd.ravel()[3::11] = -FLT_MAX
    few = rs.choice(np.array([-2.5, -1.0, 0.0, 0.5, 0.5000001, 3.0, FLT_MAX], np.float32), (M, N))
    return {"random": rnd, "sorted": np.sort(rnd, axis=1), "reversed": np.sort(rnd, axis=1)[:, ::-1].copy(),
            "equal": np.full((M, N), 1.25, np.float32), "duplicates": few}


def _sort_case(dev, ops, x, chunk):
    M, N = x.shape
    buf = Canary(dev, (M, N), x)
    ops.swd_sort_columns(buf.ptr, N, M, chunk)
    got = buf.get()
    buf.free()
    want = np.sort(x, axis=1)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (N, M, chunk)


@pytest.mark.parametrize("chunk", [0, 256], ids=["default_chunk", "chunk256"])
@pytest.mark.parametrize("N", [1, 2, 3, 63, 64, 65, 1000, 4096])
def test_sort_columns_is_numpy_sort_bit_for_bit(dev, ops, N, chunk):
    """chunk 256: N = 1000 and N = 4096 run the global form (chunks in LDS, the strides that span them through global memory)"""
    for M in (1, 5):
        for name, x in _sort_inputs(N, M, N + M).items():
            _sort_case(dev, ops, x, chunk)


@pytest.mark.parametrize("N", [1 << 15, (1 << 15) + 1], ids=["2^15_lds_form", "2^15+1_global_form"])
def test_sort_columns_at_the_threshold_between_the_forms(dev, ops, N):
    assert ops.swd_sort_max_chunk() == 1 << 15
    _sort_case(dev, ops, _sort_inputs(N, 2, 9)["random"], 0)


def test_sort_refusals(dev, ops):
    from gan_heightmaps_amd._lib import GhmError
    buf = Canary(dev, (4,), np.arange(4, dtype=np.float32)[::-1])
    for N, M, chunk in ((0, 1, 0), (4, 0, 0), (4, 1, -1), (4, 70000, 0)):
        with pytest.raises(GhmError):
            ops.swd_sort_columns(buf.ptr, N, M, chunk)
    ops.swd_sort_columns(buf.ptr, 4, 1, 3)                       # a chunk that is no power of two is rounded down: the global form
    assert np.array_equal(buf.get(), np.arange(4, dtype=np.float32))
    buf.free()


# ---- 5. projection and distance --------------------------------------------------------------------------------------------
def _device_level(dev, ops, da, db, C, dirs):
    """raw descriptors of both sets and directions [K, M] -> (projections of a [M, N], 1e3 x distance) on the device"""
    N, K = da.shape
    M = dirs.shape[1]
    ws = Canary(dev, (ops.swd_workspace() // 4,))
    dd = Canary(dev, dirs.shape, dirs)
    proj, outs = [], []
    for x in (da, db):
        desc, st, out = Canary(dev, x.shape, x), Canary(dev, (C, 2)), Canary(dev, (M, N))
        ops.swd_stats(desc.ptr, N, C, st.ptr, ws.ptr)
        ops.swd_project(desc.ptr, N, C, dd.ptr, M, st.ptr, out.ptr)
        proj.append(out.get())
        ops.swd_sort_columns(out.ptr, N, M)
        outs.append(out)
        desc.free(), st.free()
    val = 1e3 * ops.swd_l1(outs[0].ptr, outs[1].ptr, M * N, ws.ptr)
    sa, sb = outs[0].get(), outs[1].get()
    assert np.array_equal(sa, np.sort(proj[0], axis=1)) and np.array_equal(sb, np.sort(proj[1], axis=1))
    assert abs(val - 1e3 * np.abs(sa.astype(np.float64) - sb).mean()) <= 1e-9 * max(val, 1.0)      # l1: double partials
    ws.get()
    for c in outs + [ws, dd]:
        c.free()
    return proj, val


def projection_bound(norm, K):
    """(K + 8) 2^-24 max_row |d|_2, and one factor 2 for the normalisation done on the device"""
    return 2 * (K + 8) * U * float(np.sqrt((norm * norm).sum(axis=1)).max())


@pytest.mark.parametrize("C", [1, 3], ids=["K49", "K147"])
def test_projection_and_distance_against_the_restatement(dev, ops, C):
    N, K, M = 192, 49 * C, 8
    rs = np.random.RandomState(K)
    scale, shift = np.array([1.0, 0.05, 4.0])[:C, None], np.array([0.4, -0.2, 9.0])[:C, None]
    da = (rs.randn(N, C, 49) * scale + shift).astype(np.float32).reshape(N, K)
    db = (rs.randn(N, C, 49) ** 3 * scale * 0.5 + shift).astype(np.float32).reshape(N, K)
    dirs = R.directions(3, 1, 0, K, M)
    proj, val = _device_level(dev, ops, da, db, C, dirs)
    worst = 0.0
    bound = 0.0
    for x, p in zip((da, db), proj):
        norm = R.normalise(x, C)
        want = (norm @ dirs.astype(np.float64)).T
        err, b = float(np.abs(p - want).max()), projection_bound(norm, K)
        print("projection K=%d: max error %.3e (bound %.3e)" % (K, err, b))
        assert err <= b
        worst, bound = max(worst, err), max(bound, b)
    want = 1e3 * R.sorted_l1(R.normalise(da, C) @ dirs.astype(np.float64), R.normalise(db, C) @ dirs.astype(np.float64))
    print("distance K=%d: device %.6f, f64 %.6f, |difference| / 1e3 = %.3e (bound %.3e)"
          % (K, val, want, abs(val - want) / 1e3, 2 * bound))
    assert abs(val - want) / 1e3 <= 2 * bound                    # sorting is 1-Lipschitz in the sup norm
    assert want > 50.0                                           # and the two sets do differ


# ---- 6. the whole metric on SMALL ------------------------------------------------------------------------------------------
CFG = ostep.default_cfg(**SMALL)
METRIC = SW.SWD(patches_per_image=16, directions=16, repeats=2, seed=3)
N_IMG = 8


class It:
    """a host-array iterator with the reference's surface (.N, next()); ``drawn`` counts its batches"""

    def __init__(self, base=100, N=8):
        self.N, self.base, self.drawn = N, base, 0

    def __next__(self):
        _, X, Y = ostep.synthetic_batch(4, CFG, seed=self.base + self.drawn)
        self.drawn += 1
        return X, Y
    next = __next__


@pytest.fixture(scope="module", params=["f32", "bf16x3"])
def small_model(request, dev):
    m = build_model(CFG, 5, dev, dtype=request.param, use_graph=False)
    for s in range(3):                       # non-trivial BatchNorm running statistics (the deterministic pass reads them)
        m.z_fn(ostep.synthetic_batch(4, CFG, seed=40 + s)[0])
    return m


def _level_bounds(xa, xb):
    """per level 1e3 x 2 x the projection bound of the restatement's normalised descriptors of both sets"""
    C = xa.shape[1]
    out = []
    for i, (da, db) in enumerate(zip(R.descriptors(xa, 0, None, METRIC.patches_per_image, METRIC.seed),
                                     R.descriptors(xb, 1, None, METRIC.patches_per_image, METRIC.seed))):
        out.append(1e3 * 2 * max(projection_bound(R.normalise(d, C, i), 49 * C) for d in (da, db)))
    return out


def test_pix2pix_swd_is_the_restatement_of_the_deterministic_forwards(small_model):
    m = small_model
    it = It()
    state = np.random.get_state()[1].copy()
    res = m.swd(it, num_images=N_IMG, batch_size=4, metric=METRIC, seed=11)
    assert it.drawn == 2 and np.array_equal(np.random.get_state()[1], state)       # two batches, and no global draw
    assert sorted(res) == ["dcgan", "p2p"] and res["dcgan"]["levels"] == res["p2p"]["levels"] == [32, 16]
    ref_it = It()
    batches = [next(ref_it) for _ in range(2)]
    A, B = np.concatenate([b[0] for b in batches]), np.concatenate([b[1] for b in batches])
    z = np.random.RandomState(11).rand(N_IMG, SMALL["latent_dim"]).astype(np.float32)
    fake_a = np.concatenate([m.z_fn_det(z[i:i + 4]) for i in (0, 4)])
    fake_b = np.concatenate([m.gen_fn_det(A[i:i + 4]) for i in (0, 4)])
    kw = dict(patches_per_image=16, directions_=16, repeats=2, seed=3)
    for net, real, fake in (("dcgan", A, fake_a), ("p2p", B, fake_b)):
        want, bounds = R.swd(real, fake, **kw), _level_bounds(real, fake)
        for lv, got, w, b in zip(want["levels"], res[net]["swd"], want["swd"], bounds):
            print("%s %s level %d: device %.6f, f64 %.6f, |difference| %.3e (bound %.3e)"
                  % (m.engine.dtype, net, lv, got, w, abs(got - w), b))
            assert abs(got - w) <= b
        assert abs(res[net]["mean"] - want["mean"]) <= max(bounds)
    # again: the same bits; one net alone: the same bits
    again = m.swd(It(), num_images=N_IMG, batch_size=4, metric=METRIC, seed=11)
    assert again == res
    assert m.swd(It(), num_images=N_IMG, batch_size=4, which="dcgan", metric=METRIC, seed=11) == {"dcgan": res["dcgan"]}
    assert m.swd(It(), num_images=N_IMG, batch_size=4, metric=METRIC, seed=12)["dcgan"] != res["dcgan"]
    assert m.swd(It(), num_images=N_IMG, batch_size=4, which="dcgan", metric=METRIC, z=z) == {"dcgan": res["dcgan"]}


def test_sets_fed_in_batches_of_one_and_of_four_are_the_same_bits(dev, ops):
    rs = np.random.RandomState(1)
    xa, xb = rs.uniform(-1, 1, (N_IMG, 3, 32, 64)).astype(np.float32), rs.randn(N_IMG, 3, 32, 64).astype(np.float32)
    made = []
    for bs in (1, 4):
        a, b = SW.Descriptors(ops, METRIC, 0, N_IMG, 3, 32, 64, max_batch=3), SW.Descriptors(ops, METRIC, 1, N_IMG, 3, 32, 64)
        for i in range(0, N_IMG, bs):
            a.add(xa[i:i + bs])
            t = dev.tensor(xb[i:i + bs])                          # a DevTensor is read where it lies
            b.add(t)
            dev.sync()
            dev.free(t.ptr)
        made.append((a, b, [a.numpy(i) for i in range(a.L)], SW.distance(ops, a, b)))
    (a1, b1, m1, d1), (a4, b4, m4, d4) = made
    assert a1.L == 2 and all(np.array_equal(u, v) for u, v in zip(m1, m4)) and d1 == d4
    want = R.descriptors(xa, 0, None, 16, 3)
    assert all(np.abs(u - v).max() <= 64 * U for u, v in zip(m1, want))
    # the same set on both sides is at distance exactly 0; the chunked sort gives the same bits as the default one
    same = SW.distance(ops, a1, a1)
    assert same["swd"] == [0.0, 0.0] and same["mean"] == 0.0
    assert SW.distance(ops, a1, b1, sort_chunk=64) == d1
    with pytest.raises(ValueError, match="over max_mb"):
        SW.distance(ops, a1, b1, max_mb=0.001)
    for d in (a1, b1, a4, b4):
        d.close()
    with pytest.raises(ValueError, match="open Descriptors"):
        SW.distance(ops, a1, b1)


def test_compare_and_the_command_line_score_two_image_sets(dev, ops, tmp_path, capsys):
    real = R.power_law_images(10, N_IMG, 64).astype(np.float32)
    fake = R.up(R.down(R.power_law_images(12, N_IMG, 64))).astype(np.float32)
    got = SW.compare(ops, real, fake, METRIC, batch_size=3)
    want = R.swd(real, fake, patches_per_image=16, directions_=16, repeats=2, seed=3)
    assert got["levels"] == want["levels"] == [64, 32, 16]
    for g, w, b in zip(got["swd"], want["swd"], _level_bounds(real, fake)):
        assert abs(g - w) <= b
    np.save(tmp_path / "real.npy", real)
    np.save(tmp_path / "fake.npy", fake[:, 0])                   # [n, H, W] reads as one channel
    assert SW.main(["--real", str(tmp_path / "real.npy"), "--fake", str(tmp_path / "fake.npy"), "--seed", "3", "--patches", "16",
                    "--directions", "16", "--repeats", "2"]) == 0
    line = capsys.readouterr().out.strip().split("\n")[-1]
    assert line.startswith("swd") and ("64: %.4f" % got["swd"][0]) in line and ("mean %.4f" % got["mean"]) in line


def test_the_command_line_scores_a_checkpoint(tmp_path, capsys, monkeypatch):
    from gan_heightmaps_amd import experiments as EX
    made = []

    def make_model(name, **kw):
        made.append(build_model(CFG, 9 if made else 5, None, use_graph=False, **{k: v for k, v in kw.items() if k == "dtype"}))
        return made[-1]
    first = make_model("SMALL", dtype="f32")
    first.save_model(str(tmp_path / "3.model"))
    it = EX.get_iterators("synthetic", 4, True, False, False, in_shp=32, device=first.device)[1]
    want = first.swd(it, num_images=N_IMG, batch_size=4, metric=METRIC, seed=3)
    monkeypatch.setattr(EX, "make_model", make_model)
    monkeypatch.setattr(EX, "DATASET", "synthetic")
    args = [str(tmp_path / "3.model"), "--images", str(N_IMG), "--seed", "3", "--dtype", "f32", "--patches", "16", "--directions",
            "16", "--repeats", "2"]
    assert SW.main(["SMALL"] + args) == 0                        # a model of other weights (seed 9) that loads the checkpoint
    lines = capsys.readouterr().out.strip().split("\n")[-2:]
    for line, net in zip(lines, ("dcgan", "p2p")):
        assert line.startswith(net) and ("mean %.4f" % want[net]["mean"]) in line, (line, want[net])
    first.device.close()


def test_zero_variance_is_refused_with_level_and_channel(dev, ops):
    x = np.random.RandomState(2).uniform(0, 1, (2, 2, 32, 32)).astype(np.float32)
    x[:, 1] = 0.25                                               # a constant channel: Lap_0 is exactly 0 there
    with SW.Descriptors(ops, METRIC, 0, 2, 2, 32, 32) as a:
        a.add(x)
        with pytest.raises(ValueError, match="level 0, channel 1"):
            SW.distance(ops, a, a)


def _payload(m):
    buf = io.BytesIO()
    m.save_model(buf)
    return gzip.decompress(buf.getvalue())


def test_swd_moves_no_training_state(dev):
    runs = []
    for with_swd in (False, True):
        m = build_model(CFG, 7, dev)
        m.sampler = np.random.RandomState(5).rand
        m.train_fn(*ostep.synthetic_batch(4, CFG, seed=1))
        if with_swd:
            m.swd(It(), num_images=N_IMG, batch_size=4, metric=METRIC)
        runs.append((_payload(m), m.train_fn(*ostep.synthetic_batch(4, CFG, seed=2)), _payload(m)))
    assert runs[0][0] == runs[1][0] and runs[0][2] == runs[1][2]
    assert all(np.array_equal(np.asarray(u), np.asarray(v)) for u, v in zip(runs[0][1], runs[1][1]))


def test_swd_inside_ema_weights_scores_the_average(dev):
    m = build_model(CFG, 7, dev, ema=0.5)
    for s in range(3):
        m.train_fn(*ostep.synthetic_batch(4, CFG, seed=60 + s))
    live = m.swd(It(), num_images=N_IMG, batch_size=4, metric=METRIC)
    with m.ema_weights():
        avg = m.swd(It(), num_images=N_IMG, batch_size=4, metric=METRIC)
    assert avg["dcgan"]["swd"] != live["dcgan"]["swd"] and avg["p2p"]["swd"] != live["p2p"]["swd"]
    assert m.swd(It(), num_images=N_IMG, batch_size=4, metric=METRIC) == live        # and the live weights are back


def test_train_with_swd_every_leaves_the_run_as_it_is_and_writes_swd_txt(dev, tmp_path):
    runs = []
    for swd_every in (None, 1):
        m = build_model(CFG, 3, dev, ema=0.9)
        m.sampler = np.random.RandomState(5).rand
        out = str(tmp_path / ("out_%s" % swd_every))
        own = It(base=500)
        kw = {} if swd_every is None else dict(swd_every=1, swd_iterator=own, swd_images=N_IMG)
        m.train(It(), It(base=300), batch_size=4, num_epochs=2, out_dir=out, dump_images=False, **kw)
        rows = [l.split(",") for l in open(out + "/results.txt").read().strip().split("\n")]
        runs.append(([r[:-2] + r[-1:] for r in rows], model_params(m), out, own.drawn))          # (without the time column)
    (rows0, p0, out0, _), (rows1, p1, out1, drawn) = runs
    assert rows0 == rows1 and len(rows0) == 3
    assert all(np.array_equal(u, v) for k in p0 for u, v in zip(p0[k], p1[k]))
    assert drawn == 2                                            # the real sets are computed once
    import os
    assert not os.path.exists(out0 + "/swd.txt")
    lines = [l.split(",") for l in open(out1 + "/swd.txt").read().strip().split("\n")]
    assert lines[0] == ["epoch", "weights", "net", "swd_32", "swd_16", "mean"]
    assert [l[:3] for l in lines[1:]] == [[str(e), w, net] for e in (1, 2) for w in ("live", "ema") for net in ("dcgan", "p2p")]
    vals = np.array([[float(v) for v in l[3:]] for l in lines[1:]])
    assert np.isfinite(vals).all() and (vals > 0).all() and np.allclose(vals[:, :2].mean(axis=1), vals[:, 2], rtol=1e-12)
    assert not np.array_equal(vals[0], vals[4])                  # the generators moved between the epochs
