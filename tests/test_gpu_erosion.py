"""Erosion on the MI355X (csrc/erosion.hip, gan_heightmaps_amd/erosion.py): the plain form against the float64
restatement (tests/erosion_ref.py), the fused form against the plain one bit for bit, ghm_erosion_emit, window independence
on the device, the eroded TerrainWorld against erode_heightmap and itself, the refusals and the command line."""
import numpy as np
import pytest

from oracle import step as ostep
from gan_heightmaps_amd import erosion as ER
from gan_heightmaps_amd import util
from gan_heightmaps_amd._lib import GhmError
from tests import erosion_ref as R
from tests import world_ref as WR
from tests.test_erosion_ref import CASES, F32_DEV, TILE, WIN
from tests.gpu_common import build_model, dev, ERO, N_WORLD, ops, SMALL      # noqa: F401  (dev, ops: the module-scoped fixtures)

pytestmark = pytest.mark.gpu

P = R.P_TEST
TOL = 8 * F32_DEV               # the renderer's convention: the margin covers the device's own divide and sqrt order
NP = ER.PLANES


def _params(p=P):
    from gan_heightmaps_amd.device import erosion_params
    return erosion_params(**p)


def run_device(dev, ops, hm, n, fused, pitch=None, p=P):
    """hm float32 [H, W] -> the seven planes after n iterations, {name: [H, W]}.  With a pitch beyond W every cell of every
    buffer is NaN at the start and the cells beyond W are checked to be NaN still."""
    H, W = hm.shape
    pitch = W if pitch is None else pitch
    bufs = [dev.alloc(4 * H * W)] + [dev.alloc(4 * k * H * pitch) for k in (NP, NP, 3)]
    src, s0, s1, tmp = bufs
    try:
        dev.h2d(src, np.ascontiguousarray(hm, np.float32))
        for ptr, k in ((s0, NP), (s1, NP), (tmp, 3)):
            dev.h2d(ptr, np.full((k, H, pitch), np.nan, np.float32))
        ops.erosion_init(src, H, W, W, p["height_scale"], s0, pitch)
        fin = ops.erosion_iterate(_params(p), s0, s1, None if fused else tmp, H, W, pitch, n, fused)
        assert fin == (s0 if n % 2 == 0 else s1)
        dev.sync()
        out = np.empty((NP, H, pitch), np.float32)
        dev.d2h(out, fin, out.nbytes)
        other = np.empty((NP, H, pitch), np.float32)
        dev.d2h(other, s1 if fin == s0 else s0, other.nbytes)
        assert np.isnan(out[:, :, W:]).all() and np.isnan(other[:, :, W:]).all()
    finally:
        for ptr in bufs:
            dev.free(ptr)
    return {k: out[i, :, :W] for i, k in enumerate(R.FIELDS)}


_plain, _ref = {}, {}


def plain_of(dev, ops, case):
    if case not in _plain:
        H, W, n, seed = case
        _plain[case] = run_device(dev, ops, R.terrain(seed, H, W).astype(np.float32), n, fused=False)
    return _plain[case]


def ref_of(case):
    if case not in _ref:
        H, W, n, seed = case
        _ref[case] = R.erode_state(R.terrain(seed, H, W).astype(np.float32), P, n, np.float64)
    return _ref[case]


def test_the_library_tile_is_the_one_the_cases_were_sized_for(ops):
    assert ops.erosion_tile() == TILE


# ---- 1. the plain form against the float64 restatement -----------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d_n%d" % c[:3])
def test_plain_form_against_the_float64_restatement(dev, ops, case):
    got, want = plain_of(dev, ops, case), ref_of(case)
    worst = {k: float(np.abs(got[k].astype(np.float64) - want[k]).max()) for k in ("b", "d", "s")}
    print("%3d x %3d, %2d iterations: max |device - f64|: b %.3e, d %.3e, s %.3e (TOL %.2e)"
          % (case[:3] + (worst["b"], worst["d"], worst["s"], TOL)))
    for k in ("b", "d", "s"):
        assert np.isfinite(got[k]).all() and worst[k] <= TOL, (k, worst[k])
    if case[0] > 1:                                                # not idle: the ground moved, water stands, silt is in flight
        b0 = R.terrain(case[3], *case[:2]).astype(np.float32) * np.float32(P["height_scale"])
        assert np.abs(got["b"] - b0).max() > 1e-4 and got["d"].max() > 0 and got["s"].max() > 0


# ---- 2. fused against plain, bit for bit -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d_n%d" % c[:3])
def test_fused_form_equals_the_plain_form_bit_for_bit(dev, ops, case):
    H, W, n, seed = case
    plain = plain_of(dev, ops, case)
    fused = run_device(dev, ops, R.terrain(seed, H, W).astype(np.float32), n, fused=True)
    for k in R.FIELDS:
        assert np.array_equal(fused[k], plain[k]), (k, np.abs(fused[k] - plain[k]).max())


@pytest.mark.parametrize("fused", [False, True])
def test_a_row_pitch_beyond_the_width_is_honoured_and_left_alone(dev, ops, fused):
    H, W, n, seed = 37, 70, 5, 9                    # two tiles wide, three high; pitch 83 is no multiple of anything
    hm = R.terrain(seed, H, W).astype(np.float32)
    tight = run_device(dev, ops, hm, n, fused=False)
    wide = run_device(dev, ops, hm, n, fused=fused, pitch=83)          # run_device checks the cells beyond W
    for k in R.FIELDS:
        assert np.array_equal(wide[k], tight[k]), k


# ---- 3. emit -------------------------------------------------------------------------------------------------------------
def test_emit_clamps_maps_to_uint8_and_writes_sub_rectangles(dev, ops):
    rng = np.random.RandomState(3)
    H, W, pitch, hs = 13, 21, 24, 24.0
    b = (rng.uniform(-0.2, 1.2, (H, pitch)) * hs).astype(np.float32)
    b.ravel()[::5] = ((rng.randint(0, 256, b.ravel()[::5].size) + 0.5) / 255 * hs).astype(np.float32)   # near halfway
    b[0, :4] = [-3.0, 0.0, hs, 2 * hs]
    state = dev.alloc(4 * NP * H * pitch)
    dev.h2d(state, np.concatenate([b[None], np.full((NP - 1, H, pitch), np.nan, np.float32)]))
    want = np.clip(b[:, :W] / np.float32(hs), 0, 1)
    assert want.min() == 0 and want.max() == 1
    for r0, c0, nr, nc, rows, dp, yo, xo in ((0, 0, H, W, H, W, 0, 0), (2, 3, 7, 9, 11, 30, 4, 13), (H - 1, W - 1, 1, 1, 1, 1, 0, 0),
                                             (0, 5, H, 4, H + 2, 8, 1, 2)):
        for u8 in (False, True):
            dt = np.uint8 if u8 else np.float32
            out = dev.alloc(rows * dp * 4)
            fill = np.full((rows, dp), 7, dt)
            dev.h2d(out, fill)
            ops.erosion_emit(state, H, W, pitch, hs, r0, c0, nr, nc, u8, out, rows, dp, yo, xo)
            got = np.empty((rows, dp), dt)
            dev.d2h(got, out, got.nbytes)
            dev.free(out)
            sub = want[r0:r0 + nr, c0:c0 + nc]
            if u8:
                exact = sub.astype(np.float64) * 255
                assert np.abs(got[yo:yo + nr, xo:xo + nc].astype(np.float64) - exact).max() <= 1.0      # within one level
                assert np.array_equal(got[yo:yo + nr, xo:xo + nc], np.rint(exact).astype(np.uint8))   # ghm_world_crop's map
            else:
                assert np.array_equal(got[yo:yo + nr, xo:xo + nc], sub)
            got[yo:yo + nr, xo:xo + nc] = 7
            assert np.array_equal(got, fill)                                  # nothing outside the rectangle
    for bad in ((0, 0, H + 1, W, H + 1, W, 0, 0), (0, 0, H, W, H, W, 1, 0), (0, 0, H, W, H, W - 1, 0, 0), (-1, 0, 2, 2, H, W, 0, 0)):
        with pytest.raises(GhmError):
            ops.erosion_emit(state, H, W, pitch, hs, *bad[:4], False, state, *bad[4:])
    dev.free(state)


# ---- 4. window independence on the device -----------------------------------------------------------------------------
def test_a_window_with_its_halo_equals_the_larger_map_on_the_device(dev, ops):
    (Hb, Wb), (y0, x0, h, w), n = WIN["shape"], WIN["rect"], WIN["n"]
    E = ER.RADIUS * n
    big = R.terrain(1, Hb, Wb).astype(np.float32)
    full = run_device(dev, ops, big, n, fused=True)
    win = run_device(dev, ops, big[y0 - E:y0 + h + E, x0 - E:x0 + w + E], n, fused=True)
    for k in R.FIELDS:
        assert np.array_equal(full[k][y0:y0 + h, x0:x0 + w], win[k][E:E + h, E:E + w]), k
    # the public entry: erode() of the window, cropped, is erode() of the map, cropped
    a = ER.erode(ops, big, ER.Erosion(iterations=n, **P))
    b, depth = ER.erode(ops, big[None, y0 - E:y0 + h + E, x0 - E:x0 + w + E], ER.Erosion(iterations=n, **P), fused=False,
                        water=True)
    assert a.shape == (Hb, Wb) and b.shape == depth.shape == (1, h + 2 * E, w + 2 * E)
    assert np.array_equal(a[y0:y0 + h, x0:x0 + w], b[0, E:E + h, E:E + w])
    assert np.array_equal(a, np.clip(full["b"] / np.float32(P["height_scale"]), 0, 1))
    assert np.array_equal(depth[0], win["d"]) and depth.max() > 0


# ---- 5. the eroded world on SMALL ---------------------------------------------------------------------------------------
REQ = (-70, 33, 150, 97)                     # 4 x 3 chunks of 64 pixels, both signs


@pytest.fixture(scope="module", params=["f32", "bf16x3"])
def small_model(request, dev):
    m = build_model(ostep.default_cfg(**SMALL), 5, dev, dtype=request.param, use_graph=False)
    cfg = ostep.default_cfg(**SMALL)
    for s in range(3):                       # non-trivial BatchNorm running statistics (the deterministic pass reads them)
        m.z_fn(ostep.synthetic_batch(4, cfg, seed=40 + s)[0])
    return m


def test_eroded_world_equals_erode_heightmap_of_the_grown_raw_rectangle(small_model):
    m, E = small_model, ERO.halo
    y0, x0, h, w = REQ
    with m.terrain_world(42, chunk_cells=2) as raw, m.terrain_world(42, chunk_cells=2, erosion=ERO) as world:
        assert world.erosion is ERO and raw.erosion is None and E == 9
        grown = raw.heightmap(y0 - E, x0 - E, h + 2 * E, w + 2 * E)
        assert raw.eroded == 0
        want = m.erode_heightmap(grown, ERO)[:, E:E + h, E:E + w]
        got = world.heightmap(*REQ)
        assert got.shape == (1, h, w) and got.dtype == np.float32
        assert np.array_equal(got, want), np.abs(got - want).max()
        assert np.array_equal(m.erode_heightmap(grown, ERO, fused=not ER.DEFAULT_FUSED)[:, E:E + h, E:E + w], want)
        with m.terrain_world(42, chunk_cells=2, erosion=ERO) as other:           # the world on the other form of the kernels
            other._fused = not other._fused
            assert np.array_equal(other.heightmap(*REQ), got)
        d = np.abs(got - grown[:, E:E + h, E:E + w]).max()
        print("world %s: max |eroded - raw| = %.3g" % (m.engine.dtype, d))
        assert d > 0                                               # the erosion is not idle on this terrain
        # erosion=None is today's world
        assert np.array_equal(raw.heightmap(*REQ), grown[:, E:E + h, E:E + w]) and raw.eroded == 0
        u8 = world.heightmap(*REQ, uint8=True)
        assert np.array_equal(u8, util.to_uint8(util.convert_to_rgb(got, is_grayscale=True))[:, :, 0])


def test_eroded_requests_are_independent_bit_for_bit(small_model):
    m = small_model
    y0, x0, h, w = -41, 17, 90, 75
    with m.terrain_world(42, chunk_cells=2, erosion=ERO, overlap=8, batch_size=3) as world:
        a = world.heightmap(*REQ)
        n, e = world.computed, world.eroded
        assert e == 12 and n == 6 * 5                              # 4 x 3 eroded chunks from the 6 x 5 raw ones around them
        assert np.array_equal(world.heightmap(*REQ), a) and (world.computed, world.eroded) == (n, e)     # warm: nothing runs
        b = world.heightmap(-10, 60, 100, 120)
        assert np.array_equal(b[:, :90, :70], a[:, 60:150, 27:97])
        hm, tex = world.heightmap(y0, x0, h, w), world.texture(y0, x0, h, w)
        bh, bt = world.both(y0, x0, h, w)
        assert np.array_equal(bh, hm) and np.array_equal(bt, tex)
        t2 = world.texture(y0 + 30, x0 - 20, 64, 70)
        assert np.array_equal(t2[:, :60, 20:], tex[:, 30:, :50])
        # the texture is texture_heightmap's of the eroded map (§4l's statement of it)
        ey, ex, eh, ew = WR.tile_aligned_expansion(y0, x0, h, w, 32, 8)
        whole = m.texture_heightmap(world.heightmap(ey, ex, eh, ew), overlap=8, batch_size=3)
        d = np.abs(tex - whole[:, y0 - ey:y0 - ey + h, x0 - ex:x0 - ex + w]).max()
        print("eroded world %s: max |texture - texture_heightmap crop| = %.3g" % (m.engine.dtype, d))
        assert d <= 1e-6
    with m.terrain_world(42, chunk_cells=2, erosion=ERO, overlap=8, batch_size=3, cache_mb=0) as cold:
        assert np.array_equal(cold.heightmap(*REQ), a)
        assert np.array_equal(cold.heightmap(-10, 60, 100, 120), b)
        ch, ct = cold.both(y0, x0, h, w)
        assert np.array_equal(ch, hm) and np.array_equal(ct, tex)
        assert np.array_equal(cold.texture(y0, x0, h, w), tex)
        assert not cold._chunks and not cold._raw and not cold._heads and not cold._cache.order
    with m.terrain_world(42, chunk_cells=2, erosion=ERO, cache_mb=0.2) as tiny:        # twelve chunks of 16 KB: evictions
        assert np.array_equal(tiny.heightmap(*REQ), a) and len(tiny._chunks) + len(tiny._raw) <= 12
        assert np.array_equal(tiny.heightmap(-10, 60, 100, 120), b)
    with m.terrain_world(42, chunk_cells=2, erosion=ERO, overlap=8, batch_size=3) as fresh:
        assert np.array_equal(fresh.texture(y0, x0, h, w), tex)
        assert np.array_equal(fresh.heightmap(*REQ), a)
    with m.terrain_world(42, chunk_cells=2, erosion=ER.Erosion(iterations=N_WORLD + 1, **P)) as other:
        assert not np.array_equal(other.heightmap(*REQ), a)        # the parameters are part of the world's identity


def test_eroded_counters_for_a_request_that_touches_four_chunks(small_model):
    with small_model.terrain_world(7, chunk_cells=2, erosion=ERO) as world:
        world.heightmap(60, -68, 8, 8)                             # the corner of chunks (0, -2) (0, -1) (1, -2) (1, -1)
        assert (world.eroded, world.computed) == (4, 16) and len(world._chunks) == 4 and len(world._raw) == 16
        world.heightmap(0, -128, 128, 128)                         # the same four chunks, whole
        assert (world.eroded, world.computed) == (4, 16)
    with small_model.terrain_world(7, chunk_cells=2) as raw:
        raw.heightmap(60, -68, 8, 8)
        assert (raw.eroded, raw.computed) == (0, 4) and not raw._raw
        assert set(raw._cache.order) == {('e', k) for k in raw._chunks}        # nor a raw entry in the one LRU order


def test_eroded_resident_scene_equals_the_host_scene(small_model):
    rect = (-37, 19, 101, 75)
    with small_model.terrain_world(42, chunk_cells=2, erosion=ERO) as world:
        with world.scene(*rect) as host, world.scene(*rect, resident=True) as res:
            (hh, ht), (rh, rt) = host.arrays(), res.arrays()
        assert np.array_equal(rh, hh) and np.array_equal(rt, ht)
        assert np.array_equal(hh, world.heightmap(*rect)[0])       # a greyscale map in [0, 1] is its own scene plane


def test_a_training_step_drops_both_layers(dev):
    cfg = ostep.default_cfg(**SMALL)
    m = build_model(cfg, 7, dev)
    req = (-20, 10, 70, 50)
    with m.terrain_world(3, chunk_cells=2, erosion=ERO) as world:
        m.train_fn(*ostep.synthetic_batch(4, cfg, seed=1))
        a = world.heightmap(*req)
        n, e = world.computed, world.eroded
        assert world._chunks and world._raw
        assert np.array_equal(world.heightmap(*req), a) and (world.computed, world.eroded) == (n, e)
        m.train_fn(*ostep.synthetic_batch(4, cfg, seed=2))
        b = world.heightmap(*req)
        assert world.computed == 2 * n and world.eroded == 2 * e and not np.array_equal(a, b)
        with m.terrain_world(3, chunk_cells=2, erosion=ERO) as fresh:
            assert np.array_equal(fresh.heightmap(*req), b)


# ---- 6. refusals and the command line ------------------------------------------------------------------------------------
def test_refusals_on_the_device(dev, ops, small_model):
    m = small_model
    hm = np.full((8, 8), 0.5, np.float32)
    with pytest.raises(ValueError, match="one height"):
        m.erode_heightmap(np.zeros((3, 8, 8), np.float32))
    with pytest.raises(ValueError, match="one height"):
        ER.erode(ops, np.zeros((8, 8, 3), np.uint8))
    with pytest.raises(ValueError):
        ER.erode(ops, hm, erosion="fast")
    with pytest.raises(ValueError, match="out must be"):
        ER.erode(ops, hm, out=np.zeros((8, 8), np.float64))
    with pytest.raises(ValueError, match="non-finite"):
        ER.erode(ops, np.full((4, 4), np.nan, np.float32))
    with pytest.raises(ValueError, match="more than a chunk"):
        m.terrain_world(1, chunk_cells=1, erosion=ER.Erosion(iterations=11))       # E = 33 > K = 32
    assert m.terrain_world(1, chunk_cells=1, erosion=ER.Erosion(iterations=10)).erosion.halo == 30
    # the entry points refuse what the host object refuses, and bad shapes
    st = dev.alloc(4 * NP * 64 * 2)
    for bad in (dict(P, min_depth=0.0), dict(P, max_speed=40.0), dict(P, dt=0.0), dict(P, rain=-1.0),
                dict(P, gravity=float("nan")), dict(P, height_scale=0.0)):
        with pytest.raises(GhmError):
            ops.erosion_iterate(_params(bad), st, st + 4 * NP * 64, None, 8, 8, 8, 1, True)
    with pytest.raises(GhmError):
        ops.erosion_iterate(_params(), st, st, None, 8, 8, 8, 1, True)             # one state twice
    with pytest.raises(GhmError):
        ops.erosion_iterate(_params(), st, st + 4 * NP * 64, None, 8, 8, 8, 1, False)      # the plain form without workspace
    with pytest.raises(GhmError):
        ops.erosion_iterate(_params(), st, st + 4 * NP * 64, None, 8, 9, 8, 1, True)       # pitch < W
    with pytest.raises(GhmError):
        ops.erosion_init(st, 0, 8, 8, 24.0, st, 8)
    dev.free(st)
    # a uint8 input is its float map / 255; uint8 output is the float output's rint(255 v)
    u = (R.terrain(4, 20, 24) * 255).astype(np.uint8)
    ero = ER.Erosion(iterations=2, **P)
    f = ER.erode(ops, u, ero)
    assert np.array_equal(f, ER.erode(ops, u.astype(np.float32) / np.float32(255), ero))
    assert np.array_equal(ER.erode(ops, u, ero, uint8=True), np.rint(f.astype(np.float64) * 255).astype(np.uint8))


def test_cli_round_trip(dev, ops, tmp_path):
    hm = R.terrain(21, 40, 40).astype(np.float32)
    np.save(tmp_path / "in.npy", hm)
    args = [str(tmp_path / "in.npy"), str(tmp_path / "out.npy"), "--iterations", "5", "--water", str(tmp_path / "w.npy")]
    for k, v in P.items():
        args += ["--" + k.replace("_", "-"), repr(v)]
    assert ER.main(args) == 0
    want, depth = ER.erode(ops, hm, ER.Erosion(iterations=5, **P), water=True)
    assert np.array_equal(np.load(tmp_path / "out.npy"), want) and np.array_equal(np.load(tmp_path / "w.npy"), depth)
    for form in ("--plain", "--fused"):
        assert ER.main(args[:2] + [form] + args[2:]) == 0
        assert np.array_equal(np.load(tmp_path / "out.npy"), want)
    ref = R.erode(hm, P, 5, np.float64)
    assert np.abs(want - ref).max() <= TOL / P["height_scale"]
    from PIL import Image
    Image.fromarray((hm * 255).astype(np.uint8)).save(tmp_path / "in.png")
    assert ER.main([str(tmp_path / "in.png"), str(tmp_path / "out.png"), "--iterations", "2"]) == 0
    got = np.asarray(Image.open(tmp_path / "out.png"))
    assert got.shape == (40, 40) and got.dtype == np.uint8
    assert np.array_equal(got, ER.erode(ops, (hm * 255).astype(np.uint8), ER.Erosion(iterations=2), uint8=True))
