"""Resident scenes and flights on the MI355X: the two scene sinks (ghm_world_scene_height,
ghm_texture_finalize_scene) against render.Scene's host mapping bit for bit, TerrainWorld.scene(resident=True) against the
host-path scene -- planes and pictures --, TerrainWorld.flight against its contract, the refusals and the command line."""
import numpy as np
import pytest

from oracle import step as ostep
from gan_heightmaps_amd import render as RN
from gan_heightmaps_amd import world as WD
from gan_heightmaps_amd._lib import GhmError
from tests.gpu_common import build_model, dev, ops, SMALL      # noqa: F401  (dev, ops: the module-scoped fixtures)

pytestmark = pytest.mark.gpu

# (-37, 19, 101, 75): chunk boundaries on both axes at negative coordinates, a width that is no multiple of 4;
# (3, 5, 20, 17): inside one chunk and smaller than a tile; (64, -64, 64, 64): exactly one chunk (the 16-byte forms);
# (63, 63, 2, 2): the minimum scene, on four chunks; (-1, -1, 33, 130): many tile columns, two forward batches of 4
RECTS = [(-37, 19, 101, 75), (3, 5, 20, 17), (64, -64, 64, 64), (63, 63, 2, 2), (-1, -1, 33, 130)]
MAX_DIST, HS = 40.0, 10.0
RKW = dict(sun_elevation=0.6, haze=0.003)


def _model(dev, **over):
    cfg = ostep.default_cfg(**dict(SMALL, **over))
    m = build_model(cfg, 5, dev, dtype='f32', use_graph=False)
    for s in range(3):                       # non-trivial BatchNorm running statistics
        m.z_fn(ostep.synthetic_batch(4, cfg, seed=40 + s)[0])
    return m


@pytest.fixture(scope="module")
def model(dev):
    return _model(dev)


def _same_planes(world, rect):
    with world.scene(*rect) as host, world.scene(*rect, resident=True) as res:
        assert res.shape == host.shape == rect[2:] and res.origin == host.origin == rect[:2]
        (hh, ht), (rh, rt) = host.arrays(), res.arrays()
    assert hh.shape == rect[2:] and ht.shape == (3,) + rect[2:] and hh.dtype == ht.dtype == np.float32
    assert np.array_equal(rh, hh), (rect, np.abs(rh - hh).max())
    assert np.array_equal(rt, ht), (rect, np.abs(rt - ht).max())
    return hh, ht


# ---- 1. planes, bit for bit -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("overlap", [0, None])
def test_resident_planes_equal_the_host_path(dev, model, overlap):
    with model.terrain_world(42, chunk_cells=2, overlap=overlap) as warm:
        warm.both(*RECTS[1])                                 # the engine keeps the forward plans this builds
    before = dev.bytes_allocated
    with model.terrain_world(42, chunk_cells=2, overlap=overlap) as world:
        assert world.chunk_px == 64 and world.batch_size == 4
        for rect in RECTS:
            hm, tex = _same_planes(world, rect)
            assert hm.min() >= 0.0 and hm.max() <= 1.0 and tex.min() >= 0.0 and tex.max() <= 1.0
            assert hm.std() > 0 and tex.std() > 0
        # arrays() is what the host path uploads: Scene's own mapping of both()
        a, b = world.both(*RECTS[0])
        want_h = RN._unit_planes(a, True, "heightmap")[0]
        want_t = RN._unit_planes(b, False, "texture")
        hm, tex = _same_planes(world, RECTS[0])
        assert hm.shape == (101, 75) and np.array_equal(hm, want_h) and np.array_equal(tex, want_t)
    assert dev.bytes_allocated == before                     # scenes and transients are all returned


# ---- 2. value ranges ------------------------------------------------------------------------------------------------
def test_unit_range_texture(dev):
    m = _model(dev, is_b_grayscale=True)                     # a one-channel texture in [0, 1]: replicated, not remapped
    with m.terrain_world(42, chunk_cells=2) as world:
        hm, tex = _same_planes(world, RECTS[0])
        assert np.array_equal(tex[0], tex[1]) and np.array_equal(tex[0], tex[2])
        assert np.array_equal(tex[:1], np.clip(world.texture(*RECTS[0]), 0, 1))


def test_three_channel_tanh_range_heightmap(dev):
    m = _model(dev, is_a_grayscale=False)                    # the height is the double-precision mean of three mapped channels
    with m.terrain_world(42, chunk_cells=2) as world:
        assert world.geometry.channels == 3
        hm, _ = _same_planes(world, RECTS[0])
        a = world.heightmap(*RECTS[0])
        assert np.array_equal(hm, RN._unit_planes(a, False, "h").astype(np.float64).mean(0).astype(np.float32))


# ---- 3. rendering ---------------------------------------------------------------------------------------------------
def test_renders_from_the_resident_scene_equal_the_host_paths(model):
    cam = RN.Camera((-20.5, 11.25, 14.0), 0.5, -0.35, fov=1.0, size=(20, 28))
    rect = cam.footprint(MAX_DIST)
    with model.terrain_world(42, chunk_cells=2) as world:
        with world.scene(*rect, height_scale=HS) as host, world.scene(*rect, resident=True, height_scale=HS) as res:
            assert res.height_scale == host.height_scale == HS
            hit = False
            for uint8 in (False, True):
                for accel in (True, False):
                    dh, dr = np.empty(cam.size, np.float32), np.empty(cam.size, np.float32)
                    want = host.render(cam, max_dist=MAX_DIST, uint8=uint8, accel=accel, depth=dh, **RKW)
                    got = res.render(cam, max_dist=MAX_DIST, uint8=uint8, accel=accel, depth=dr, **RKW)
                    assert got.dtype == want.dtype and np.array_equal(got, want), (uint8, accel)
                    assert np.array_equal(dr, dh), (uint8, accel)
                    hit = hit or np.isfinite(dr).any()
            assert hit
        assert np.array_equal(world.view(cam, MAX_DIST, height_scale=HS, uint8=False, **RKW),
                              host_render(world, model, rect, cam))


def host_render(world, m, rect, cam, **kw):
    """the contract's right-hand side: the host-path scene of ``rect``, rendered"""
    hm, tex = world.both(*rect)
    with RN.Scene(hm, tex, origin=rect[:2], height_scale=HS, value_range=(m.is_a_grayscale, m.is_b_grayscale),
                  device=m.device) as sc:
        return sc.render(cam, max_dist=MAX_DIST, **dict(dict(uint8=False, **RKW), **kw))


# ---- 4. flight ------------------------------------------------------------------------------------------------------
def _path(n=12):
    return [RN.Camera((-200.5 + 400.0 * i / (n - 1), 11.25, 14.0), 0.5, -0.35, fov=1.0, size=(20, 28)) for i in range(n)]


WINDOW_MB = 128 * 128 * WD.SCENE_BYTES_PER_PIXEL / float(1 << 20)      # windows of at most 128 x 128 pixels


def test_flight_frames_are_their_windows_host_path_renders(model):
    cams = _path()
    with model.terrain_world(42, chunk_cells=2) as world:
        view0 = world.view(cams[0], MAX_DIST, height_scale=HS, uint8=False, **RKW)
        plan = world.flight_plan(cams, MAX_DIST, window_mb=WINDOW_MB)
        assert len(plan) >= 3 and plan[0][0][0] < 0 < plan[-1][0][0] + plan[-1][0][2]          # crosses y = 0
        frames = list(world.flight(cams, MAX_DIST, window_mb=WINDOW_MB, height_scale=HS, uint8=False, **RKW))
        assert len(frames) == 12
        for rect, i, j in plan:
            hm, tex = world.both(*rect)
            with RN.Scene(hm, tex, origin=rect[:2], height_scale=HS, device=model.device,
                          value_range=(model.is_a_grayscale, model.is_b_grayscale)) as sc:
                for k in range(i, j + 1):
                    want = sc.render(cams[k], max_dist=MAX_DIST, uint8=False, **RKW)
                    assert frames[k].shape == (3, 20, 28) and np.array_equal(frames[k], want), (k, rect)
        assert not np.array_equal(frames[0], frames[-1])
        # a second flight over the same path: every chunk comes from the cache, and the frames are the same
        n = world.computed
        again = list(world.flight(cams, MAX_DIST, window_mb=WINDOW_MB, height_scale=HS, **RKW))
        assert world.computed == n and len(again) == 12 and again[0].dtype == np.uint8
        u8 = list(world.flight(cams[:2], MAX_DIST, window_mb=WINDOW_MB, height_scale=HS, **RKW))
        assert np.array_equal(u8[0], again[0]) and np.array_equal(u8[1], again[1])
        # a flight abandoned half way closes its scene; view is what it was
        before = model.device.bytes_allocated
        it = world.flight(cams, MAX_DIST, window_mb=WINDOW_MB, height_scale=HS, **RKW)
        next(it)
        assert model.device.bytes_allocated > before
        it.close()
        assert model.device.bytes_allocated == before
        assert np.array_equal(world.view(cams[0], MAX_DIST, height_scale=HS, uint8=False, **RKW), view0)


# ---- 5. refusals ----------------------------------------------------------------------------------------------------
def test_flight_and_resident_scene_refusals(model):
    cams = _path()
    world = model.terrain_world(42, chunk_cells=2)
    world.both(0, 0, 8, 8)                                   # the chunks and head maps of this rectangle are cached now
    n, before = world.computed, model.device.bytes_allocated
    with pytest.raises(ValueError, match="frame 0"):
        world.flight(cams, MAX_DIST, window_mb=0.001)        # raised by the call, before any device work
    for rect in ((0, 0, 1, 64), (0, 0, 64, 1), (0, 0, 0, 4), (0.5, 0, 4, 4)):
        with pytest.raises(ValueError):
            world.scene(*rect, resident=True)
    with pytest.raises(ValueError, match="height_scale"):
        world.scene(0, 0, 8, 8, resident=True, height_scale=-1.0)
    assert model.device.bytes_allocated == before            # the buffers of the refused scene were freed
    assert world.computed == n
    world.close()
    with pytest.raises(ValueError, match="closed"):
        world.flight(cams, MAX_DIST)
    with pytest.raises(ValueError, match="closed"):
        world.scene(0, 0, 64, 64, resident=True)
    assert model.device.bytes_allocated <= before


def _upload(dev, a):
    p = dev.alloc(a.nbytes)
    dev.h2d(p, a)
    return p


def _download(dev, p, shape, dtype=np.float32):
    a = np.empty(shape, dtype)
    dev.d2h(a, p, a.nbytes)
    return a


def _host_scene_planes(dev, hm, tex, vr):
    """what render.Scene uploads for these arrays, through Scene itself"""
    with RN.Scene(hm, tex, value_range=vr, device=dev) as sc:
        return sc.arrays()


@pytest.mark.parametrize("Cc,grey,K", [(1, True, 64), (1, False, 37), (3, False, 32), (3, False, 21), (3, True, 16)])
def test_height_sink_against_the_host_mapping(dev, ops, Cc, grey, K):
    rng = np.random.RandomState(Cc * 100 + K)
    x = rng.uniform(-1.3, 1.3, (Cc, K, K)).astype(np.float32)
    x.ravel()[::7] = (rng.randint(0, 256, x.ravel()[::7].size) + 0.5).astype(np.float32) / np.float32(255)
    x.ravel()[::11] = rng.randint(0, 256, x.ravel()[::11].size) * np.float32(2) / np.float32(255) - np.float32(1)
    x.ravel()[::13] = rng.choice(np.array([0.0, -0.0, 1.0, -1.0, 1e-30, -1e-30, 1e-45], np.float32), x.ravel()[::13].size)
    chunk, flag = _upload(dev, x), _upload(dev, np.zeros(4, np.int32))
    H, W = K + 3, K + 8
    # (r0, c0, nr, nc, y, x): the whole chunk; odd everything; one pixel into the last corner; the 16-byte form (K % 4 == 0)
    for r0, c0, nr, nc, y, xx in ((0, 0, K, K, 0, 0), (3, 5, 7, 9, 2, 11), (K - 1, K - 1, 1, 1, H - 1, W - 1),
                                  (4, 8, 5, 8, 1, 4), (2, 4, 3, 4, 0, W - 4), (0, 1, K, K - 1, 3, 0)):
        fill = np.full((H, W), -7.0, np.float32)
        dst = _upload(dev, fill)
        ops.world_scene_height(chunk, Cc, K, r0, c0, nr, nc, grey, dst, H, W, y, xx, flag)
        got = _download(dev, dst, (H, W))
        crop = np.ascontiguousarray(x[:, r0:r0 + nr, c0:c0 + nc])
        if nr >= 2 and nc >= 2:
            want, _ = _host_scene_planes(dev, crop, np.zeros((3, nr, nc), np.float32), (grey, True))
        else:                                                # below Scene's minimum size: its two lines, by hand
            u = RN._unit_planes(crop, grey, "h")
            want = u[0] if Cc == 1 else u.astype(np.float64).mean(0).astype(np.float32)
        assert np.array_equal(got[y:y + nr, xx:xx + nc], want), (r0, c0, nr, nc)
        got[y:y + nr, xx:xx + nc] = -7.0
        assert np.array_equal(got, fill)                     # nothing outside its rectangle
        dev.free(dst)
    assert not _download(dev, flag, (4,), np.int32).any()    # finite inputs leave the flag alone
    for p in (chunk, flag):
        dev.free(p)


@pytest.mark.parametrize("Cc,grey,w", [(3, False, 37), (3, False, 40), (1, True, 37), (1, False, 24), (3, True, 21)])
def test_texture_sink_against_finalize_and_the_host_mapping(dev, ops, Cc, grey, w):
    T, o, y0, x0, h = 16, 4, -7, 5, 30
    st = T - o
    p_lo, p_hi = WD.axis_tiles(y0, h, T, o)
    q_lo, q_hi = WD.axis_tiles(x0, w, T, o)
    ny, nx = p_hi - p_lo + 3, q_hi - q_lo + 3
    pad_y, pad_x = y0 - p_lo * st + st, x0 - q_lo * st + st
    Wp = (w + 3) // 4 * 4
    rng = np.random.RandomState(w + Cc)
    flag = _upload(dev, np.zeros(4, np.int32))
    fill = np.full((3, h, w), -7.0, np.float32)
    scene = _upload(dev, fill)
    want = fill.copy()
    stage = dev.alloc(Cc * T * Wp * 4)
    for p in range(p_lo, p_hi + 1):
        a = rng.uniform(-1.6, 1.6, (Cc, T, Wp)).astype(np.float32)          # any band: finalize divides what it finds
        a.ravel()[::9] = rng.choice(np.array([0.0, -0.0, 1.0, -1.0, 0.5], np.float32), a.ravel()[::9].size)
        acc = _upload(dev, a)
        last = p == p_hi
        yr = p * st - y0
        r_lo, r_hi = max(0, -yr), min(T if last else st, h - yr)
        n = r_hi - r_lo
        assert n > 0
        ops.texture_finalize(acc, Wp, T, Cc, r_lo, n, yr, ny, pad_y, nx, pad_x, o, False, grey, stage)
        v = _download(dev, stage, (Cc, n, Wp))[:, :, :w]
        want[:, yr + r_lo:yr + r_hi] = np.broadcast_to(RN._unit_planes(np.ascontiguousarray(v), grey, "t"), (3, n, w))
        ops.texture_finalize_scene(acc, Wp, T, Cc, r_lo, n, yr, ny, pad_y, nx, pad_x, o, grey, scene, h, w, flag)
        dev.sync()
        dev.free(acc)
    got = _download(dev, scene, (3, h, w))
    assert (want != -7.0).all()                              # the bands cover the scene
    assert np.array_equal(got, want)
    assert not _download(dev, flag, (4,), np.int32).any()
    for p in (stage, scene, flag):
        dev.free(p)


def test_raw_sinks_refuse_with_nothing_written_and_flag_non_finite_values(dev, ops):
    K, H, W, T, o = 16, 20, 24, 16, 4
    rng = np.random.RandomState(3)
    x = rng.uniform(-1, 1, (3, K, K)).astype(np.float32)
    chunk = _upload(dev, x)
    hfill, tfill = np.full((H, W), -7.0, np.float32), np.full((3, H, W), -7.0, np.float32)
    hm, tex = _upload(dev, hfill), _upload(dev, tfill)
    flag = _upload(dev, np.zeros(4, np.int32))
    acc = _upload(dev, rng.uniform(-1, 1, (3, T, W)).astype(np.float32))
    ok = dict(chunk_ptr=chunk, Cc=3, K=K, r0=2, c0=3, nr=5, nc=6, grey=False, hm_ptr=hm, H=H, W=W, y=1, x=2, flag_ptr=flag)
    for kw in (dict(chunk_ptr=None), dict(hm_ptr=None), dict(flag_ptr=None), dict(Cc=2), dict(Cc=0), dict(Cc=4), dict(K=0),
               dict(r0=-1), dict(c0=-1), dict(nr=-1), dict(nc=-1), dict(r0=12), dict(c0=11), dict(nr=K + 1), dict(nc=K + 1),
               dict(y=-1), dict(x=-1), dict(y=H - 4), dict(x=W - 5), dict(H=0), dict(W=0), dict(H=1 << 16, W=1 << 15),
               dict(r0=1 << 30, nr=1 << 30), dict(y=(1 << 31) - 2)):
        with pytest.raises(GhmError):
            ops.world_scene_height(**dict(ok, **kw))
    # the first band of a plan whose first tile starts one stride before the scene, on both axes
    ny, nx = WD.axis_tiles(0, H, T, o)[1] + 3, WD.axis_tiles(0, W, T, o)[1] + 3
    tok = dict(acc_ptr=acc, W=W, T=T, Cc=3, r0=0, nrows=T - o, yc0=0, ny=ny, pad_y=T - o, nx=nx, pad_x=T - o, overlap=o,
               b_grey=False, tex_ptr=tex, H=H, Ws=W, flag_ptr=flag)
    for kw in (dict(acc_ptr=None), dict(tex_ptr=None), dict(flag_ptr=None), dict(Cc=2), dict(Cc=0), dict(Cc=4), dict(r0=-1),
               dict(nrows=-1), dict(r0=8, nrows=T - 7), dict(yc0=-1), dict(yc0=H - 11), dict(H=0), dict(Ws=0),
               dict(Ws=W + 1), dict(H=1 << 27), dict(overlap=T), dict(overlap=-1), dict(T=0)):
        with pytest.raises(GhmError):
            ops.texture_finalize_scene(**dict(tok, **kw))
    dev.sync()
    assert np.array_equal(_download(dev, hm, (H, W)), hfill) and np.array_equal(_download(dev, tex, (3, H, W)), tfill)
    assert not _download(dev, flag, (4,), np.int32).any()
    # the calls the refusals were variations of go through, and empty rectangles are no error
    ops.world_scene_height(**dict(ok, nr=0))
    ops.texture_finalize_scene(**dict(tok, nrows=0))
    assert np.array_equal(_download(dev, hm, (H, W)), hfill) and np.array_equal(_download(dev, tex, (3, H, W)), tfill)
    ops.world_scene_height(**ok)
    ops.texture_finalize_scene(**tok)
    assert (_download(dev, hm, (H, W))[1:6, 2:8] != -7.0).all() and (_download(dev, tex, (3, H, W))[:, :T - o] != -7.0).all()
    assert not _download(dev, flag, (4,), np.int32).any()
    # non-finite inputs are read like any other value, and set the flag: one NaN and one inf in a synthetic chunk
    bad = x.copy()
    bad[1, 3, 4], bad[2, 5, 7] = np.nan, np.inf
    dev.h2d(chunk, bad)
    ops.world_scene_height(**dict(ok, r0=8, c0=8, nr=8, nc=8))              # a rectangle that holds neither
    assert not _download(dev, flag, (4,), np.int32).any()
    for r0, c0 in ((3, 4), (5, 7)):                                        # the NaN alone, the inf alone
        dev.memset_zero(flag, 16)
        ops.world_scene_height(**dict(ok, r0=r0, c0=c0, nr=1, nc=1))
        assert _download(dev, flag, (4,), np.int32).tolist() == [1, 0, 0, 0]
    dev.memset_zero(flag, 16)
    a = rng.uniform(-1, 1, (3, T, W)).astype(np.float32)
    a[2, 1, 5] = np.inf
    dev.h2d(acc, a)
    ops.texture_finalize_scene(**dict(tok, r0=2))                          # rows 2 ..: not the inf's
    assert not _download(dev, flag, (4,), np.int32).any()
    ops.texture_finalize_scene(**tok)
    assert _download(dev, flag, (4,), np.int32).tolist() == [1, 0, 0, 0]
    a[2, 1, 5], a[0, 0, 0] = 0.0, np.nan
    dev.h2d(acc, a)
    dev.memset_zero(flag, 16)
    ops.texture_finalize_scene(**dict(tok, Cc=1))
    assert _download(dev, flag, (4,), np.int32).tolist() == [1, 0, 0, 0]
    # Scene.from_device: its refusals free the buffers it was given
    before = dev.bytes_allocated
    for kw in (dict(H=1), dict(W=1), dict(height_scale=0.0), dict(origin=(0.5, 0))):
        a_, b_ = dev.alloc(4 * H * W), dev.alloc(12 * H * W)
        with pytest.raises(ValueError):
            RN.Scene.from_device(dev, a_, b_, **dict(dict(H=H, W=W), **kw))
        assert dev.bytes_allocated == before
    for p in (chunk, hm, tex, flag, acc):
        dev.free(p)


# ---- 6. command line ------------------------------------------------------------------------------------------------
def test_cli_writes_a_windowed_path(tmp_path, monkeypatch):
    from PIL import Image
    from gan_heightmaps_amd import experiments
    cfg = ostep.default_cfg(**SMALL)
    src = build_model(cfg, 13, None, use_graph=False, dtype='f32')
    src.z_fn(ostep.synthetic_batch(4, cfg, seed=1)[0])
    src.save_model(str(tmp_path / "m.model"))
    args = [str(tmp_path / "f.png"), "--world", "SMALL", str(tmp_path / "m.model"), "--seed", "4", "--chunk-cells", "2",
            "--dtype", "f32", "--pos", "-100.5,11.25,14", "--yaw", "28.6", "--pitch", "-20", "--fov", "57.3", "--size", "20x28",
            "--max-dist", "40", "--height-scale", "10", "--frames", "3", "--to", "100,11.25,14", "--window-mb", "%r" % WINDOW_MB]
    a = RN.parse_args(args)
    cams = RN.cameras_of(a)
    with src.terrain_world(4, chunk_cells=2) as world:
        assert len(world.flight_plan(cams, 40.0, window_mb=WINDOW_MB)) >= 2
        want = list(world.flight(cams, 40.0, window_mb=WINDOW_MB, height_scale=10.0))
    src.device.close()
    monkeypatch.setattr(experiments, "make_model", lambda name, **kw: build_model(cfg, 99, None, use_graph=False, dtype=kw['dtype']))
    assert RN.main(args) == 0
    for i in range(3):
        got = np.asarray(Image.open(tmp_path / ("f_%04d.png" % i)))
        assert got.shape == (20, 28, 3) and np.array_equal(got, want[i]), i
    assert not np.array_equal(want[0], want[2])
