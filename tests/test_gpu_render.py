"""The heightfield ray caster on the MI355X (csrc/render.hip, gan_heightmaps_amd/render.py): ghm_render_view
against the float64 restatement (tests/render_ref.py) on the nine calibrated views, the accelerated march against the plain
one bit for bit, the shapes that break the tiling and the pyramid, the refusals, Scene, TerrainWorld.view and the command
line."""
import math

import numpy as np
import pytest

from oracle import step as ostep
from gan_heightmaps_amd import render as RN
from gan_heightmaps_amd._lib import GhmError
from tests import render_ref as R
from tests.gpu_common import build_model, dev, ops, SMALL      # noqa: F401  (dev, ops: the module-scoped fixtures)
from tests.test_render_plan import F32_DEV

pytestmark = pytest.mark.gpu

TOL = 8 * F32_DEV            # a different operation order and the device's exp / sqrt: a margin over the reference's own error
MAX_FAIL = 0.005             # silhouette pixels where one ulp changes which sample hits


class GpuScene:
    """hm [H, W], tex [3, H, W] and the pyramid on the device, through the raw Ops entry points"""

    def __init__(self, dev, ops, hm, tex):
        self.dev, self.ops = dev, ops
        self.H, self.W = hm.shape
        self.hm, self.tex = dev.alloc(hm.nbytes), dev.alloc(tex.nbytes)
        dev.h2d(self.hm, np.ascontiguousarray(hm, np.float32))
        dev.h2d(self.tex, np.ascontiguousarray(tex, np.float32))
        self.mip = ops.render_maxmip(self.hm, self.H, self.W)

    def render(self, cam, size, height_scale, shadows, accel, u8=False, **kw):
        from gan_heightmaps_amd.device import render_params
        args = dict(R.VIEW_KW)
        args.update(kw)
        p = render_params(cam['pos'], cam['yaw'], cam['pitch'], cam['fov'], size, height_scale, args['step'],
                          args['max_dist'], args['sun_azimuth'], args['sun_elevation'], shadows, args['softness'],
                          args['ambient'], args['haze'], R.DEFAULT_SKY['horizon'], R.DEFAULT_SKY['zenith'], accel=accel,
                          out_u8=u8)
        Hi, Wi = size
        out = np.empty((Hi, Wi, 3), np.uint8) if u8 else np.empty((3, Hi, Wi), np.float32)
        depth = np.empty((Hi, Wi), np.float32)
        o, d = self.dev.alloc(out.nbytes), self.dev.alloc(depth.nbytes)
        try:
            self.ops.render_view(p, self.hm, self.tex, self.H, self.W, self.mip, o, d)
            self.dev.d2h(out, o, out.nbytes)
            self.dev.d2h(depth, d, depth.nbytes)
        finally:
            self.dev.free(o)
            self.dev.free(d)
        return out, depth

    def close(self):
        for p in (self.hm, self.tex, self.mip.ptr):
            self.dev.free(p)


@pytest.fixture(scope="module")
def scenes(dev, ops):
    s = {seed: GpuScene(dev, ops, *R.terrain(seed)) for seed in R.SEEDS}
    yield s
    for g in s.values():
        g.close()


def check_parity(got, depth, want, want_t, what, got8=None):
    """the issue's criterion: a pixel passes if its three channels are within TOL; at most MAX_FAIL of an image may fail, or
    disagree on hit / miss -- whole pixels, so none at all in an image of fewer than 200; uint8 within one level on the
    passing pixels"""
    err = np.abs(got.astype(np.float64) - want).max(0)
    bad = err > TOL
    flips = np.isfinite(depth) != np.isfinite(want_t)
    allowed = int(math.floor(MAX_FAIL * bad.size))
    print("%s: max err %.3e, median %.3e, failing %d / %d (allowed %d), hit/miss flips %d"
          % (what, err.max(), np.median(err), bad.sum(), bad.size, allowed, flips.sum()))
    assert bad.sum() <= allowed, (what, bad.sum(), err.max())
    assert flips.sum() <= allowed, (what, flips.sum())
    if got8 is not None and (~bad).any():
        lv = np.abs(got8.astype(np.int64) - R.to_uint8(want).astype(np.int64)).max(2)
        assert lv[~bad].max() <= 1, (what, lv[~bad].max())


# ---- 1. parity on the nine views, and the accelerated march against the plain one ----------------------------------
@pytest.mark.parametrize("shadows", [False, True])
@pytest.mark.parametrize("seed,cam", R.views())
def test_nine_views_against_the_float64_restatement(scenes, seed, cam, shadows):
    g = scenes[seed]
    want, want_t = R.reference(seed, cam, shadows, 'float64')
    got, depth = g.render(R.CAMERAS[cam], R.VIEW_SIZE, R.HEIGHT_SCALE, shadows, True)
    got8, _ = g.render(R.CAMERAS[cam], R.VIEW_SIZE, R.HEIGHT_SCALE, shadows, True, u8=True)
    check_parity(got, depth, want, want_t, "seed %d camera %d shadows %d" % (seed, cam, shadows), got8)
    # the reference at float32 stays at 0 % on these inputs (the cap above is a condition, not a budget)
    w32, t32 = R.reference(seed, cam, shadows, 'float32')
    assert (np.abs(w32 - want).max(0) <= TOL).all() and np.array_equal(np.isfinite(t32), np.isfinite(want_t))
    plain, pdepth = g.render(R.CAMERAS[cam], R.VIEW_SIZE, R.HEIGHT_SCALE, shadows, False)
    plain8, _ = g.render(R.CAMERAS[cam], R.VIEW_SIZE, R.HEIGHT_SCALE, shadows, False, u8=True)
    assert np.array_equal(got, plain) and np.array_equal(depth, pdepth) and np.array_equal(got8, plain8)


# ---- 2. shapes that break the tiling and the pyramid ----------------------------------------------------------------
def _identity_and_parity(dev, ops, hm, tex, cam, size, hs, **kw):
    g = GpuScene(dev, ops, hm, tex)
    try:
        for shadows in (False, True):
            a, da = g.render(cam, size, hs, shadows, True, **kw)
            b, db = g.render(cam, size, hs, shadows, False, **kw)
            assert np.array_equal(a, b) and np.array_equal(da, db), (size, shadows)
            a8, _ = g.render(cam, size, hs, shadows, True, u8=True, **kw)
            b8, _ = g.render(cam, size, hs, shadows, False, u8=True, **kw)
            assert np.array_equal(a8, b8), (size, shadows)
        args = dict(R.VIEW_KW)
        args.update(kw)
        want, want_t = R.render(hm, tex, size=size, height_scale=hs, shadows=True, dtype=np.float64, **cam, **args)
        check_parity(a, da, want, want_t, "scene %s image %s" % (hm.shape, size), a8)
        return a, da
    finally:
        g.close()


def _odd_terrain(H, W, seed):
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    hm = 0.5 + 0.25 * np.sin(0.11 * yy + 0.3) * np.cos(0.09 * xx) + 0.2 * np.sin(0.05 * (yy + xx))
    hm = np.clip(hm, 0, 1).astype(np.float32)
    return hm, rng.uniform(0, 1, (3, H, W)).astype(np.float32)


# the two tiny images may have no failing pixel at all (0.5 % of them is less than one), so their camera looks steeply down
# at open ground: every ray hits, none grazes a silhouette (the restatement at float32 deviates by 3e-6 there)
STEEP = dict(pos=(8.2, 40.7, 45.0), yaw=0.2, pitch=-0.9, fov=0.5)
WIDE = dict(pos=(8.2, 40.7, 35.0), yaw=0.2, pitch=-0.4, fov=1.0)


@pytest.mark.parametrize("size,cam", [((48, 64), WIDE), ((1, 1), STEEP), ((7, 5), STEEP), ((33, 65), WIDE)])
def test_odd_scene_and_ragged_images(dev, ops, size, cam):
    hm, tex = _odd_terrain(97, 83, 5)
    _, depth = _identity_and_parity(dev, ops, hm, tex, cam, size, 20.0, max_dist=120.0)
    if cam is STEEP:
        assert np.isfinite(depth).all()


def test_two_by_two_scene(dev, ops):
    hm = np.array([[0.1, 0.9], [0.5, 0.3]], np.float32)
    tex = np.random.RandomState(1).uniform(0, 1, (3, 2, 2)).astype(np.float32)
    cam = dict(pos=(-3.1, 1.2, 4.0), yaw=0.1, pitch=-0.6, fov=0.9)
    _, depth = _identity_and_parity(dev, ops, hm, tex, cam, (24, 24), 2.0, max_dist=20.0, step=0.25)
    assert np.isfinite(depth).any() and not np.isfinite(depth).all()


def test_camera_outside_looking_in_and_looking_away(dev, ops):
    hm, tex = _odd_terrain(97, 83, 6)
    _, depth = _identity_and_parity(dev, ops, hm, tex, dict(pos=(-40.3, 30.1, 30.0), yaw=0.15, pitch=-0.3, fov=1.0), (24, 40),
                                    20.0, max_dist=200.0)
    assert np.isfinite(depth).any()
    _, depth = _identity_and_parity(dev, ops, hm, tex, dict(pos=(-40.3, 30.1, 30.0), yaw=math.pi, pitch=-0.3, fov=1.0), (24, 40),
                                    20.0, max_dist=200.0)
    assert not np.isfinite(depth).any()                      # all sky


def test_max_dist_shorter_than_the_first_hit_and_a_step_that_is_not_dyadic(dev, ops):
    hm, tex = _odd_terrain(97, 83, 7)
    cam = dict(pos=(20.3, 41.2, 60.0), yaw=0.4, pitch=-0.5, fov=0.9)
    _, depth = _identity_and_parity(dev, ops, hm, tex, cam, (24, 40), 20.0, max_dist=30.0)
    assert not np.isfinite(depth).any()
    _, depth = _identity_and_parity(dev, ops, hm, tex, cam, (24, 40), 20.0, max_dist=150.0, step=0.37)
    assert np.isfinite(depth).any()


# ---- 3. refusals: an error, and nothing written ---------------------------------------------------------------------
def test_refusals_write_nothing(dev, ops):
    from gan_heightmaps_amd.device import render_params
    hm, tex = _odd_terrain(16, 300, 8)
    g = GpuScene(dev, ops, hm, tex)
    other = ops.render_maxmip(g.hm, 300, 16)                 # the same elements, another size
    Hi, Wi = 6, 8
    fill = np.full((3, Hi, Wi), -7.0, np.float32)
    out = dev.alloc(fill.nbytes)
    dev.h2d(out, fill)

    def params(**kw):
        a = dict(pos=(2.0, 3.0, 30.0), yaw=0.1, pitch=-0.5, fov=1.0, size=(Hi, Wi), height_scale=10.0, step=0.5,
                 max_dist=50.0, sun_azimuth=0.6, sun_elevation=0.5, shadows=True, softness=8.0, ambient=0.25, haze=0.001,
                 horizon=(0.8, 0.8, 0.9), zenith=(0.3, 0.5, 0.8))
        a.update(kw)
        return render_params(**a)

    ok = dict(hm=g.hm, tex=g.tex, H=16, W=300, mip=g.mip, out=out)
    nan, inf = float('nan'), float('inf')
    cases = [(params(), dict(hm=None)), (params(), dict(tex=None)), (params(), dict(out=None)), (params(), dict(mip=None)),
             (None, {}),
             (params(), dict(H=1, W=300)), (params(), dict(H=16, W=1)), (params(), dict(H=1 << 16, W=1 << 15)),
             (params(size=(1 << 16, 1 << 15)), {}), (params(size=(0, 4)), {}),
             (params(step=0.0), {}), (params(step=-1.0), {}), (params(step=nan), {}),
             (params(max_dist=0.0), {}), (params(max_dist=-5.0), {}), (params(max_dist=inf), {}),
             (params(max_dist=1e6, step=0.5), {}),                                  # more than 2^20 samples per ray
             (params(fov=0.0), {}), (params(fov=math.pi), {}), (params(fov=4.0), {}), (params(fov=nan), {}),
             (params(pos=(nan, 0.0, 1.0)), {}), (params(pos=(0.0, inf, 1.0)), {}), (params(pos=(0.0, 0.0, -inf)), {}),
             (params(yaw=nan), {}), (params(pitch=inf), {}), (params(height_scale=0.0), {}), (params(height_scale=nan), {}),
             (params(), dict(mip=other)), (params(), dict(H=300, W=16))]
    for p, kw in cases:
        a = dict(ok)
        a.update(kw)
        with pytest.raises(GhmError):
            ops.render_view(p, a['hm'], a['tex'], a['H'], a['W'], a['mip'], a['out'])
    with pytest.raises(GhmError):
        ops.render_maxmip(g.hm, 1, 300)                       # scene 1 x 300
    with pytest.raises(GhmError):
        ops.render_maxmip(g.hm, 1 << 16, 1 << 15)
    # the pyramid builder itself: null pointers and a buffer of another size, with nothing written
    import ctypes as C
    from gan_heightmaps_amd._lib import call
    n = g.mip.elems
    mfill = np.full(n, -3.0, np.float32)
    mbuf = dev.alloc(mfill.nbytes)
    dev.h2d(mbuf, mfill)
    for hm_p, mip_p, H_, W_, elems in ((None, mbuf, 16, 300, n), (g.hm, None, 16, 300, n), (g.hm, mbuf, 16, 300, n - 1),
                                       (g.hm, mbuf, 16, 300, n + 1), (g.hm, mbuf, 16, 300, 16 * 300), (g.hm, mbuf, 1, 300, n),
                                       (g.hm, mbuf, 16, 1, n)):
        with pytest.raises(GhmError):
            call("ghm_render_maxmip", dev.h, C.c_void_p(hm_p), H_, W_, C.c_void_p(mip_p), elems)
    dev.sync()
    mgot = np.empty_like(mfill)
    dev.d2h(mgot, mbuf, mgot.nbytes)
    assert np.array_equal(mgot, mfill)
    call("ghm_render_maxmip", dev.h, C.c_void_p(g.hm), 16, 300, C.c_void_p(mbuf), n)
    dev.d2h(mgot, mbuf, mgot.nbytes)
    assert mgot.min() >= 0.0 and mgot[-1] == hm.max()        # the 1 x 1 top level
    dev.free(mbuf)
    with pytest.raises(ValueError):
        RN.Scene(np.zeros((1, 300), np.float32), np.zeros((3, 1, 300), np.float32), device=dev)
    dev.sync()
    got = np.empty_like(fill)
    dev.d2h(got, out, got.nbytes)
    assert np.array_equal(got, fill)
    # the plain march needs no pyramid, and the call the refusals were variations of goes through
    ops.render_view(params(accel=False), g.hm, g.tex, 16, 300, None, out)
    ops.render_view(params(), g.hm, g.tex, 16, 300, g.mip, out)
    dev.d2h(got, out, got.nbytes)
    assert np.isfinite(got).all() and got.min() >= 0.0
    dev.free(out)
    dev.free(other.ptr)
    g.close()


# ---- 4. Scene -------------------------------------------------------------------------------------------------------
def test_scene_renders_repeat_honour_out_and_follow_the_origin(dev):
    hm, tex = R.terrain(1)
    c1 = RN.Camera(**R.CAMERAS[0], size=(30, 44))
    c2 = RN.Camera(**R.CAMERAS[1], size=(30, 44))
    kw = dict(max_dist=150.0, sun_azimuth=0.6, sun_elevation=0.5, haze=0.002)
    before = dev.bytes_allocated
    with RN.Scene(hm, tex, height_scale=R.HEIGHT_SCALE, value_range=(True, True), device=dev) as sc:
        a1 = sc.render(c1, **kw)
        a2 = sc.render(c2, uint8=False, **kw)
        assert a1.shape == (30, 44, 3) and a1.dtype == np.uint8 and a2.shape == (3, 30, 44) and a2.dtype == np.float32
        out = np.zeros((30, 44, 3), np.uint8)
        assert sc.render(c1, out=out, **kw) is out and np.array_equal(out, a1)
        for bad in (np.zeros((30, 44, 3), np.float32), np.zeros((44, 30, 3), np.uint8), np.zeros((30, 88, 3), np.uint8)[:, ::2]):
            with pytest.raises(ValueError):
                sc.render(c1, out=bad, **kw)
        assert np.array_equal(sc.render(c1, accel=False, **kw), a1)
        want, _ = R.render(hm, tex, size=(30, 44), height_scale=R.HEIGHT_SCALE, **R.CAMERAS[1], **dict(R.VIEW_KW))
        assert (np.abs(a2 - want).max(0) > TOL).mean() <= MAX_FAIL
    assert dev.bytes_allocated == before                     # close() frees what the scene took
    with RN.Scene(hm, tex, height_scale=R.HEIGHT_SCALE, value_range=(True, True), device=dev) as f1:
        assert np.array_equal(f1.render(c1, **kw), a1)
    with RN.Scene(hm, tex, height_scale=R.HEIGHT_SCALE, value_range=(True, True), device=dev) as f2:
        assert np.array_equal(f2.render(c2, uint8=False, **kw), a2)
    # uint8 and fp32 inputs of the same picture
    h8 = np.rint(hm * 255).astype(np.uint8)
    t8 = np.rint(tex * 255).astype(np.uint8)
    with RN.Scene(h8, np.ascontiguousarray(t8.transpose(1, 2, 0)), height_scale=R.HEIGHT_SCALE, device=dev) as s8, \
            RN.Scene(h8.astype(np.float32) / np.float32(255), t8.astype(np.float32) / np.float32(255),
                     height_scale=R.HEIGHT_SCALE, value_range=(True, True), device=dev) as sf:
        assert np.array_equal(s8.render(c1, uint8=False, **kw), sf.render(c1, uint8=False, **kw))
    # the tanh range maps as util.convert_to_rgb maps it
    with RN.Scene(hm, tex * np.float32(2) - np.float32(1), height_scale=R.HEIGHT_SCALE, value_range=(True, False),
                  device=dev) as st:
        assert np.abs(st.render(c1, uint8=False, **kw) - f1_float(dev, hm, tex, c1, kw)).max() < 1e-5
    # origin: the scene and the camera moved by the same integers
    moved = c1.moved((c1.pos[0] - 70, c1.pos[1] + 33, c1.pos[2]))
    with RN.Scene(hm, tex, origin=(-70, 33), height_scale=R.HEIGHT_SCALE, value_range=(True, True), device=dev) as so:
        assert np.array_equal(so.render(moved, **kw), a1)


def f1_float(dev, hm, tex, cam, kw):
    with RN.Scene(hm, tex, height_scale=R.HEIGHT_SCALE, value_range=(True, True), device=dev) as s:
        return s.render(cam, uint8=False, **kw)


# ---- 5. TerrainWorld.view -------------------------------------------------------------------------------------------
def test_world_view(dev):
    cfg = ostep.default_cfg(**SMALL)
    m = build_model(cfg, 5, dev, dtype='f32', use_graph=False)
    for s in range(3):
        m.z_fn(ostep.synthetic_batch(4, cfg, seed=40 + s)[0])
    cam = RN.Camera((-20.5, 11.25, 14.0), 0.5, -0.35, fov=1.0, size=(20, 28))
    max_dist, kw = 40.0, dict(sun_elevation=0.6, haze=0.003)
    with m.terrain_world(42, chunk_cells=2) as world:
        got = world.view(cam, max_dist, height_scale=10.0, uint8=False, **kw)
        fp = cam.footprint(max_dist)
        hm, tex = world.both(*fp)
        with RN.Scene(hm, tex, origin=fp[:2], height_scale=10.0, value_range=(m.is_a_grayscale, m.is_b_grayscale),
                      device=dev) as sc:
            assert np.array_equal(sc.render(cam, max_dist=max_dist, uint8=False, **kw), got)
        assert got.shape == (3, 20, 28) and np.isfinite(got).all()
        u8 = world.view(cam, max_dist, height_scale=10.0, **kw)
        assert u8.dtype == np.uint8 and np.abs(u8.astype(np.int64) - R.to_uint8(got)).max() <= 0
        # a larger scene around the footprint: no ray leaves the footprint, so every pixel sees the same terrain.  The
        # kernel's coordinates are float32 and scene-local, so another origin rounds a sample's position differently: the
        # two images agree as the kernel agrees with the restatement, not bit for bit
        big = (fp[0] - 13, fp[1] - 9, fp[2] + 30, fp[3] + 21)
        d_big, d_fp = np.empty(cam.size, np.float32), np.empty(cam.size, np.float32)
        with world.scene(*big, height_scale=10.0) as sb:
            wide = sb.render(cam, max_dist=max_dist, uint8=False, depth=d_big, **kw)
        with world.scene(*fp, height_scale=10.0) as sf:
            assert np.array_equal(sf.render(cam, max_dist=max_dist, uint8=False, depth=d_fp, **kw), got)
        err = np.abs(wide.astype(np.float64) - got).max(0)
        flips = np.isfinite(d_big) != np.isfinite(d_fp)
        hit = np.isfinite(d_big) & np.isfinite(d_fp)
        allowed = int(math.floor(MAX_FAIL * err.size))
        print("view against the larger scene: max %.3e, above TOL %d / %d, hit/miss flips %d, hits %d, max |dt| %.3e"
              % (err.max(), (err > TOL).sum(), err.size, flips.sum(), hit.sum(), np.abs(d_big[hit] - d_fp[hit]).max()))
        assert hit.any() and (err > TOL).sum() <= allowed
        # a footprint that was not conservative would show first as terrain the smaller scene lacks: flipped pixels
        assert flips.sum() <= allowed
        # and against the restatement on the footprint's arrays
        sc_hm = np.clip(hm[0], 0, 1)
        sc_tex = np.clip((tex * 127.5 + 127.5) / 255.0, 0, 1) if not m.is_b_grayscale else np.clip(tex, 0, 1)
        sc_tex = np.broadcast_to(sc_tex, (3,) + sc_tex.shape[1:])
        local = (cam.pos[0] - fp[0], cam.pos[1] - fp[1], cam.pos[2])
        d = dict(RN.DEFAULTS)
        want, _ = R.render(sc_hm, sc_tex, local, cam.yaw, cam.pitch, cam.fov, cam.size, 10.0, step=0.5, max_dist=max_dist,
                           sun_azimuth=d['sun_azimuth'], sun_elevation=0.6, shadows=True, softness=d['softness'],
                           ambient=d['ambient'], haze=0.003, horizon=d['horizon'], zenith=d['zenith'])
        assert (np.abs(got - want).max(0) > TOL).mean() <= MAX_FAIL
    # Pix2Pix.render_terrain on the same arrays
    cam_local = cam.moved(local)
    assert np.array_equal(m.render_terrain(hm, tex, cam_local, height_scale=10.0, max_dist=max_dist, uint8=False, **kw), got)


# ---- 6. command line ------------------------------------------------------------------------------------------------
def test_cli_writes_two_frames(tmp_path):
    from PIL import Image
    hm, tex = R.terrain(2)
    h8 = np.rint(hm * 255).astype(np.uint8)
    t8 = np.ascontiguousarray(np.rint(tex * 255).astype(np.uint8).transpose(1, 2, 0))
    np.save(tmp_path / "hm.npy", h8)
    Image.fromarray(t8).save(tmp_path / "tex.png")
    args = [str(tmp_path / "view.png"), "--heightmap", str(tmp_path / "hm.npy"), "--texture", str(tmp_path / "tex.png"),
            "--pos", "-10,64,50", "--look-at", "64,64,10", "--size", "36x48", "--height-scale", "24", "--max-dist", "200",
            "--frames", "2", "--to", "10,70,45", "--sun", "35,30"]
    assert RN.main(args) == 0
    frames = [np.asarray(Image.open(tmp_path / ("view_%04d.png" % i))) for i in range(2)]
    with RN.Scene(h8, t8, height_scale=24.0) as sc:
        for i, pos in enumerate(((-10.0, 64.0, 50.0), (10.0, 70.0, 45.0))):
            cam = RN.Camera.look_at(pos, (64.0, 64.0, 10.0), size=(36, 48))
            want = sc.render(cam, max_dist=200.0, sun_azimuth=math.radians(35), sun_elevation=math.radians(30))
            assert frames[i].shape == (36, 48, 3) and np.array_equal(frames[i], want)
    assert not np.array_equal(frames[0], frames[1])
