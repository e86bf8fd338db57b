"""The light of the sky on the MI355X (csrc/skylight.hip, gan_heightmaps_amd/skylight.py): ghm_skylight_bake
against the float64 restatement (tests/skylight_ref.py), the tiled form against the plain one bit for bit, pitches and
canaries, window independence on the device, uint8, the refusals; the sky-lit ray caster; the sky-lit TerrainWorld's scenes
and flights."""
import math

import numpy as np
import pytest

from oracle import step as ostep
from gan_heightmaps_amd import erosion as ER
from gan_heightmaps_amd import render as RN
from gan_heightmaps_amd import skylight as SK
from gan_heightmaps_amd import world as WD
from gan_heightmaps_amd._lib import GhmError
from tests import erosion_ref
from tests import render_ref as R
from tests import skylight_ref as S
from tests.gpu_common import build_model, dev, ops, SMALL      # noqa: F401  (dev, ops: the module-scoped fixtures)
from tests.test_render_plan import F32_DEV
from tests.test_skylight_ref import SKY_F32_DEV

pytestmark = pytest.mark.gpu

TOL = 8 * SKY_F32_DEV           # the renderer's convention: a margin over the number format's own error for the device's divide
CANARY = 0xAB


def device_bake(dev, ops, src, sky, hs, rect=None, cols=None, out_pitch=None, uint8=False, tiled=False):
    """src float32 [rows, pitch] -> the rectangle (default: everything) baked through the raw entry point, [h, w].  The output
    lies inside a larger buffer of canary bytes -- a row above and below, two cells to the left, the pitch's rest to the right
    -- which are checked to be untouched."""
    src = np.ascontiguousarray(src, np.float32)
    rows, pitch = src.shape
    cols = pitch if cols is None else cols
    y0, x0, h, w = (0, 0, rows, cols) if rect is None else rect
    out_pitch = w + 2 if out_pitch is None else out_pitch
    assert out_pitch >= w + 2
    cell = 1 if uint8 else 4
    whole = np.full((h + 2) * out_pitch * cell, CANARY, np.uint8)
    bufs = [dev.alloc(src.nbytes), dev.alloc(whole.nbytes)]
    try:
        dev.h2d(bufs[0], src)
        dev.h2d(bufs[1], whole)
        ops.skylight_bake(bufs[0], rows, cols, pitch, ops.skylight_table(sky), sky.directions, sky.steps, sky.reach, y0, x0,
                          h, w, hs, sky.strength, tiled, uint8, bufs[1] + (out_pitch + 2) * cell, out_pitch)
        dev.sync()
        dev.d2h(whole, bufs[1], whole.nbytes)
    finally:
        dev.sync()
        for p in bufs:
            dev.free(p)
    grid = whole.reshape(h + 2, out_pitch * cell)
    body = grid[1:h + 1, 2 * cell:(2 + w) * cell]
    mask = np.ones(grid.shape, bool)
    mask[1:h + 1, 2 * cell:(2 + w) * cell] = False
    assert (grid[mask] == CANARY).all(), "bytes around the output rectangle were written"
    return np.ascontiguousarray(body).view(np.uint8 if uint8 else np.float32).reshape(h, w).copy()


# ---- 1. the bake against the restatement, both forms ----------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(S.CASES)))
def test_bake_against_the_float64_restatement_and_tiled_equals_plain(dev, ops, case):
    H, W, seed, hs, kw = S.CASES[case]
    sky = SK.SkyLight(**kw)
    src = S.terrain(seed, H, W)
    plain = device_bake(dev, ops, src, sky, hs)
    err = np.abs(plain.astype(np.float64) - S.reference(case, 'float64'))
    differ = int((plain != S.reference(case, 'float32')).sum())
    print("case %d %d x %d: max err %.3e, %d of %d elements differ from the float32 restatement"
          % (case, H, W, err.max(), differ, H * W))
    assert (err <= TOL).all(), err.max()                               # every element: the quantity is continuous
    tiled = device_bake(dev, ops, src, sky, hs, tiled=True)
    assert np.array_equal(tiled, plain)                                # bit for bit
    # the public call, both forms and the default
    for t in (None, False, True):
        assert np.array_equal(SK.bake(ops, src, sky, height_scale=hs, tiled=t), plain)


def test_pitches_are_honoured_and_a_window_with_a_margin_is_the_larger_maps_interior(dev, ops):
    sky = SK.SkyLight()
    m, hs = sky.reach, 24.0
    big = S.terrain(7, 50 + 2 * m, 41 + 2 * m)
    rows, cols = big.shape
    whole = device_bake(dev, ops, big, sky, hs)
    wide = np.full((rows, cols + 5), np.nan, np.float32)               # a source pitch beyond its width: NaN beyond
    wide[:, :cols] = big
    y0, x0, h, w = m + 3, m + 2, 37, 35
    for tiled in (False, True):
        got = device_bake(dev, ops, wide, sky, hs, cols=cols, out_pitch=cols + 9, tiled=tiled)
        assert np.array_equal(got, whole)
        sub = device_bake(dev, ops, wide, sky, hs, rect=(y0, x0, h, w), cols=cols, out_pitch=w + 7, tiled=tiled)
        assert np.array_equal(sub, whole[y0:y0 + h, x0:x0 + w])
        # the same rectangle from a window of its own with margin = reach
        win = np.ascontiguousarray(big[y0 - m:y0 + h + m, x0 - m:x0 + w + m])
        assert np.array_equal(device_bake(dev, ops, win, sky, hs, rect=(m, m, h, w), tiled=tiled), sub)
        assert np.array_equal(SK.bake(ops, win, sky, height_scale=hs, margin=m, tiled=tiled), sub)
    assert not np.array_equal(SK.bake(ops, np.ascontiguousarray(big[y0:y0 + h, x0:x0 + w]), sky, height_scale=hs), sub)


def test_uint8_is_the_rounded_float_plane(dev, ops):
    H, W, seed, hs, kw = S.CASES[1]
    sky, src = SK.SkyLight(**kw), S.terrain(seed, H, W)
    f = device_bake(dev, ops, src, sky, hs)
    want = np.rint(f.astype(np.float64) * 255.0).astype(np.uint8)
    for tiled in (False, True):
        assert np.array_equal(device_bake(dev, ops, src, sky, hs, uint8=True, tiled=tiled), want)
    out = np.empty((H, W), np.uint8)
    assert SK.bake(ops, src, sky, height_scale=hs, uint8=True, out=out) is out and np.array_equal(out, want)
    u8src = np.rint(src * 255).astype(np.uint8)                        # a uint8 heightmap is v / 255
    assert np.array_equal(SK.bake(ops, u8src, sky, height_scale=hs),
                          SK.bake(ops, u8src.astype(np.float32) / np.float32(255), sky, height_scale=hs))


def test_a_reach_beyond_the_lds_budget_falls_back_to_the_plain_form(dev, ops):
    sky = SK.SkyLight(directions=4, steps=40, step=2.0)               # reach 81: a window of 195^2 floats, beyond 128 KiB
    assert sky.reach == 81 and ops.skylight_lds_bytes(sky.reach) == -1 and ops.skylight_lds_bytes(74) == 181 * 181 * 4
    assert ops.skylight_lds_bytes(SK.SkyLight().reach) == 107 * 107 * 4
    src = S.terrain(2, 40, 45)
    with pytest.raises(GhmError, match="LDS"):
        device_bake(dev, ops, src, sky, 24.0, tiled=True)
    plain = device_bake(dev, ops, src, sky, 24.0)
    assert np.array_equal(SK.bake(ops, src, sky, height_scale=24.0, tiled=True), plain)
    want = S.bake(src, 24.0, np.float64, directions=4, steps=40, step=2.0)
    assert (np.abs(plain - want) <= TOL).all()


def test_refusals_with_nothing_written(dev, ops):
    sky = SK.SkyLight(directions=8, steps=6, step=1.0)
    src = np.full((20, 24), 0.5, np.float32)
    p, out, tab = dev.alloc(src.nbytes), dev.alloc(src.nbytes), ops.skylight_table(sky)
    canary = np.full(src.shape, np.float32(-7.0))
    try:
        dev.h2d(p, src)
        dev.h2d(out, canary)
        good = dict(src=p, rows=20, cols=24, pitch=24, table=tab, directions=8, steps=6, reach=sky.reach, y0=0, x0=0, h=20,
                    w=24, hs=24.0, strength=1.0, tiled=False, u8=False, out=out, out_pitch=24)

        def call(**kw):
            a = dict(good, **kw)
            ops.skylight_bake(a["src"], a["rows"], a["cols"], a["pitch"], a["table"], a["directions"], a["steps"], a["reach"],
                              a["y0"], a["x0"], a["h"], a["w"], a["hs"], a["strength"], a["tiled"], a["u8"], a["out"],
                              a["out_pitch"])
        bad = [dict(src=None), dict(table=None), dict(out=None), dict(y0=-1), dict(x0=-1), dict(y0=1), dict(x0=1),
               dict(h=21), dict(w=25), dict(h=0), dict(w=0), dict(pitch=23), dict(out_pitch=23),
               dict(rows=1 << 16, pitch=1 << 15, cols=1 << 15), dict(directions=0), dict(directions=65), dict(steps=0),
               dict(steps=257), dict(reach=0), dict(hs=0.0), dict(hs=-1.0), dict(hs=float("inf")), dict(hs=float("nan")),
               dict(strength=-0.01), dict(strength=1.01), dict(strength=float("nan")), dict(tiled=True, reach=75)]
        for kw in bad:
            for tiled in (False, True):
                with pytest.raises(GhmError, match="ghm_skylight_bake"):
                    call(**dict(dict(tiled=tiled), **kw))
        dev.sync()
        back = np.empty_like(canary)
        dev.d2h(back, out, back.nbytes)
        assert np.array_equal(back, canary)                            # nothing was written
        call()                                                         # and the arguments they vary are good ones
        dev.sync()
        dev.d2h(back, out, back.nbytes)
        assert (back == 1).all()
    finally:
        dev.sync()
        dev.free(p)
        dev.free(out)


# ---- 2. the ray caster ------------------------------------------------------------------------------------------------
VIEW = dict(max_dist=R.VIEW_KW['max_dist'], step=R.VIEW_KW['step'], sun_azimuth=R.VIEW_KW['sun_azimuth'],
            sun_elevation=R.VIEW_KW['sun_elevation'], softness=R.VIEW_KW['softness'], ambient=R.VIEW_KW['ambient'],
            haze=R.VIEW_KW['haze'], horizon=R.DEFAULT_SKY['horizon'], zenith=R.DEFAULT_SKY['zenith'])


def _camera(i):
    c = R.CAMERAS[i]
    return RN.Camera(c['pos'], c['yaw'], c['pitch'], fov=c['fov'], size=R.VIEW_SIZE)


def test_strength_zero_renders_the_bits_of_a_scene_without_sky(dev):
    hm, tex = R.terrain(0)
    with RN.Scene(hm, tex, height_scale=R.HEIGHT_SCALE, value_range=(True, True), device=dev) as plain, \
            RN.Scene(hm, tex, height_scale=R.HEIGHT_SCALE, value_range=(True, True), device=dev,
                     sky=SK.SkyLight(strength=0)) as lit:
        assert (lit.sky_plane() == 1).all()
        with pytest.raises(ValueError, match="without sky"):
            plain.sky_plane()
        for i in range(3):
            for uint8 in (False, True):
                for accel in (True, False):
                    a = plain.render(_camera(i), uint8=uint8, accel=accel, **VIEW)
                    b = lit.render(_camera(i), uint8=uint8, accel=accel, **VIEW)
                    assert np.array_equal(a, b), (i, uint8, accel)


def test_with_a_white_texture_and_full_ambient_the_image_is_the_sampled_plane(dev, ops):
    hm, _ = R.terrain(1)
    sky = SK.SkyLight()
    kw = dict(VIEW, ambient=1.0, haze=0.0)
    with RN.Scene(hm, np.ones_like(hm), height_scale=R.HEIGHT_SCALE, value_range=(True, True), device=dev, sky=sky) as lit:
        plane = lit.sky_plane()
        assert np.array_equal(plane, SK.bake(ops, hm, sky, height_scale=R.HEIGHT_SCALE)) and plane.min() < 0.9
        with RN.Scene(hm, plane, height_scale=R.HEIGHT_SCALE, value_range=(True, True), device=dev) as flat:
            for i in range(3):
                d = np.empty(R.VIEW_SIZE, np.float32)
                a = lit.render(_camera(i), uint8=False, depth=d, **kw)
                b = flat.render(_camera(i), uint8=False, **kw)
                assert np.isfinite(d).any() and np.array_equal(a, b), i        # both are ren_bil(plane, Q)


@pytest.mark.parametrize("seed,cam", [(0, 0), (1, 1), (2, 2)])
def test_a_sky_lit_view_against_the_float64_restatement(dev, seed, cam):
    hm, tex = R.terrain(seed)
    sky = SK.SkyLight()
    plane = S.bake(hm, R.HEIGHT_SCALE, np.float64)
    want, want_t = S.render_sky(hm, tex, plane, size=R.VIEW_SIZE, height_scale=R.HEIGHT_SCALE, shadows=True,
                                **R.CAMERAS[cam], **R.VIEW_KW)
    with RN.Scene(hm, tex, height_scale=R.HEIGHT_SCALE, value_range=(True, True), device=dev, sky=sky) as lit:
        assert (np.abs(lit.sky_plane() - plane) <= TOL).all()
        depth, depth0 = np.empty(R.VIEW_SIZE, np.float32), np.empty(R.VIEW_SIZE, np.float32)
        got = lit.render(_camera(cam), uint8=False, depth=depth, **VIEW)
        off = lit.render(_camera(cam), uint8=False, accel=False, depth=depth0, **VIEW)
        assert np.array_equal(got, off) and np.array_equal(depth, depth0)          # accel on equals off
        assert np.array_equal(lit.render(_camera(cam), accel=True, **VIEW), lit.render(_camera(cam), accel=False, **VIEW))
    err = np.abs(got.astype(np.float64) - want).max(0)
    bad = err > 8 * F32_DEV
    flips = np.isfinite(depth) != np.isfinite(want_t)
    allowed = int(math.floor(0.005 * bad.size))                        # §4m's share for hit / miss flips
    print("seed %d camera %d: max err %.3e, median %.3e, failing %d / %d (allowed %d), flips %d"
          % (seed, cam, err.max(), np.median(err), bad.sum(), bad.size, allowed, flips.sum()))
    assert bad.sum() <= allowed and flips.sum() <= allowed
    unlit, _ = R.reference(seed, cam, True, 'float64')
    assert np.abs(want - unlit).max() > 0.01                           # the sky light is not idle on this view


# ---- 3. the world -------------------------------------------------------------------------------------------------------
SKY = SK.SkyLight(directions=8, steps=6, step=1.5)                    # reach 10: the grown rectangle stays within a few chunks
RECT = (-37, 19, 101, 75)
MAX_DIST, HS = 40.0, 10.0
RKW = dict(sun_elevation=0.6, haze=0.003)
ERO = ER.Erosion(iterations=3, **erosion_ref.P_TEST)


@pytest.fixture(scope="module")
def small_model(dev):
    m = build_model(ostep.default_cfg(**SMALL), 5, dev, dtype="f32", use_graph=False)
    cfg = ostep.default_cfg(**SMALL)
    for s in range(3):                       # non-trivial BatchNorm running statistics (the deterministic pass reads them)
        m.z_fn(ostep.synthetic_batch(4, cfg, seed=40 + s)[0])
    return m


def _grown(rect, m):
    return rect[0] - m, rect[1] - m, rect[2] + 2 * m, rect[3] + 2 * m


def _planes(scene):
    return scene.arrays() + (scene.sky_plane(),)


@pytest.mark.parametrize("eroded", [False, True])
def test_world_scenes_are_lit_by_the_world_not_by_their_borders(small_model, eroded):
    m, r = small_model, SKY.reach
    assert r == 10
    wkw = dict(erosion=ERO) if eroded else {}
    with m.terrain_world(42, chunk_cells=2, **wkw) as world:
        with world.scene(*RECT, sky=SKY, height_scale=HS) as host:
            # no chunk was computed twice: the grown request and the scene's own share the cache
            n, e = world.computed, world.eroded
            if eroded:
                assert e == len(world._chunks) and n == len(world._raw) and e > 0
            else:
                assert n == len(world._chunks) and e == 0
            a_lo, a_hi = WD.axis_chunks(RECT[0] - r, RECT[2] + 2 * r, 64)
            b_lo, b_hi = WD.axis_chunks(RECT[1] - r, RECT[3] + 2 * r, 64)
            assert all((a, b) in world._chunks for a in range(a_lo, a_hi + 1) for b in range(b_lo, b_hi + 1))
            hh, ht, hs_ = _planes(host)
            # the plane is skylight.bake of the world's heights around the rectangle
            grown = world.heightmap(*_grown(RECT, r))[0]
            assert grown.min() >= 0 and grown.max() <= 1               # a greyscale map in [0, 1] is its own scene plane
            assert np.array_equal(hs_, m.sky_visibility(grown, SKY, height_scale=HS, margin=r))
            assert hs_.shape == RECT[2:] and hs_.min() < 1 and hs_.max() <= 1
            assert not np.array_equal(hs_, m.sky_visibility(hh, SKY, height_scale=HS))       # the borders would show
            with world.scene(*RECT, resident=True, sky=SKY, height_scale=HS) as res:
                assert (world.computed, world.eroded) == (n, e)        # warm: nothing runs
                rh, rt, rs = _planes(res)
                assert np.array_equal(rh, hh) and np.array_equal(rt, ht) and np.array_equal(rs, hs_)
                cam = RN.Camera((-20.5, 40.25, 14.0), 0.5, -0.35, fov=1.0, size=(20, 28))
                for uint8 in (False, True):
                    assert np.array_equal(res.render(cam, max_dist=MAX_DIST, uint8=uint8, **RKW),
                                          host.render(cam, max_dist=MAX_DIST, uint8=uint8, **RKW))
            with world.scene(*RECT, height_scale=HS) as dark:          # without sky the scene is what it was
                dh, dt_ = dark.arrays()
                assert np.array_equal(dh, hh) and np.array_equal(dt_, ht)
        # an overlapping scene agrees on the overlap, host and resident
        other = (-10, 60, 90, 70)
        for resident in (False, True):
            with world.scene(*other, resident=resident, sky=SKY, height_scale=HS) as sc:
                assert np.array_equal(sc.sky_plane()[:74, :34], hs_[27:, 41:])
    if eroded:
        with m.terrain_world(42, chunk_cells=2) as raw, raw.scene(*RECT, sky=SKY, height_scale=HS) as sc:
            assert not np.array_equal(sc.sky_plane(), hs_)             # an eroded world is lit as the eroded world


def test_flight_frames_are_their_windows_host_path_scenes_rendered_with_sky(small_model):
    m = small_model
    cams = [RN.Camera((-100.5 + 200.0 * i / 5, 11.25, 14.0), 0.5, -0.35, fov=1.0, size=(20, 28)) for i in range(6)]
    mb = 128 * 128 * WD.SKY_SCENE_BYTES_PER_PIXEL / float(1 << 20)
    with m.terrain_world(42, chunk_cells=2) as world:
        plan = world.flight_plan(cams, MAX_DIST, window_mb=mb, sky=SKY)
        assert len(plan) >= 2
        frames = list(world.flight(cams, MAX_DIST, window_mb=mb, height_scale=HS, sky=SKY, uint8=False, **RKW))
        assert len(frames) == 6
        # a second flight: every chunk comes from the cache, and neither a scene nor a grown height plane is left behind
        n, before = world.computed, m.device.bytes_allocated
        again = list(world.flight(cams, MAX_DIST, window_mb=mb, height_scale=HS, sky=SKY, uint8=False, **RKW))
        assert world.computed == n and m.device.bytes_allocated == before
        assert all(np.array_equal(a, b) for a, b in zip(again, frames))
        for rect, i, j in plan:
            with world.scene(*rect, sky=SKY, height_scale=HS) as sc:
                for k in range(i, j + 1):
                    want = sc.render(cams[k], max_dist=MAX_DIST, uint8=False, **RKW)
                    assert np.array_equal(frames[k], want), (k, rect)
        dark = list(world.flight(cams[:1], MAX_DIST, window_mb=mb, height_scale=HS, uint8=False, **RKW))
        assert not np.array_equal(dark[0], frames[0])
        assert np.array_equal(world.view(cams[0], MAX_DIST, height_scale=HS, sky=SKY, uint8=False, **RKW).shape, (3, 20, 28))


# ---- 4. the command line and the model's methods ----------------------------------------------------------------------
def test_command_line_and_render_terrain(tmp_path, dev, ops, small_model):
    from PIL import Image
    H, W, seed, hs, kw = S.CASES[1]
    src = S.terrain(seed, H, W)
    want = device_bake(dev, ops, src, SK.SkyLight(**kw), hs)
    np.save(tmp_path / "in.npy", src)
    for form in ([], ["--plain"], ["--tiled"]):
        assert SK.main([str(tmp_path / "in.npy"), str(tmp_path / "out.npy"), "--height-scale", str(hs)] + form) == 0
        assert np.array_equal(np.load(tmp_path / "out.npy"), want)
    assert SK.main([str(tmp_path / "in.npy"), str(tmp_path / "out.png"), "--height-scale", str(hs)]) == 0
    assert np.array_equal(np.asarray(Image.open(tmp_path / "out.png")), np.rint(want.astype(np.float64) * 255).astype(np.uint8))
    half = SK.SkyLight(strength=0.5)
    assert SK.main([str(tmp_path / "in.npy"), str(tmp_path / "out.npy"), "--height-scale", str(hs), "--strength", "0.5"]) == 0
    assert np.array_equal(np.load(tmp_path / "out.npy"), device_bake(dev, ops, src, half, hs))
    # Pix2Pix.render_terrain(sky=) is the scene's render
    m = small_model
    hm, tex = R.terrain(2)
    cam = _camera(0)
    got = m.render_terrain(hm, tex, cam, height_scale=R.HEIGHT_SCALE, sky=SKY, uint8=False, **VIEW)
    with RN.Scene(hm, tex, height_scale=R.HEIGHT_SCALE, value_range=(m.is_a_grayscale, m.is_b_grayscale), device=dev,
                  sky=SKY) as sc:
        assert np.array_equal(got, sc.render(cam, uint8=False, **VIEW))
    assert not np.array_equal(got, m.render_terrain(hm, tex, cam, height_scale=R.HEIGHT_SCALE, uint8=False, **VIEW))
