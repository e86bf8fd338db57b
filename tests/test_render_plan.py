"""The heightfield ray caster without a GPU: known answers for the host restatement (tests/render_ref.py), the
camera's footprint, the validation of Camera and of the command line, and the calibration of the GPU test's bound: what the
restatement loses when every quantity is float32."""
import math

import numpy as np
import pytest

from gan_heightmaps_amd import render as RN
from tests import render_ref as R

# The largest deviation of any channel of any pixel between the float32 and the float64 restatement on the nine views,
# shadows off and on.  Measured: 3.41e-05 (seed 1, camera 1; the same with shadows), no hit/miss flips, per-view medians
# 1.5e-07 .. 6.1e-07.  The constant leaves a factor of three for other numpy versions' sin / exp.
F32_DEV = 1e-4

KW0 = dict(sun_azimuth=0.6, sun_elevation=0.5, softness=8.0, ambient=0.25)


def test_flat_scene_hits_where_the_ray_meets_the_plane():
    hm = np.full((128, 128), 0.5)
    tex = np.full((3, 128, 128), 0.5)
    pos, size = (32.3, 40.2, 40.0), (24, 32)
    yaw, pitch, fov = 0.3, -0.6, 0.9
    _, t = R.render(hm, tex, pos, yaw, pitch, fov, size, 24.0, max_dist=150.0, shadows=False, haze=0.0, **KW0)
    d = R.rays(yaw, pitch, fov, size)
    want = (12.0 - pos[2]) / d[..., 2]
    q = np.asarray(pos) + want[..., None] * d
    inside = (q[..., 0] > 1) & (q[..., 0] < 127) & (q[..., 1] > 1) & (q[..., 1] < 127) & (want < 149)
    assert inside.mean() > 0.5
    assert np.abs(t[inside] - want[inside]).max() < 1e-12


def test_nadir_camera_over_a_ramp_gives_texture_times_lambert():
    H = W = 96
    hs = 30.0
    hm = np.broadcast_to(0.5 * np.arange(W) / (W - 1.0), (H, W)).copy()
    rng = np.random.RandomState(3)
    tex = rng.uniform(0, 1, (3, H, W))
    pos, size, fov = (48.0, 47.0, 200.0), (16, 20), 0.3
    img, t = R.render(hm, tex, pos, 0.0, -math.pi / 2, fov, size, hs, max_dist=250.0, shadows=False, haze=0.0, **KW0)
    d = R.rays(0.0, -math.pi / 2, fov, size)
    c = hs * 0.5 / (W - 1.0)                              # h = c (x - 0.5) between the first and the last pixel centre
    want_t = (c * (pos[1] - 0.5) - pos[2]) / (d[..., 2] - c * d[..., 1])
    assert np.abs(t - want_t).max() < 1e-9
    q = np.asarray(pos) + want_t[..., None] * d
    s = R.sun_vector(KW0['sun_azimuth'], KW0['sun_elevation'])
    lambert = (-c * s[1] + s[2]) / math.sqrt(c * c + 1.0)
    want = R.bilinear(tex, q[..., 0], q[..., 1]) * (0.25 + 0.75 * lambert)
    assert np.abs(img - want).max() < 1e-9


def test_west_is_on_the_right_of_a_south_facing_camera():
    hm = np.zeros((64, 64))
    tex = np.zeros((3, 64, 64))
    tex[:, 40, 22] = 1.0                                   # west (a smaller column) of the camera's axis at x = 32
    img, t = R.render(hm, tex, (10.0, 32.0, 20.0), 0.0, -0.6, 1.0, (32, 48), 10.0, max_dist=100.0, shadows=False,
                      haze=0.0, sun_azimuth=0.0, sun_elevation=math.pi / 2, softness=8.0, ambient=1.0)
    ground = np.where(np.isfinite(t), img[0], 0.0)                             # the sky is brighter than black ground
    v, u = np.unravel_index(np.argmax(ground), ground.shape)
    assert ground[v, u] > 0.2
    assert u >= 24 and ground[:, :24].max() == 0.0


def test_a_ray_that_starts_below_the_surface_hits_at_once():
    hm = np.full((32, 32), 0.5)
    tex = np.full((3, 32, 32), 0.5)
    _, t = R.render(hm, tex, (16.0, 16.0, 3.0), 0.4, 0.2, 1.0, (6, 8), 24.0, max_dist=40.0, shadows=False, **KW0)
    assert (t == 0).all()


def test_a_camera_outside_sees_terrain_only_after_entering():
    hm = np.full((64, 64), 0.25)
    tex = np.full((3, 64, 64), 0.5)
    size = (12, 16)
    # above the plane (z = 6): every hit point lies inside the rectangle
    pos = (-30.0, 32.0, 20.0)
    _, t = R.render(hm, tex, pos, 0.0, -0.3, 0.8, size, 24.0, max_dist=200.0, shadows=False, **KW0)
    d = R.rays(0.0, -0.3, 0.8, size)
    hit = np.isfinite(t)
    assert hit.any()
    q = np.asarray(pos) + np.where(hit, t, 0.0)[..., None] * d
    assert (q[hit][:, 0] >= 0).all() and (q[hit][:, 0] <= 64).all()
    # below the plane's height: the first sample inside the rectangle hits, with no finite sample before it -- t_hit is
    # that sample's t_k, and it lies past the border
    pos = (-30.0, 32.0, 2.0)
    _, t = R.render(hm, tex, pos, 0.0, 0.0, 0.5, size, 8.0 * 24.0, step=0.37, max_dist=200.0, shadows=False, **KW0)
    assert np.isfinite(t).all()
    d = R.rays(0.0, 0.0, 0.5, size)
    k = t / 0.37
    assert np.abs(k - np.rint(k)).max() < 1e-9
    y = pos[0] + t * d[..., 0]
    assert (y >= 0).all() and (y - 0.37 * d[..., 0] < 0).all()


def test_shadow_of_a_wall_and_open_ground():
    hm = np.zeros((96, 96))
    hm[:, 60:64] = 1.0
    s = R.sun_vector(math.pi / 2, 0.2)                      # low, along the columns
    Q = np.array([[48.0, 40.0, 0.0], [48.0, 80.0, 0.0]])    # behind the wall as seen from the sun; past it
    sh = R.shadow_factor(hm, 24.0, Q, s, 0.5, 150.0, 8.0)
    assert sh[0] == 0.0 and sh[1] == 1.0
    assert R.shadow_factor(hm, 24.0, np.array([[48.0, 95.9, 0.0]]), s, 0.5, 0.4, 8.0)[0] == 1.0      # no samples at all


def test_footprint_holds_every_sample_of_every_ray():
    rng = np.random.RandomState(11)
    for i in range(40):
        pos = tuple(rng.uniform(-300, 300, 2)) + (rng.uniform(0, 80),)
        size = (int(rng.randint(1, 9)), int(rng.randint(1, 9)))
        cam = RN.Camera(pos, rng.uniform(-4, 4), rng.uniform(-math.pi / 2, math.pi / 2), fov=rng.uniform(0.2, 2.6), size=size)
        max_dist, step = rng.uniform(1, 200), rng.choice([0.5, 0.37, 1.0])
        y0, x0, h, w = cam.footprint(max_dist)
        assert all(isinstance(v, int) for v in (y0, x0, h, w))
        d = R.rays(cam.yaw, cam.pitch, cam.fov, cam.size).reshape(-1, 3)
        t = np.arange(R.n_steps(max_dist, step) + 1) * step
        P = np.asarray(cam.pos)[None, None, :] + t[None, :, None] * d[:, None, :]
        assert P[..., 0].min() >= y0 + 1 and P[..., 0].max() <= y0 + h - 1, i
        assert P[..., 1].min() >= x0 + 1 and P[..., 1].max() <= x0 + w - 1, i
    # the far end of a bundle of rays bulges beyond its corners: the axis reaches max_dist, the corners stop short of it
    cam = RN.Camera((0.0, 0.0, 5.0), 0.0, 0.0, fov=1.5, size=(8, 8))
    y0, x0, h, w = cam.footprint(100.0)
    assert y0 + h >= 102
    assert RN.union_footprint([(0, 0, 4, 4), (-3, 2, 5, 9)]) == (-3, 0, 7, 11)


def test_camera_validation():
    ok = RN.Camera((1, 2.5, 3), 0.1, -0.2, fov=1.0, size=(4, 6))
    assert ok.pos == (1.0, 2.5, 3.0) and ok.size == (4, 6)
    for kw in (dict(pos=(1, 2)), dict(pos=(1, 2, float('nan'))), dict(pos=5), dict(yaw=float('inf')), dict(pitch=2.0),
               dict(pitch="x"), dict(fov=0.0), dict(fov=math.pi), dict(fov=-1), dict(size=(0, 4)), dict(size=(4,)),
               dict(size=(4.0, 4)), dict(size=(1 << 16, 1 << 15)), dict(pos=(True, 0, 0))):
        args = dict(pos=(0, 0, 1), yaw=0.0, pitch=0.0, fov=1.0, size=(4, 4))
        args.update(kw)
        with pytest.raises(ValueError):
            RN.Camera(**args)
    with pytest.raises(ValueError):
        RN.Camera.look_at((1, 2, 3), (1, 2, 3))
    with pytest.raises(ValueError):
        ok.footprint(0)
    cam = RN.Camera.look_at((10.0, 10.0, 30.0), (40.0, 50.0, 5.0), size=(6, 8))
    fw = cam.basis()[0]
    want = np.array([30.0, 40.0, -25.0])
    assert np.allclose(fw, want / np.linalg.norm(want), atol=1e-12)
    down = RN.Camera.look_at((3.0, 4.0, 9.0), (3.0, 4.0, 0.0))
    assert down.pitch == -math.pi / 2
    # the camera's basis is the restatement's
    for a, b in zip(cam.basis(), R.basis(cam.yaw, cam.pitch)):
        assert np.array_equal(a, b)


def test_command_line_parsing():
    a = RN.parse_args(["o.png", "--heightmap", "h.png", "--texture", "t.npy", "--pos", "-3,4.5,60", "--look-at", "100,100,0",
                       "--size", "90x120", "--sun", "-120,30", "--no-shadows"])
    assert a.pos == (-3.0, 4.5, 60.0) and a.look_at == (100.0, 100.0, 0.0) and a.size == (90, 120) and a.no_shadows
    assert a.sun == (-120.0, 30.0) and a.frames is None
    assert RN.frame_names(a) == ["o.png"] and len(RN.cameras_of(a)) == 1
    a = RN.parse_args(["out.png", "--world", "exp", "model.npz", "--seed", "7", "--max-dist", "300", "--pos", "0,0,50",
                       "--yaw", "-45", "--pitch", "-20", "--frames", "3", "--to", "-100,0,50", "--chunk-cells", "2"])
    assert a.world == ["exp", "model.npz"] and a.seed == 7 and a.yaw == -45.0 and a.to == (-100.0, 0.0, 50.0)
    cams = RN.cameras_of(a)
    assert [c.pos for c in cams] == [(0.0, 0.0, 50.0), (-50.0, 0.0, 50.0), (-100.0, 0.0, 50.0)]
    assert abs(cams[0].yaw + math.pi / 4) < 1e-15 and cams[0].size == RN.DEFAULTS['size']
    assert RN.frame_names(a) == ["out_0000.png", "out_0001.png", "out_0002.png"]
    base = ["o.png", "--heightmap", "h.png", "--texture", "t.png", "--pos", "1,2,3"]
    for bad in (base,                                                         # no direction
                base + ["--yaw", "10"],                                       # no pitch
                base + ["--yaw", "10", "--pitch", "5", "--look-at", "1,1,1"],
                base + ["--look-at", "1,2,3"],
                base + ["--look-at", "5,5,0", "--seed", "3"],
                base + ["--look-at", "5,5,0", "--frames", "3"],
                base + ["--look-at", "5,5,0", "--frames", "1", "--to", "1,1,1"],
                base + ["--look-at", "5,5,0", "--fov", "180"],
                base + ["--look-at", "5,5,0", "--step", "0"],
                base + ["--look-at", "5,5,0", "--size", "10"],
                base + ["--look-at", "5,5"],
                ["o.png", "--heightmap", "h.png", "--pos", "1,2,3", "--look-at", "5,5,0"],
                ["o.png", "--pos", "1,2,3", "--look-at", "5,5,0"],
                ["o.png", "--world", "e", "m", "--pos", "1,2,3", "--look-at", "5,5,0", "--max-dist", "10"],      # no seed
                ["o.png", "--world", "e", "m", "--seed", "1", "--pos", "1,2,3", "--look-at", "5,5,0"],          # no max-dist
                ["o.jpg", "--heightmap", "h.png", "--texture", "t.png", "--pos", "1,2,3", "--look-at", "5,5,0"]):
        with pytest.raises(SystemExit):
            RN.parse_args(bad)


def test_float32_restatement_stays_within_the_calibrated_bound():
    worst = 0.0
    for shadows in (False, True):
        for seed, cam in R.views():
            a, ta = R.reference(seed, cam, shadows, 'float64')
            b, tb = R.reference(seed, cam, shadows, 'float32')
            assert b.dtype == np.float32 and tb.dtype == np.float32
            assert np.array_equal(np.isfinite(ta), np.isfinite(tb)), (seed, cam)            # no hit / miss flips
            dev = float(np.abs(a - b).max())
            print("seed %d camera %d shadows %d: max |f32 - f64| = %.3e" % (seed, cam, shadows, dev))
            worst = max(worst, dev)
            assert dev <= F32_DEV, (seed, cam, shadows, dev)
    print("worst: %.3e (F32_DEV = %.1e)" % (worst, F32_DEV))
    # the shadow march is not idle on these views
    lit, _ = R.reference(0, 0, False, 'float64')
    dark, _ = R.reference(0, 0, True, 'float64')
    assert (dark <= lit + 1e-15).all() and (lit - dark).max() > 0.05
