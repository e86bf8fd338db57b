"""Host restatement of the heightfield ray caster, written from the definition: numpy, vectorised over the rays
of an image, with its own plain loop over the samples k.  Every quantity is kept in ``dtype`` (float64 or float32), so the
float32 run shows what the number format alone costs (tests/test_render_plan.py calibrates the GPU test's bound with it).

Axes are (y, x, z): y down the rows, x along the columns, z up.  Also here: the nine views both test files use.
"""
import functools
import math

import numpy as np

DEFAULT_SKY = dict(horizon=(0.80, 0.86, 0.92), zenith=(0.30, 0.50, 0.85))


def bilinear(img, y, x):
    """img [..., H, W] sampled at the positions (y, x) (arrays of one shape): moved by -0.5, clamped to the pixel centres"""
    dt = y.dtype.type
    H, W = img.shape[-2:]
    fy = np.clip(y - dt(0.5), dt(0), dt(H - 1))
    fx = np.clip(x - dt(0.5), dt(0), dt(W - 1))
    i0 = np.floor(fy).astype(np.int64)
    j0 = np.floor(fx).astype(np.int64)
    i1 = np.minimum(i0 + 1, H - 1)
    j1 = np.minimum(j0 + 1, W - 1)
    wy = fy - i0.astype(y.dtype)
    wx = fx - j0.astype(y.dtype)
    top = img[..., i0, j0] + wx * (img[..., i0, j1] - img[..., i0, j0])
    bot = img[..., i1, j0] + wx * (img[..., i1, j1] - img[..., i1, j0])
    return top + wy * (bot - top)


def basis(yaw, pitch, dtype=np.float64):
    """(forward, right, up) of a camera"""
    cy, sy, cp, sp = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch)
    return (np.array([cp * cy, cp * sy, sp], dtype), np.array([sy, -cy, 0.0], dtype),
            np.array([-sp * cy, -sp * sy, cp], dtype))


def rays(yaw, pitch, fov, size, dtype=np.float64):
    """unit directions [Hi, Wi, 3] of the image's pixels"""
    dt = np.dtype(dtype).type
    Hi, Wi = size
    fw, rt, up = basis(yaw, pitch, dtype)
    f = dt((Hi / 2.0) / math.tan(fov / 2.0))
    a = (np.arange(Wi).astype(dtype) + dt(0.5) - dt(Wi / 2.0))[None, :, None]
    b = (np.arange(Hi).astype(dtype) + dt(0.5) - dt(Hi / 2.0))[:, None, None]
    d = f * fw + a * rt - b * up
    return d / np.sqrt((d * d).sum(-1, keepdims=True))


def sun_vector(azimuth, elevation, dtype=np.float64):
    ce = math.cos(elevation)
    return np.array([ce * math.cos(azimuth), ce * math.sin(azimuth), math.sin(elevation)], dtype)


def n_steps(max_dist, step):
    return int(math.floor(max_dist / step))


def march(hm, height_scale, o, d, step, max_dist):
    """o [3], d [n, 3] -> (t_hit [n], +inf where the ray hits nothing; k_hit [n], -1 likewise)"""
    dtype = d.dtype
    dt = dtype.type
    H, W = hm.shape
    n = d.shape[0]
    hs, stp = dt(height_scale), dt(step)
    t_hit = np.full(n, np.inf, dtype)
    k_hit = np.full(n, -1, np.int64)
    g_prev = np.full(n, np.inf, dtype)
    live = np.arange(n)
    for k in range(n_steps(max_dist, step) + 1):
        if live.size == 0:
            break
        t = dt(k) * stp
        P = o + t * d[live]
        y, x, z = P[:, 0], P[:, 1], P[:, 2]
        inside = (y >= 0) & (y <= H) & (x >= 0) & (x <= W)
        g = np.full(live.size, np.inf, dtype)
        g[inside] = z[inside] - hs * bilinear(hm, y[inside], x[inside])
        hit = g <= 0
        if hit.any():
            gp, gh = g_prev[live][hit], g[hit]
            th = np.full(gh.size, t, dtype)
            sec = np.isfinite(gp) & (k > 0)
            th[sec] = dt(k - 1) * stp + stp * gp[sec] / (gp[sec] - gh[sec])
            t_hit[live[hit]] = th
            k_hit[live[hit]] = k
        g_prev[live] = g
        live = live[~hit]
    return t_hit, k_hit


def shadow_factor(hm, height_scale, Q, s, step, max_dist, softness):
    """Q [n, 3] hit points, s [3] unit sun vector -> clamp(softness min_m (z_m - h_m) / (m step), 0, 1), 1 without samples"""
    dtype = Q.dtype
    dt = dtype.type
    H, W = hm.shape
    hs, stp = dt(height_scale), dt(step)
    lo = np.full(Q.shape[0], np.inf, dtype)
    live = np.arange(Q.shape[0])
    for m in range(1, n_steps(max_dist, step) + 1):
        if live.size == 0:
            break
        t = dt(m) * stp
        P = Q[live] + t * s
        y, x, z = P[:, 0], P[:, 1], P[:, 2]
        go = (y >= 0) & (y <= H) & (x >= 0) & (x <= W) & (z <= hs)
        live, y, x, z = live[go], y[go], x[go], z[go]
        lo[live] = np.minimum(lo[live], (z - hs * bilinear(hm, y, x)) / t)
    out = np.ones(Q.shape[0], dtype)
    some = np.isfinite(lo)
    out[some] = np.clip(dt(softness) * lo[some], dt(0), dt(1))
    return out


def render(hm, tex, pos, yaw, pitch, fov, size, height_scale, step=0.5, max_dist=150.0, sun_azimuth=0.6, sun_elevation=0.5,
           shadows=True, softness=8.0, ambient=0.25, haze=0.002, horizon=DEFAULT_SKY['horizon'],
           zenith=DEFAULT_SKY['zenith'], dtype=np.float64):
    """-> (image [3, Hi, Wi], t_hit [Hi, Wi] with +inf for sky), both ``dtype``.  hm [H, W] and tex [3, H, W] in [0, 1]."""
    dtype = np.dtype(dtype)
    dt = dtype.type
    hm = np.asarray(hm, dtype)
    tex = np.asarray(tex, dtype)
    Hi, Wi = size
    o = np.asarray(pos, dtype)
    d = rays(yaw, pitch, fov, size, dtype).reshape(-1, 3)
    hs = dt(height_scale)
    hor, zen = np.asarray(horizon, dtype), np.asarray(zenith, dtype)
    sky = hor[None, :] + np.maximum(d[:, 2], dt(0))[:, None] * (zen - hor)[None, :]
    t_hit, _ = march(hm, height_scale, o, d, step, max_dist)
    img = sky.copy()
    idx = np.nonzero(np.isfinite(t_hit))[0]
    if idx.size:
        th = t_hit[idx]
        Q = o + th[:, None] * d[idx]
        qy, qx = Q[:, 0], Q[:, 1]
        one = dt(1)
        gy = hs * (bilinear(hm, qy + one, qx) - bilinear(hm, qy - one, qx)) / dt(2)
        gx = hs * (bilinear(hm, qy, qx + one) - bilinear(hm, qy, qx - one)) / dt(2)
        s = sun_vector(sun_azimuth, sun_elevation, dtype)
        ndots = (-gy * s[0] - gx * s[1] + s[2]) / np.sqrt(gy * gy + gx * gx + one)
        sh = shadow_factor(hm, height_scale, Q, s, step, max_dist, softness) if shadows else np.ones(idx.size, dtype)
        shade = dt(ambient) + (one - dt(ambient)) * np.maximum(ndots, dt(0)) * sh
        c = bilinear(tex, qy, qx).T * shade[:, None]
        F = one - np.exp(-dt(haze) * th)
        img[idx] = c * (one - F)[:, None] + sky[idx] * F[:, None]
    return img.T.reshape(3, Hi, Wi).astype(dtype), t_hit.reshape(Hi, Wi)


def to_uint8(img):
    """[3, Hi, Wi] -> uint8 [Hi, Wi, 3], round(255 clamp(c, 0, 1)) half to even"""
    return np.rint(np.clip(np.asarray(img, np.float64), 0, 1) * 255.0).astype(np.uint8).transpose(1, 2, 0)


# ---- the nine views of the parity tests: three smooth terrains x three cameras ------------------------------------------
SCENE_N = 128
HEIGHT_SCALE = 24.0
VIEW_SIZE = (48, 64)
VIEW_KW = dict(step=0.5, max_dist=150.0, sun_azimuth=0.6, sun_elevation=0.5, softness=8.0, ambient=0.25, haze=0.002)
CAMERAS = (dict(pos=(10.3, 64.2, 40.0), yaw=0.1, pitch=-0.45, fov=1.0),
           dict(pos=(64.5, 20.1, 25.0), yaw=1.3, pitch=-0.2, fov=1.2),
           dict(pos=(64.0, 64.0, 60.0), yaw=0.7, pitch=-1.4, fov=1.0))
SEEDS = (0, 1, 2)


@functools.lru_cache(maxsize=None)
def terrain(seed, H=SCENE_N, W=SCENE_N):
    """(hm [H, W], tex [3, H, W]) float32: 12 random sinusoids normalised to [0, 1], and uniform noise"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    hm = np.zeros((H, W))
    for _ in range(12):
        fy, fx = rng.uniform(-0.12, 0.12, 2)
        hm += rng.uniform(0.3, 1.0) * np.sin(fy * yy + fx * xx + rng.uniform(0, 2 * np.pi))
    hm = (hm - hm.min()) / max(hm.max() - hm.min(), 1e-12)
    tex = rng.uniform(0, 1, (3, H, W))
    hm, tex = hm.astype(np.float32), tex.astype(np.float32)
    hm.setflags(write=False)
    tex.setflags(write=False)
    return hm, tex


def views():
    """[(seed, camera index)] of the nine views"""
    return [(s, c) for s in SEEDS for c in range(len(CAMERAS))]


@functools.lru_cache(maxsize=None)
def reference(seed, cam, shadows, dtype_name):
    """(image, t_hit) of one of the nine views from the restatement; computed once per process, read-only"""
    hm, tex = terrain(seed)
    img, t = render(hm, tex, size=VIEW_SIZE, height_scale=HEIGHT_SCALE, shadows=shadows, dtype=np.dtype(dtype_name),
                    **CAMERAS[cam], **VIEW_KW)
    img.setflags(write=False)
    t.setflags(write=False)
    return img, t
