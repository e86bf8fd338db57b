"""Host restatement of the sky-light bake (gan_heightmaps_amd/skylight.py, csrc/skylight.hip), written from the
definition: numpy, vectorised over the texels of a plane, with its own plain loops over the directions and the samples.  Every
quantity is kept in ``dtype``: float64 is the reference, float32 the kernels' arithmetic (every operation rounded on its own,
in the order of the definition).  The table of samples is rebuilt here, entry by entry, independently of skylight.py.  Also
here: the cases the tests share, and the float64 restatement of a sky-lit render on tests/render_ref.py's parts.
"""
import functools
import math

import numpy as np

from tests import erosion_ref
from tests import render_ref as R

DEFAULTS = dict(directions=16, steps=24, step=1.5, strength=1.0)


def table(directions, steps, step):
    """[(iy, ix, wy, wx, inv_r)] per direction, per sample: Python ints and numpy float32s"""
    out = []
    for d in range(directions):
        phi = 2.0 * math.pi * d / directions
        row = []
        for m in range(1, steps + 1):
            r = m * float(step)
            oy, ox = r * math.cos(phi), r * math.sin(phi)
            iy, ix = math.floor(oy), math.floor(ox)
            row.append((int(iy), int(ix), np.float32(oy - iy), np.float32(ox - ix), np.float32(1.0 / r)))
        out.append(row)
    return out


def reach(tab):
    return max(max(-iy, iy + 1, -ix, ix + 1) for row in tab for iy, ix, _, _, _ in row)


def bake(plane, height_scale, dtype, margin=0, directions=16, steps=24, step=1.5, strength=1.0):
    """the sky light of the interior of ``plane`` ((H + 2 margin, W + 2 margin), values in [0, 1]) in ``dtype`` arithmetic;
    indices are clamped to the plane"""
    dtype = np.dtype(dtype)
    dt = dtype.type
    p = np.asarray(plane, np.float32).astype(dtype)
    rows, cols = p.shape
    H, W = rows - 2 * margin, cols - 2 * margin
    i, j = np.mgrid[margin:margin + H, margin:margin + W]

    def at(y, x):
        return p[np.clip(y, 0, rows - 1), np.clip(x, 0, cols - 1)]
    h0 = at(i, j)
    hs = dt(height_scale)
    total = np.zeros((H, W), dtype)
    for row in table(directions, steps, step):
        T = np.zeros((H, W), dtype)
        for iy, ix, wy, wx, inv_r in row:
            wy, wx, inv_r = dt(wy), dt(wx), dt(inv_r)
            a, b, c, e = at(i + iy, j + ix), at(i + iy, j + ix + 1), at(i + iy + 1, j + ix), at(i + iy + 1, j + ix + 1)
            t = a + wx * (b - a)
            u = c + wx * (e - c)
            hv = t + wy * (u - t)
            T = np.maximum(T, (hv - h0) * inv_r)
        q = hs * T
        total = total + dt(1) / (dt(1) + q * q)
    V = total / dt(directions)
    out = dt(1) - dt(strength) * (dt(1) - V)
    assert out.dtype == dtype
    return out


@functools.lru_cache(maxsize=None)
def terrain(seed, H, W):
    """tests/erosion_ref.terrain as the float32 plane the device reads; read-only"""
    t = erosion_ref.terrain(seed, H, W).astype(np.float32)
    t.setflags(write=False)
    return t


# (H, W, seed, height_scale, SkyLight arguments): the cases of the device and host-build tests.  48 x 40 and 70 x 33 have
# partial 32 x 32 tiles in both axes; 5 x 90 is narrower than the reach (37), so it clamps on both sides at once
CASES = ((33, 70, 3, 64.0, dict(directions=8, steps=6, step=1.0)),
         (48, 40, 4, 24.0, {}),
         (70, 33, 5, 24.0, {}),
         (5, 90, 6, 24.0, {}))


@functools.lru_cache(maxsize=None)
def reference(case, dtype_name):
    """bake of CASES[case] in float64 or float32; computed once per process, read-only"""
    H, W, seed, hs, kw = CASES[case]
    out = bake(terrain(seed, H, W), hs, np.dtype(dtype_name), **dict(DEFAULTS, **kw))
    out.setflags(write=False)
    return out


def render_sky(hm, tex, sky, pos, yaw, pitch, fov, size, height_scale, step=0.5, max_dist=150.0, sun_azimuth=0.6,
               sun_elevation=0.5, shadows=True, softness=8.0, ambient=0.25, haze=0.002, horizon=R.DEFAULT_SKY['horizon'],
               zenith=R.DEFAULT_SKY['zenith'], dtype=np.float64):
    """tests/render_ref.render with the light of the sky: shade = ambient sky(Q) + (1 - ambient) max(0, n.s) shadow, sky(Q) the
    bilinear sample of the baked plane ``sky`` [H, W] at the hit.  -> (image [3, Hi, Wi], t_hit [Hi, Wi])"""
    dtype = np.dtype(dtype)
    dt = dtype.type
    hm, tex, sky = np.asarray(hm, dtype), np.asarray(tex, dtype), np.asarray(sky, dtype)
    Hi, Wi = size
    o = np.asarray(pos, dtype)
    d = R.rays(yaw, pitch, fov, size, dtype).reshape(-1, 3)
    hs = dt(height_scale)
    hor, zen = np.asarray(horizon, dtype), np.asarray(zenith, dtype)
    back = hor[None, :] + np.maximum(d[:, 2], dt(0))[:, None] * (zen - hor)[None, :]
    t_hit, _ = R.march(hm, height_scale, o, d, step, max_dist)
    img = back.copy()
    idx = np.nonzero(np.isfinite(t_hit))[0]
    if idx.size:
        th = t_hit[idx]
        Q = o + th[:, None] * d[idx]
        qy, qx = Q[:, 0], Q[:, 1]
        one = dt(1)
        gy = hs * (R.bilinear(hm, qy + one, qx) - R.bilinear(hm, qy - one, qx)) / dt(2)
        gx = hs * (R.bilinear(hm, qy, qx + one) - R.bilinear(hm, qy, qx - one)) / dt(2)
        s = R.sun_vector(sun_azimuth, sun_elevation, dtype)
        ndots = (-gy * s[0] - gx * s[1] + s[2]) / np.sqrt(gy * gy + gx * gx + one)
        sh = R.shadow_factor(hm, height_scale, Q, s, step, max_dist, softness) if shadows else np.ones(idx.size, dtype)
        shade = dt(ambient) * R.bilinear(sky, qy, qx) + (one - dt(ambient)) * np.maximum(ndots, dt(0)) * sh
        c = R.bilinear(tex, qy, qx).T * shade[:, None]
        F = one - np.exp(-dt(haze) * th)
        img[idx] = c * (one - F)[:, None] + back[idx] * F[:, None]
    return img.T.reshape(3, Hi, Wi).astype(dtype), t_hit.reshape(Hi, Wi)
