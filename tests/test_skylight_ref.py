"""The sky-light bake's restatement (tests/skylight_ref.py) against known answers, the table and its reach, the
window independence the world's scenes rest on, and the calibration of the device tests' bound.  No GPU."""
import math

import numpy as np
import pytest

from gan_heightmaps_amd import skylight as SK
from tests import skylight_ref as S

# The largest |float32 - float64| of the restatement on any texel of the four cases of the device test (S.CASES).
# Measured: 3.38e-07 (33 x 70 with 8 directions of 6 steps at height_scale 64); the default cases give 1.7e-07 .. 2.2e-07.
# The constant leaves a factor of three for other numpy versions.
SKY_F32_DEV = 1e-6


def test_a_flat_plane_sees_the_whole_sky():
    for dtype in (np.float32, np.float64):
        assert (S.bake(np.full((9, 13), 0.4, np.float32), 64.0, dtype) == 1).all()


def test_strength_zero_gives_one_and_strength_scales_the_loss():
    t = S.terrain(1, 20, 24)
    assert (S.bake(t, 64.0, np.float64, strength=0.0) == 1).all() and (S.bake(t, 64.0, np.float32, strength=0.0) == 1).all()
    full, half = S.bake(t, 64.0, np.float64), S.bake(t, 64.0, np.float64, strength=0.5)
    assert full.min() < 0.9 and np.allclose(1 - half, 0.5 * (1 - full), rtol=0, atol=1e-15)


def test_an_infinite_ramp_gives_the_closed_form():
    """p = c + g x on a plane wide enough that no sample is clamped: the bilinear sample is exact, so towards azimuth phi
    every sample has the slope g sin(phi) and vis = 1 / (1 + (height_scale max(0, g sin phi))^2)"""
    g, hs, D = 0.004, 30.0, 12
    sky = dict(directions=D, steps=5, step=1.7)
    m = S.reach(S.table(**sky))
    plane = (0.2 + g * np.arange(8 + 2 * m))[None, :].repeat(6 + 2 * m, 0)
    want = sum(1.0 / (1.0 + (hs * max(0.0, g * math.sin(2 * math.pi * d / D))) ** 2) for d in range(D)) / D
    got = S.bake(plane, hs, np.float64, margin=m, **sky)
    assert got.shape == (6, 8) and np.abs(got - want).max() < 2e-7      # the plane itself is rounded to float32
    assert 0.99 < want < 1.0
    # and along y
    assert np.abs(S.bake(plane.T, hs, np.float64, margin=m, **sky) - want).max() < 2e-7


def test_a_pits_floor_is_darker_than_its_rim():
    yy, xx = np.mgrid[0:65, 0:65]
    r = np.hypot(yy - 32, xx - 32)
    plane = np.where(r < 10, 0.2, 0.6).astype(np.float32)
    out = S.bake(plane, 32.0, np.float64)
    assert out[32, 32] < 0.5 < out[32, 32 + 11] and out[32, 32 + 11] == 1.0 and out[32, 32] == out[32:33, 32:33].min()
    assert out[32, 32] < out[32, 38] or out[32, 38] < out[32, 32 + 11]           # darker inside than on the rim, everywhere
    assert out[r < 10].max() < out[(r >= 10) & (r < 12)].min()


@pytest.mark.parametrize("kw", [dict(), dict(directions=8, steps=6, step=1.0), dict(directions=5, steps=7, step=0.3),
                                dict(directions=64, steps=3, step=2.9), dict(directions=1, steps=1, step=4.0)])
def test_the_table_and_its_reach(kw):
    sky = SK.SkyLight(**kw)
    tab, ref = sky.table(), S.table(sky.directions, sky.steps, sky.step)
    assert tab.shape == (sky.directions, sky.steps) and tab.dtype == SK.SAMPLE_DTYPE and tab.dtype.itemsize == 20
    for d in range(sky.directions):
        for m in range(sky.steps):
            assert tuple(tab[d, m]) == ref[d][m]
    # (an offset a rounding error below an integer has the float32 weight 1: the sample is the next pixel, as it should be)
    assert ((tab["wy"] >= 0) & (tab["wy"] <= 1) & (tab["wx"] >= 0) & (tab["wx"] <= 1)).all()
    # reach is the table's extent: the largest index distance any entry reads, not ceil(steps step) + 1
    far = max(max(abs(iy), abs(iy + 1), abs(ix), abs(ix + 1)) for row in ref for iy, ix, _, _, _ in row)
    assert sky.reach == S.reach(ref) == far
    assert sky.reach <= math.ceil(sky.steps * sky.step) + 1


def test_the_default_reach_and_the_overshoot_of_the_ceiling():
    assert SK.SkyLight().reach == 37 == math.ceil(24 * 1.5) + 1
    assert SK.SkyLight(directions=8, steps=6, step=1.0).reach == 7
    assert SK.SkyLight(directions=4, steps=3, step=1.4).reach == 5 < math.ceil(3 * 1.4) + 1          # 4.2 reads columns 4, 5


@pytest.mark.parametrize("kw,hs", [(dict(), 24.0), (dict(directions=8, steps=6, step=1.0), 64.0)])
def test_a_window_with_a_halo_of_reach_gives_the_larger_maps_interior_bit_for_bit(kw, hs):
    sky = dict(S.DEFAULTS, **kw)
    m = S.reach(S.table(sky["directions"], sky["steps"], sky["step"]))
    big = S.terrain(7, 60 + 2 * m, 50 + 2 * m)
    whole = S.bake(big, hs, np.float32, **sky)
    y0, x0, h, w = m + 9, m + 4, 23, 31                               # a rectangle at least ``reach`` from every edge
    win = S.bake(big[y0 - m:y0 + h + m, x0 - m:x0 + w + m], hs, np.float32, margin=m, **sky)
    assert win.dtype == np.float32 and np.array_equal(win, whole[y0:y0 + h, x0:x0 + w])
    # with half the halo the clamping shows
    k = m // 2
    short = S.bake(big[y0 - k:y0 + h + k, x0 - k:x0 + w + k], hs, np.float32, margin=k, **sky)
    assert short.shape == win.shape and not np.array_equal(short, win)


def test_float32_stays_within_the_calibrated_bound_of_float64():
    worst = 0.0
    for c in range(len(S.CASES)):
        a, b = S.reference(c, 'float64'), S.reference(c, 'float32')
        assert a.dtype == np.float64 and b.dtype == np.float32 and a.shape == S.CASES[c][:2]
        dev = float(np.abs(a - b).max())
        print("case %d %s: max |f32 - f64| = %.3e, mean %.3f, min %.3f" % (c, S.CASES[c][:2], dev, a.mean(), a.min()))
        worst = max(worst, dev)
        assert dev <= SKY_F32_DEV, (c, dev)
        assert 0.0 < a.min() < 0.6 and 0.5 < a.mean() < 0.9 and a.max() <= 1.0       # the bake is not idle on these planes
    print("worst: %.3e (SKY_F32_DEV = %.1e)" % (worst, SKY_F32_DEV))
    assert worst >= SKY_F32_DEV / 30                                   # the constant is of the measured order
