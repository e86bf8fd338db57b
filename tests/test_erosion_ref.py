"""The erosion model's host restatement (tests/erosion_ref.py) held to the model's own properties: a flat
ground stays flat, water is conserved, the model has no preferred axis, N iterations reach exactly 3 N cells, and the
float32 arithmetic stays within F32_DEV of the float64 one on the cases the device tests run."""
import numpy as np
import pytest

from tests import erosion_ref as R

P = R.P_TEST
TILE = (16, 64)              # GHM_EROSION_TILE_H x GHM_EROSION_TILE_W (tests/test_gpu_erosion.py checks the library's)

# (H, W, iterations, terrain seed): what tests/test_gpu_erosion.py runs on the device
CASES = [(1, 1, 2, 1), (7, 5, 3, 2), (33, 31, 4, 3), (67, 129, 8, 4), (64, 64, 32, 5),
         (TILE[0] - 1, TILE[1] + 1, 3, 6), (TILE[0], TILE[1], 3, 7), (2 * TILE[0] + 1, 2 * TILE[1] - 1, 3, 8)]

# The largest deviation of b, d or s (height units, ground range 24) between the float32 and the float64 restatement over
# CASES.  Measured: 2.07e-05 (64 x 64, 32 iterations); the cases of at most 8 iterations stay below 6e-06.  The constant
# leaves a factor of three for another numpy's sqrt and division order.
F32_DEV = 6.5e-5


def _states_equal(a, b, sl_a, sl_b):
    return all(np.array_equal(a[k][sl_a], b[k][sl_b]) for k in R.FIELDS)


def test_flat_ground_under_uniform_water_stays_flat():
    for dtype in (np.float32, np.float64):
        st = R.init_state(np.full((9, 11), 0.375), P, dtype)
        b0 = st["b"].copy()
        st["d"][...] = 0.5
        for _ in range(6):
            st = R.step(st, P, dtype)
        assert np.array_equal(st["b"], b0)
        assert not st["s"].any() and not any(st[k].any() for k in ("fL", "fR", "fT", "fB"))
        assert np.ptp(st["d"]) == 0 and st["d"][0, 0] > 0


def test_water_is_conserved_without_rain_and_evaporation():
    p = dict(P, rain=0.0, evaporation=0.0)
    st = R.init_state(R.terrain(11, 32, 32), p, np.float64)
    st["d"][...] = 0.5
    total = st["d"].sum()
    for _ in range(20):
        st = R.step(st, p, np.float64)
    assert np.ptp(st["d"]) > 0.1                                  # the water did move
    assert abs(st["d"].sum() - total) <= 1e-9 * total


def test_transposed_input_gives_the_transposed_output():
    t = R.terrain(12, 21, 34)
    a = R.erode_state(t, P, 6, np.float64)
    b = R.erode_state(t.T.copy(), P, 6, np.float64)
    swap = dict(b="b", d="d", s="s", fL="fT", fR="fB", fT="fL", fB="fR")
    for k in R.FIELDS:
        assert np.abs(a[k].T - b[swap[k]]).max() <= 1e-12, k
    assert np.abs(a["s"]).max() > 1e-4                            # not vacuous: sediment is in flight


WIN = dict(shape=(80, 90), rect=(30, 25, 17, 23), n=4)           # also the device's window check


def test_a_window_with_halo_3n_equals_the_larger_map_bit_for_bit():
    (Hb, Wb), (y0, x0, h, w), n = WIN["shape"], WIN["rect"], WIN["n"]
    E = 3 * n
    big = R.terrain(1, Hb, Wb).astype(np.float32)
    full = R.erode_state(big, P, n, np.float32)
    win = R.erode_state(big[y0 - E:y0 + h + E, x0 - E:x0 + w + E], P, n, np.float32)
    inner = (slice(E, E + h), slice(E, E + w))
    assert _states_equal(full, win, (slice(y0, y0 + h), slice(x0, x0 + w)), inner)
    # and against another window origin (the backtrace weights must not depend on absolute indices)
    win2 = R.erode_state(big[y0 - E - 7:y0 + h + E, x0 - E - 11:x0 + w + E + 2], P, n, np.float32)
    assert _states_equal(win, win2, inner, (slice(E + 7, E + 7 + h), slice(E + 11, E + 11 + w)))
    assert not np.array_equal(R.emit(full, P), big)               # something was eroded


def test_a_ring_beyond_the_reach_changes_nothing_at_the_centre():
    n = 3
    E = 3 * n
    c = E + 3
    t = R.terrain(2, 2 * c + 1, 2 * c + 1)
    base = R.erode_state(t, P, n, np.float64)
    yy, xx = np.mgrid[0:2 * c + 1, 0:2 * c + 1]
    ring = np.maximum(np.abs(yy - c), np.abs(xx - c))
    moved = t.copy()
    moved[ring == E + 1] += 0.05
    far = R.erode_state(moved, P, n, np.float64)
    assert all(far[k][c, c] == base[k][c, c] for k in R.FIELDS)
    # the bound is about reach, not about a model that ignores its input: a ring next to the centre is felt
    moved = t.copy()
    moved[ring == 1] += 0.05
    near = R.erode_state(moved, P, n, np.float64)
    assert any(near[k][c, c] != base[k][c, c] for k in R.FIELDS)


def test_sizes_below_two_read_the_cell_itself():
    for shape in ((1, 1), (1, 5), (4, 1)):
        st = R.erode_state(np.full(shape, 0.5), P, 3, np.float32)
        assert all(np.isfinite(st[k]).all() for k in R.FIELDS)
        assert np.array_equal(st["b"], np.full(shape, 12.0, np.float32))      # flat: nothing moves


def test_float32_stays_within_f32_dev_of_float64_on_the_device_cases():
    worst = 0.0
    for H, W, n, seed in CASES:
        t = R.terrain(seed, H, W).astype(np.float32)
        a, b = R.erode_state(t, P, n, np.float32), R.erode_state(t, P, n, np.float64)
        dev = max(float(np.abs(a[k].astype(np.float64) - b[k]).max()) for k in ("b", "d", "s"))
        print("%3d x %3d, %2d iterations: max |f32 - f64| over b, d, s = %.3e" % (H, W, n, dev))
        worst = max(worst, dev)
        assert dev <= F32_DEV, (H, W, n, dev)
    print("worst: %.3e (F32_DEV = %.1e)" % (worst, F32_DEV))
