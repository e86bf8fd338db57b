"""The float64 restatement of the sliced Wasserstein distance (tests/swd_ref.py) against its own known answers: the filters'
reflection, exact zeros of the Laplacian, reconstruction, the sorted L1 of shifted columns, draws that do not depend on
batching, agreement with the package's draws, and that the metric tells a blurred set from a fresh sample.  No GPU."""
import numpy as np
import pytest

from gan_heightmaps_amd import swd as SW
from tests import swd_ref as R


def test_constant_image_has_a_zero_laplacian():
    x = np.full((2, 3, 32, 48), 0.7)
    lap = R.laplacian_pyramid(x, 2)
    assert np.array_equal(lap[0], np.zeros_like(x))                # exactly: the weights are dyadic and sum to one
    assert np.array_equal(lap[1], np.full((2, 3, 16, 24), 0.7))


def test_ramp_interior_has_a_zero_laplacian():
    yy, xx = np.mgrid[0:64, 0:64].astype(np.float64)
    for ramp in (xx, yy, 0.25 * xx - 3.0 * yy + 5.0):
        lap0 = R.laplacian_pyramid(ramp[None, None], 2)[0][0, 0]
        assert np.abs(lap0[5:-5, 5:-5]).max() <= 1e-12             # more than 4 pixels from the edge
        assert np.abs(lap0).max() > 1e-3                           # the reflection bends the ramp at the edge


def test_down_of_a_corner_delta_pins_the_reflection():
    x = np.zeros((16, 16))
    x[0, 0] = 256.0
    d = R.down(x)
    # row 0 reads columns refl(-2..2) = 2 1 0 1 2: the delta once, with weight 6; output 1 reads 0..4: weight 1
    want = np.zeros((8, 8))
    want[0, 0], want[0, 1], want[1, 0], want[1, 1] = 36.0, 6.0, 6.0, 1.0
    assert np.array_equal(d, want)
    x = np.zeros((16, 16))
    x[15, 15] = 256.0
    d = R.down(x)
    # output 7 reads 12..16 -> 12 13 14 15 14: the last column once, with weight 4
    want = np.zeros((8, 8))
    want[7, 7] = 16.0
    assert np.array_equal(d, want)
    x = np.zeros((16, 16))
    x[14, 1] = 256.0
    d = R.down(x)
    # rows: output 7 reads 12 13 14 15 14 -> weights 6 + 1 = 7, output 6 reads 10..14 -> 1;
    # columns: output 0 reads 2 1 0 1 2 -> 4 + 4 = 8, output 1 reads 0..4 -> 4
    want = np.zeros((8, 8))
    want[7, 0], want[7, 1], want[6, 0], want[6, 1] = 56.0, 28.0, 8.0, 4.0
    assert np.array_equal(d, want)


def test_up_of_a_delta_and_of_the_edges():
    y = np.zeros((8, 8))
    y[3, 4] = 64.0
    u = R.up(y)
    k = np.array([1.0, 4.0, 6.0, 4.0, 1.0])
    want = np.zeros((16, 16))
    want[4:9, 6:11] = np.outer(k, k)
    assert np.array_equal(u, want)
    y = np.zeros((8, 8))
    y[7, 7] = 64.0
    u = R.up(y)
    # position 14 is the last even one: 15 reads (4 z[14] + 4 z[16 -> 14]) / 8, 14 reads (z[12] + 6 z[14] + z[16 -> 14]) / 8
    assert u[15, 15] == 64.0 and u[14, 14] == 49.0 and u[14, 15] == 56.0 and u[13, 13] == 16.0 and u[12, 12] == 1.0


def test_the_pyramid_reconstructs_the_image():
    x = np.random.RandomState(0).uniform(-1, 1, (2, 3, 64, 96))
    lap = R.laplacian_pyramid(x, 3)
    assert [l.shape[2:] for l in lap] == [(64, 96), (32, 48), (16, 24)]
    assert np.abs(R.reconstruct(lap) - x).max() <= 1e-12


def test_the_distance_of_a_set_from_itself_is_zero():
    x = R.power_law_images(3, 8, 32)
    d = R.descriptors(x, 0, patches_per_image=16)
    assert [m.shape for m in d] == [(128, 49), (128, 49)]
    for i, m in enumerate(d):
        assert R.level_distance(m, m, 1, i, 16, 2) == 0.0
    r = R.swd(x, x, patches_per_image=16, directions_=16, repeats=2, sets=(0, 0))
    assert r["swd"] == [0.0, 0.0] and r["mean"] == 0.0 and r["levels"] == [32, 16]
    # the two sets draw their windows apart: the same images as set 0 and as set 1 are two samples of one distribution
    r = R.swd(x, x, patches_per_image=16, directions_=16, repeats=2)
    assert 0.0 < r["mean"] < 400.0


def test_sorted_l1_of_a_shifted_column_is_the_shift():
    a = np.random.RandomState(1).randn(1000, 3)
    for delta in (0.25, -1.5):
        assert abs(R.sorted_l1(a, a + delta) - abs(delta)) <= 1e-12
        assert abs(R.sorted_l1(a, a[::-1] + delta) - abs(delta)) <= 1e-12       # the order within a column means nothing


def test_draws_do_not_depend_on_batching_and_match_the_package():
    n, P, H, W = 6, 5, 32, 48
    whole = R.corners(7, 1, 2, n, P, H, W)
    assert whole.shape == (n, P, 2) and whole[..., 0].max() <= H - 7 and whole[..., 1].max() <= W - 7 and whole.min() >= 0
    # fed in batches of 1, 2 or 3 a set reads rows [i0, i1) of one table drawn for the whole set
    x = np.random.RandomState(2).uniform(-1, 1, (n, 2, H, W))
    full = R.gather(x, whole)
    for bs in (1, 2, 3):
        parts = [R.gather(x[i:i + bs], whole[i:i + bs]) for i in range(0, n, bs)]
        assert np.array_equal(np.concatenate(parts), full)
    assert not np.array_equal(whole, R.corners(7, 0, 2, n, P, H, W))           # the sets draw apart
    assert not np.array_equal(whole, R.corners(7, 1, 1, n, P, H, W))           # and so do the levels
    m = SW.SWD(patches_per_image=P, directions=9, repeats=2, seed=7)
    assert np.array_equal(SW.corners(m, 1, 2, n, H, W), whole) and SW.corners(m, 1, 2, n, H, W).dtype == np.int32
    d = R.directions(7, 1, 0, 98, 9)
    assert d.dtype == np.float32 and d.shape == (98, 9) and np.abs((d.astype(np.float64) ** 2).sum(0) - 1).max() < 1e-6
    assert np.array_equal(SW.directions(m, 1, 0, 98), d)
    assert not np.array_equal(d, R.directions(7, 1, 1, 98, 9))
    # the descriptor layout: column c * 49 + dy * 7 + dx
    y, x0 = whole[1, 3]
    assert full[1 * P + 3, 1 * 49 + 2 * 7 + 5] == x[1, 1, y + 2, x0 + 5]
    for H_, W_, L in ((512, 512, 6), (32, 32, 2), (16, 16, 1), (64, 96, 3), (48, 48, 2)):
        assert R.default_levels(H_, W_) == L == SW.SWD().num_levels(H_, W_)


def test_a_blurred_set_scores_higher_than_a_fresh_sample_at_the_finest_level():
    """Power-law noise, 64 x 64, 32 images per set, 3 levels, 32 patches, 64 directions x 2 repeats, seeds fixed.  The
    restatement's values (1e3 x): the blurred set 159.2 / 77.3 / 67.1 at 64 / 32 / 16 pixels, the fresh sample 57.4 / 57.3 /
    58.3: a ratio of 2.77 at the finest level, asserted at 2.77 / 1.5 = 1.85; at the coarsest level, where the blur has
    nothing left to remove, the ratio is 1.15."""
    real = R.power_law_images(10, 32, 64)
    fresh = R.power_law_images(11, 32, 64)
    blurred = R.up(R.down(R.power_law_images(12, 32, 64)))
    kw = dict(levels=3, patches_per_image=32, directions_=64, repeats=2, seed=0)
    b, f = R.swd(real, blurred, **kw), R.swd(real, fresh, **kw)
    print("blurred", b["swd"], "fresh", f["swd"])
    assert b["levels"] == [64, 32, 16]
    assert b["swd"][0] >= 1.85 * f["swd"][0]
    assert b["swd"][0] / f["swd"][0] >= 1.5 * b["swd"][2] / f["swd"][2]        # the fine scale tells them apart, the coarse less
