"""Tiled texturing, host side: the tiling plan, its weights, the batch-composition rule, the blend restatement against a
brute-force paste, and the command line (gan_heightmaps_amd/texture.py).  No GPU."""
import numpy as np
import pytest

from gan_heightmaps_amd import texture as TX
from tests import texture_ref as R

T = 64
LENGTHS = [1, 17, T - 1, T, T + 1, 2 * T - T // 4, 3 * T, 1000]
OVERLAPS = [0, 1, T // 8, T // 4, T // 2]


@pytest.mark.parametrize("o", OVERLAPS)
@pytest.mark.parametrize("L", LENGTHS)
def test_axis_plan_properties(L, o):
    p = TX.axis_plan(L, T, o)
    s = T - o
    assert p.s == s and p.o == o and p.T == T
    assert p.n == 1 + -(-max(L - T, 0) // s)
    starts = p.starts
    assert len(starts) == p.n
    assert all(b - a == s for a, b in zip(starts, starts[1:]))          # uniform stride: every overlap is exactly o
    assert p.padded == T + (p.n - 1) * s and p.padded >= L
    assert p.pad == (p.padded - L) // 2 and starts[0] == -p.pad        # centred
    assert starts[-1] + T - L in (p.pad, p.pad + 1)                     # the other side gets the same (or one more)
    wts = [TX.axis_weights(p, i) for i in range(p.n)]
    for y in range(L):
        cov = p.covering(y)
        assert 1 <= len(cov) <= 2                                       # [0, L) covered, by one or two tiles
        ws = [float(wts[i][y - p.start(i)]) for i in cov]
        if len(cov) == 1:
            assert ws[0] == 1.0                                          # exactly 1 where one tile covers
        assert sum(ws) > 0
        assert cov == list(range(cov[0], cov[0] + len(cov)))
    if o == 0:
        assert all(len(p.covering(y)) == 1 for y in range(L))


def test_axis_weights_are_the_ramps():
    p = TX.axis_plan(200, T, 16)
    assert p.n >= 3
    w = TX.axis_weights(p, 1)
    t = np.arange(T)
    np.testing.assert_array_equal(w[:16], ((t[:16] + 0.5) / 16).astype(np.float32))
    np.testing.assert_array_equal(w[T - 16:], ((T - t[T - 16:] - 0.5) / 16).astype(np.float32))
    assert (w[16:T - 16] == 1).all()
    assert (TX.axis_weights(p, 0)[:16] == 1).all()                      # no neighbour before tile 0
    assert (TX.axis_weights(p, p.n - 1)[T - 16:] == 1).all()            # nor after the last
    # the two ramps of an overlap add up to 1 (in exact arithmetic)
    np.testing.assert_allclose(TX.axis_weights(p, 0)[T - 16:].astype(np.float64) + w[:16], 1.0, atol=1e-7)


@pytest.mark.parametrize("bad", [-1, T // 2 + 1, T, 2.5, True])
def test_invalid_overlap_raises(bad):
    with pytest.raises(ValueError):
        TX.axis_plan(100, T, bad)
    with pytest.raises(ValueError):
        TX.check_overlap(T, bad)


@pytest.mark.parametrize("tile", [0, -4, 3.0, None])
def test_invalid_tile_size_raises(tile):
    with pytest.raises(ValueError):
        TX.axis_plan(100, tile, 0)


@pytest.mark.parametrize("L", [0, -3])
def test_invalid_length_raises(L):
    with pytest.raises(ValueError):
        TX.axis_plan(L, T, 0)


def test_default_overlap_is_a_quarter_tile():
    assert TX.check_overlap(512) == 128 and TX.axis_plan(1000, 512).o == 128
    assert TX.check_overlap(512, 256) == 256 and TX.check_overlap(512, 0) == 0


def test_reflect_rule_is_half_sample_symmetric():
    L = 5
    got = TX.reflect_index(np.arange(-12, 18), L)
    ref = np.pad(np.arange(L), 20, mode='symmetric')[20 - 12:20 + 18]
    np.testing.assert_array_equal(got, ref)
    assert (TX.reflect_index(np.arange(-7, 9), 1) == 0).all()


def test_batch_composition_rule():
    assert TX.tile_batches(7, 3) == [(0, 3), (3, 3), (6, 1)]
    assert TX.tile_batches(4, 4) == [(0, 4)]
    assert TX.tile_batches(1, 8) == [(0, 1)]
    assert TX.tile_batches(5, 1) == [(j, 1) for j in range(5)]
    with pytest.raises(ValueError):
        TX.tile_batches(3, 0)
    # the padded batch repeats its last real tile: the host restatement rebuilds exactly these batches
    seen = []

    def gen(batch):
        seen.append(batch.copy())
        return batch[:, :1] * 2
    x = np.random.RandomState(0).rand(1, 40, 70).astype(np.float32)
    py, px, U = R.tile_outputs(gen, x, 16, 4, 3)
    assert len(seen) == py.n * len(TX.tile_batches(px.n, 3))
    last = seen[len(TX.tile_batches(px.n, 3)) - 1]
    nv = TX.tile_batches(px.n, 3)[-1][1]
    for b in range(nv, 3):
        np.testing.assert_array_equal(last[b], last[nv - 1])
    np.testing.assert_array_equal(U[0, 0, 0], R.host_tile(x, py, px, 0, 0)[0] * 2)


@pytest.mark.parametrize("o", [0, 1, 4, 8, 16])
@pytest.mark.parametrize("H,W", [(1, 1), (17, 45), (32, 32), (75, 33), (100, 131)])
def test_blend_restatement_matches_brute_force_paste(H, W, o):
    rng = np.random.RandomState(H * 1000 + W + o)
    Tt = 32
    py, px = TX.axis_plan(H, Tt, o), TX.axis_plan(W, Tt, o)
    U = rng.uniform(-1, 1, (py.n, px.n, 3, Tt, Tt)).astype(np.float32)
    a = R.blend_gather(py, px, U)
    b = R.blend_paste(py, px, U)
    np.testing.assert_allclose(a, b, rtol=0, atol=1e-12)
    m = R.single_cover_mask(py, px)
    single = R.single_cover_values(py, px, U)
    assert np.array_equal(a[:, m].astype(np.float32), single[:, m])
    if o == 0:
        assert m.all()


def test_constant_tiles_blend_to_the_constant():
    py, px = TX.axis_plan(90, 32, 8), TX.axis_plan(130, 32, 8)
    U = np.full((py.n, px.n, 1, 32, 32), 0.25, np.float32)
    np.testing.assert_allclose(R.blend_gather(py, px, U), 0.25, atol=1e-15)


def test_cli_arguments():
    a = TX.parse_args(["test1_nobn_bilin_both", "m.pkl.gz", "in.png", "out.png"])
    assert (a.experiment, a.model, a.input, a.output) == ("test1_nobn_bilin_both", "m.pkl.gz", "in.png", "out.png")
    assert a.overlap is None and a.batch_size == 4 and a.dtype == "bf16x3"
    a = TX.parse_args(["e", "m", "in.npy", "out.npy", "--overlap", "128", "--batch-size", "8", "--dtype", "f32"])
    assert a.overlap == 128 and a.batch_size == 8 and a.dtype == "f32"
    for bad in (["e", "m", "i"], ["e", "m", "i", "o", "--batch-size", "0"], ["e", "m", "i", "o", "--overlap", "-2"],
                ["e", "m", "i", "o", "--dtype", "f64"]):
        with pytest.raises(SystemExit):
            TX.parse_args(bad)


def test_cli_reads_npy_through_mmap_and_png(tmp_path):
    from PIL import Image
    x = (np.arange(30 * 50) % 251).astype(np.uint8).reshape(30, 50)
    np.save(tmp_path / "h.npy", x)
    got = TX.read_heightmap(str(tmp_path / "h.npy"), 1)
    assert isinstance(got, np.memmap) and np.array_equal(got, x)
    Image.fromarray(x).save(tmp_path / "h.png")
    assert np.array_equal(TX.read_heightmap(str(tmp_path / "h.png"), 1), x)
    assert TX.read_heightmap(str(tmp_path / "h.png"), 3).shape == (30, 50, 3)


def test_input_layouts_are_checked():
    TX._input_layout(np.zeros((5, 7), np.uint8), 1)
    TX._input_layout(np.zeros((5, 7, 3), np.uint8), 3)
    TX._input_layout(np.zeros((1, 5, 7), np.float32), 1)
    for a, c in ((np.zeros((5, 7), np.float64), 1), (np.zeros((5, 7, 3), np.uint8), 1), (np.zeros((5,), np.uint8), 1),
                 (np.zeros((2, 5, 7), np.float32), 1)):
        with pytest.raises(ValueError):
            TX._input_layout(a, c)
