"""The unbounded world on the host (gan_heightmaps_amd/world.py): addressable latents, the chunk and tile covers,
the default chunk size, the float64 chunk-from-its-own-window against the whole-canvas restatement (tests/world_ref.py), the
anchored tile plan, refusals and the command line.  No GPU."""
import numpy as np
import pytest

from gan_heightmaps_amd import terrain as TR
from gan_heightmaps_amd import texture as TX
from gan_heightmaps_amd import world as WD
from tests import texture_ref as XR
from tests import world_ref as WR
from tests.test_terrain_plan import REF, SMALL, _gen, _seeded_gen, _with_trunk_layer
from gan_heightmaps_amd import layers as L


class _Model:
    """what a TerrainWorld reads of a Pix2Pix before its first request"""

    def __init__(self, gen, latent_dim, sampler=None):
        self.dcgan = {'gen': gen}
        self.latent_dim = latent_dim
        self.sampler = sampler or (lambda n, d: np.random.normal(0, 1, size=(n, d)))
        self.is_a_grayscale = self.is_b_grayscale = True
        self.engine = None


def _world(cfg=SMALL, seed=42, gen=None, **kw):
    return WD.TerrainWorld(_Model(gen if gen is not None else _gen(cfg), cfg['latent_dim']), seed, **kw)


# ---- latents --------------------------------------------------------------------------------------------------------
def test_latent_is_a_pure_function_of_seed_and_cell():
    w = _world()
    np.random.seed(5)
    np.random.rand(3)
    before = np.random.get_state()
    a = w.latent(3, -7)
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    assert a.shape == (24,) and a.dtype == np.float32
    np.random.rand(100)
    assert np.array_equal(a, w.latent(3, -7))                     # whatever the global stream did in between
    assert np.array_equal(a, _world().latent(3, -7))              # a fresh world of the same seed
    assert not np.array_equal(a, w.latent(-7, 3))                 # the order of i and j matters
    assert not np.array_equal(a, _world(seed=43).latent(3, -7))
    assert not np.array_equal(w.latent(0, 0), w.latent(0, 1))
    # negative and huge indices wrap mod 2^32 and stay deterministic
    assert np.array_equal(w.latent(-1, -1), w.latent(2 ** 32 - 1, 2 ** 32 - 1))
    assert np.array_equal(w.latent(-2 ** 31, 5), w.latent(-2 ** 31, 5))
    # the user's distribution is kept: the draw is sampler(1, d)[0] under the array seed
    st = np.random.get_state()
    np.random.seed(np.array([42, 3, (-7) % 2 ** 32], np.uint32))
    want = np.float32(np.random.normal(0, 1, size=(1, 24)))[0]
    np.random.set_state(st)
    assert np.array_equal(a, want)
    u = WD.TerrainWorld(_Model(_gen(SMALL), 24, sampler=lambda n, d: np.random.uniform(2, 3, (n, d))), 1)
    assert (u.latent(0, 0) >= 2).all()


def test_latent_fn_replaces_the_sampler():
    w = _world(latent_fn=lambda i, j: np.full(24, i * 10 + j))
    assert np.array_equal(w.latent(-2, 3), np.full(24, -17, np.float32))
    with pytest.raises(ValueError, match="latent_fn"):
        _world(latent_fn=lambda i, j: np.zeros(5)).latent(0, 0)
    with pytest.raises(ValueError):
        w.latent(0.5, 1)


# ---- covers ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 7, 64])
def test_chunk_cover_is_exact_and_minimal(K):
    for y0 in (-3 * K - 1, -K, -K + 1, -1, 0, 1, K - 1, K, 5 * K + 3):
        for n in (1, 2, K, K + 1, 3 * K):
            lo, hi = WD.axis_chunks(y0, n, K)
            want = sorted({y // K for y in range(y0, y0 + n)})
            assert list(range(lo, hi + 1)) == want, (y0, n, K)
    assert WD.axis_chunks(-70, 150, 64) == (-2, 1) and WD.axis_chunks(33, 97, 64) == (0, 2)


@pytest.mark.parametrize("T,o", [(32, 0), (32, 8), (32, 16), (8, 3)])
def test_tile_cover_is_exact_and_minimal(T, o):
    st = T - o
    for y0 in (-100, -T, -st, -1, 0, 1, st - 1, st, 77):
        for n in (1, o + 1, T, 3 * T + 5):
            lo, hi = WD.axis_tiles(y0, n, T, o)
            want = sorted({p for y in range(y0, y0 + n) for p in WR.covering_tiles(y, T, o)})
            assert list(range(lo, hi + 1)) == want, (y0, n)


@pytest.mark.parametrize("s", [2, 3, 4])
def test_seed_cells_match_the_blend(s):
    for bil in (False, True):
        for y0 in range(-3 * s, 3 * s):
            for n in (1, 2, s, 2 * s + 1):
                cells = sorted({i for y in range(y0, y0 + n) for i, wt in WR.axis_cover(y, s, bil) if wt != 0 or True})
                assert WD.seed_cells(y0, n, s, bil) == (cells[0], cells[-1])


def test_unclamped_blend_is_the_finite_blend_translated():
    s = 4
    fin = TR.axis_blend(5, s, True)
    for y in range(s // 2, 5 * s - s // 2):                       # away from the clamped half cells
        for shift in (0, -3, 7):
            got = WR.axis_cover(y + shift * s, s, True)
            assert [(i - shift, wt) for i, wt in got if wt != 0.0] == [c for c in fin[y] if c[1] != 0.0]
    assert WR.axis_cover(-1, s, False) == [(-1, 1.0)] and WR.axis_cover(-s, s, False) == [(-1, 1.0)]


def test_slot_batches_anchor_a_tile_to_its_slot():
    for q_lo, q_hi, B in ((-5, 6, 4), (0, 0, 4), (3, 4, 4), (-1, -1, 3), (2, 9, 1)):
        seen = []
        for qs, slot0, nb in WD.slot_batches(q_lo, q_hi, B):
            assert len(qs) == B and all(q_lo <= q <= q_hi for q in qs)
            for k in range(slot0, slot0 + nb):
                assert qs[k] % B == k                             # tile q always runs in slot q mod B
                seen.append(qs[k])
        assert seen == list(range(q_lo, q_hi + 1))


# ---- chunk size -----------------------------------------------------------------------------------------------------
def test_default_chunk_cells_follows_the_budget():
    w = _world(REF)
    geo = w.geometry
    assert (geo.s, geo.F, geo.halo, geo.nch, geo.out) == (4, 128, 4, 512, 512)
    assert WD.window_elements(geo, 4) == 64 * 3072 ** 2
    assert WD.window_elements(geo, 4) * 4 <= TR.WINDOW_BUDGET < WD.window_elements(geo, 8) * 4
    assert w.chunk_cells == 4 and w.chunk_px == 2048
    assert _world(REF, chunk_cells=1).chunk_px == 512
    with pytest.raises(ValueError, match="2\\^31"):
        _world(REF, chunk_cells=16)
    c = _world(SMALL).chunk_cells
    assert c & (c - 1) == 0 and WD.window_elements(_world(SMALL).geometry, c) * 4 <= TR.WINDOW_BUDGET
    assert WD.window_elements(_world(SMALL).geometry, 2 * c) * 4 > TR.WINDOW_BUDGET
    with pytest.raises(AttributeError):
        w.chunk_cells = 2                                         # part of the world's identity: read-only


# ---- float64: the halo is exact in two dimensions -------------------------------------------------------------------
@pytest.mark.parametrize("blend", TR.BLENDS)
@pytest.mark.parametrize("bilinear_upsample", [False, True])
def test_chunk_from_its_own_window_equals_the_whole_canvas_crop(blend, bilinear_upsample):
    g = _seeded_gen(SMALL, 31, bilinear_upsample=bilinear_upsample)
    w = _world(gen=g, seed=9)
    for (a, b), c in (((-1, 0), 1), ((0, -2), 2)):
        K = c * 32
        got = WR.chunk(g, w.latent, a, b, c, blend)
        want = WR.region(g, w.latent, a * K, b * K, K, K, blend)
        assert got.shape == want.shape == (1, K, K)
        assert np.abs(got - want).max() <= 1e-12, (a, b, c)
    # one seed pixel less of halo is not exact
    geo = w.geometry
    S = WR.seed_rect(WR.head_fn(g, w.latent), -(geo.halo - 1), -(geo.halo - 1), 4 + 2 * (geo.halo - 1),
                     4 + 2 * (geo.halo - 1), 4, blend)
    u = WR.R.trunk(g, S)[:, (geo.halo - 1) * 8:(geo.halo - 1) * 8 + 32, (geo.halo - 1) * 8:(geo.halo - 1) * 8 + 32]
    assert np.abs(u - WR.region(g, w.latent, 0, 0, 32, 32, blend)).max() > 1e-9


@pytest.mark.parametrize("blend", TR.BLENDS)
def test_request_spanning_chunks_with_negative_origin_has_no_seams(blend):
    g = _seeded_gen(SMALL, 33)
    w = _world(gen=g, seed=4)
    y0, x0, h, wd = -40, -5, 50, 45                               # chunks (-2 .. 0) x (-1 .. 1) at chunk_cells = 1
    got = WR.assemble(g, w.latent, y0, x0, h, wd, 1, blend)
    want = WR.region(g, w.latent, y0, x0, h, wd, blend)
    assert np.abs(got - want).max() <= 1e-12
    # and another chunk size gives the same world
    assert np.abs(WR.assemble(g, w.latent, y0, x0, h, wd, 2, blend) - want).max() <= 1e-12


# ---- anchored tiles -------------------------------------------------------------------------------------------------
def _stub_unet(tile):
    """any fixed per-tile function: two output channels that see the whole tile"""
    t = np.asarray(tile, np.float64)
    return np.stack([np.tanh(t[0] + 0.1 * t[0].mean()), np.flipud(t[0]) * 0.5 + t[0].std()])


def _fake_heightmap(y0, x0, h, w):
    y, x = np.meshgrid(np.arange(y0, y0 + h), np.arange(x0, x0 + w), indexing='ij')
    return (np.sin(0.37 * y) * np.cos(0.21 * x) + 0.01 * ((y * 7 + x * 13) % 11))[None]


@pytest.mark.parametrize("T,o", [(16, 4), (16, 8), (16, 0), (12, 5)])
def test_anchored_tile_plan_weights_and_texture_heightmap_equivalence(T, o):
    y0, x0, h, w = -23, 9, 41, 30
    tex, den = WR.texture_region(_fake_heightmap, _stub_unet, y0, x0, h, w, T, o)
    # every pixel's weights: the product of the per-axis sums over its covering tiles
    wt = WR.tile_weights(T, o)
    st = T - o
    for (r, c) in ((0, 0), (5, 7), (h - 1, w - 1), (17, 3)):
        sy = sum(wt[y0 + r - p * st] for p in WR.covering_tiles(y0 + r, T, o))
        sx = sum(wt[x0 + c - q * st] for q in WR.covering_tiles(x0 + c, T, o))
        assert abs(den[r, c] - sy * sx) < 1e-12
    # texture_heightmap over the tile-aligned expansion E, in float64 with §4j's restatement: equal >= o from E's border
    ey, ex, eh, ew = WR.tile_aligned_expansion(y0, x0, h, w, T, o)
    assert ey % st == 0 and ex % st == 0 and ey <= y0 - o and ex <= x0 - o and ey + eh >= y0 + h + o and ex + ew >= x0 + w + o
    xn = _fake_heightmap(ey, ex, eh, ew)
    py, px = TX.axis_plan(eh, T, o), TX.axis_plan(ew, T, o)
    assert py.pad == 0 and px.pad == 0 and py.starts == [i * st for i in range(py.n)]
    U = np.stack([np.stack([_stub_unet(XR.host_tile(xn, py, px, i, j)) for j in range(px.n)]) for i in range(py.n)])
    whole = XR.blend_gather(py, px, U)
    crop = whole[:, y0 - ey:y0 - ey + h, x0 - ex:x0 - ex + w]
    assert np.abs(crop - tex).max() <= 1e-12


# ---- refusals -------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused():
    for kw in (dict(blend='cubic'), dict(chunk_cells=0), dict(chunk_cells=2.0), dict(chunk_cells=True), dict(batch_size=0),
               dict(batch_size=WD.MAX_BATCH + 1), dict(cache_mb=-1), dict(overlap=17), dict(overlap=-1), dict(latent_fn=3)):
        with pytest.raises(ValueError):
            _world(**kw)
    with pytest.raises(ValueError):
        _world(seed=1.5)
    with pytest.raises(NotImplementedError, match="deterministic"):
        _world(deterministic=False)
    w = _world(chunk_cells=2)
    assert (w.chunk_cells, w.chunk_px, w.overlap, w.geometry.halo) == (2, 64, 8, 4)
    for region in ((0, 0, 0, 5), (0, 0, 5, -1), (0.5, 0, 5, 5), (0, 0, 5, 1 << 24), (1 << 45, 0, 5, 5)):
        with pytest.raises(ValueError):
            w.heightmap(*region)
        with pytest.raises(ValueError):
            w.texture(*region)
    w.close()
    with pytest.raises(ValueError, match="closed"):
        w.heightmap(0, 0, 4, 4)
    with _world() as w2:
        assert w2.chunk_cells >= 1


def test_generators_split_generator_refuses_are_refused():
    bad = _with_trunk_layer(lambda n: L.MaxPool2DLayer(n, 2))
    with pytest.raises(NotImplementedError, match="MaxPool2DLayer"):
        WD.TerrainWorld(_Model(bad, 8), 1)


# ---- command line ---------------------------------------------------------------------------------------------------
def test_cli_arguments():
    a = WD.parse_args(["test1_nobn_bilin_both", "m.model", "out.npy", "--seed", "42", "--region", "-70000,33000,1000,1500"])
    assert (a.experiment, a.model, a.output, a.seed, a.region) == \
        ("test1_nobn_bilin_both", "m.model", "out.npy", 42, (-70000, 33000, 1000, 1500))
    assert (a.chunk_cells, a.blend, a.dtype, a.texture, a.overlap, a.batch_size) == (None, "bilinear", "bf16x3", None, None, 4)
    a = WD.parse_args(["e", "m", "o.png", "--region=-1,-2,3,4", "--seed", "-7", "--chunk-cells", "2", "--blend", "mosaic",
                       "--dtype", "f32", "--texture", "t.png", "--overlap", "64", "--batch-size", "8"])
    assert (a.region, a.seed, a.chunk_cells, a.blend, a.dtype, a.texture, a.overlap, a.batch_size) == \
        ((-1, -2, 3, 4), -7, 2, "mosaic", "f32", "t.png", 64, 8)
    assert WD.parse_args(["e", "m", "o", "--seed", "1", "--region", "5,-6,7,8"]).region == (5, -6, 7, 8)
    assert WD.parse_args(["e", "m", "o", "--seed", "1", "--region", " -5, +6,7,8"]).region == (-5, 6, 7, 8)
    for bad in (["e", "m", "o.png", "--seed", "1"], ["e", "m", "o.png", "--region", "0,0,4,4"],
                ["e", "m", "o.png", "--seed", "1", "--region", "0,0,4"], ["e", "m", "o.png", "--seed", "1", "--region", "0,0,0,4"],
                ["e", "m", "o.png", "--seed", "1", "--region", "0,0,4,-4"],
                ["e", "m", "o.png", "--seed", "1", "--region", "0,0,4,4", "--chunk-cells", "0"],
                ["e", "m", "o.png", "--seed", "1", "--region", "0,0,4,4", "--overlap", "8"],
                ["e", "m", "o.png", "--seed", "1", "--region", "0,0,4,4", "--blend", "x"]):
        with pytest.raises(SystemExit):
            WD.parse_args(bad)
