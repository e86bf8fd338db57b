"""Terrain generation on the host (gan_heightmaps_amd/terrain.py): the trunk's halo, the window plan, the blend
weights, the float64 banded trunk against the whole-canvas trunk, refusals and the command line.  No GPU."""
import numpy as np
import pytest

from gan_heightmaps_amd import layers as L
from gan_heightmaps_amd import terrain as TR
from gan_heightmaps_amd.architectures import dcgan
from gan_heightmaps_amd.nonlinearities import linear
from tests import terrain_ref as R

REF = dict(latent_dim=1000, nch=512, div=[2, 2, 4, 4, 8, 8, 8])       # the test1_* generators (widths 256 .. 64)
SMALL = dict(latent_dim=24, nch=16, div=[2, 2, 4])                      # tests/test_gpu_step.py SMALL's generator


def _gen(cfg, **kw):
    return dcgan.default_generator(cfg['latent_dim'], True, nch=cfg['nch'], div=cfg['div'], **kw)


def _seeded_gen(cfg, seed, **kw):
    """a generator with random weights and non-trivial BatchNorm running statistics"""
    np.random.seed(seed)
    g = _gen(cfg, **kw)
    rng = np.random.RandomState(seed + 1)
    for p in L.get_all_params(g):
        if p.name.endswith(".mean") or p.name.endswith(".beta") or p.name.endswith(".b"):
            p.set_value(0.1 * rng.randn(*p.shape))
        elif p.name.endswith(".inv_std") or p.name.endswith(".gamma"):
            p.set_value(rng.uniform(0.5, 1.5, p.shape))
    return g


# ---- halo -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,kw,halo", [(REF, {}, 4), (SMALL, {}, 4), (REF, dict(num_repeats=1), 8),
                                         (SMALL, dict(num_repeats=1), 8), (REF, dict(bilinear_upsample=True), 5),
                                         (SMALL, dict(bilinear_upsample=True), 5)])
def test_halo_of_the_generators(cfg, kw, halo):
    _, _, trunk = TR.split_generator(_gen(cfg, **kw))
    assert TR.trunk_halo(trunk) == halo


def test_trunk_scale_and_output_size():
    geo = TR.TerrainGeometry(_gen(REF), 3, 2)
    assert (geo.s, geo.F, geo.out, geo.nch, geo.channels) == (4, 128, 512, 512, 1)
    assert (geo.H, geo.W, geo.Hs, geo.Ws) == (1536, 1024, 12, 8)
    geo = TR.TerrainGeometry(_gen(SMALL), 2, 5)
    assert (geo.out, geo.H, geo.W) == (32, 64, 160)


# ---- windows --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [1, 2, 5, 8, 9, 12, 13, 17, 40, 64, 101])
@pytest.mark.parametrize("band", [1, 2, 3, 8, 24])
@pytest.mark.parametrize("halo", [0, 1, 4, 5, 8])
def test_window_plan(H, band, halo):
    plan = TR.window_plan(H, band, halo)
    win = min(H, band + 2 * halo)
    covered = np.zeros(H, int)
    for w0, klo, khi in plan:
        assert 0 <= w0 and w0 + win <= H                       # one height, clamped inside the canvas
        assert w0 <= klo < khi <= w0 + win
        covered[klo:khi] += 1
        if w0 > 0:
            assert klo - w0 >= halo                             # interior top edge
        if w0 + win < H:
            assert w0 + win - khi >= halo                       # interior bottom edge
    assert (covered == 1).all()                                 # the kept ranges tile [0, H) exactly once
    assert plan[0][0] == 0 and plan[-1][0] + win == H
    assert [k[1] for k in plan] == sorted(k[1] for k in plan)
    if H <= band + 2 * halo:
        assert plan == [(0, 0, H)]                              # a short canvas is a single window


def test_window_plan_rejects_bad_arguments():
    for args in ((0, 1, 1), (5, 0, 1), (5, 1, -1)):
        with pytest.raises(ValueError):
            TR.window_plan(*args)


def test_default_band_follows_the_budget_and_is_at_least_one():
    geo = TR.TerrainGeometry(_gen(REF), 16, 16)
    assert geo.per_row == 64 * 128 * 128 * 64                   # the 64-channel 512-row stage, per seed row
    assert geo.band == TR.WINDOW_BUDGET // 4 // geo.per_row - 2 * geo.halo == 8
    assert geo.win * geo.per_row * 4 <= TR.WINDOW_BUDGET
    assert TR.TerrainGeometry(_gen(REF), 4, 48).band == 1
    assert TR.TerrainGeometry(_gen(REF), 16, 16, band=4).win == 12


# ---- blend weights --------------------------------------------------------------------------------------------------
def test_axis_blend_weights():
    s = 4
    m = TR.axis_blend(3, s, False)
    assert all(c == [(y // s, 1.0)] for y, c in enumerate(m))
    b = TR.axis_blend(3, s, True)
    for y, c in enumerate(b):
        assert abs(sum(w for _, w in c) - 1.0) < 1e-15
        assert all(0 <= i < 3 for i, _ in c)
    # the first and last half cells clamp both corners onto one cell: weight 1 there
    assert b[0] == [(0, 1.0)] and b[1] == [(0, 1.0)] and b[-1] == [(2, 1.0)] and b[-2] == [(2, 1.0)]
    assert b[2] == [(0, 0.875), (1, 0.125)] and b[5] == [(0, 0.125), (1, 0.875)]
    assert TR.axis_blend(1, s, True) == [[(0, 1.0)]] * s        # one cell: the identity


def test_seed_canvas_one_cell_is_the_identity_and_equal_cells_blend_to_the_mosaic():
    rng = np.random.RandomState(3)
    P1 = rng.randn(1, 1, 6, 4, 4)
    for blend in TR.BLENDS:
        assert np.array_equal(R.seed_canvas(P1, blend), P1[0, 0])
    P = np.broadcast_to(rng.randn(1, 1, 6, 4, 4), (3, 5, 6, 4, 4)).copy()
    np.testing.assert_allclose(R.seed_canvas(P, 'bilinear'), R.seed_canvas(P, 'mosaic'), rtol=0, atol=1e-12)
    # one row / one column: the clamped axis copies
    Pr = rng.randn(1, 4, 6, 4, 4)
    Sb, Sm = R.seed_canvas(Pr, 'bilinear'), R.seed_canvas(Pr, 'mosaic')
    assert not np.allclose(Sb, Sm)
    assert np.array_equal(R.seed_canvas(Pr[:, :1], 'bilinear'), Sm[:, :, :4])


def test_bilinear_equals_the_head_on_an_interpolated_latent_field():
    g = _seeded_gen(SMALL, 5)
    z = np.random.RandomState(6).randn(3, 2, SMALL['latent_dim'])
    S = R.seed_canvas(R.head_maps(g, z), 'bilinear')
    s = 4
    by, bx = TR.axis_blend(3, s, True), TR.axis_blend(2, s, True)
    for y, x in ((0, 0), (2, 5), (6, 3), (11, 7), (5, 4)):
        zf = sum(wy * wx * z[i, j] for i, wy in by[y] for j, wx in bx[x])
        P = R.head_maps(g, zf[None, None])[0, 0]
        np.testing.assert_allclose(S[:, y, x], P[:, y % s, x % s], rtol=0, atol=1e-12)


# ---- banded trunk == whole-canvas trunk (float64) -------------------------------------------------------------------
@pytest.mark.parametrize("blend", TR.BLENDS)
@pytest.mark.parametrize("bilinear_upsample", [False, True])
def test_banded_trunk_equals_whole_canvas(blend, bilinear_upsample):
    g = _seeded_gen(SMALL, 11, bilinear_upsample=bilinear_upsample)
    z = np.random.RandomState(12).randn(5, 3, SMALL['latent_dim'])
    S = R.seed_canvas(R.head_maps(g, z), blend)
    whole = R.trunk(g, S)
    assert whole.shape == (1, 160, 96)
    for band in (1, 2, 7):
        banded = R.trunk_banded(g, S, band)
        assert np.abs(banded - whole).max() <= 1e-12, band
    # one row less of halo is not exact: the halo is the trunk's true reach
    assert np.abs(R.trunk_banded(g, S, 1, halo=TR.trunk_halo(TR.split_generator(g)[2]) - 1) - whole).max() > 1e-9


def test_one_cell_terrain_is_the_generator():
    g = _seeded_gen(SMALL, 21)
    z = np.random.RandomState(22).randn(1, 1, SMALL['latent_dim'])
    full = R._run([l for l in L.get_all_layers(g) if not isinstance(l, L.InputLayer)], z[0], np.float64)[0]
    for blend in TR.BLENDS:
        np.testing.assert_allclose(R.terrain(g, z, blend), full, rtol=0, atol=1e-13)


# ---- graph plumbing -------------------------------------------------------------------------------------------------
def test_trunk_clone_shares_the_generators_params():
    g = _gen(SMALL)
    geo = TR.TerrainGeometry(g, 2, 3)
    t = geo.trunk_graph()
    assert t.output_shape == (None, 1, geo.win * 8, 96)
    clone = [l for l in L.get_all_layers(t) if not isinstance(l, L.InputLayer)]
    assert len(clone) == len(geo.trunk) and all(a is not b for a, b in zip(clone, geo.trunk))
    assert all(p is q for a, b in zip(clone, geo.trunk) for p, q in zip(a.params, b.params))
    assert L.get_all_params(t) == L.get_all_params(g)[-len(L.get_all_params(t)):]
    assert g.output_shape == (None, 1, 32, 32)                  # the original graph is untouched


# ---- refusals -------------------------------------------------------------------------------------------------------
def _with_trunk_layer(make):
    net = L.InputLayer((None, 8))
    net = L.DenseLayer(net, 16 * 4 * 4, nonlinearity=linear)
    net = L.BatchNormLayer(net)
    net = L.ReshapeLayer(net, (-1, 16, 4, 4))
    net = make(net)
    return L.Conv2DLayer(net, 1, 5, pad='same', nonlinearity=linear)


@pytest.mark.parametrize("make,what", [
    (lambda n: L.Conv2DLayer(n, 8, 3, stride=2, pad=1), "Conv2DLayer"),
    (lambda n: L.Conv2DLayer(n, 8, 3, pad='valid'), "Conv2DLayer"),
    (lambda n: L.MaxPool2DLayer(n, 2), "MaxPool2DLayer"),
    (lambda n: L.TransposedConv2DLayer(n, 8, 2, stride=2), "TransposedConv2DLayer"),
    (lambda n: L.InstanceNormLayer(n), "InstanceNormLayer"),
])
def test_unsupported_trunks_are_refused(make, what):
    with pytest.raises(NotImplementedError, match=what):
        TR.split_generator(_with_trunk_layer(make))


def test_supported_odd_trunk_layers_pass():
    g = _with_trunk_layer(lambda n: L.DropoutLayer(L.NonlinearityLayer(n), p=0.3))
    assert TR.trunk_halo(TR.split_generator(g)[2]) == 2          # one 5 x 5 convolution at seed resolution


def test_too_wide_canvas_is_refused_with_the_widest_allowed():
    TR.TerrainGeometry(_gen(REF), 3, 56)
    with pytest.raises(ValueError, match=r"widest canvas allowed is 56 cells \(28672 px\)"):
        TR.TerrainGeometry(_gen(REF), 3, 57)
    with pytest.raises(ValueError, match="band=40"):
        TR.TerrainGeometry(_gen(REF), 64, 40, band=40)


def test_bad_arguments_are_refused():
    g = _gen(SMALL)
    with pytest.raises(NotImplementedError, match="deterministic"):
        TR.generate_terrain(None, g, 24, np.random.rand, True, grid=(2, 2), deterministic=False)
    for kw in (dict(grid=(2, 2), blend='cubic'), dict(), dict(grid=(0, 2)), dict(grid=(2, 2.5)),
               dict(z=np.zeros((2, 3, 23))), dict(grid=(2, 2), z=np.zeros((2, 3, 24)))):
        with pytest.raises(ValueError):
            TR.generate_terrain(None, g, 24, np.random.rand, True, **kw)
    with pytest.raises(ValueError, match="band"):
        TR.TerrainGeometry(g, 2, 2, band=0)


# ---- command line ---------------------------------------------------------------------------------------------------
def test_cli_arguments():
    a = TR.parse_args(["test1_nobn_bilin_both", "m.model", "out.npy", "--cells", "16x8"])
    assert (a.experiment, a.model, a.output, a.cells) == ("test1_nobn_bilin_both", "m.model", "out.npy", (16, 8))
    assert (a.seed, a.blend, a.band, a.dtype, a.texture, a.overlap, a.batch_size) == \
        (None, "bilinear", None, "bf16x3", None, None, 4)
    a = TR.parse_args(["e", "m", "o.png", "--cells", "3X2", "--seed", "7", "--blend", "mosaic", "--band", "2",
                       "--dtype", "f32", "--texture", "t.png", "--overlap", "64", "--batch-size", "8"])
    assert (a.cells, a.seed, a.blend, a.band, a.dtype, a.texture, a.overlap, a.batch_size) == \
        ((3, 2), 7, "mosaic", 2, "f32", "t.png", 64, 8)
    for bad in (["e", "m", "o.png"], ["e", "m", "o.png", "--cells", "3"], ["e", "m", "o.png", "--cells", "0x2"],
                ["e", "m", "o.png", "--cells", "2x2", "--band", "0"], ["e", "m", "o.png", "--cells", "2x2", "--blend", "x"],
                ["e", "m", "o.png", "--cells", "2x2", "--overlap", "8"]):
        with pytest.raises(SystemExit):
            TR.parse_args(bad)
