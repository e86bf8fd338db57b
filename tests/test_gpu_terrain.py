"""Terrain generation on the MI355X (csrc/terrain.hip, gan_heightmaps_amd/terrain.py): the seed and emit kernels
against the host restatement (tests/terrain_ref.py) and util's uint8 map, and Pix2Pix.generate_terrain end to end against
z_fn_det, the float64 restatement and itself (banded against one whole-canvas window)."""
import numpy as np
import pytest

from oracle import step as ostep
from gan_heightmaps_amd import terrain as TR
from gan_heightmaps_amd import util
from tests import terrain_ref as R
from tests.gpu_common import build_model, dev, model_params, ops, rel, SMALL      # noqa: F401  (dev, ops: the module-scoped fixtures)

pytestmark = pytest.mark.gpu


# ---- 1. seed --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gy,gx,C,s", [(3, 2, 16, 4), (2, 5, 8, 4), (1, 1, 5, 4), (4, 3, 3, 3), (2, 7, 4, 2)])
def test_seed_kernel_against_the_restatement(dev, ops, gy, gx, C, s):
    rng = np.random.RandomState(gy * 10 + gx)
    P = rng.randn(gy, gx, C, s, s).astype(np.float32)
    Pd = dev.tensor(P.reshape(gy * gx, C * s * s))
    for blend in TR.BLENDS:
        ref = R.seed_canvas(P.astype(np.float64), blend)
        for row0, rows in ((0, s * gy), (1, s * gy - 1), (s * gy - 2, 2), (s // 2, 1)):
            if rows < 1:
                continue
            out = dev.empty((1, C, rows, s * gx))
            ops.terrain_seed(Pd, gy, gx, s, row0, rows, blend == 'bilinear', out)
            got = out.numpy()[0]
            want = ref[:, row0:row0 + rows]
            if blend == 'mosaic':
                assert np.array_equal(got, want.astype(np.float32)), (row0, rows)
            else:
                assert np.abs(got - want).max() <= 1e-6 * max(1.0, np.abs(want).max()), (row0, rows)
            dev.free(out.ptr)
        if gy == 1 and gx == 1:                                 # one cell: both blends copy P bit for bit
            out = dev.empty((1, C, s, s))
            ops.terrain_seed(Pd, 1, 1, s, 0, s, blend == 'bilinear', out)
            assert np.array_equal(out.numpy()[0], P[0, 0])
            dev.free(out.ptr)
    dev.free(Pd.ptr)


# ---- 2. emit --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,grey,W", [(1, True, 64), (1, True, 37), (3, False, 64), (3, False, 21), (3, True, 16)])
def test_emit_kernel_fp32_copy_and_uint8_map(dev, ops, C, grey, W):
    rng = np.random.RandomState(C * 100 + W)
    H = 11
    x = rng.uniform(-1.3, 1.3, (C, H, W)).astype(np.float32)
    x.ravel()[::7] = (rng.randint(0, 256, x.ravel()[::7].size) + 0.5).astype(np.float32) / np.float32(255)   # halfway
    x.ravel()[::11] = (rng.randint(0, 256, x.ravel()[::11].size) * np.float32(2) / np.float32(255) - np.float32(1))
    src = dev.tensor(x[None])
    for r0, n in ((0, H), (3, 5), (H - 1, 1)):
        out = dev.alloc(C * n * W * 4)
        ops.terrain_emit(src, r0, n, False, grey, out)
        got = np.empty((C, n, W), np.float32)
        dev.d2h(got, out, got.nbytes)
        assert np.array_equal(got, x[:, r0:r0 + n])
        ref = util.to_uint8(util.convert_to_rgb(x[:, r0:r0 + n], is_grayscale=grey))
        ref = ref[:, :, 0] if C == 1 else ref
        ops.terrain_emit(src, r0, n, True, grey, out)
        got8 = np.empty(ref.shape, np.uint8)
        dev.d2h(got8, out, got8.nbytes)
        assert np.array_equal(got8, ref), (r0, n)
        dev.free(out)
    dev.free(src.ptr)


# ---- 3-7. end to end ------------------------------------------------------------------------------------------------
def _small(dev, dtype, seed=5, **kw):
    return build_model(ostep.default_cfg(**SMALL), seed, dev, dtype=dtype, **kw)


@pytest.fixture(scope="module", params=["f32", "bf16x3"])
def small_model(request, dev):
    m = _small(dev, request.param, use_graph=False)
    # non-trivial BatchNorm running statistics (the deterministic pass reads them)
    cfg = ostep.default_cfg(**SMALL)
    for s in range(3):
        m.z_fn(ostep.synthetic_batch(4, cfg, seed=40 + s)[0])
    return m


@pytest.mark.parametrize("blend", TR.BLENDS)
def test_one_cell_is_z_fn_det(small_model, blend):
    m = small_model
    z = np.random.RandomState(3).rand(1, 1, m.latent_dim).astype(np.float32)
    ref = m.z_fn_det(z[0])[0]
    got = m.generate_terrain(z=z, blend=blend)
    assert got.shape == ref.shape and got.dtype == np.float32
    assert np.abs(got - ref).max() <= 1e-6
    print("1x1 %s %s: bit-identical to z_fn_det: %s" % (m.engine.dtype, blend, np.array_equal(got, ref)))


@pytest.mark.parametrize("grid", [(3, 2), (2, 5)])
@pytest.mark.parametrize("blend", TR.BLENDS)
def test_small_grids_against_the_float64_restatement(small_model, grid, blend):
    m = small_model
    z = np.random.RandomState(grid[0] * 7 + grid[1]).rand(grid[0], grid[1], m.latent_dim).astype(np.float32)
    got = m.generate_terrain(z=z, blend=blend)
    ref = R.terrain(m.dcgan['gen'], z.astype(np.float64), blend)
    assert got.shape == ref.shape == (1, 32 * grid[0], 32 * grid[1])
    assert rel(got, ref) < 1e-5                    # test_gpu_step's bound on z_fn_det
    # band=1: many windows, the same map
    b1 = m.generate_terrain(z=z, blend=blend, band=1)
    assert np.abs(b1 - got).max() <= 1e-6
    u8 = m.generate_terrain(z=z, blend=blend, uint8=True)
    assert np.array_equal(u8, util.to_uint8(util.convert_to_rgb(got, is_grayscale=True))[:, :, 0])


def test_grid_draws_from_the_sampler(small_model):
    m = small_model
    np.random.seed(17)
    a = m.generate_terrain(grid=(2, 3))
    np.random.seed(17)
    z = np.asarray(m.sampler(6, m.latent_dim), np.float32).reshape(2, 3, m.latent_dim)
    assert np.array_equal(a, m.generate_terrain(z=z))


def test_out_memmap_matches_the_returned_array(small_model, tmp_path):
    m = small_model
    z = np.random.RandomState(8).rand(5, 3, m.latent_dim).astype(np.float32)
    ref = m.generate_terrain(z=z, band=1)
    out = np.lib.format.open_memmap(str(tmp_path / "hm.npy"), mode="w+", dtype=np.float32, shape=ref.shape)
    assert m.generate_terrain(z=z, band=1, out=out) is out
    out.flush()
    assert np.array_equal(np.load(tmp_path / "hm.npy"), ref)
    with pytest.raises(ValueError):
        m.generate_terrain(z=z, out=np.zeros((1, 10, 10), np.float32))


def test_full_size_generator_banded_equals_one_window(dev):
    from gan_heightmaps_amd.experiments import make_model
    for dtype in ("f32", "bf16x3"):
        m = make_model('test1_nobn_bilin_both', device=dev, seed=0, verbose=False, use_graph=False, dtype=dtype)
        z = np.random.RandomState(2).rand(3, 2, m.latent_dim).astype(np.float32)
        geo = TR.TerrainGeometry(m.dcgan['gen'], 3, 2)
        assert len(geo.windows) == 1 and geo.halo == 4
        whole = m.generate_terrain(z=z)
        assert whole.shape == (1, 1536, 1024) and np.isfinite(whole).all()
        banded = m.generate_terrain(z=z, band=1)
        assert np.abs(banded - whole).max() <= 1e-6, dtype
        one = m.generate_terrain(z=z[:1, :1])
        assert np.abs(one - m.z_fn_det(z[0, :1])[0]).max() <= 1e-6


def test_terrain_leaves_the_training_state_untouched(dev):
    cfg = ostep.default_cfg(**SMALL)
    batches = [ostep.synthetic_batch(4, cfg, seed=s) for s in (1, 2)]
    z = np.random.RandomState(9).rand(2, 3, cfg['latent_dim']).astype(np.float32)
    runs = []
    for terrain in (False, True):
        m = build_model(cfg, 7, dev)                 # the default Pix2Pix: recorded / graph step
        losses = [m.train_fn(*batches[0])]
        if terrain:
            a = m.generate_terrain(z=z)
            m.generate_terrain(z=z, blend='mosaic', band=1, uint8=True)
        losses.append(m.train_fn(*batches[1]))
        if terrain:
            # the second step's parameters are what the next call sees, with nothing re-uploaded
            b = m.generate_terrain(z=z)
            assert not np.array_equal(a, b)
            assert rel(b, R.terrain(m.dcgan['gen'], z.astype(np.float64), 'bilinear')) < 1e-5
        runs.append((np.asarray(losses, np.float64), model_params(m)))
    assert np.array_equal(runs[0][0], runs[1][0])
    for k in runs[0][1]:
        for x, y in zip(runs[0][1][k], runs[1][1][k]):
            assert np.array_equal(x, y), k


def test_cli_end_to_end_with_texture(tmp_path, monkeypatch):
    from gan_heightmaps_amd import experiments
    cfg = ostep.default_cfg(**SMALL)
    src = build_model(cfg, 13, None, use_graph=False, dtype='f32')
    src.z_fn(ostep.synthetic_batch(4, cfg, seed=1)[0])
    src.save_model(str(tmp_path / "m.model"))
    np.random.seed(4)
    ref_hm = src.generate_terrain(grid=(3, 2))
    ref_tex = src.texture_heightmap(ref_hm, uint8=True, overlap=4, batch_size=2)
    src.device.close()
    monkeypatch.setattr(experiments, "make_model", lambda name, **kw: build_model(cfg, 99, None, use_graph=False, dtype=kw['dtype']))
    args = ["SMALL", str(tmp_path / "m.model"), str(tmp_path / "hm.npy"), "--cells", "3x2", "--seed", "4", "--dtype", "f32",
            "--texture", str(tmp_path / "tex.npy"), "--overlap", "4", "--batch-size", "2"]
    assert TR.main(args) == 0
    assert np.array_equal(np.load(tmp_path / "hm.npy"), ref_hm)
    assert np.array_equal(np.load(tmp_path / "tex.npy"), ref_tex)
    args = ["SMALL", str(tmp_path / "m.model"), str(tmp_path / "hm.png"), "--cells", "3x2", "--seed", "4", "--dtype", "f32",
            "--texture", str(tmp_path / "tex.png"), "--overlap", "4", "--batch-size", "2"]
    assert TR.main(args) == 0
    from PIL import Image
    assert np.array_equal(np.asarray(Image.open(tmp_path / "hm.png")),
                          util.to_uint8(util.convert_to_rgb(ref_hm, is_grayscale=True))[:, :, 0])
    assert np.array_equal(np.asarray(Image.open(tmp_path / "tex.png")), ref_tex)
