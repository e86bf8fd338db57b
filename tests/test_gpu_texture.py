"""Tiled texturing on the MI355X (csrc/texture.hip, gan_heightmaps_amd/texture.py): the gather / blend /
finalize kernels against ghm_image_batch and the float64 host restatement (tests/texture_ref.py), and
Pix2Pix.texture_heightmap end to end against gen_fn_det on the same tiles."""
import numpy as np
import pytest

from oracle import step as ostep
from gan_heightmaps_amd import texture as TX
from gan_heightmaps_amd import util
from tests import texture_ref as R
from tests.gpu_common import build_model, dev, model_params, ops, SMALL      # noqa: F401  (dev, ops: the module-scoped fixtures)

pytestmark = pytest.mark.gpu


def _upload_bytes(dev, arr):
    arr = np.ascontiguousarray(arr)
    p = dev.alloc(arr.nbytes)
    dev.h2d(p, arr)
    return p


# ---- 1. gather ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,tanh", [(1, False), (3, True)])
def test_gather_interior_crop_equals_image_batch(dev, ops, C, tanh):
    rng = np.random.RandomState(C)
    H, W, T = 90, 130, 32
    img = rng.randint(0, 256, (H, W, C)).astype(np.uint8)
    y0, x0, s, B = 20, 11, 24, 3
    band = _upload_bytes(dev, img)
    got = dev.empty((B, C, T, T))
    ops.texture_gather(band, True, C, H, 0, H, W, y0, x0, s, B, tanh, got)
    crops = np.stack([img[y0:y0 + T, x0 + b * s:x0 + b * s + T] for b in range(B)])
    src = _upload_bytes(dev, crops)
    xf = _upload_bytes(dev, np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0], np.float64), B))
    ref = dev.empty((B, C, T, T))
    ops.image_batch(src, B, T, T, C, xf, tanh, ref)
    assert np.array_equal(got.numpy(), ref.numpy())
    for p in (band, src, xf):
        dev.free(p)


@pytest.mark.parametrize("C,tanh", [(1, False), (3, True)])
def test_gather_border_tiles_reflect_and_normalise(dev, ops, C, tanh):
    rng = np.random.RandomState(10 + C)
    H, W, T, o = 45, 70, 32, 8
    img = rng.randint(0, 256, (H, W, C)).astype(np.uint8)
    xn = R.normalise_u8(img, not tanh)
    py, px = TX.axis_plan(H, T, o), TX.axis_plan(W, T, o)
    for iy in range(py.n):
        rows = TX.reflect_index(np.arange(py.start(iy), py.start(iy) + T), H)
        lo, hi = int(rows.min()), int(rows.max()) + 1
        band = _upload_bytes(dev, img[lo:hi])         # only the rows this tile row needs
        got = dev.empty((px.n + 1, C, T, T))
        # a batch one longer than the row: the extra slot repeats the last tile
        ops.texture_gather(band, True, C, hi - lo, lo, H, W, py.start(iy), px.start(0), T - o, px.n, tanh, got)
        g = got.numpy()
        for j in range(px.n + 1):
            ref = R.host_tile(xn, py, px, iy, min(j, px.n - 1))
            assert np.array_equal(g[j], ref), (iy, j)
        dev.free(band)


def test_gather_fp32_input_is_copied_exactly_and_honours_the_sample_stride(dev, ops):
    rng = np.random.RandomState(3)
    C, H, W, T, o = 3, 50, 41, 32, 16
    x = rng.standard_normal((C, H, W)).astype(np.float32)
    py, px = TX.axis_plan(H, T, o), TX.axis_plan(W, T, o)
    band = _upload_bytes(dev, x)
    wide = dev.tensor(np.full((2, C + 2, T, T), 7.0, np.float32))
    view = wide.channels(1, 1 + C)                   # sample stride (C + 2) T T: a slice of a wider buffer
    ops.texture_gather(band, False, C, H, 0, H, W, py.start(1), px.start(0), T - o, 2, False, view)
    w = wide.numpy()
    for j in range(2):
        assert np.array_equal(w[j, 1:1 + C], R.host_tile(x, py, px, 1, j))
    assert (w[:, 0] == 7).all() and (w[:, 1 + C:] == 7).all()
    dev.free(band)


# ---- 2. blend + finalize on random tile stacks ----------------------------------------------------------------------
def _blend_on_device(dev, ops, U, py, px, nb, uint8=False, b_grey=False):
    """drive blend / finalize over a whole canvas as the executor does (batches of nb tiles, o rows carried)"""
    ny, nx, C, T = U.shape[0], U.shape[1], U.shape[2], U.shape[3]
    H, W, o, s = py.L, px.L, py.o, py.s
    acc = dev.alloc(C * T * W * 4)
    dev.memset_zero(acc, C * T * W * 4)
    out = np.zeros((H, W, 3), np.uint8) if uint8 else np.zeros((C, H, W), np.float32)
    for iy in range(ny):
        y0 = py.start(iy)
        for j0, nv in TX.tile_batches(nx, nb):
            u = dev.tensor(np.ascontiguousarray(U[iy, j0:j0 + nv]))
            ops.texture_blend(acc, W, T, C, u, nv, iy, ny, j0, nx, px.pad, o)
            dev.sync()
            dev.free(u.ptr)
        last = iy == ny - 1
        r_lo, r_hi = max(0, -y0), min(T if last else s, H - y0)
        if r_hi > r_lo:
            n = r_hi - r_lo
            nbytes = n * W * (3 if uint8 else 4 * C)
            st = dev.alloc(nbytes)
            ops.texture_finalize(acc, W, T, C, r_lo, n, y0, ny, py.pad, nx, px.pad, o, uint8, b_grey, st)
            buf = np.empty(nbytes, np.uint8)
            dev.d2h(buf, st, nbytes)
            dev.free(st)
            if uint8:
                out[y0 + r_lo:y0 + r_hi] = buf.reshape(n, W, 3)
            else:
                out[:, y0 + r_lo:y0 + r_hi] = buf.view(np.float32).reshape(C, n, W)
        if not last:
            for c in range(C):
                base = acc + c * T * W * 4
                if o:
                    dev.d2d(base, base + s * W * 4, o * W * 4)
                dev.memset_zero(base + o * W * 4, (T - o) * W * 4)
    dev.free(acc)
    return out


@pytest.mark.parametrize("o", [0, 4, 8, 16])
@pytest.mark.parametrize("H,W,C,nb", [(75, 101, 3, 2), (32, 32, 1, 1), (20, 130, 1, 4), (130, 64, 3, 3)])
def test_blend_finalize_against_the_float64_restatement(dev, ops, H, W, C, nb, o):
    T = 32
    rng = np.random.RandomState(H + W + o)
    py, px = TX.axis_plan(H, T, o), TX.axis_plan(W, T, o)
    U = rng.uniform(-1.2, 1.2, (py.n, px.n, C, T, T)).astype(np.float32)
    got = _blend_on_device(dev, ops, U, py, px, nb)
    ref = R.blend_gather(py, px, U)
    assert np.abs(got - ref).max() <= 1e-6
    m = R.single_cover_mask(py, px)
    assert np.array_equal(got[:, m], R.single_cover_values(py, px, U)[:, m])
    if o == 0:
        assert np.array_equal(got, R.single_cover_values(py, px, U))
    for b_grey in (False, True):
        u8 = _blend_on_device(dev, ops, U, py, px, nb, uint8=True, b_grey=b_grey)
        assert np.array_equal(u8, util.to_uint8(util.convert_to_rgb(got, is_grayscale=b_grey)))


# ---- 3-7. end to end ------------------------------------------------------------------------------------------------
def _small(dev, dtype, seed=5, **kw):
    return build_model(ostep.default_cfg(**SMALL), seed, dev, dtype=dtype, **kw)


@pytest.fixture(scope="module", params=["f32", "bf16x3"])
def small_model(request, dev):
    return _small(dev, request.param, use_graph=False)


def test_single_tile_canvas_is_gen_fn_det(small_model):
    m = small_model
    T = m.in_shp
    x = np.random.RandomState(1).randint(0, 256, (T, T)).astype(np.uint8)
    ref = m.gen_fn_det(R.normalise_u8(x, m.is_a_grayscale)[None])[0]
    for o in (0, 1, T // 8, T // 4, T // 2):
        got = m.texture_heightmap(x, overlap=o, batch_size=1)
        assert got.dtype == np.float32 and got.shape == ref.shape
        assert np.array_equal(got, ref), o


@pytest.mark.parametrize("batch_size", [1, 3])
@pytest.mark.parametrize("ofrac", [0, 4, 2])
def test_canvas_against_host_restatement(small_model, batch_size, ofrac):
    m = small_model
    T = m.in_shp
    o = T // ofrac if ofrac else 0
    x = np.random.RandomState(2).randint(0, 256, (150, 230)).astype(np.uint8)
    got = m.texture_heightmap(x, overlap=o, batch_size=batch_size)
    py, px, U = R.tile_outputs(m.gen_fn_det, R.normalise_u8(x, m.is_a_grayscale), T, o, batch_size)
    ref = R.blend_gather(py, px, U)
    assert np.abs(got - ref).max() <= 1e-6
    mask = R.single_cover_mask(py, px)
    assert np.array_equal(got[:, mask], R.single_cover_values(py, px, U)[:, mask])
    u8 = m.texture_heightmap(x, overlap=o, batch_size=batch_size, uint8=True)
    assert np.array_equal(u8, util.to_uint8(util.convert_to_rgb(got, is_grayscale=m.is_b_grayscale)))
    # float32 input already normalised: the same texture
    f = m.texture_heightmap(R.normalise_u8(x, m.is_a_grayscale), overlap=o, batch_size=batch_size)
    assert np.array_equal(f, got)


def test_streaming_from_memmap_and_constant_device_memory(small_model, tmp_path, monkeypatch):
    from gan_heightmaps_amd import device
    m = small_model
    T = m.in_shp
    H, W = 7 * T + 5, 3 * T - 3
    x = np.random.RandomState(4).randint(0, 256, (4 * H, W)).astype(np.uint8)
    np.save(tmp_path / "in.npy", x)
    xin = np.load(tmp_path / "in.npy", mmap_mode="r")
    mem = m.texture_heightmap(np.ascontiguousarray(x), uint8=True, batch_size=2)
    out = np.lib.format.open_memmap(str(tmp_path / "out.npy"), mode="w+", dtype=np.uint8, shape=(4 * H, W, 3))
    assert m.texture_heightmap(xin, uint8=True, batch_size=2, out=out) is out
    out.flush()
    assert np.array_equal(np.load(tmp_path / "out.npy"), mem)
    # device memory of the call: the same for H and 4H (the forward plan is already built)
    seen = []
    orig = device.Device.alloc

    def alloc(self, nbytes):
        seen.append(nbytes)
        return orig(self, nbytes)
    monkeypatch.setattr(device.Device, "alloc", alloc)
    per_h = []
    for h in (H, 4 * H):
        seen.clear()
        m.texture_heightmap(np.ascontiguousarray(x[:h]), batch_size=2)
        per_h.append(sum(seen))
    assert per_h[0] == per_h[1] > 0


def test_input_and_option_errors(small_model):
    m = small_model
    x = np.zeros((40, 40), np.uint8)
    with pytest.raises(NotImplementedError):
        m.texture_heightmap(x, deterministic=False)
    with pytest.raises(ValueError):
        m.texture_heightmap(x, overlap=m.in_shp // 2 + 1)
    with pytest.raises(ValueError):
        m.texture_heightmap(np.zeros((40, 40, 3), np.uint8))
    with pytest.raises(ValueError):
        m.texture_heightmap(x, out=np.zeros((40, 40, 3), np.float32))


def test_texturing_leaves_the_training_state_untouched(dev):
    cfg = ostep.default_cfg(**SMALL)
    batches = [ostep.synthetic_batch(4, cfg, seed=s) for s in (1, 2)]
    x = np.random.RandomState(9).randint(0, 256, (70, 90)).astype(np.uint8)
    runs = []
    for texture in (False, True):
        m = build_model(cfg, 7, dev)                 # the default Pix2Pix: recorded / graph step
        losses = [m.train_fn(*batches[0])]
        if texture:
            m.texture_heightmap(x, batch_size=3)
            m.texture_heightmap(x, batch_size=2, uint8=True)
        losses.append(m.train_fn(*batches[1]))
        runs.append((np.asarray(losses, np.float64), model_params(m)))
    assert np.array_equal(runs[0][0], runs[1][0])
    for k in runs[0][1]:
        for a, b in zip(runs[0][1][k], runs[1][1][k]):
            assert np.array_equal(a, b), k


def test_full_size_unet_on_a_large_canvas(dev):
    from gan_heightmaps_amd.experiments import make_model
    m = make_model('test1_nobn_bilin_both', device=dev, seed=0, verbose=False, use_graph=False)
    x = np.random.RandomState(6).randint(0, 256, (1100, 1300)).astype(np.uint8)
    got = m.texture_heightmap(x)
    assert got.shape == (3, 1100, 1300) and np.isfinite(got).all()
    py, px, U = R.tile_outputs(m.gen_fn_det, R.normalise_u8(x, True), 512, 128, 4)
    mask = R.single_cover_mask(py, px)
    assert mask.any()
    assert np.array_equal(got[:, mask], R.single_cover_values(py, px, U)[:, mask])
    assert np.abs(got - R.blend_gather(py, px, U)).max() <= 1e-5
