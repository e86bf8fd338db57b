"""The unbounded world on the MI355X (csrc/world.hip, gan_heightmaps_amd/world.py): the four kernels against the
host restatement (tests/world_ref.py), ghm_terrain_seed and util's uint8 map; TerrainWorld end to end against
generate_terrain crops, the float64 restatement, texture_heightmap and itself (request independence, bit for bit)."""
import numpy as np
import pytest

from oracle import step as ostep
from gan_heightmaps_amd import terrain as TR
from gan_heightmaps_amd import util
from gan_heightmaps_amd import world as WD
from tests import terrain_ref as R
from tests import world_ref as WR
from tests.gpu_common import build_model, dev, model_params, ops, rel, SMALL      # noqa: F401  (dev, ops: the module-scoped fixtures)

pytestmark = pytest.mark.gpu


# ---- 1. kernels -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,s", [(16, 4), (5, 4), (3, 3), (4, 2)])
def test_seed_kernel_against_the_restatement_and_terrain_seed(dev, ops, C, s):
    rng = np.random.RandomState(C * 10 + s)
    ci0, cj0, ncy, ncx = -4, -3, 7, 8
    P = rng.randn(ncy, ncx, C, s, s).astype(np.float32)
    Pd = dev.tensor(P.reshape(ncy * ncx, C * s * s))
    P64 = P.astype(np.float64)
    head = lambda i, j: P64[i - ci0, j - cj0]
    for blend in TR.BLENDS:
        bil = blend == 'bilinear'
        # rectangles inside the cells the table holds, both signs, odd sizes and origins
        ylo, yhi = (ci0 + bil) * s + (s // 2 if bil else 0), (ci0 + ncy - bil) * s - (s // 2 if bil else 0)
        xlo, xhi = (cj0 + bil) * s + (s // 2 if bil else 0), (cj0 + ncx - bil) * s - (s // 2 if bil else 0)
        for y0, x0, rows, cols in ((ylo, xlo, yhi - ylo, xhi - xlo), (-5, -3, 7, 9), (-1, 1, 3, 8), (ylo + 1, -2, 2, 4),
                                   (0, xlo, 1, 12)):
            out = dev.empty((1, C, rows, cols))
            ops.world_seed(Pd, ci0, cj0, ncy, ncx, s, y0, x0, bil, out)
            got = out.numpy()[0]
            want = WR.seed_rect(head, y0, x0, rows, cols, s, blend)
            if blend == 'mosaic':
                assert np.array_equal(got, want.astype(np.float32)), (y0, x0, rows, cols)
            else:
                assert np.abs(got - want).max() <= 1e-6 * max(1.0, np.abs(want).max()), (y0, x0, rows, cols)
            dev.free(out.ptr)
        # the interior of the finite canvas over the same cells: ghm_terrain_seed's values (bit for bit for s = 2^k)
        rows, cols = s * ncy - s, s * ncx - s
        fin = dev.empty((1, C, s * ncy, s * ncx))
        ops.terrain_seed(Pd, ncy, ncx, s, 0, s * ncy, bil, fin)
        f = fin.numpy()[0][:, s // 2:s // 2 + rows, :]
        for xa, wd in ((s // 2, cols), (s, 4 * ((cols - s) // 4))):        # scalar and 16-byte forms
            out = dev.empty((1, C, rows, wd))
            ops.world_seed(Pd, ci0, cj0, ncy, ncx, s, ci0 * s + s // 2, cj0 * s + xa, bil, out)
            got, want = out.numpy()[0], f[:, :, xa:xa + wd]
            if s & (s - 1) == 0 or not bil:
                assert np.array_equal(got, want), (blend, xa)
            else:
                assert np.abs(got - want).max() <= 1e-6 * max(1.0, np.abs(want).max())
            dev.free(out.ptr)
        dev.free(fin.ptr)
    # a rectangle that reads a cell outside the table is refused, not read
    from gan_heightmaps_amd._lib import GhmError
    out = dev.empty((1, C, 2, 4))
    for y0, x0, bil in ((ci0 * s - 1, 0, False), (0, (cj0 + ncx) * s - 3, False), (ci0 * s, 0, True),
                        ((ci0 + ncy) * s - 2, 0, True)):
        with pytest.raises(GhmError):
            ops.world_seed(Pd, ci0, cj0, ncy, ncx, s, y0, x0, bil, out)
    dev.free(out.ptr)
    dev.free(Pd.ptr)


@pytest.mark.parametrize("C,grey,K", [(1, True, 64), (1, True, 37), (3, False, 32), (3, False, 21), (3, True, 16)])
def test_emit_and_crop_kernels(dev, ops, C, grey, K):
    rng = np.random.RandomState(C * 100 + K)
    H, W = K + 9, K + 12
    x = rng.uniform(-1.3, 1.3, (C, H, W)).astype(np.float32)
    x.ravel()[::7] = (rng.randint(0, 256, x.ravel()[::7].size) + 0.5).astype(np.float32) / np.float32(255)   # halfway
    x.ravel()[::11] = (rng.randint(0, 256, x.ravel()[::11].size) * np.float32(2) / np.float32(255) - np.float32(1))
    src = dev.tensor(x[None])
    chunk = dev.alloc(C * K * K * 4)
    for r0, c0 in ((4, 8), (3, 5), (9, 12), (0, 0)):
        ops.world_emit(src, r0, c0, K, chunk)
        got = np.empty((C, K, K), np.float32)
        dev.d2h(got, chunk, got.nbytes)
        assert np.array_equal(got, x[:, r0:r0 + K, c0:c0 + K]), (r0, c0)
    ch = x[:, :K, :K]
    for r0, c0, nr, nc, pitch, xoff in ((0, 0, K, K, K, 0), (3, 5, 7, 9, 31, 11), (K - 1, K - 1, 1, 1, 4, 3),
                                        (4, 8, 5, 8, 24, 12), (2, 4, 3, 4, 9, 4), (0, 1, K, K - 1, K + 2, 0)):
        stage = dev.alloc(C * nr * pitch * 4)
        dev.memset_zero(stage, C * nr * pitch * 4)
        ops.world_crop(chunk, C, K, r0, c0, nr, nc, False, grey, stage, pitch, xoff)
        got = np.empty((C, nr, pitch), np.float32)
        dev.d2h(got, stage, got.nbytes)
        assert np.array_equal(got[:, :, xoff:xoff + nc], ch[:, r0:r0 + nr, c0:c0 + nc]), (r0, c0, nr, nc)
        assert not got[:, :, :xoff].any() and not got[:, :, xoff + nc:].any()          # nothing outside its columns
        ref = util.to_uint8(util.convert_to_rgb(ch[:, r0:r0 + nr, c0:c0 + nc], is_grayscale=grey))
        ref = ref[:, :, 0] if C == 1 else ref
        dev.memset_zero(stage, C * nr * pitch * 4)
        ops.world_crop(chunk, C, K, r0, c0, nr, nc, True, grey, stage, pitch, xoff)
        got8 = np.empty((nr, pitch) if C == 1 else (nr, pitch, 3), np.uint8)
        dev.d2h(got8, stage, got8.nbytes)
        assert np.array_equal(got8[:, xoff:xoff + nc], ref), (r0, c0, nr, nc)
        assert not got8[:, :xoff].any() and not got8[:, xoff + nc:].any()
        dev.free(stage)
    dev.free(chunk)
    dev.free(src.ptr)


@pytest.mark.parametrize("C,T,K", [(1, 32, 64), (3, 16, 16), (1, 12, 30), (2, 32, 32)])
def test_gather_kernel_copies_tiles_across_chunk_buffers(dev, ops, C, T, K):
    rng = np.random.RandomState(T + K)
    world = rng.randn(C, 2 * K, 2 * K).astype(np.float32)           # four chunk buffers side by side
    bufs = {}
    for a in (0, 1):
        for b in (0, 1):
            bufs[(a, b)] = dev.tensor(np.ascontiguousarray(world[:, a * K:(a + 1) * K, b * K:(b + 1) * K])[None])

    def tile(y, x, full=False):
        down, right = y + T > K, x + T > K
        ptrs = (bufs[(0, 0)].ptr, bufs[(0, 1)].ptr if right or full else 0, bufs[(1, 0)].ptr if down or full else 0,
                bufs[(1, 1)].ptr if (down and right) or full else 0)
        return (ptrs, y, x)
    for B, origins in ((4, [(0, 0), (0, K - T // 2), (K - T // 2, 0), (K - T // 4, K - T // 2)]),      # 1, 2, 2, 4 buffers
                       (4, [(K - T, K - T), (3, 5)]),                                                # ragged; odd origin
                       (3, [(K - 1, K - 1)]), (1, [(4, K - 4)])):
        origins = [(y, x) for y, x in origins if y < K and x < K]
        dst = dev.empty((B + 1, C, T, T)).samples(0, B)              # a view: the sample stride is honoured
        big = dev.empty((B, C + 1, T, T))
        for view in (dst, big.channels(0, C)):
            ops.world_gather([tile(y, x) for y, x in origins], K, view)
            got = view.numpy()
            for b in range(B):
                y, x = origins[min(b, len(origins) - 1)]
                assert np.array_equal(got[b], world[:, y:y + T, x:x + T]), (b, y, x)
        dev.free(dst.base.ptr)
        dev.free(big.ptr)
    from gan_heightmaps_amd._lib import GhmError
    dst = dev.empty((1, C, T, T))
    with pytest.raises(GhmError):                                    # a tile that runs into a chunk it has no buffer for
        ops.world_gather([((bufs[(0, 0)].ptr, 0, 0, 0), K - 1, 0)], K, dst)
    with pytest.raises(GhmError):
        ops.world_gather([((bufs[(0, 0)].ptr, 0, 0, 0), 0, K)], K, dst)
    dev.free(dst.ptr)
    for t in bufs.values():
        dev.free(t.ptr)


# ---- 2-5. end to end on SMALL ---------------------------------------------------------------------------------------
def _small(dev, dtype, seed=5, **kw):
    return build_model(ostep.default_cfg(**SMALL), seed, dev, dtype=dtype, **kw)


@pytest.fixture(scope="module", params=["f32", "bf16x3"])
def small_model(request, dev):
    m = _small(dev, request.param, use_graph=False)
    cfg = ostep.default_cfg(**SMALL)
    for s in range(3):                       # non-trivial BatchNorm running statistics (the deterministic pass reads them)
        m.z_fn(ostep.synthetic_batch(4, cfg, seed=40 + s)[0])
    return m


def _terrain_crop(m, world, y0, x0, h, w, blend='bilinear'):
    """the contract's reference on the device: generate_terrain over the covering cell block + margin, cropped"""
    geo = world.geometry
    i0, j0, ni, nj = WR.covering_block(geo, y0, x0, h, w)
    z = WR.latent_block(world.latent, i0, j0, ni, nj).astype(np.float32)
    full = m.generate_terrain(z=z, blend=blend)
    ya, xa = y0 - i0 * geo.out, x0 - j0 * geo.out
    return full[:, ya:ya + h, xa:xa + w]


REQ = (-70, 33, 150, 97)                     # 4 x 3 chunks of 64 pixels, both signs


@pytest.mark.parametrize("blend", TR.BLENDS)
def test_request_against_generate_terrain_and_the_restatement(small_model, blend):
    m = small_model
    with m.terrain_world(42, chunk_cells=2, blend=blend) as world:
        assert (world.chunk_cells, world.chunk_px, world.geometry.halo, world.geometry.s) == (2, 64, 4, 4)
        assert WD.axis_chunks(REQ[0], REQ[2], 64) == (-2, 1) and WD.axis_chunks(REQ[1], REQ[3], 64) == (0, 2)
        got = world.heightmap(*REQ)
        assert got.shape == (1, 150, 97) and got.dtype == np.float32 and world.computed == 12
        want = _terrain_crop(m, world, *REQ, blend=blend)
        d = np.abs(got - want).max()
        print("world %s %s: max |heightmap - generate_terrain crop| = %.3g" % (m.engine.dtype, blend, d))
        assert d <= 1e-6
        ref = WR.region(m.dcgan['gen'], world.latent, *REQ, blend)
        print("world %s %s: rel-L2 to the float64 restatement = %.3g" % (m.engine.dtype, blend, rel(got, ref)))
        assert rel(got, ref) < 1e-5
        u8 = world.heightmap(*REQ, uint8=True)
        assert np.array_equal(u8, util.to_uint8(util.convert_to_rgb(got, is_grayscale=True))[:, :, 0])


def test_requests_are_independent_bit_for_bit(small_model, tmp_path):
    m = small_model
    with m.terrain_world(42, chunk_cells=2) as world:
        a = world.heightmap(*REQ)
        n = world.computed
        # the same request from a warm cache computes nothing and returns the same bits
        assert np.array_equal(world.heightmap(*REQ), a) and world.computed == n
        # an overlapping request, other origin, other size
        b = world.heightmap(-10, 60, 100, 120)
        assert np.array_equal(b[:, :90, :70], a[:, 60:150, 27:97])
        # into an open_memmap
        out = np.lib.format.open_memmap(str(tmp_path / "hm.npy"), mode="w+", dtype=np.float32, shape=a.shape)
        assert world.heightmap(*REQ, out=out) is out
        out.flush()
        assert np.array_equal(np.load(tmp_path / "hm.npy"), a)
        with pytest.raises(ValueError):
            world.heightmap(*REQ, out=np.zeros((1, 10, 10), np.float32))
    with m.terrain_world(42, chunk_cells=2, cache_mb=0) as cold:
        assert np.array_equal(cold.heightmap(*REQ), a)
        n = cold.computed
        assert np.array_equal(cold.heightmap(-10, 60, 100, 120), b) and cold.computed > n      # nothing was kept
        assert not cold._chunks and not cold._heads
    with m.terrain_world(42, chunk_cells=2, cache_mb=0.05) as tiny:      # room for three chunks of 16 KB: evictions mid-request
        assert np.array_equal(tiny.heightmap(*REQ), a) and len(tiny._chunks) <= 3
        assert np.array_equal(tiny.heightmap(-10, 60, 100, 120), b)
    with m.terrain_world(42, chunk_cells=2) as fresh:
        assert np.array_equal(fresh.heightmap(*REQ), a)
    with m.terrain_world(43, chunk_cells=2) as other:
        assert not np.array_equal(other.heightmap(*REQ), a)
    for c in (1, 4):                                              # another chunk size: §4k's banded bound
        with m.terrain_world(42, chunk_cells=c) as w2:
            d = np.abs(w2.heightmap(*REQ) - a).max()
            print("world %s: chunk_cells %d vs 2: max abs %.3g" % (m.engine.dtype, c, d))
            assert d <= 1e-6


@pytest.mark.parametrize("o", [8, 0, 5])
def test_texture_against_texture_heightmap(small_model, o):
    m = small_model
    T = 32
    y0, x0, h, w = -41, 17, 90, 75
    with m.terrain_world(42, chunk_cells=2, overlap=o, batch_size=3) as world:
        tex = world.texture(y0, x0, h, w)
        assert tex.shape[1:] == (h, w) and tex.dtype == np.float32 and np.isfinite(tex).all()
        ey, ex, eh, ew = WR.tile_aligned_expansion(y0, x0, h, w, T, o)
        E = world.heightmap(ey, ex, eh, ew)
        whole = m.texture_heightmap(E, overlap=o, batch_size=3)
        want = whole[:, y0 - ey:y0 - ey + h, x0 - ex:x0 - ex + w]
        d = np.abs(tex - want).max()
        print("world %s overlap %d: max |texture - texture_heightmap crop| = %.3g, bit-identical: %s"
              % (m.engine.dtype, o, d, np.array_equal(tex, want)))
        assert d <= 1e-6
        u8 = world.texture(y0, x0, h, w, uint8=True)
        assert u8.shape == (h, w, 3) and np.array_equal(u8, util.to_uint8(util.convert_to_rgb(tex, is_grayscale=m.is_b_grayscale)))
        # overlapping texture requests agree bit for bit; so does another batch size's slotting of the same tiles' values
        t2 = world.texture(y0 + 30, x0 - 20, 64, 70)
        assert np.array_equal(t2[:, :60, 20:], tex[:, 30:, :50])
        hm = world.heightmap(y0, x0, h, w)
        bh, bt = world.both(y0, x0, h, w)
        assert np.array_equal(bh, hm) and np.array_equal(bt, tex)
        bh8, bt8 = world.both(y0, x0, h, w, uint8=True)
        assert np.array_equal(bt8, u8) and np.array_equal(bh8, world.heightmap(y0, x0, h, w, uint8=True))
    with m.terrain_world(42, chunk_cells=2, overlap=o, batch_size=3, cache_mb=0) as cold:
        bh, bt = cold.both(y0, x0, h, w)
        assert np.array_equal(bh, hm) and np.array_equal(bt, tex)
    with pytest.raises(NotImplementedError, match="deterministic"):
        m.terrain_world(42, deterministic=False)


def test_world_stays_fresh_and_leaves_the_training_state_untouched(dev):
    cfg = ostep.default_cfg(**SMALL)
    batches = [ostep.synthetic_batch(4, cfg, seed=s) for s in (1, 2)]
    req = (-20, 10, 70, 50)
    runs = []
    for with_world in (False, True):
        m = build_model(cfg, 7, dev)                 # the default Pix2Pix: recorded / graph step
        world = m.terrain_world(3, chunk_cells=2)
        losses = [m.train_fn(*batches[0])]
        if with_world:
            a = world.heightmap(*req)
            world.both(*req, uint8=True)
            n = world.computed
            assert np.array_equal(world.heightmap(*req), a) and world.computed == n
        losses.append(m.train_fn(*batches[1]))
        if with_world:
            b = world.heightmap(*req)                # the cache was dropped: the second step's parameters
            assert world.computed > n and not np.array_equal(a, b)
            assert rel(b, WR.region(m.dcgan['gen'], world.latent, *req, 'bilinear')) < 1e-5
            # a host write to a parameter is seen too
            p = [q for q in m.engine.stores['dcgan_gen'].params if 'trainable' in q.tags][-1]
            v = p.get_value()
            p.set_value(v + 0.1)
            c = world.heightmap(*req)
            assert not np.array_equal(b, c)
            p.set_value(v)
            assert np.array_equal(world.heightmap(*req), b)
        world.close()
        runs.append((np.asarray(losses, np.float64), model_params(m)))
    assert np.array_equal(runs[0][0], runs[1][0])
    for k in runs[0][1]:
        for x, y in zip(runs[0][1][k], runs[1][1][k]):
            assert np.array_equal(x, y), k


# ---- 6. full size ---------------------------------------------------------------------------------------------------
def test_full_size_generator_chunks_against_generate_terrain(dev):
    from gan_heightmaps_amd.experiments import make_model
    for dtype in ("f32", "bf16x3"):
        m = make_model('test1_nobn_bilin_both', device=dev, seed=0, verbose=False, use_graph=False, dtype=dtype)
        assert m.terrain_world(1).chunk_cells == 4
        with m.terrain_world(11, chunk_cells=1) as world:
            assert world.chunk_px == 512 and world.geometry.halo == 4
            one = world.heightmap(-512, 0, 512, 512)                 # chunk (-1, 0), whole
            assert one.shape == (1, 512, 512) and np.isfinite(one).all()
            d = np.abs(one - _terrain_crop(m, world, -512, 0, 512, 512)).max()
            print("full size %s: one chunk vs generate_terrain crop: max abs %.3g" % (dtype, d))
            assert d <= 1e-6, dtype
            req = (-100, 450, 200, 130)                              # crosses the corner of chunks (-1, 0) (0, 0) (-1, 1) (0, 1)
            got = world.heightmap(*req)
            assert np.isfinite(got).all() and world.computed == 4
            d = np.abs(got - _terrain_crop(m, world, *req)).max()
            print("full size %s: corner request vs generate_terrain crop: max abs %.3g" % (dtype, d))
            assert d <= 1e-6, dtype
            assert np.array_equal(got[:, :100, :62], one[:, 412:, 450:])


# ---- 7. command line ------------------------------------------------------------------------------------------------
def test_cli_end_to_end_with_texture(tmp_path, monkeypatch):
    from gan_heightmaps_amd import experiments
    cfg = ostep.default_cfg(**SMALL)
    src = build_model(cfg, 13, None, use_graph=False, dtype='f32')
    src.z_fn(ostep.synthetic_batch(4, cfg, seed=1)[0])
    src.save_model(str(tmp_path / "m.model"))
    with src.terrain_world(4, chunk_cells=2, overlap=4, batch_size=2) as world:
        ref_hm = world.heightmap(-70, 33, 90, 61)
        ref_tex = world.texture(-70, 33, 90, 61, uint8=True)
    src.device.close()
    monkeypatch.setattr(experiments, "make_model", lambda name, **kw: build_model(cfg, 99, None, use_graph=False, dtype=kw['dtype']))
    common = ["--seed", "4", "--region", "-70,33,90,61", "--chunk-cells", "2", "--dtype", "f32", "--overlap", "4",
              "--batch-size", "2"]
    args = ["SMALL", str(tmp_path / "m.model"), str(tmp_path / "hm.npy"), "--texture", str(tmp_path / "tex.npy")] + common
    assert WD.main(args) == 0
    assert np.array_equal(np.load(tmp_path / "hm.npy"), ref_hm)
    assert np.array_equal(np.load(tmp_path / "tex.npy"), ref_tex)
    args = ["SMALL", str(tmp_path / "m.model"), str(tmp_path / "hm.png"), "--texture", str(tmp_path / "tex.png")] + common
    assert WD.main(args) == 0
    from PIL import Image
    assert np.array_equal(np.asarray(Image.open(tmp_path / "hm.png")),
                          util.to_uint8(util.convert_to_rgb(ref_hm, is_grayscale=True))[:, :, 0])
    assert np.array_equal(np.asarray(Image.open(tmp_path / "tex.png")), ref_tex)
