"""Adaptive meshes on the device (csrc/mesh.hip, gan_heightmaps_amd/mesh.py): the error plane and the extraction
against the per-vertex restatement of tests/mesh_ref.py, bit for bit, in both forms of the error kernels, at the smallest
shapes where each mechanism can go wrong; meshes of the unbounded world that stitch."""
import numpy as np
import pytest

from oracle import step as ostep
from gan_heightmaps_amd import mesh as MS
from tests import mesh_ref as M
from tests.gpu_common import build_model, dev, ops, SMALL      # noqa: F401  (dev, ops: the module-scoped fixtures)

pytestmark = pytest.mark.gpu


# (seed, rows, cols, k): T = 2, 4, 8 have k <= the fused levels, so the root-diagonal rule applies inside the fused block;
# 17 x 17 is smaller than a block; 65 x 65 is exactly one block and its shared edge; 81 x 97 has blocks cut by the plane's
# edge; 129 x 257 has plain scales above the fused ones and two tiles that share a border
CASES = ((1, 5, 7, 1), (2, 9, 13, 2), (3, 17, 25, 3), (4, 17, 17, 4), (5, 65, 65, 6), (6, 81, 97, 4), (7, 129, 257, 7))
TOLS = (0.0, 0.02, 1.0)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_errors_and_meshes_against_the_restatement(ops, case, fused):
    seed, rows, cols, k = CASES[case]
    h, e = M.case(seed, rows, cols, k)
    faces = []
    with MS.ErrorMap(ops, h, tile=1 << k, fused=fused) as em:
        got = em.errors()
        assert got.tobytes() == e.tobytes(), int((got != e).sum())
        for tol in TOLS:
            g, hh, t = M.case_mesh(seed, rows, cols, k, tol)
            m = em.extract(tol)
            assert em.count(tol) == (m.vertices, m.faces) == (len(g), len(t))
            assert np.array_equal(m.grid, g) and m.heights.tobytes() == hh.tobytes() and np.array_equal(m.triangles, t)
            assert (m.shape, m.origin, m.tile, m.max_error, m.valid_shape) == ((rows, cols), (0, 0), 1 << k, tol, (rows, cols))
            faces.append(m.faces)
    # one map, three tolerances: the triangles do not grow with the tolerance, from every pixel's two down to two per tile
    assert faces[0] >= faces[1] >= faces[2] == 2 * ((rows - 1) >> k) * ((cols - 1) >> k)
    assert faces[0] > faces[1] > faces[2] or k == 1


@pytest.mark.parametrize("fused", [False, True])
def test_pitches_beyond_the_widths_and_a_rectangle_of_tiles(dev, ops, fused):
    seed, rows, cols, k = 9, 49, 65, 4
    h, e = M.case(seed, rows, cols, k)
    pitch, err_pitch, rect, tol = cols + 5, cols + 3, (16, 16, 16, 32), 0.015
    wide = np.full((rows, pitch), np.nan, np.float32)
    wide[:, :cols] = h
    errs = np.full((rows, err_pitch), np.nan, np.float32)
    g, hh, t = M.extract(h, e, k, tol, rect)
    y0, x0, hr, wr = rect
    bufs = [dev.alloc(n) for n in (wide.nbytes, errs.nbytes, ops.mesh_workspace(hr, wr), 4 * (hr + 1) * (wr + 1), 8 * len(g),
                                   4 * len(g), 12 * len(t))]
    try:
        src, err, ws, index, d_grid, d_heights, d_tris = bufs
        dev.h2d(src, wide)
        dev.h2d(err, errs)
        ops.mesh_errors(src, rows, cols, pitch, k, fused, err, err_pitch)
        dev.sync()
        dev.d2h(errs, err, errs.nbytes)
        assert np.isnan(errs[:, cols:]).all() and errs[:, :cols].tobytes() == e.tobytes()    # the cells beyond stay untouched
        assert ops.mesh_count(err, rows, cols, err_pitch, k, y0, x0, hr, wr, tol, ws) == (len(g), len(t))
        ops.mesh_extract(src, pitch, err, rows, cols, err_pitch, k, y0, x0, hr, wr, tol, ws, index, d_grid, d_heights, d_tris,
                         len(g), len(t))
        dev.sync()
        grid, heights, tris = np.empty(g.shape, g.dtype), np.empty(hh.shape, hh.dtype), np.empty(t.shape, t.dtype)
        for host, ptr in ((grid, d_grid), (heights, d_heights), (tris, d_tris)):
            dev.d2h(host, ptr, host.nbytes)
        assert np.array_equal(grid, g) and heights.tobytes() == hh.tobytes() and np.array_equal(tris, t)
        # totals that are not the mesh's are refused, with nothing written
        from gan_heightmaps_amd._lib import GhmError
        with pytest.raises(GhmError, match="the arrays hold"):
            ops.mesh_extract(src, pitch, err, rows, cols, err_pitch, k, y0, x0, hr, wr, tol, ws, index, d_grid, d_heights,
                             d_tris, len(g) - 1, len(t))
        for bad in (dict(rows=rows + 1), dict(k=0), dict(k=13), dict(pitch=cols - 1), dict(err_pitch=cols - 1), dict(src=None)):
            a = dict(src=src, rows=rows, cols=cols, pitch=pitch, k=k, err_pitch=err_pitch)
            a.update(bad)
            with pytest.raises(GhmError):
                ops.mesh_errors(a["src"], a["rows"], a["cols"], a["pitch"], a["k"], fused, err, a["err_pitch"])
        for bad_tol in (-1.0, float("nan"), float("inf")):
            with pytest.raises(GhmError, match="max_error"):
                ops.mesh_count(err, rows, cols, err_pitch, k, y0, x0, hr, wr, bad_tol, ws)
        with pytest.raises(GhmError, match="rectangle"):
            ops.mesh_count(err, rows, cols, err_pitch, k, y0, x0 + 8, hr, wr, tol, ws)
    finally:
        dev.sync()
        for p in bufs:
            dev.free(p)


# ---- the model's entry points ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_model(dev):
    m = build_model(ostep.default_cfg(**SMALL), 5, dev, dtype="f32", use_graph=False)
    cfg = ostep.default_cfg(**SMALL)
    for s in range(3):                       # non-trivial BatchNorm running statistics (the deterministic pass reads them)
        m.z_fn(ostep.synthetic_batch(4, cfg, seed=40 + s)[0])
    return m


def test_heightmap_mesh_of_a_size_that_does_not_fit(small_model):
    hm = M.terrain(11, 40, 52)
    plane, valid = MS.fit(hm, 32)
    e = M.errors(plane, 5)
    for tol, fused in ((0.01, None), (0.05, False)):
        m = small_model.heightmap_mesh(hm[None], tol, fused=fused)                 # tile=None: 32, fitted to 65 x 65
        g, hh, t = M.extract(plane, e, 5, tol)
        assert np.array_equal(m.grid, g) and np.array_equal(m.heights, hh) and np.array_equal(m.triangles, t)
        assert (m.shape, m.tile, m.valid_shape) == ((65, 65), 32, (40, 52)) and valid == (40, 52)
    u8 = (hm * 255).astype(np.uint8)
    m8 = small_model.heightmap_mesh(u8, 0.01, tile=8)
    assert m8.shape == (41, 57) and np.array_equal(m8.heights, (u8.astype(np.float32) / np.float32(255))[
        np.minimum(m8.grid[:, 0], 39), np.minimum(m8.grid[:, 1], 51)])


def _points(m):
    return M.as_points(m.grid, m.triangles, m.origin), m.heights[m.triangles.astype(np.int64)]


def _check_world(world, counter):
    T, tol = 32, 0.01
    big_rect, left_rect, right_rect = (-64, 0, 64, 96), (-64, 0, 64, 64), (-64, 64, 64, 32)
    big = world.mesh(*big_rect, max_error=tol, tile=T)
    done = (world.computed, world.eroded)
    # the grown rectangle [-96, 32] x [-32, 128] touches 3 x 4 chunks of 64 pixels: each is made once
    assert counter(world) == 12
    left, right = world.mesh(*left_rect, max_error=tol, tile=T), world.mesh(*right_rect, max_error=tol, tile=T, fused=False)
    assert (world.computed, world.eroded) == done                                  # ... and never again
    assert (left.origin, left.shape, right.origin, right.shape) == ((-64, 0), (65, 65), (-64, 64), (65, 33))
    # the mesh's heights are the world's, as a scene maps them
    with world.scene(-64, 0, 65, 97) as scene:
        plane = scene.arrays()[0]
    assert np.array_equal(big.heights, plane[big.grid[:, 0], big.grid[:, 1]])
    # the shared border: the same vertices with the same heights
    lb, rb = left.grid[:, 1] == 64, right.grid[:, 1] == 0
    assert lb.sum() >= 3 and np.array_equal(left.grid[lb, 0], right.grid[rb, 0])
    assert left.heights[lb].tobytes() == right.heights[rb].tobytes()
    # each is the part of the larger mesh inside it, in the same order, in world coordinates
    pw, vw = _points(big)
    for part, r in ((left, left_rect), (right, right_rect)):
        p, v = _points(part)
        inside = ((pw[:, :, 0] >= r[0]) & (pw[:, :, 0] <= r[0] + r[2]) & (pw[:, :, 1] >= r[1]) &
                  (pw[:, :, 1] <= r[1] + r[3])).all(1)
        assert np.array_equal(p, pw[inside]) and v.tobytes() == vw[inside].tobytes()
    union = np.concatenate([_points(left)[0], _points(right)[0]])
    assert M.multiset(union) == M.multiset(pw) and M.bad_edges(union, big_rect) == 0
    assert 2 * 6 < big.faces < 2 * 64 * 96
    # against the restatement, from the world's own pixels
    grown = world.scene(-96, -32, 129, 161)
    try:
        g = grown.arrays()[0]
    finally:
        grown.close()
    want = M.extract(g, M.errors(g, 5), 5, tol, (T, T, 64, 96))
    assert np.array_equal(big.grid, want[0]) and np.array_equal(big.heights, want[1]) and np.array_equal(big.triangles, want[2])
    return big


def test_world_meshes_stitch_bit_for_bit(small_model):
    with small_model.terrain_world(42, chunk_cells=2) as world:
        big = _check_world(world, lambda w: w.computed)
        m, tex = world.mesh(-64, 0, 64, 96, max_error=0.01, tile=32, texture=True)
        assert np.array_equal(m.triangles, big.triangles) and tex.shape == (65, 97, 3) and tex.dtype == np.uint8
        assert np.array_equal(tex, world.texture(-64, 0, 65, 97, uint8=True))
        with pytest.raises(ValueError, match="multiple of the tile"):
            world.mesh(-64, 0, 64, 90, max_error=0.01, tile=32)


def test_an_eroded_world_meshes_as_the_eroded_world(small_model):
    from tests.gpu_common import ERO
    with small_model.terrain_world(42, chunk_cells=2, erosion=ERO) as world, small_model.terrain_world(42, chunk_cells=2) as raw:
        big = _check_world(world, lambda w: w.eroded)
        plain = raw.mesh(-64, 0, 64, 96, max_error=0.01, tile=32)
        assert plain.vertices != big.vertices or not np.array_equal(plain.heights, big.heights)     # the erosion is not idle


# ---- command lines --------------------------------------------------------------------------------------------------------
def _glb(path):
    """(vertices, triangles, has an embedded PNG) of a written .glb"""
    import json
    import struct
    raw = open(path, "rb").read()
    n, = struct.unpack_from("<I", raw, 12)
    doc = json.loads(raw[20:20 + n].decode("utf-8"))
    prim, = doc["meshes"][0]["primitives"]
    png = False
    if "images" in doc:
        view = doc["bufferViews"][doc["images"][0]["bufferView"]]
        png = raw[28 + n + view["byteOffset"]:][:8] == b"\x89PNG\r\n\x1a\n"
    return doc["accessors"][prim["attributes"]["POSITION"]]["count"], doc["accessors"][prim["indices"]]["count"] // 3, png


def test_mesh_cli_turns_a_png_and_its_texture_into_a_glb(tmp_path):
    from PIL import Image
    hm = (M.terrain(21, 512, 512) * 255).astype(np.uint8)
    Image.fromarray(hm).save(tmp_path / "hm.png")
    Image.fromarray(np.stack([hm, hm // 2, 255 - hm], -1)).save(tmp_path / "tex.png")
    faces = []
    for tol, form in (("0.01", "--plain"), ("0.03", "--fused"), ("0.1", "--plain")):
        out = tmp_path / ("land_%s.glb" % tol)
        assert MS.main([str(tmp_path / "hm.png"), str(out), "--texture", str(tmp_path / "tex.png"), "--max-error", tol, form]) == 0
        V, F, png = _glb(out)
        assert png and 4 <= V <= 513 * 513 and 2 * 4 <= F
        faces.append(F)
    assert 2 * 512 * 512 > faces[0] > faces[1] > faces[2] >= 8                     # fewer triangles as the tolerance rises
    assert MS.main([str(tmp_path / "hm.png"), str(tmp_path / "land.npz"), "--max-error", "0.03", "--tile", "64"]) == 0
    z = np.load(tmp_path / "land.npz")
    assert tuple(z["shape"]) == (513, 513) and tuple(z["valid_shape"]) == (512, 512) and int(z["tile"]) == 64
    assert np.array_equal(z["heights"], (MS.fit(hm, 64)[0].astype(np.float32) / np.float32(255))[z["grid"][:, 0], z["grid"][:, 1]])


def test_world_cli_writes_meshes_that_share_their_border(tmp_path, monkeypatch):
    from gan_heightmaps_amd import experiments
    from gan_heightmaps_amd import world as WD
    cfg = ostep.default_cfg(**SMALL)
    src = build_model(cfg, 13, None, use_graph=False, dtype='f32')
    src.z_fn(ostep.synthetic_batch(4, cfg, seed=1)[0])
    src.save_model(str(tmp_path / "m.model"))
    with src.terrain_world(4, chunk_cells=2, overlap=4, batch_size=2) as world:
        want, tex = world.mesh(-32, 32, 64, 32, max_error=0.02, tile=32, texture=True)
    src.device.close()
    monkeypatch.setattr(experiments, "make_model", lambda name, **kw: build_model(cfg, 99, None, use_graph=False, dtype=kw['dtype']))
    common = ["--seed", "4", "--chunk-cells", "2", "--dtype", "f32", "--max-error", "0.02", "--tile", "32"]
    args = ["SMALL", str(tmp_path / "m.model"), str(tmp_path / "a.png"), "--region=-32,32,64,32", "--mesh", str(tmp_path / "a.npz"),
            "--texture", str(tmp_path / "a_tex.png"), "--overlap", "4", "--batch-size", "2"] + common
    assert WD.main(args) == 0
    a = np.load(tmp_path / "a.npz")
    assert np.array_equal(a["grid"], want.grid) and np.array_equal(a["heights"], want.heights)
    assert np.array_equal(a["triangles"], want.triangles) and tuple(a["origin"]) == (-32, 32) and np.array_equal(a["texture"], tex)
    args = ["SMALL", str(tmp_path / "m.model"), str(tmp_path / "b.png"), "--region=-32,64,64,64", "--mesh", str(tmp_path / "b.npz")] + common
    assert WD.main(args) == 0
    b = np.load(tmp_path / "b.npz")
    ea, eb = a["grid"][:, 1] == 32, b["grid"][:, 1] == 0                           # world column 64 in both files
    assert ea.sum() >= 3 and np.array_equal(a["grid"][ea, 0], b["grid"][eb, 0])
    assert a["heights"][ea].tobytes() == b["heights"][eb].tobytes()
    assert WD.main(["SMALL", str(tmp_path / "m.model"), str(tmp_path / "c.png"), "--region=-32,64,64,64", "--mesh",
                    str(tmp_path / "c.glb")] + common) == 0
    assert _glb(tmp_path / "c.glb")[:2] == (len(b["heights"]), len(b["triangles"]))
