"""Adaptive meshes on the host.  The device code of csrc/mesh.hip compiled for the CPU
(tests/mesh_host/harness.cpp): the same source text the GPU runs, the kernels with barriers run phase by phase, once more
under the address and undefined-behaviour sanitizers.  And the host logic of gan_heightmaps_amd/mesh.py and world.py on
tests/fake_device.py: the refusals, what a call sends to the device, fit, the default tile, the writers, the command lines.
No GPU."""
import dataclasses
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from gan_heightmaps_amd import mesh as MS
from gan_heightmaps_amd import world as WD
from tests import mesh_ref as M
from tests.fake_device import FakeDevice, RecordingOps
from tests.test_render_host import CSRC, ROOT, _compiler
from tests.test_world_plan import _world


# ---- the kernels' source on the host ------------------------------------------------------------------------------------
def _build(d, name, extra=()):
    head, sep, _ = open(os.path.join(CSRC, "mesh.hip")).read().partition('extern "C" {')
    assert sep and '#include "common.h"' in head
    inc = d / "mesh.hip.inc"
    inc.write_text(head.replace('#include "common.h"', ""))
    exe = d / name
    cmd = [_compiler(), "-x", "c++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
           '-DMESH_DEVICE_INC="%s"' % inc] + list(extra) + [os.path.join(ROOT, "tests", "mesh_host", "harness.cpp"), "-o", str(exe)]
    return exe, subprocess.run(cmd, capture_output=True, text=True)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("mesh_host")
    exe, r = _build(d, "mesh_host")
    assert r.returncode == 0, r.stderr[-3000:]
    return d, exe


def run_mesh(harness, src, k, tol, cols=None, err_pitch=None, rect=None):
    """src [rows, pitch] float32 -> (plain errors, fused errors [rows, err_pitch], index, grid, heights, triangles)"""
    d, exe = harness
    rows, pitch = src.shape
    cols = pitch if cols is None else cols
    err_pitch = cols if err_pitch is None else err_pitch
    y0, x0, h, w = rect if rect is not None else (0, 0, rows - 1, cols - 1)
    (d / "in.bin").write_bytes(np.ascontiguousarray(src, np.float32).tobytes())
    args = ["mesh", rows, cols, pitch, err_pitch, k, y0, x0, h, w, repr(float(tol)), d / "in.bin", d / "out.bin"]
    r = subprocess.run([str(exe)] + [str(v) for v in args], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    raw = (d / "out.bin").read_bytes()
    n = rows * err_pitch
    plain = np.frombuffer(raw, np.float32, n).reshape(rows, err_pitch)
    fused = np.frombuffer(raw, np.float32, n, 4 * n).reshape(rows, err_pitch)
    at = 8 * n
    V, F = (int(v) for v in np.frombuffer(raw, np.int64, 2, at))
    at += 16
    nv = (h + 1) * (w + 1)
    index = np.frombuffer(raw, np.int32, nv, at).reshape(h + 1, w + 1)
    at += 4 * nv
    grid = np.frombuffer(raw, np.int32, 2 * V, at).reshape(V, 2)
    at += 8 * V
    heights = np.frombuffer(raw, np.float32, V, at)
    at += 4 * V
    tris = np.frombuffer(raw, np.uint32, 3 * F, at).reshape(F, 3)
    assert at + 12 * F == len(raw)
    return plain, fused, index, grid, heights, tris


# (seed, rows, cols, k): T = 2, 4, 8 have k <= the fused levels (the root rule inside the block); 17 x 17 is smaller than a
# block; 65 x 65 one block and its shared edge; 81 x 97 is cut by the plane's edge; 129 x 257 has plain scales above the fused
CASES = ((1, 5, 7, 1), (2, 9, 13, 2), (3, 17, 25, 3), (4, 17, 17, 4), (5, 65, 65, 6), (6, 81, 97, 4), (7, 129, 257, 7),
         (8, 73, 137, 3))


@pytest.mark.parametrize("case", range(len(CASES)))
def test_both_forms_and_the_extraction_on_the_host_build(harness, case):
    seed, rows, cols, k = CASES[case]
    h, e = M.case(seed, rows, cols, k)
    for tol in (0.0, 0.02, 1.0):
        plain, fused, index, grid, heights, tris = run_mesh(harness, h, k, tol)
        assert plain.tobytes() == fused.tobytes() == e.tobytes()                   # bit for bit, the fused form phase by phase
        g, hh, t = M.case_mesh(seed, rows, cols, k, tol)
        assert np.array_equal(grid, g) and heights.tobytes() == hh.tobytes() and np.array_equal(tris, t)
        assert np.array_equal(index >= 0, e > np.float32(tol)) and np.array_equal(index[index >= 0], np.arange(len(g)))


def test_pitches_and_a_rectangle_of_tiles_on_the_host_build(harness):
    seed, rows, cols, k = 9, 49, 65, 4
    h, e = M.case(seed, rows, cols, k)
    wide = np.full((rows, cols + 5), np.nan, np.float32)
    wide[:, :cols] = h
    rect = (16, 16, 16, 32)
    plain, fused, index, grid, heights, tris = run_mesh(harness, wide, k, 0.015, cols=cols, err_pitch=cols + 3, rect=rect)
    assert plain.tobytes() == fused.tobytes()
    assert np.isnan(plain[:, cols:]).all() and np.array_equal(plain[:, :cols], e)  # the cells beyond the width are untouched
    g, hh, t = M.extract(h, e, k, 0.015, rect)
    assert np.array_equal(grid, g) and np.array_equal(heights, hh) and np.array_equal(tris, t)
    pts = M.as_points(grid, tris, rect[:2])
    assert M.bad_edges(pts, rect) == 0 and (M.crosses(pts) > 0).all() and M.crosses(pts).sum() == 2 * 16 * 32
    # ... and is the part of the whole plane's mesh that lies inside it
    whole = M.as_points(*M.extract(h, e, k, 0.015)[::2])
    inside = ((whole[:, :, 0] >= 16) & (whole[:, :, 0] <= 32) & (whole[:, :, 1] >= 16) & (whole[:, :, 1] <= 48)).all(1)
    assert np.array_equal(pts, whole[inside])


def test_the_harness_under_the_sanitizers(tmp_path):
    """the same stand-alone program with -fsanitize=address,undefined, on the smallest cases: out-of-bounds LDS or plane
    indices and signed overflow in the kernels' index arithmetic end it"""
    exe, r = _build(tmp_path, "mesh_host_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])
    if r.returncode != 0:
        pytest.skip("the host compiler cannot link the sanitizer runtimes: " + r.stderr[-300:])
    for seed, rows, cols, k in CASES[:4] + ((5, 65, 65, 6), (8, 73, 137, 3)):
        h, e = M.case(seed, rows, cols, k)
        plain, fused, _, grid, _, tris = run_mesh((tmp_path, exe), h, k, 0.02)
        assert plain.tobytes() == fused.tobytes() == e.tobytes()
        assert np.array_equal(tris, M.case_mesh(seed, rows, cols, k, 0.02)[2])


# ---- fit, the default tile, the refusals ----------------------------------------------------------------------------------
def test_fit_replicates_the_edge_to_whole_tiles():
    a = np.arange(40 * 52, dtype=np.float32).reshape(40, 52)
    f, shape = MS.fit(a, 32)
    assert f.shape == (65, 65) and shape == (40, 52) and np.array_equal(f[:40, :52], a)
    assert (f[40:, :52] == a[-1:, :]).all() and (f[:40, 52:] == a[:, -1:]).all() and (f[40:, 52:] == a[-1, -1]).all()
    assert MS.fit(np.zeros((512, 512)), 256)[0].shape == (513, 513)
    same, _ = MS.fit(np.zeros((513, 257)), 256)
    assert same.shape == (513, 257) and MS.fit(np.zeros((1, 1)), 2)[0].shape == (3, 3)
    # the replicated strip has no error: it costs nothing at any tolerance
    e = M.errors(MS.fit(M.terrain(3, 9, 9), 8)[0], 3)
    assert (e[10:16, :] == 0).all() and (e[:, 10:16] == 0).all()
    for bad in (3, 0, 1, 8192, 2.0, True):
        with pytest.raises(ValueError, match="tile"):
            MS.fit(a, bad)
    with pytest.raises(ValueError, match="must be \\(H, W\\)"):
        MS.fit(np.zeros((2, 3, 4)), 4)


def test_the_default_tile():
    assert [MS.default_tile(*s) for s in ((512, 512), (40, 52), (256, 1000), (255, 300), (2, 2), (3, 9), (4096, 4096))] == \
        [256, 32, 256, 128, 2, 2, 256]
    with pytest.raises(ValueError, match="too small"):
        MS.default_tile(1, 100)


def _ops():
    ops = RecordingOps(FakeDevice())
    ops.mesh_workspace = lambda h, w: 16 * (((h + 1) * (w + 1) + 255) // 256 + 1)
    ops.mesh_count = lambda *a: (ops.calls.append(("mesh_count", a, {})), (5, 2))[1]
    return ops


def test_refusals_before_a_device():
    ok = np.zeros((9, 17), np.float32)
    for bad in (np.zeros((2, 9, 9), np.float32), np.zeros(9, np.float32), np.zeros((0, 4), np.float32)):
        with pytest.raises(ValueError, match="must be \\(H, W\\) or \\(1, H, W\\)"):
            MS.ErrorMap(None, bad, tile=8)
    with pytest.raises(ValueError, match="uint8 or floating"):
        MS.ErrorMap(None, np.zeros((9, 9), np.int32), tile=8)
    with pytest.raises(ValueError, match="non-finite"):
        MS.ErrorMap(None, np.full((9, 9), np.nan), tile=8)
    with pytest.raises(ValueError, match="lie in \\[0, 1\\]"):
        MS.ErrorMap(None, np.full((9, 9), 1.5), tile=8)
    for tile in (3, 1, 8192, "8", 8.0):
        with pytest.raises(ValueError, match="tile"):
            MS.ErrorMap(None, ok, tile=tile)
    for shape in ((9, 16), (8, 17), (9, 9 + 4), (5, 9)):
        with pytest.raises(ValueError, match="is not \\(R tile \\+ 1\\)"):
            MS.ErrorMap(None, np.zeros(shape, np.float32), tile=8)
    with pytest.raises(ValueError, match="2\\^31"):
        MS.ErrorMap(None, MS.DevicePlane(1 << 20, (1 << 15) + 1, (1 << 16) + 1), tile=256)
    ops = _ops()
    with MS.ErrorMap(ops, ok, tile=8) as em:
        for tol in (-0.1, float("nan"), float("inf"), "0.1", True, None):
            with pytest.raises(ValueError, match="max_error"):
                em.extract(tol)
            with pytest.raises(ValueError, match="max_error"):
                em.count(tol)
        for rect in ((0, 0, 8, 9), (0, 4, 8, 8), (0, 0, 16, 8), (0, 16, 8, 8), (-8, 0, 8, 8), (0, 0, 0, 8), (0, 0, 8), 3,
                     (0, 0, 8.0, 8)):
            with pytest.raises(ValueError, match="rect"):
                em.extract(0.1, rect=rect)
    for call in (em.errors, lambda: em.count(0.1), lambda: em.extract(0.1)):
        with pytest.raises(ValueError, match="closed"):
            call()
    for bad in (np.zeros((2, 9, 9), np.float32), np.zeros((1, 9), np.float32)):
        with pytest.raises(ValueError):
            MS.heightmap_mesh(None, bad, 0.1)
    with pytest.raises(ValueError, match="max_error"):
        MS.heightmap_mesh(None, ok, -1)


def test_what_a_mesh_sends_to_the_device():
    ops = _ops()
    dev = ops.dev
    hm = np.zeros((1, 40, 52), np.uint8)
    m = MS.heightmap_mesh(ops, hm, 0.25, fused=False)                              # tile=None: 32; fitted to 65 x 65
    names = [c[0] for c in ops.calls]
    assert names == ["mesh_errors", "mesh_count", "mesh_extract"] and dev.uploads == 1
    src, rows, cols, pitch, k, fused, err, err_pitch = ops.calls[0][1]
    assert (rows, cols, pitch, k, fused, err_pitch) == (65, 65, 65, 5, False, 65) and src != err
    assert ops.calls[1][1][:10] == (err, 65, 65, 65, 5, 0, 0, 64, 64, 0.25)
    a = ops.calls[2][1]
    assert a[:13] == (src, 65, err, 65, 65, 65, 5, 0, 0, 64, 64, 0.25, ops.calls[1][1][10]) and a[17:] == (5, 2)
    assert len(set(a[12:17])) == 5                                                 # workspace, index, grid, heights, triangles
    assert (m.grid.shape, m.heights.shape, m.triangles.shape) == ((5, 2), (5,), (2, 3))
    assert (m.grid.dtype, m.heights.dtype, m.triangles.dtype) == (np.int32, np.float32, np.uint32)
    assert (m.shape, m.origin, m.tile, m.max_error, m.valid_shape) == ((65, 65), (0, 0), 32, 0.25, (40, 52))
    with pytest.raises(dataclasses.FrozenInstanceError):
        m.tile = 4
    # a device plane is not uploaded, and not freed unless owned; a rectangle moves the origin
    ops = _ops()
    freed = []
    ops.dev.free = freed.append
    with MS.ErrorMap(ops, MS.DevicePlane(12345, 25, 33), tile=8, origin=(-8, 16), own=False) as em:
        assert em.fused == MS.DEFAULT_FUSED and ops.dev.uploads == 0 and ops.calls[0][1][0] == 12345
        assert em.count(0.5, rect=(8, 8, 8, 16)) == (5, 2) and ops.calls[-1][1][5:10] == (8, 8, 8, 16, 0.5)
        m = em.extract(0.5, rect=(8, 8, 8, 16))
        assert (m.shape, m.origin, m.valid_shape) == ((9, 17), (0, 24), (9, 17))
    assert 12345 not in freed and len(freed) >= 1
    assert MS.DEFAULT_FUSED in (False, True) and MS.MAX_TILE == 4096


# ---- positions, uvs, writers --------------------------------------------------------------------------------------------
def _mesh(tol=0.02, origin=(0, 0), valid=None):
    seed, rows, cols, k = 4, 17, 17, 4
    g, h, t = M.case_mesh(seed, rows, cols, k, tol)
    return MS.TerrainMesh(g, h, t, (rows, cols), origin, 1 << k, tol, valid or (rows, cols))


def test_positions_and_uvs():
    m = _mesh(origin=(-32, 48), valid=(12, 16))
    p, uv = m.positions(height_scale=10), m.uvs()
    assert p.dtype == np.float32 and p.shape == (m.vertices, 3) and uv.dtype == np.float32 and uv.shape == (m.vertices, 2)
    assert np.array_equal(p[:, 0], m.grid[:, 1] + 48.0) and np.array_equal(p[:, 2], m.grid[:, 0] - 32.0)
    assert np.array_equal(p[:, 1], np.float32(10) * m.heights)
    assert np.array_equal(uv[:, 0], np.clip((m.grid[:, 1] + 0.5) / 16, 0, 1).astype(np.float32))
    assert np.array_equal(uv[:, 1], np.clip((m.grid[:, 0] + 0.5) / 12, 0, 1).astype(np.float32))
    assert uv.max() == 1.0 and uv.min() > 0
    # seen from above the written faces turn counter-clockwise: their normals point up
    f = m.front_faces()
    a, b, c = (p[f[:, i]].astype(np.float64) for i in range(3))
    assert (np.cross(b - a, c - a)[:, 1] > 0).all()
    with pytest.raises(ValueError, match="height_scale"):
        m.positions(float("nan"))


def _read_glb(path):
    """a minimal reader of binary glTF 2.0: (the JSON document, the binary chunk)"""
    raw = open(path, "rb").read()
    magic, version, total = struct.unpack_from("<4sII", raw, 0)
    assert magic == b"glTF" and version == 2 and total == len(raw) and total % 4 == 0
    n, kind = struct.unpack_from("<I4s", raw, 12)
    assert kind == b"JSON" and n % 4 == 0
    doc = json.loads(raw[20:20 + n].decode("utf-8"))
    m, kind = struct.unpack_from("<I4s", raw, 20 + n)
    assert kind == b"BIN\0" and m % 4 == 0 and 28 + n + m == len(raw)
    return doc, raw[28 + n:]


def _accessor(doc, binary, i):
    acc = doc["accessors"][i]
    view = doc["bufferViews"][acc["bufferView"]]
    dtype, width = {5126: np.float32, 5125: np.uint32}[acc["componentType"]], {"SCALAR": 1, "VEC2": 2, "VEC3": 3}[acc["type"]]
    assert view["buffer"] == 0 and view["byteOffset"] % 4 == 0 and view["byteLength"] == acc["count"] * width * 4
    return np.frombuffer(binary, dtype, acc["count"] * width, view["byteOffset"]).reshape(acc["count"], width)


def test_a_written_glb_reads_back(tmp_path):
    import io
    from PIL import Image
    m = _mesh()
    tex = np.random.RandomState(0).randint(0, 256, (17, 17, 3)).astype(np.uint8)
    for texture in (None, tex):
        path = m.save(str(tmp_path / "t.glb"), texture=texture, height_scale=32)
        doc, binary = _read_glb(path)
        assert doc["asset"]["version"] == "2.0" and doc["buffers"] == [{"byteLength": len(binary)}]
        assert len(doc["meshes"]) == 1 and doc["scenes"][doc["scene"]]["nodes"] == [0] and doc["nodes"][0]["mesh"] == 0
        prim, = doc["meshes"][0]["primitives"]
        assert prim["mode"] == 4 and set(prim["attributes"]) == {"POSITION", "TEXCOORD_0"}
        pos, uv = (_accessor(doc, binary, prim["attributes"][k]) for k in ("POSITION", "TEXCOORD_0"))
        idx = _accessor(doc, binary, prim["indices"])
        assert np.array_equal(pos, m.positions(32)) and np.array_equal(uv, m.uvs())
        pa = doc["accessors"][prim["attributes"]["POSITION"]]
        assert pa["count"] == m.vertices and pa["min"] == pos.min(0).tolist() and pa["max"] == pos.max(0).tolist()
        ia = doc["accessors"][prim["indices"]]
        assert ia["componentType"] == 5125 and ia["count"] == 3 * m.faces and idx.max() < m.vertices
        assert np.array_equal(idx.reshape(-1, 3), m.front_faces())
        if texture is None:
            assert "images" not in doc and "material" not in prim
        else:
            img = doc["images"][doc["textures"][doc["materials"][prim["material"]]["pbrMetallicRoughness"]
                                                ["baseColorTexture"]["index"]]["source"]]
            view = doc["bufferViews"][img["bufferView"]]
            png = binary[view["byteOffset"]:view["byteOffset"] + view["byteLength"]]
            assert img["mimeType"] == "image/png" and png[:8] == b"\x89PNG\r\n\x1a\n"
            assert np.array_equal(np.asarray(Image.open(io.BytesIO(png))), tex)


def test_a_written_obj_and_npz_read_back(tmp_path):
    from PIL import Image
    m = _mesh()
    tex = np.random.RandomState(1).randint(0, 256, (17, 17)).astype(np.uint8)
    path = m.save(str(tmp_path / "land.obj"), texture=tex)
    v, vt, f, other = [], [], [], []
    for line in open(path):
        tok = line.split()
        {"v": v, "vt": vt, "f": f}.get(tok[0], other).append(tok[1:])
    assert ["land.mtl"] in other and ["terrain"] in other
    assert np.array_equal(np.asarray(v, np.float64).astype(np.float32), m.positions())
    uv = np.asarray(vt, np.float64)
    assert np.allclose(uv[:, 0], m.uvs()[:, 0], atol=1e-7) and np.allclose(1.0 - uv[:, 1], m.uvs()[:, 1], atol=1e-7)
    faces = np.asarray([[c.split("/") for c in face] for face in f], np.int64)
    assert (faces[:, :, 0] == faces[:, :, 1]).all() and np.array_equal(faces[:, :, 0] - 1, m.front_faces())
    assert "map_Kd land.png" in open(tmp_path / "land.mtl").read()
    assert np.array_equal(np.asarray(Image.open(tmp_path / "land.png")), tex)
    m.save(str(tmp_path / "bare.obj"))
    assert not (tmp_path / "bare.mtl").exists() and "mtllib" not in open(tmp_path / "bare.obj").read()
    z = np.load(m.save(str(tmp_path / "m.npz")))
    assert np.array_equal(z["grid"], m.grid) and np.array_equal(z["heights"], m.heights)
    assert np.array_equal(z["triangles"], m.triangles) and tuple(z["shape"]) == m.shape and int(z["tile"]) == 16
    with pytest.raises(ValueError, match="glb, .obj or .npz"):
        m.save(str(tmp_path / "m.stl"))
    with pytest.raises(ValueError, match="texture must be uint8"):
        m.save(str(tmp_path / "m.glb"), texture=np.zeros((17, 17, 3), np.float32))


# ---- the world ----------------------------------------------------------------------------------------------------------
def test_world_mesh_refuses_unaligned_regions_before_a_device():
    w = _world(chunk_cells=2)
    for args in ((0, 0, 64, 60), (0, 8, 64, 64), (-3, 0, 64, 64), (0, 0, 0, 64), (0, 0, 32.0, 32), (0, 0, 64, -64)):
        with pytest.raises(ValueError, match="multiple of the tile|at least one tile"):
            w.mesh(*args, max_error=0.1, tile=32)
    with pytest.raises(ValueError, match="tile"):
        w.mesh(0, 0, 48, 48, max_error=0.1, tile=48)
    with pytest.raises(ValueError, match="max_error"):
        w.mesh(0, 0, 64, 64, max_error=-1, tile=32)
    with pytest.raises(ValueError, match="2\\^31"):
        w.mesh(0, 0, 1 << 16, 1 << 15, max_error=0.1, tile=256)
    w.close()
    with pytest.raises(ValueError, match="closed"):
        w.mesh(0, 0, 64, 64, max_error=0.1, tile=32)


# ---- command lines --------------------------------------------------------------------------------------------------------
def test_mesh_cli_arguments():
    a = MS.parse_args(["in.png", "out.glb"])
    assert (a.input, a.output, a.texture, a.max_error, a.tile, a.height_scale, a.plain, a.fused) == \
        ("in.png", "out.glb", None, 0.01, None, 64.0, False, False)
    a = MS.parse_args(["in.npy", "out.obj", "--texture", "t.png", "--max-error", "0.05", "--tile", "64", "--height-scale", "24",
                       "--plain"])
    assert (a.texture, a.max_error, a.tile, a.height_scale, a.plain) == ("t.png", 0.05, 64, 24.0, True)
    assert MS.parse_args(["a", "b.npz", "--fused"]).fused
    for bad in (["in.png"], ["a", "b.stl"], ["a", "b.glb", "--max-error", "-1"], ["a", "b.glb", "--max-error", "nan"],
                ["a", "b.glb", "--tile", "48"], ["a", "b.glb", "--tile", "1"], ["a", "b.glb", "--height-scale", "inf"],
                ["a", "b.glb", "--plain", "--fused"]):
        with pytest.raises(SystemExit):
            MS.parse_args(bad)


def test_world_cli_takes_a_mesh():
    base = ["EXP", "m.model", "out.png", "--seed", "1"]
    a = WD.parse_args(base + ["--region", "0,256,512,256"])
    assert (a.mesh, a.max_error, a.tile) == (None, None, None)
    a = WD.parse_args(base + ["--region", "-256,256,512,256", "--mesh", "m.glb"])
    assert (a.mesh, a.max_error, a.tile, a.region) == ("m.glb", 0.01, 256, (-256, 256, 512, 256))
    a = WD.parse_args(base + ["--region", "32,0,64,96", "--mesh", "m.obj", "--max-error", "0.1", "--tile", "32", "--texture", "t.png"])
    assert (a.max_error, a.tile, a.texture) == (0.1, 32, "t.png")
    for bad in (["--region", "0,0,100,256", "--mesh", "m.glb"], ["--region", "0,8,64,64", "--mesh", "m.glb", "--tile", "32"],
                ["--region", "0,0,256,256", "--mesh", "m.stl"], ["--region", "0,0,256,256", "--mesh", "m.glb", "--tile", "3"],
                ["--region", "0,0,256,256", "--mesh", "m.glb", "--max-error", "-2"],
                ["--region", "0,0,256,256", "--max-error", "0.1"], ["--region", "0,0,256,256", "--tile", "64"]):
        with pytest.raises(SystemExit):
            WD.parse_args(base + bad)
