"""The host side of the scatter (gan_heightmaps_amd/scatter.py): Habitat's and Species' validation and tables, the
refusals that are made before the device is touched, the launch sequence on a recording device, the command lines' parsing, the
.npz / .csv / .glb writers.  And the device code of csrc/scatter.hip compiled for the CPU (tests/scatter_host/harness.cpp): the
same source text the GPU runs, the tiled form phase by phase, the chance, the candidates and both forms of the thinning bit for
bit against tests/scatter_ref.py on the planes of the device tests, once more under the address and undefined-behaviour
sanitizers.  No device."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from gan_heightmaps_amd import hydrology as HY
from gan_heightmaps_amd import scatter as SC
from tests import scatter_ref as S
from tests.test_render_host import CSRC, ROOT, _compiler


# ---- validation and tables ----------------------------------------------------------------------------------------------------
def test_habitat_validation_and_tables():
    h = SC.Habitat()
    assert (h.altitude, h.altitude_fade, h.slope, h.slope_fade, h.density, h.water) == ((0.0, 1.0), 0.05, (0.0, 30.0), 10.0, 1.0, None)
    assert (h.lake_clearance, h.river_clearance, h.road_clearance, h.river_threshold, h.lake_min_depth) == (0.0, 0.0, 1.0, 256, 1.0 / 512)
    assert SC.Habitat(altitude=[0, np.float32(0.5)], density=1, river_threshold=np.int64(9)) == \
        SC.Habitat(altitude=(0.0, 0.5), density=1.0, river_threshold=9) and hash(h) == hash(SC.Habitat())
    with pytest.raises(Exception):
        h.density = 0.5                                                    # frozen
    for kw in (dict(altitude=(0.5, 0.2)), dict(altitude=0.5), dict(altitude=(0, float("nan"))), dict(altitude=(0, 1, 2)),
               dict(slope=(-1, 30)), dict(slope=(0, 91)), dict(slope=("0", 30)), dict(altitude_fade=-0.1), dict(slope_fade=91),
               dict(slope_fade=float("inf")), dict(density=1.5), dict(density=-0.1), dict(density=True), dict(density=None),
               dict(water=(1.5, 4)), dict(water=(0.5, 0)), dict(water=(0.5, 33)), dict(water=0.5), dict(water=(0.5, None)),
               dict(lake_clearance=33), dict(river_clearance=-1), dict(road_clearance="1"), dict(river_threshold=0),
               dict(river_threshold=2.0), dict(river_threshold=1 << 32), dict(lake_min_depth=-1)):
        with pytest.raises(ValueError):
            SC.Habitat(**kw)
    assert SC.Habitat(lake_clearance=None, road_clearance=None).lake_clearance is None
    # the tables: float64, rounded once
    t = h.tables()
    assert t.dtype == np.float32 and t.shape == (384,) and t[319] == 0 and t[256:319].tobytes() == S.slope_bounds().tobytes()
    assert SC.slope_bounds().tobytes() == S.slope_bounds().tobytes()
    assert (t[:256] == 1).all() and (t[320:320 + 21] == 1).all() and t[320 + 29] == 0 and 0 < t[320 + 24] < 1
    assert (np.diff(t[320:]) <= 0).all() and ((t >= 0) & (t[:256].max() <= 1)).all()
    band = SC.Habitat(altitude=(0.4, 0.6), altitude_fade=0.1, slope=(10, 20), slope_fade=0).tables()
    a = np.arange(256) / 255.0
    want = np.clip((a - 0.3) / 0.1, 0, 1) * np.clip((0.7 - a) / 0.1, 0, 1)
    assert band[:256].tobytes() == want.astype(np.float32).tobytes() and band[102] == 1 and band[76] == 0 and 0 < band[90] < 1
    mid = (np.arange(64) + 0.5) * 90 / 64
    assert np.array_equal(band[320:] == 1, (mid >= 10) & (mid <= 20)) and set(band[320:].tolist()) == {0.0, 1.0}
    assert h.water_table() is None and h.water_reach == 0
    w = SC.Habitat(water=(0.75, 3.5))
    wt = w.water_table()
    assert w.water_reach == 4 and wt.dtype == np.float32 and wt.shape == (18,) and wt[0] == 1 and wt[-1] == 0.25 == wt[13]
    assert wt[4] == np.float32(0.25 + 0.75 * (1 - 2 / 3.5)) and (np.diff(wt[:10]) < 0).all()
    assert SC.Habitat(water=(1.0, 32)).water_table().shape == (1026,)


def test_species_validation():
    s = SC.Species("pine", 2.5)
    assert (s.name, s.spacing, s.habitat, s.scale, s.seed_stream, s.s2) == ("pine", 2.5, SC.Habitat(), (0.8, 1.25), 0, 7)
    assert [SC.Species("a", v).s2 for v in (0.1, 1, 1.0001, 1.5, 2, 8, 31.99, 32)] == [1, 1, 2, 3, 4, 64, 1024, 1024]
    assert SC.Species("a", np.float32(2), scale=[1, 2], seed_stream=np.int32(4)) == SC.Species("a", 2.0, None, (1.0, 2.0), 4)
    with pytest.raises(Exception):
        s.spacing = 3
    for args in (("", 2), ("a,b", 2), (3, 2), ("a", 0), ("a", 32.5), ("a", float("nan")), ("a", None), ("a", True),
                 ("a", 2, dict(density=1)), ("a", 2, None, (0, 1)), ("a", 2, None, (2, 1)), ("a", 2, None, 1.0),
                 ("a", 2, None, (1, 2), -1), ("a", 2, None, (1, 2), 1 << 32), ("a", 2, None, (1, 2), 1.0)):
        with pytest.raises(ValueError):
            SC.Species(*args)
    assert SC.Species("a", 2).seed(5) == 5 and SC.Species("a", 2, seed_stream=1).seed(5) != SC.Species("a", 2, seed_stream=2).seed(5)
    assert 0 <= SC.Species("a", 2, seed_stream=(1 << 32) - 1).seed(-1) < 1 << 64
    assert (SC.TILE, SC.MAX_S2, SC.ONE, SC.NONE, SC.UNDECIDED, SC.KEPT, SC.REJECTED) == \
        (S.TILE, S.MAX_S2, S.ONE, S.NONE, S.UNDECIDED, S.KEPT, S.REJECTED)
    assert (SC.MIX_A, SC.MIX_B, SC.MIX_STEP) == (S.MIX_A, S.MIX_B, S.MIX_STEP)
    assert [SC._reach_of(v) for v in (1, 2, 3, 4, 5, 10, 16, 17, 1024)] == [0, 1, 2, 2, 2, 3, 4, 4, 32]
    r, c = np.mgrid[-4:4, -4:4]
    for seed in (0, 9, -1, 1 << 63):
        assert np.array_equal(SC.hash32(seed, 3, r, c), S.hash32(seed, 3, r, c))
    text = open(os.path.join(ROOT, "include", "ghm.h")).read()
    for name, v in (("MIX_A", S.MIX_A), ("MIX_B", S.MIX_B), ("MIX_STEP", S.MIX_STEP)):
        assert "#define GHM_SCATTER_%s 0x%08xu" % (name, v) in text
    assert "#define GHM_SCATTER_TILE 32" in text and "#define GHM_SCATTER_MAX_S2 1024" in text


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_before_the_device_is_touched():
    ops = None                                                            # nothing may reach for it
    h = S.heights(8, 9, 1)
    sp = SC.Species("a", 2)
    for bad in (np.zeros((2, 8, 9), np.float32), np.zeros(8, np.float32), np.zeros((8, 9), np.int32), np.zeros((0, 9), np.float32)):
        with pytest.raises(ValueError):
            SC.scatter(ops, bad, sp)
        with pytest.raises(ValueError):
            SC.chance(ops, bad)
    x = h.copy()
    x[3, 4] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        SC.scatter(ops, x, sp)
    huge = np.lib.stride_tricks.as_strided(np.zeros(1, np.float32), shape=(1 << 16, 1 << 15), strides=(0, 0), writeable=False)
    with pytest.raises(ValueError, match="out of range"):
        SC.scatter(ops, huge, sp)
    with pytest.raises(ValueError, match="out of range"):
        SC.thin(ops, np.lib.stride_tricks.as_strided(np.zeros(1, np.uint8), shape=huge.shape, strides=(0, 0)),
                np.lib.stride_tricks.as_strided(np.zeros(1, np.uint32), shape=huge.shape, strides=(0, 0)), 4)
    for bad in (None, [], "pine", [sp, "pine"], [sp, SC.Species("a", 3)], SC.Habitat()):
        with pytest.raises(ValueError, match="[Ss]pecies"):
            SC.scatter(ops, h, bad)
    for bad in (1.5, None, "3"):
        with pytest.raises(ValueError, match="seed"):
            SC.scatter(ops, h, sp, seed=bad)
    for bad in (3, (1,), (1.5, 2), None, (1, 2, 3)):
        with pytest.raises(ValueError, match="origin"):
            SC.scatter(ops, h, sp, origin=bad)
    for bad in ((1 << 31, 0), (0, (1 << 31) - 8), (-(1 << 31) - 1, 0), (0, -(1 << 40))):
        with pytest.raises(ValueError, match="int32"):
            SC.scatter(ops, h, sp, origin=bad)
    for bad in (0, -1, float("inf"), None, 1e-60):
        with pytest.raises(ValueError, match="height_scale"):
            SC.scatter(ops, h, sp, height_scale=bad)
        with pytest.raises(ValueError, match="height_scale"):
            SC.chance(ops, h, height_scale=bad)
    with pytest.raises(ValueError, match="keep"):
        SC.scatter(ops, h, sp, keep=('points',))
    with pytest.raises(ValueError, match="Habitat"):
        SC.chance(ops, h, dict(density=1))
    z = np.zeros((8, 9), np.float32)
    for bad in (h, HY.Hydrology((8, 9), (1, 1), 1, False, depth=z), HY.Hydrology((8, 9), (1, 1), 1, False, accumulation=z)):
        with pytest.raises(ValueError, match="depth"):
            SC.scatter(ops, h, sp, hydro=bad)
    with pytest.raises(ValueError, match="differ in size"):
        SC.scatter(ops, h, sp, hydro=HY.Hydrology((9, 8), (1, 1), 1, False, depth=z.T, accumulation=z.T))
    for name in ("roads", "blocked"):
        for bad in (np.zeros((9, 8), np.uint8), np.zeros((8, 9), np.float32), 3):
            with pytest.raises(ValueError, match=name):
                SC.scatter(ops, h, sp, **{name: bad})
            with pytest.raises(ValueError, match=name):
                SC.chance(ops, h, **{name: bad})
    st, pr = np.ones((8, 9), np.uint8), np.zeros((8, 9), np.uint32)
    for bad in (0, 1025, 4.0, None, True):
        with pytest.raises(ValueError, match="s2"):
            SC.thin(ops, st, pr, bad)
    for a, b in ((st.astype(np.int32), pr), (st, pr.astype(np.int32)), (st, pr[:, :8]), (st[0], pr[0])):
        with pytest.raises(ValueError, match="uint8"):
            SC.thin(ops, a, b, 4)
    placed = SC.Scatter((8, 9), (0, 0), True, [])
    tex = np.zeros((8, 9, 3), np.uint8)
    with pytest.raises(ValueError, match="Scatter"):
        SC.paint(ops, tex, None)
    one = SC.Scatter((8, 9), (0, 0), True, [SC.Layer(sp, np.zeros((0, 2), np.int32), *(np.zeros(0, np.float32),) * 3, 0, 1)])
    for bad in ((1, 2), (1.5, 0, 0), [(0, 0, 0), (1, 1, 1)], None):
        with pytest.raises(ValueError, match="colours"):
            SC.paint(ops, tex, one, bad)
    for bad in (-1, 5, 1.0):
        with pytest.raises(ValueError, match="radius"):
            SC.paint(ops, tex, one, radius=bad)
    with pytest.raises(ValueError, match="opacity"):
        SC.paint(ops, tex, one, opacity=2)
    assert np.array_equal(SC.paint(ops, tex, placed), tex)                  # no layers: nothing to paint, no device
    with pytest.raises(ValueError, match="npz or .csv"):
        placed.save("points.txt")


def test_scatter_sends_three_launches_per_species_inside_one_scratch():
    from tests.fake_device import FakeDevice, RecordingOps

    class Ops(RecordingOps):
        def scatter_workspace(self, H, W):
            return 256 + H * W

        def scatter_thin(self, *args):
            self.calls.append(("scatter_thin", args, {}))
            return 3

    ops = Ops(FakeDevice())
    h = S.heights(8, 9, 1)
    a, b = SC.Species("a", 2.5, SC.Habitat(density=0.5)), SC.Species("b", 4, seed_stream=7)
    got = SC.scatter(ops, h[None], [a, b], seed=-2, origin=(3, -4), blocked=np.eye(8, 9, dtype=bool), height_scale=32, tiled=False,
                     keep=('chance', 'state'))
    assert [c[0] for c in ops.calls] == ["scatter_chance", "scatter_candidates", "scatter_thin"] * 2
    ch, ca, th = (ops.calls[i][1] for i in range(3))
    assert ch[1:4] == (9, 8, 9) and ch[5:7] == (32.0, 0.5) and ch[8] == 9 and ch[9] is None and ch[11] is None and ch[13] is not None
    assert ca[1:6] == (9, 8, 9, a.seed(-2 & ((1 << 64) - 1)), (3, -4)) and ca[0] == ch[7]
    assert th[0] == ca[8] and th[2] == ca[6] and th[4:8] == (8, 9, 7, False)
    assert ops.calls[4][1][4] == b.seed(-2 & ((1 << 64) - 1)) and ops.calls[5][1][6] == 16
    assert got.shape == (8, 9) and got.origin == (3, -4) and got.tiled is False and got.sweeps == (3, 3)
    assert [len(l) for l in got.layers] == [0, 0] and got["b"].species is b and got.layers[0].priority is None
    assert got.layers[0].chance.shape == (8, 9) and "a: 0" in repr(got) and not got.raster().any()
    with pytest.raises(KeyError):
        got["c"]
    ops = Ops(FakeDevice())
    st, sweeps = SC.thin(ops, np.ones((8, 9), np.uint8), np.zeros((8, 9), np.uint32), 50)
    assert [c[0] for c in ops.calls] == ["scatter_thin"] and ops.calls[0][1][4:8] == (8, 9, 50, SC.DEFAULT_TILED) and sweeps == 3
    ops = Ops(FakeDevice())
    c = SC.chance(ops, h)
    assert [x[0] for x in ops.calls] == ["scatter_chance"] and c.dtype == np.uint32 and c.shape == (8, 9)


# ---- the writers ----------------------------------------------------------------------------------------------------------------
def _placed():
    a, b, c = SC.Species("pine", 3, scale=(1, 2)), SC.Species("rock", 5, seed_stream=2), SC.Species("fern", 2, seed_stream=3)
    pa = np.array([[10, -5], [10, -3], [12, -4]], np.int32)
    pb = np.array([[11, -1]], np.int32)
    la = SC.Layer(a, pa, np.array([0.25, 0.5, 0.75], np.float32), *SC._instances(a, a.seed(9), pa), 7, 4)
    lb = SC.Layer(b, pb, np.array([0.125], np.float32), *SC._instances(b, b.seed(9), pb), 3, 2)
    lc = SC.Layer(c, np.zeros((0, 2), np.int32), np.zeros(0, np.float32), np.zeros(0, np.float32), np.zeros(0, np.float32), 0, 1)
    return SC.Scatter((4, 6), (9, -6), True, [la, lb, lc])


def test_instances_raster_and_save(tmp_path):
    placed = _placed()
    la, lb, _ = placed.layers
    assert la.yaw.dtype == la.scale.dtype == np.float32 and ((la.yaw >= 0) & (la.yaw < np.float32(2 * np.pi) + 1e-6)).all()
    assert ((la.scale >= 1) & (la.scale <= 2)).all() and len(set(la.yaw.tolist())) == 3 and len(set(la.scale.tolist())) == 3
    u = (S.hash32(la.species.seed(9), 2, 10, -5) >> np.uint32(8)) / float(1 << 24)
    assert la.yaw[0] == np.float32(u * 2 * np.pi)
    m = placed.raster()
    assert m.dtype == np.uint32 and m.shape == (4, 6) and m.sum() == 3 + 2 and m[1, 1] == 1 and m[3, 2] == 1 and m[2, 5] == 2
    placed.save(str(tmp_path / "p.npz"))
    z = np.load(str(tmp_path / "p.npz"))
    assert z["names"].tolist() == ["pine", "rock", "fern"] and z["origin"].tolist() == [9, -6] and z["shape"].tolist() == [4, 6]
    assert np.array_equal(z["points_0"], la.points) and z["yaw_1"].tobytes() == lb.yaw.tobytes() and z["points_2"].shape == (0, 2)
    assert z["height_0"].tobytes() == la.height.tobytes() and z["scale_0"].tobytes() == la.scale.tobytes()
    placed.save(str(tmp_path / "p.csv"))
    lines = open(str(tmp_path / "p.csv")).read().splitlines()
    assert lines[0] == "species,row,col,height,yaw,scale" and len(lines) == 5 and lines[4].startswith("rock,11,-1,0.125,")
    f = lines[1].split(",")
    assert f[:4] == ["pine", "10", "-5", "0.25"] and np.float32(f[4]) == la.yaw[0] and np.float32(f[5]) == la.scale[0]


def _chunks(blob):
    magic, version, total = struct.unpack("<4sII", blob[:12])
    assert magic == b"glTF" and version == 2 and total == len(blob)
    n, kind = struct.unpack("<I4s", blob[12:20])
    assert kind == b"JSON"
    doc = json.loads(blob[20:20 + n].decode("utf-8"))
    m, kind = struct.unpack("<I4s", blob[20 + n:28 + n])
    assert kind == b"BIN\0" and 28 + n + m == total
    return doc, blob[28 + n:]


def test_the_glb_gains_one_instanced_node_per_species(tmp_path):
    from gan_heightmaps_amd import mesh as MS
    grid = np.array([[0, 0], [0, 5], [3, 0], [3, 5]], np.int32)
    mesh = MS.TerrainMesh(grid, np.array([0.1, 0.2, 0.3, 0.4], np.float32), np.array([[0, 1, 2], [1, 3, 2]], np.uint32), (4, 6),
                          (9, -6), 4, 0.01, (4, 6))
    tex = np.arange(4 * 6 * 3, dtype=np.uint8).reshape(4, 6, 3)
    placed = _placed()
    for texture in (None, tex):
        plain = open(mesh.save(str(tmp_path / "a.glb"), texture, 32.0), "rb").read()
        assert plain == MS._glb(mesh, texture, 32.0) == open(mesh.save(str(tmp_path / "b.glb"), texture, 32.0, instances=None), "rb").read()
        doc0, _ = _chunks(plain)
        assert "extensionsUsed" not in doc0 and len(doc0["nodes"]) == 1 and len(doc0["meshes"]) == 1
        doc, binary = _chunks(open(mesh.save(str(tmp_path / "c.glb"), texture, 32.0, instances=placed), "rb").read())
        assert doc["extensionsUsed"] == ["EXT_mesh_gpu_instancing"] and doc["scenes"][0]["nodes"] == [0, 1, 2]
        assert [n["name"] for n in doc["nodes"]] == ["terrain", "pine", "rock"] and len(doc["meshes"]) == 2       # no fern: no points
        assert doc["accessors"][:3] == doc0["accessors"] and doc["bufferViews"][:len(doc0["bufferViews"])] == doc0["bufferViews"]

        def read(i, dtype, width):
            acc = doc["accessors"][i]
            v = doc["bufferViews"][acc["bufferView"]]
            assert v["byteOffset"] % 4 == 0
            data = np.frombuffer(binary[v["byteOffset"]:v["byteOffset"] + v["byteLength"]], dtype).reshape(-1, width)
            assert len(data) == acc["count"] or width == 1
            return data
        cone = doc["meshes"][1]["primitives"][0]
        verts, faces = read(cone["attributes"]["POSITION"], np.float32, 3), read(cone["indices"], np.uint16, 1).reshape(-1, 3)
        assert verts.shape == (5, 3) and faces.shape == (6, 3) and faces.max() == 4
        centre = verts.mean(0)
        for f in faces:                                                # every face looks away from the middle
            nrm = np.cross(verts[f[1]] - verts[f[0]], verts[f[2]] - verts[f[0]])
            assert np.dot(nrm, verts[f].mean(0) - centre) > 0
        for node, layer in zip(doc["nodes"][1:], placed.layers):
            at = node["extensions"]["EXT_mesh_gpu_instancing"]["attributes"]
            tr, rot, sc = read(at["TRANSLATION"], np.float32, 3), read(at["ROTATION"], np.float32, 4), read(at["SCALE"], np.float32, 3)
            assert len(tr) == len(rot) == len(sc) == len(layer) and node["mesh"] == 1
            assert np.array_equal(tr[:, 0], layer.points[:, 1]) and np.array_equal(tr[:, 2], layer.points[:, 0])
            assert tr[:, 1].tobytes() == (np.float32(32) * layer.height).tobytes()
            assert np.allclose(np.linalg.norm(rot, axis=1), 1, atol=1e-6) and (rot[:, [0, 2]] == 0).all()
            assert np.allclose(2 * np.arctan2(rot[:, 1], rot[:, 3]) % (2 * np.pi), layer.yaw, atol=1e-5)
            assert (sc == layer.scale[:, None]).all()
    # the terrain's own vertices follow the same convention: a point on a vertex stands on it
    pos = mesh.positions(32.0)
    assert pos[3].tolist() == [-1.0, np.float32(32) * np.float32(0.4), 12.0]
    for path, inst in (("m.obj", placed), ("m.npz", placed), ("m.glb", [1, 2])):
        with pytest.raises(ValueError, match="instances"):
            mesh.save(str(tmp_path / path), None, 32.0, instances=inst)


# ---- command lines ------------------------------------------------------------------------------------------------------------------
def test_command_line_parsing():
    a = SC.parse_args(["in.png", "out.npz", "--spacing", "4"])
    assert (a.input, a.output, a.seed, a.hydrology, a.texture, a.painted, a.form, a.height_scale) == \
        ("in.png", "out.npz", 0, False, None, None, None, 64.0)
    assert a.species == SC.Species("tree", 4.0)
    a = SC.parse_args(["i.npy", "o.csv", "--spacing", "2.5", "--density", "0.1", "--altitude", "0.2,0.7", "--altitude-fade", "0.1",
                       "--slope", "5,25", "--slope-fade", "3", "--water", "0.5,6", "--lake-clearance", "2", "--river-clearance", "1.5",
                       "--river-threshold", "64", "--lake-min-depth", "0.01", "--height-scale", "32", "--scale", "1,3", "--name", "oak",
                       "--seed", "-7", "--hydrology", "--texture", "t.png", "--painted", "p.png", "--colour", "0.5,0.25,0", "--radius",
                       "2", "--tiled"])
    hab = SC.Habitat(altitude=(0.2, 0.7), altitude_fade=0.1, slope=(5, 25), slope_fade=3, density=0.1, water=(0.5, 6), lake_clearance=2,
                     river_clearance=1.5, river_threshold=64, lake_min_depth=0.01)
    assert a.species == SC.Species("oak", 2.5, hab, (1, 3)) and a.seed == -7 and a.form is True and a.hydrology
    assert (a.texture, a.painted, a.colour, a.radius, a.height_scale) == ("t.png", "p.png", (0.5, 0.25, 0.0), 2, 32.0)
    assert SC.parse_args(["i", "o.npz", "--spacing", "1", "--plain"]).form is False
    for bad in (["i", "o.npz"], ["i", "--spacing", "2"], ["i", "o.txt", "--spacing", "2"], ["i", "o.npz", "--spacing", "0"],
                ["i", "o.npz", "--spacing", "33"], ["i", "o.npz", "--spacing", "2", "--plain", "--tiled"],
                ["i", "o.npz", "--spacing", "2", "--density", "2"], ["i", "o.npz", "--spacing", "2", "--altitude", "0.5"],
                ["i", "o.npz", "--spacing", "2", "--altitude", "0.7,0.2"], ["i", "o.npz", "--spacing", "2", "--slope", "0,100"],
                ["i", "o.npz", "--spacing", "2", "--water", "0.5,4"], ["i", "o.npz", "--spacing", "2", "--texture", "t.png"],
                ["i", "o.npz", "--spacing", "2", "--painted", "p.png"], ["i", "o.npz", "--spacing", "2", "--height-scale", "0"],
                ["i", "o.npz", "--spacing", "2", "--name", "a,b"], ["i", "o.npz", "--spacing", "2", "--texture", "t", "--painted", "p",
                                                                  "--radius", "9"],
                ["i", "o.npz", "--spacing", "2", "--texture", "t", "--painted", "p", "--colour", "2,0,0"]):
        with pytest.raises(SystemExit):
            SC.parse_args(bad)


def test_the_worlds_command_line_takes_scatter():
    from gan_heightmaps_amd import world as WD
    base = ["exp", "model.npz", "out.png", "--seed", "3", "--region", "-70,33,150,97"]
    a = WD.parse_args(base)
    assert a.scatter is None and a.spacing is None
    a = WD.parse_args(base + ["--scatter", "trees.csv", "--spacing", "6"])
    assert a.scatter == "trees.csv" and a.species == SC.Species("tree", 6.0)
    for bad in (["--scatter", "t.npz"], ["--spacing", "3"], ["--scatter", "t.txt", "--spacing", "3"], ["--scatter", "t.npz", "--spacing", "40"]):
        with pytest.raises(SystemExit):
            WD.parse_args(base + bad)


# ---- the kernels' source on the host ----------------------------------------------------------------------------------------------
def _build(d, name, extra=()):
    head, sep, _ = open(os.path.join(CSRC, "scatter.hip")).read().partition('extern "C" {')
    assert sep and '#include "common.h"' in head and '#include "relax.h"' in head
    inc = d / "scatter.hip.inc"
    inc.write_text(head.replace('#include "common.h"', "").replace('#include "relax.h"', ""))
    exe = d / name
    cmd = [_compiler(), "-x", "c++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
           '-DSCATTER_DEVICE_INC="%s"' % inc] + list(extra) + [os.path.join(ROOT, "tests", "scatter_host", "harness.cpp"),
                                                              "-o", str(exe)]
    return exe, subprocess.run(cmd, capture_output=True, text=True)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("scatter_host")
    exe, r = _build(d, "scatter_host")
    assert r.returncode == 0, r.stderr[-3000:]
    return d, exe


def run_thin(harness, state, prio, s2):
    """-> (states of the plain form, of the tiled form, sweeps, launches); the planes go in with rows of W + 3 cells whose padding
    holds candidates of priority 0 and must come back untouched"""
    d, exe = harness
    H, W = state.shape
    p = W + 3
    st, pr = np.full((H, p), S.UNDECIDED, np.uint8), np.zeros((H, p), np.uint32)
    st[:, :W], pr[:, :W] = state, prio
    (d / "in.bin").write_bytes(st.tobytes() + pr.tobytes())
    r = subprocess.run([str(exe), "thin"] + [str(v) for v in (H, W, p, s2, d / "in.bin", d / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    raw = (d / "out.bin").read_bytes()
    planes = np.frombuffer(raw[:2 * H * p], np.uint8).reshape(2, H, p)
    assert (planes[:, :, W:] == S.UNDECIDED).all(), "cells beyond a row's width were written"
    counts = np.frombuffer(raw[2 * H * p:], np.int64)
    return planes[0, :, :W], planes[1, :, :W], int(counts[0]), int(counts[1])


def run_chance(harness, h, tab, height_scale, density, seed, origin, dist2=None, water=None, blocked=None, threshold=0):
    """-> (chance, priority, state); inputs in rows of W + 3 cells with NaN, far and blocked padding, outputs in rows of W + 2 cells
    whose padding must come back untouched"""
    d, exe = harness
    H, W = h.shape
    pi, po = W + 3, W + 2
    planes = []
    for plane, dtype, fill in ((h, np.float32, np.nan), (dist2, np.int32, 0), (blocked, np.uint32, 0xFFFFFFFF)):
        wide = np.full((H, pi), fill, dtype)
        if plane is not None:
            wide[:, :W] = plane
        planes.append(wide.tobytes())
    wt = np.zeros(1, np.float32) if water is None else np.asarray(water, np.float32)
    (d / "in.bin").write_bytes(b"".join(planes) + np.asarray(tab, np.float32).tobytes() + wt.tobytes())
    args = ["chance", H, W, pi, po, seed & ((1 << 64) - 1), origin[0], origin[1], repr(float(height_scale)), repr(float(density)),
            wt.size - 1, threshold, d / "in.bin", d / "out.bin"]
    r = subprocess.run([str(exe)] + [str(v) for v in args], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    raw = np.frombuffer((d / "out.bin").read_bytes(), np.uint8)
    words = raw[:2 * H * po * 4].reshape(2, H, po * 4)
    state = raw[2 * H * po * 4:].reshape(H, po)
    assert (words[:, :, W * 4:] == 0xAB).all() and (state[:, W:] == 0xAB).all(), "cells beyond a row's width were written"
    body = np.ascontiguousarray(words[:, :, :W * 4]).view(np.uint32).reshape(2, H, W)
    return body[0], body[1], np.ascontiguousarray(state[:, :W])


@pytest.mark.parametrize("kind", S.KINDS)
def test_both_forms_of_the_thinning_on_the_host_build(harness, kind):
    for shape in S.SHAPES:
        for s2 in S.S2S:
            state, prio = S.thin_case(kind, shape)
            want = S.thin_expected(kind, shape, s2)
            plain, tiled, sweeps, launches = run_thin(harness, state, prio, s2)
            assert np.array_equal(plain, want), (kind, shape, s2, "plain")
            assert np.array_equal(tiled, want), (kind, shape, s2, "tiled")
            assert 1 <= launches <= sweeps <= shape[0] * shape[1] + 1


@pytest.mark.parametrize("rising", (True, False))
def test_the_staircases_on_the_host_build(harness, rising):
    for shape in ((1, 300), (300, 1)):
        state, prio = S.staircase(shape, rising)
        plain, tiled, sweeps, launches = run_thin(harness, state, prio, 2)
        want = S.thin(state, prio, 2)
        assert np.array_equal(plain, want) and np.array_equal(tiled, want)
        # the host runs the tiles one after the other, so a later tile sees what an earlier one wrote in the same launch: a chain
        # that rises with the tile order is done at once
        assert sweeps == 301 and launches <= 10 + 1 and (launches == 2) == rising


def chance_cases():
    """(label, h, tables, height_scale, density, seed, origin, dist2, water, blocked, threshold)"""
    tab, water = S.habitat_tables(3)
    out = []
    for k, shape in enumerate(((1, 1), (1, 40), (40, 1), (33, 65), (70, 45))):
        H, W = shape
        rng = np.random.RandomState(50 + k)
        d2 = rng.randint(-1, 30, size=shape).astype(np.int32)
        blocked = rng.randint(0, 6, size=shape).astype(np.uint32)
        out.append(("plain", S.heights(H, W, k), tab, 2.0, 1.0, 5, (0, 0), None, None, None, 0))
        out.append(("all", S.heights(H, W, k), tab, 48.0, 0.37, 0xFEEDFACE12345678, (-1000, 70000), d2, water, blocked, 4))
        out.append(("wild", S.heights(H, W, k, -2.0, 3.0), tab, 1.0, 0.9, -1, (-5, -(1 << 31)), d2, water, None, 0))
        out.append(("level", np.full(shape, 0.55, np.float32), tab, 64.0, 1.0, 1 << 40, ((1 << 31) - 3, -W), None, None, blocked, 1))
    return out


def test_the_chance_and_the_candidates_on_the_host_build(harness):
    seen = dict(zero=0, one=0, between=0, cand=0)
    for label, h, tab, hs, dens, seed, origin, d2, water, blocked, thr in chance_cases():
        want = S.chance(h, tab, hs, dens, d2, water, blocked, thr)
        ws, wp = S.candidates(want, seed, origin)
        c, p, s = run_chance(harness, h, tab, hs, dens, seed, origin, d2, water, blocked, thr)
        assert np.array_equal(c, want) and np.array_equal(p, wp) and np.array_equal(s, ws), (label, h.shape)
        seen['zero'] += int((want == 0).sum())
        seen['one'] += int((want == S.ONE).sum())
        seen['between'] += int(((want > 0) & (want < S.ONE)).sum())
        seen['cand'] += int(ws.sum())
    assert min(seen.values()) > 100, seen


def test_the_harness_under_the_sanitizers(tmp_path):
    """the same stand-alone program with -fsanitize=address,undefined: out-of-bounds LDS or plane indices and signed overflow in
    the kernels' index arithmetic end it"""
    exe, r = _build(tmp_path, "scatter_host_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])
    if r.returncode != 0:
        pytest.skip("the host compiler cannot link the sanitizer runtimes: " + r.stderr[-300:])
    h = (tmp_path, exe)
    for kind in ('random', 'sparse', 'corner'):
        for shape, s2 in (((1, 1), 1), ((1, 300), 2), ((300, 1), 50), ((33, 65), 1024), ((70, 45), 16), ((33, 65), 3)):
            state, prio = S.thin_case(kind, shape)
            plain, tiled, _, _ = run_thin(h, state, prio, s2)
            want = S.thin_expected(kind, shape, s2)
            assert np.array_equal(plain, want) and np.array_equal(tiled, want), (kind, shape, s2)
    for case in chance_cases()[:8]:
        label, hh, tab, hs, dens, seed, origin, d2, water, blocked, thr = case
        want = S.chance(hh, tab, hs, dens, d2, water, blocked, thr)
        c, p, s = run_chance(h, hh, tab, hs, dens, seed, origin, d2, water, blocked, thr)
        assert np.array_equal(c, want) and np.array_equal(s, S.candidates(want, seed, origin)[0])
