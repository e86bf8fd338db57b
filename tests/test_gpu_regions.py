"""The regions on the MI355X (csrc/regions.hip, gan_heightmaps_amd/regions.py): the labelling in both forms, the count,
the trace and the extraction through the raw entry points against tests/regions_ref.py bit for bit -- the definition is integer,
so there are no tolerances.  The labels go in with a pitch of W + 3 whose padding repeats the row's last label, so a read across the
pitch would join regions; component and polygon lie in canary canvases; the workspace, the per-edge buffers and every dense output
are followed by canary bytes.  Then ``regions``, the paint, the model's and the world's methods, the command line, and the
refusals of the raw entry points."""
import json

import numpy as np
import pytest

from oracle import step as ostep
from gan_heightmaps_amd import regions as RG
from tests import regions_ref as R
from tests.gpu_common import build_model, CANARY, Canvas, dev, model_params, ops, same, SMALL      # noqa: F401  (dev, ops: the module-scoped fixtures)

pytestmark = pytest.mark.gpu

TAIL = 64                    # canary bytes behind the workspace, the per-edge buffers and every dense array
DENSE = (("vertex", np.int32, "V"), ("ring_offsets", np.int64, "R1"), ("ring_polygon", np.int32, "R"), ("ring_hole", np.uint8, "R"),
         ("seed", np.int32, "P"), ("label", np.int32, "P"), ("cells", np.uint32, "P"))


def guarded(dev, bufs, nbytes):
    """a device buffer of nbytes followed by TAIL canary bytes -> (pointer, its host image)"""
    whole = np.full(nbytes + TAIL, CANARY, np.uint8)
    p = dev.alloc(whole.nbytes)
    bufs.append(p)
    dev.h2d(p, whole)
    return p, whole


def raw_regions(dev, ops, L, form, max_rounds=32):
    """-> dict of component, polygon, the dense arrays and the counts through the raw entry points"""
    H, W = L.shape
    bufs = []
    try:
        wide = np.empty((H, W + 3), np.int32)
        wide[:, :W] = L
        wide[:, W:] = L[:, -1:]
        d_l = dev.alloc(wide.nbytes)
        bufs.append(d_l)
        dev.h2d(d_l, wide)
        comp, poly = Canvas(dev, H, W, np.int32), Canvas(dev, H, W, np.int32)
        bufs += [comp.base, poly.base]
        d_w, ws = guarded(dev, bufs, ops.regions_workspace(H, W))
        sweeps = ops.regions_label(d_l, W + 3, H, W, RG.FORMS.index(form), comp.ptr, comp.pitch, d_w)
        E, P = ops.regions_count(d_l, W + 3, comp.ptr, comp.pitch, H, W, d_w)
        d_t, tr = guarded(dev, bufs, ops.regions_trace_bytes(E))
        first = ops.regions_trace(H, W, d_w, d_t, E, P, max_rounds)
        Rn, V, rounds = ops.regions_trace(H, W, d_w, d_t, E, P, max_rounds)          # a second trace finds what the count left
        assert first == (Rn, V, rounds)
        sizes = dict(V=V, R=Rn, R1=Rn + 1, P=P)
        host, ptrs = [], []
        for name, dtype, n in DENSE:
            nbytes = sizes[n] * np.dtype(dtype).itemsize
            p, whole = guarded(dev, bufs, nbytes)
            host.append((name, dtype, nbytes, whole))
            ptrs.append(p)
        ops.regions_extract(d_l, W + 3, comp.ptr, comp.pitch, H, W, d_w, d_t, E, P, Rn, V, *ptrs, poly.ptr, poly.pitch)
        dev.sync()
        got = dict(edges=E, polygons=P, rings=Rn, vertices=V, rounds=rounds, sweeps=sweeps, component=comp.read(), polygon=poly.read())
        for (name, dtype, nbytes, whole), p in zip(host, ptrs):
            dev.d2h(whole, p, whole.nbytes)
            assert (whole[nbytes:] == CANARY).all(), "bytes behind %s were written" % name
            got[name] = whole[:nbytes].view(dtype).copy()
        for what, whole, p in (("workspace", ws, d_w), ("per-edge buffers", tr, d_t)):
            dev.d2h(whole, p, whole.nbytes)
            assert (whole[-TAIL:] == CANARY).all(), "bytes behind the %s were written" % what
        return got
    finally:
        dev.sync()
        for b in bufs:
            dev.free(b)


KEYS = ("component", "polygon") + tuple(d[0] for d in DENSE)
COUNTS = ("edges", "polygons", "rings", "vertices", "rounds")


# ---- 1. the raw entry points, case by case, in both forms -----------------------------------------------------------------------------
@pytest.mark.parametrize("form", RG.FORMS)
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_every_array_equals_the_restatement(dev, ops, name, form):
    want = R.expected(name)
    if name in R.TABLE:
        assert tuple(want[k] for k in ("edges", "rings", "polygons", "holes", "vertices")) == R.TABLE[name]
    got = raw_regions(dev, ops, R.case(name), form)
    for k in KEYS:
        assert same(got[k], want[k]), (name, form, k)
    for k in COUNTS:
        assert got[k] == want[k], (name, form, k)
    if name == "checker96":
        assert got["edges"] == 4 * 96 * 96 and got["rings"] == got["polygons"] == 96 * 96
    if name == "empty":
        assert got["sweeps"] == 0
    elif form == 'union':
        assert got["sweeps"] == 1
    else:                                                                  # the sweeps race one another: their number is bounded, not fixed
        assert 1 <= got["sweeps"] <= R.case(name).size + 1
        if name in ("serpentine", "moat"):
            assert got["sweeps"] >= 2                                      # the seed's label travels against raster order through four tiles


# ---- 2. regions, the paint, the model's methods -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_model(dev):
    m = build_model(ostep.default_cfg(**SMALL), 5, dev, dtype="f32", use_graph=False)
    cfg = ostep.default_cfg(**SMALL)
    for s in range(3):                       # non-trivial BatchNorm running statistics (the deterministic pass reads them)
        m.z_fn(ostep.synthetic_batch(4, cfg, seed=40 + s)[0])
    return m


def reference(L, areas, origin):
    """what ``regions`` must give for a label plane, by the definition"""
    e = R.definition(L)
    return e, RG.report(e["vertex"], e["ring_offsets"], e["ring_polygon"], e["ring_hole"], e["seed"], e["label"], e["cells"], areas, origin,
                        L.shape, polygon_plane=e["polygon"].copy())


def same_regions(got, want):
    for k in ("vertex", "ring_offsets", "points", "ring_polygon", "hole", "seed", "label", "cells", "bbox", "perimeter"):
        assert same(getattr(got, k), getattr(want, k)), k
    return True


def test_regions_equals_the_definition(dev, ops):
    from gan_heightmaps_amd._lib import GhmError
    L = R.case("bands96")
    for areas in (RG.Areas(), RG.Areas(min_cells=12, holes=False)):
        e, want = reference(L, areas, (100, -20))
        for form in RG.FORMS:
            got = RG.regions(ops, L, areas, origin=(100, -20), form=form, keep=('polygon',))
            assert same_regions(got, want) and same(got.polygon_plane, want.polygon_plane) and got.form == form
            assert got.rounds == e["rounds"] > 10 and got.sweeps >= 1
    assert len(want) < e["polygons"] and not want.hole.any() and RG.regions(ops, L).form == RG.DEFAULT_FORM
    assert RG.regions(ops, L).polygon_plane is None
    whole = RG.regions(ops, L, keep='polygon')
    assert whole.at(0, 0) == e["polygon"][0, 0] and (whole.raster() == 1).all()
    with pytest.raises(GhmError, match="%d boundary edges" % e["edges"]):
        RG.regions(ops, L, max_edges=e["edges"] - 1)
    assert len(RG.regions(ops, L, max_edges=e["edges"])) == e["polygons"]
    # a wider integer plane, a row, a column, a plane without a region
    assert same_regions(RG.regions(ops, L.astype(np.int64)), reference(L, RG.Areas(), (0, 0))[1])
    for name in ("row", "column", "one"):
        assert same_regions(RG.regions(ops, R.case(name)), reference(R.case(name), RG.Areas(), (0, 0))[1])
    none = RG.regions(ops, R.case("empty"), keep='polygon')
    assert len(none) == 0 and none.sweeps == 0 and none.ring_offsets.tolist() == [0] and (none.polygon_plane == -1).all()


def test_the_models_methods_and_the_paint(small_model, dev, ops):
    from tests import hydrology_ref as HR
    from gan_heightmaps_amd import hydrology as HY
    from gan_heightmaps_amd.contour import Levels
    m = small_model
    before = model_params(m)
    h = HR.terrain(70, 90, None, 43)
    hydro = HY.analyse(ops, h)
    for of, labels, kw in (("lakes", RG.lakes(hydro), {}), ("basins", RG.basins(hydro), {}), ("land", RG.land(h, 0.5), dict(sea_level=0.5)),
                           ("bands", RG.bands(h, Levels(8.0)), dict(levels=Levels(8.0)))):
        _, want = reference(labels, RG.Areas(), (0, 0))
        assert same_regions(m.heightmap_regions(h, of, form='union', **kw), want), of
        assert same_regions(m.heightmap_regions(labels), want) and len(want) >= 1, of
    water = m.heightmap_regions(h, 'lakes', RG.Areas(min_cells=2))
    assert 1 <= len(water) and (water.cells >= 2).all()
    tex = np.random.RandomState(3).randint(0, 256, (70, 90, 3)).astype(np.uint8)
    for outline in (False, True):
        on = water.raster(outline) == 1
        painted = m.paint_regions(tex, water, (0.0, 1.0, 0.0), 1.0, outline)
        assert painted.dtype == np.uint8 and same(painted[~on], tex[~on]) and on.any()      # unpainted pixels keep their bits
        assert (painted[on] == [0, 255, 0]).all()
    filled = RG.lakes(hydro) >= 0
    assert not (water.raster() == 1)[~filled].any() and ((water.raster(True) == 1) <= (water.raster() == 1)).all()
    ftex = np.random.RandomState(4).rand(3, 70, 90).astype(np.float32) * 2 - 1
    on = water.raster() == 1
    fp = m.paint_regions(ftex, water)
    assert same(fp[:, ~on], ftex[:, ~on]) and (fp[:, on] != ftex[:, on]).any()
    after = model_params(m)
    for k in before:
        for x, y in zip(before[k], after[k]):
            assert np.array_equal(x, y), k


# ---- 3. the world -----------------------------------------------------------------------------------------------------------------------
def test_the_worlds_regions_are_the_rectangles_in_world_coordinates(small_model, dev, ops):
    from tests.gpu_common import ERO
    m = small_model
    with m.terrain_world(42, chunk_cells=2, erosion=ERO) as world:
        hm = world._unit_height(-20, 10, 70, 90)
        a = world.regions(-20, 10, 70, 90, of='land', sea_level=0.5)
        _, want = reference(RG.land(hm, 0.5), RG.Areas(), (-20, 10))
        assert a.origin == (-20, 10) and a.shape == (70, 90) and len(a) >= 1 and same_regions(a, want)
        p = a.points
        assert (p[:, 0] >= -20).all() and (p[:, 0] <= 50).all() and (p[:, 1] >= 10).all() and (p[:, 1] <= 100).all()
        b = world.regions(-20, 10, 70, 90, of='basins', areas=RG.Areas(min_cells=4))
        _, want = reference(RG.basins(world.hydrology(-20, 10, 70, 90, keep=('basin',))), RG.Areas(min_cells=4), (-20, 10))
        assert same_regions(b, want) and len(b) >= 1
        with pytest.raises(ValueError, match="sea_level"):
            world.regions(-20, 10, 70, 90, of='land')
        with pytest.raises(ValueError, match="of must be"):
            world.regions(-20, 10, 70, 90, of='seas')


# ---- 4. the command line ---------------------------------------------------------------------------------------------------------------
def test_command_line_writes_the_regions(ops, tmp_path, capsys):
    from tests import hydrology_ref as HR
    from gan_heightmaps_amd.util import read_image, save_png
    h = HR.terrain(70, 90, None, 43)
    np.save(str(tmp_path / "h.npy"), h)
    tex = np.random.RandomState(3).randint(0, 256, h.shape + (3,)).astype(np.uint8)
    save_png(str(tmp_path / "t.png"), tex)
    args = [str(tmp_path / "h.npy"), str(tmp_path / "o.geojson"), "--land", "0.5", "--union", "--min-cells", "3",
            "--texture", str(tmp_path / "t.png"), "--painted", str(tmp_path / "p.png"), "--colour", "1,0,0", "--opacity", "1"]
    assert RG.main(args) == 0
    want = RG.regions(ops, RG.land(h, 0.5), RG.Areas(3))
    assert capsys.readouterr().out.startswith("%d polygons with %d holes, %d vertices" % (len(want), int(want.hole.sum()), len(want.vertex)))
    assert json.load(open(str(tmp_path / "o.geojson")))["features"] == want.features() and len(want) >= 1
    on = want.raster() == 1
    painted = read_image(str(tmp_path / "p.png"))
    assert same(painted[~on], tex[~on]) and (painted[on] == [255, 0, 0]).all()
    np.save(str(tmp_path / "l.npy"), R.case("nested"))
    assert RG.main([str(tmp_path / "l.npy"), str(tmp_path / "o.npz"), "--labels", "--no-holes", "--sweep"]) == 0
    z = np.load(str(tmp_path / "o.npz"))
    assert z["cells"].tolist() == [16, 8, 1] and z["hole"].tolist() == [0, 0, 0] and z["areas"].tolist() == [1, 0]


# ---- 5. refusals of the raw entry points ----------------------------------------------------------------------------------------------
def test_refusals_of_the_entry_points(dev, ops):
    from gan_heightmaps_amd._lib import GhmError
    L, want = R.case("serpentine"), R.expected("serpentine")
    H, W = L.shape
    n = H * W
    E, P, Rn, V = (want[k] for k in ("edges", "polygons", "rings", "vertices"))
    d_l, d_c, d_p = dev.alloc(4 * n), dev.alloc(4 * n), dev.alloc(4 * n)
    d_w, d_t = dev.alloc(ops.regions_workspace(H, W)), dev.alloc(ops.regions_trace_bytes(E))
    outs = [np.full(4096, CANARY, np.uint8) for _ in range(7)]
    d_o = [dev.alloc(o.nbytes) for o in outs]
    try:
        dev.h2d(d_l, L)
        for p, o in zip(d_o, outs):
            dev.h2d(p, o)
        assert ops.regions_workspace(0, 5) == -1 and ops.regions_workspace(1 << 16, 1 << 15) == -1 and ops.regions_workspace(1, 9) > 0
        assert ops.regions_workspace(4 * 65535 + 1, 1) == -1 and ops.regions_workspace(1, (1 << 31) - 2) == -1      # 2^31 corners
        assert ops.regions_trace_bytes(-1) == -1 and ops.regions_trace_bytes(1 << 31) == -1 and ops.regions_trace_bytes(0) > 0

        def do_label(l=d_l, pl=W, Hh=H, Ww=W, form=0, c=d_c, pc=W, w=d_w):
            return ops.regions_label(l, pl, Hh, Ww, form, c, pc, w)

        for kw, match in ((dict(l=None), "null"), (dict(c=None), "null"), (dict(w=None), "null"), (dict(pl=W - 1), "pitch"),
                          (dict(pc=W - 1), "pitch"), (dict(Hh=0), "out of range"), (dict(Hh=4 * 65535 + 1, Ww=1), "out of range"),
                          (dict(Hh=1 << 16, Ww=1 << 15, pl=1 << 15, pc=1 << 15), "out of range"), (dict(form=2), "form"), (dict(form=-1), "form")):
            with pytest.raises(GhmError, match=match):
                do_label(**kw)

        def do_count(l=d_l, pl=W, c=d_c, pc=W, w=d_w, cap=(1 << 31) - 1):
            return ops.regions_count(l, pl, c, pc, H, W, w, cap)

        def do_trace(w=d_w, t=d_t, e=E, p=P, cap=32, Hh=H):
            return ops.regions_trace(Hh, W, w, t, e, p, cap)

        def do_extract(l=d_l, c=d_c, w=d_w, t=d_t, e=E, p=P, r=Rn, v=V, o=tuple(d_o), poly=d_p, pp=W):
            ops.regions_extract(l, W, c, W, H, W, w, t, e, p, r, v, *o, poly, pp)

        dev.h2d(d_w, np.full(ops.regions_workspace(H, W), CANARY, np.uint8))
        with pytest.raises(GhmError, match="counted"):                    # a workspace nothing has counted in
            do_trace()
        with pytest.raises(GhmError, match="counted"):
            do_extract()
        dev.h2d(d_c, np.zeros(n, np.int32))                               # a component plane that is nobody's labelling
        with pytest.raises(GhmError, match="component plane"):
            do_count()
        assert do_label() >= 2
        for kw, match in ((dict(l=None), "null"), (dict(c=None), "null"), (dict(w=None), "null"), (dict(pl=W - 1), "pitch"),
                          (dict(cap=-1), "max_edges"), (dict(cap=1 << 31), "max_edges"), (dict(cap=E - 1), "%d boundary edges" % E)):
            with pytest.raises(GhmError, match=match):
                do_count(**kw)
        with pytest.raises(GhmError, match="counted"):                    # the refused counts left none
            do_trace()
        assert do_count(cap=E) == (E, P)
        for kw, match in ((dict(w=None), "null"), (dict(t=None), "null"), (dict(e=E + 1), "counted"), (dict(p=P + 1), "counted"),
                          (dict(Hh=H + 1), "counted"), (dict(cap=0), "max_rounds"), (dict(cap=33), "max_rounds"),
                          (dict(cap=5), "after 5 rounds"), (dict(cap=10), "after 10 rounds")):
            with pytest.raises(GhmError, match=match):
                do_trace(**kw)
        with pytest.raises(GhmError, match="no trace"):                   # the refused traces left none
            do_extract()
        assert do_trace(cap=11) == (Rn, V, 11) and want["rounds"] == 11
        for kw, match in ((dict(l=None), "null"), (dict(c=None), "null"), (dict(w=None), "null"), (dict(t=None), "null"),
                          (dict(o=(None,) + tuple(d_o[1:])), "null"), (dict(o=tuple(d_o[:6]) + (None,)), "null"), (dict(e=E - 1), "counted"),
                          (dict(r=Rn + 1), "traced"), (dict(v=V - 1), "traced"), (dict(pp=W - 1), "pitch")):
            with pytest.raises(GhmError, match=match):
                do_extract(**kw)
        dev.sync()
        for p, o in zip(d_o, outs):                                        # no refusal has touched the outputs
            dev.d2h(o, p, o.nbytes)
            assert (o == CANARY).all()
        do_extract(poly=None, pp=0)                                        # the polygon plane may be left out
        dev.sync()
        dev.d2h(outs[0], d_o[0], outs[0].nbytes)
        assert same(outs[0][:4 * V].view(np.int32), want["vertex"]) and (outs[0][4 * V:] == CANARY).all()
        dev.d2h(outs[6], d_o[6], outs[6].nbytes)
        assert outs[6][:4].view(np.uint32).tolist() == [611] and (outs[6][4:] == CANARY).all()
    finally:
        dev.sync()
        for b in [d_l, d_c, d_p, d_w, d_t] + d_o:
            dev.free(b)
