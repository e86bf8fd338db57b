"""The rivers on the MI355X (csrc/rivers.hip, gan_heightmaps_amd/rivers.py): the count, the trace in both forms and
the extraction through the raw entry points, and the host's orders, against tests/rivers_ref.py bit for bit -- the definition is
integer, so there are no tolerances.  The directions go in with a pitch of W + 3 whose padding points east, the accumulation with
one whose padding is 2^32 - 1 and must never become a stream cell; kind lies in a canary canvas with a pitch of W + 2; the
workspace, the list and the dense outputs are followed by canary bytes.  Then ``rivers``, the paint, the model's and the world's
methods, sources as route sources, the command line, and the refusals of the raw entry points."""
import json

import numpy as np
import pytest

from oracle import step as ostep
from gan_heightmaps_amd import hydrology as HY
from gan_heightmaps_amd import rivers as RV
from tests import hydrology_ref as HR
from tests import rivers_ref as R
from tests.gpu_common import build_model, CANARY, Canvas, dev, model_params, ops, padded, same, SMALL      # noqa: F401  (dev, ops: the module-scoped fixtures)

pytestmark = pytest.mark.gpu

TAIL = 64                    # canary bytes behind every dense array


def raw_rivers(dev, ops, direction, A, T, form, max_rounds=32):
    """-> dict of kind, the dense arrays, the orders and the counts through the raw entry points"""
    H, W = direction.shape
    bufs = []
    try:
        d_d, pd = padded(dev, direction, np.int8, 3, 2)
        bufs.append(d_d)
        d_a, pa = padded(dev, A, np.uint32, 3, 0xffffffff)
        bufs.append(d_a)
        kind = Canvas(dev, H, W, np.uint8)
        bufs.append(kind.base)
        ws = np.full(ops.rivers_workspace(H, W) + TAIL, CANARY, np.uint8)
        d_w = dev.alloc(ws.nbytes)
        bufs.append(d_w)
        dev.h2d(d_w, ws)
        cells, Rn, sources, confluences, mouths, isolated = ops.rivers_count(d_d, pd, d_a, pa, H, W, T, kind.ptr, kind.pitch, d_w)
        d_l, lst = None, None
        if form == 'list':
            lst = np.full(ops.rivers_list_bytes(cells) + TAIL, CANARY, np.uint8)
            d_l = dev.alloc(lst.nbytes)
            bufs.append(d_l)
            dev.h2d(d_l, lst)
        V, rounds = ops.rivers_trace(d_d, pd, kind.ptr, kind.pitch, H, W, RV.FORMS.index(form), d_w, d_l, cells, Rn, max_rounds)
        host, ptrs = [], []
        for name, dtype, n in (("vertex", np.int32, V), ("offsets", np.int64, Rn + 1), ("downstream", np.int32, Rn)):
            nbytes = n * np.dtype(dtype).itemsize
            whole = np.full(nbytes + TAIL, CANARY, np.uint8)
            p = dev.alloc(whole.nbytes)
            bufs.append(p)
            dev.h2d(p, whole)
            host.append((name, dtype, nbytes, whole))
            ptrs.append(p)
        ops.rivers_extract(d_d, pd, kind.ptr, kind.pitch, H, W, d_w, d_l, cells, Rn, V, *ptrs)
        dev.sync()
        got = dict(cells=cells, reaches=Rn, sources=sources, confluences=confluences, mouths=mouths, isolated=isolated, rounds=rounds,
                   kind=kind.read())
        for (name, dtype, nbytes, whole), p in zip(host, ptrs):
            dev.d2h(whole, p, whole.nbytes)
            assert (whole[nbytes:] == CANARY).all(), "bytes behind %s were written" % name
            got[name] = whole[:nbytes].view(dtype).copy()
        for what, whole, p in (("workspace", ws, d_w), ("list", lst, d_l)):
            if whole is not None:
                dev.d2h(whole, p, whole.nbytes)
                assert (whole[-TAIL:] == CANARY).all(), "bytes behind the %s were written" % what
        got["area"] = RV.reach_areas(got["vertex"], got["offsets"], got["downstream"], direction, A)
        got["order"], got["magnitude"], got["main"] = ops.rivers_order(got["downstream"], got["area"])
        return got
    finally:
        dev.sync()
        for b in bufs:
            dev.free(b)


KEYS = ("kind", "vertex", "offsets", "downstream", "area", "order", "magnitude", "main")
COUNTS = ("cells", "reaches", "sources", "confluences", "mouths", "isolated", "rounds")


# ---- 1. the raw entry points, case by case, in both forms -----------------------------------------------------------------------------
@pytest.mark.parametrize("form", RV.FORMS)
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_every_array_equals_the_restatement(dev, ops, name, form):
    want = R.expected(name)
    if name == "serpentine_t8":
        assert want["rounds"] == 9 and len(want["vertex"]) == 506 and want["reaches"] == 1
    if name == "comb":
        assert want["reaches"] == 1799 and (np.diff(want["offsets"]) == 2).all()
    if name == "noise0_t1":
        assert want["reaches"] == 3063 and want["isolated"] == 246 and int(want["order"].max()) == 6
    got = raw_rivers(dev, ops, *R.planes(name), form)
    for k in KEYS:
        assert same(got[k], want[k]), (name, form, k)
    for k in COUNTS:
        assert got[k] == want[k], (name, form, k)


# ---- 2. rivers, the paint, the model's methods -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_model(dev):
    m = build_model(ostep.default_cfg(**SMALL), 5, dev, dtype="f32", use_graph=False)
    cfg = ostep.default_cfg(**SMALL)
    for s in range(3):                       # non-trivial BatchNorm running statistics (the deterministic pass reads them)
        m.z_fn(ostep.synthetic_batch(4, cfg, seed=40 + s)[0])
    return m


def reference(hydro, network, origin):
    """what ``rivers`` must give for a Hydrology, by the definition"""
    e = R.definition(hydro.direction, hydro.accumulation, network.river_threshold)
    return e, RV.report(e["vertex"], e["offsets"], e["downstream"], e["order"], e["magnitude"], e["main"], e["area"], network, origin,
                        hydro.shape, filled=hydro.filled, depth=hydro.depth)


def same_rivers(got, want):
    for k in ("vertex", "offsets", "points", "downstream", "order", "magnitude", "main", "area", "length"):
        assert same(getattr(got, k), getattr(want, k)), k
    for k in ("height", "lake"):
        assert (getattr(got, k) is None) == (getattr(want, k) is None)
        if getattr(want, k) is not None:
            assert same(getattr(got, k), getattr(want, k)), k
    return True


@pytest.fixture(scope="module")
def plane_hydro(ops):
    """the hydrology of a 70 x 90 plane, analysed once on the device and shared"""
    h = HR.terrain(70, 90, None, 43)
    hydro = HY.analyse(ops, h)
    for k in HY.KEEP:
        getattr(hydro, k).setflags(write=False)
    return h, hydro


def test_rivers_equals_the_definition(dev, ops, plane_hydro):
    h, hydro = plane_hydro
    net = RV.Network(8, 1, 1.0 / 512)
    e, want = reference(hydro, net, (100, -20))
    got = {form: RV.rivers(ops, hydro, net, origin=(100, -20), form=form, keep=('kind',)) for form in RV.FORMS}
    for form in RV.FORMS:
        assert same_rivers(got[form], want) and same(got[form].kind, e["kind"]) and got[form].form == form
        assert got[form].rounds == e["rounds"] >= 1
        assert (got[form].sources_count, got[form].confluences_count, got[form].mouths_count, got[form].isolated) == (
            e["sources"], e["confluences"], e["mouths"], e["isolated"])
    assert len(want) > 20 and int(want.order.max()) >= 3 and want.lake.any() and RV.rivers(ops, hydro, net).form == RV.DEFAULT_FORM
    assert want.height.dtype == np.float32 and same(want.height, hydro.filled.ravel()[want.vertex])
    top = RV.rivers(ops, hydro, RV.Network(8, 2), origin=(100, -20))
    _, want2 = reference(hydro, RV.Network(8, 2), (100, -20))
    assert same_rivers(top, want2) and 0 < len(top) < len(want) and (top.order >= 2).all()
    with pytest.raises(ValueError, match="%d reaches" % e["reaches"]):
        RV.rivers(ops, hydro, net, max_reaches=e["reaches"] - 1)
    assert len(RV.rivers(ops, hydro, net, max_reaches=e["reaches"])) == len(want)
    bare = HY.Hydrology(hydro.shape, hydro.sweeps, hydro.rounds, hydro.tiled, direction=hydro.direction, accumulation=hydro.accumulation)
    r = RV.rivers(ops, bare, net)
    assert r.height is None and r.lake is None and same(r.vertex, want.vertex)
    for rows, cols in ((slice(0, 1), slice(None)), (slice(None), slice(0, 1)), (slice(0, 1), slice(0, 1))):
        thin = HY.analyse(ops, np.ascontiguousarray(h[rows, cols]))
        _, w = reference(thin, RV.Network(1), (0, 0))
        assert same_rivers(RV.rivers(ops, thin, RV.Network(1)), w)
    from gan_heightmaps_amd._lib import GhmError
    wrong = hydro.accumulation.copy()
    wrong[35, 45] = 0xffffffff
    with pytest.raises(GhmError, match="accumulation"):
        RV.rivers(ops, HY.Hydrology(hydro.shape, hydro.sweeps, hydro.rounds, hydro.tiled, direction=hydro.direction, accumulation=wrong), net)


def test_the_models_methods_the_paint_and_the_planes_that_fit(small_model, dev, ops, plane_hydro):
    m = small_model
    before = model_params(m)
    h, hydro = plane_hydro
    net = RV.Network(8)
    want = RV.rivers(ops, hydro, net)
    got = m.heightmap_rivers(h, net, form='list')
    assert same_rivers(got, want) and len(got) > 20 and got.form == 'list'
    assert same_rivers(m.heightmap_rivers(hydro, net), want)
    tex = np.random.RandomState(3).randint(0, 256, (70, 90, 3)).astype(np.uint8)
    for least, width in ((1, 0), (2, 1)):
        on = got.raster() >= least
        near = np.zeros((70, 90), bool)
        for r, c in np.argwhere(on):
            near[max(r - width, 0):r + width + 1, max(c - width, 0):c + width + 1] = True
        painted = m.paint_rivers(tex, got, least, width, (0.0, 1.0, 0.0), 1.0)
        assert painted.dtype == np.uint8 and same(painted[~near], tex[~near])              # unpainted pixels keep their bits
        assert (painted[near] == [0, 255, 0]).all() and near.sum() >= 4
    ftex = np.random.RandomState(4).rand(3, 70, 90).astype(np.float32) * 2 - 1
    on = got.raster() >= 1
    fp = m.paint_rivers(ftex, got)
    assert same(fp[:, ~on], ftex[:, ~on]) and (fp[:, on] != ftex[:, on]).any()
    # towns at the springs and where rivers meet: the planes fit
    roads = m.heightmap_routes(h, got.sources())
    assert roads.cost.shape == (70, 90) and all(roads.cost[r, c] == 0 for r, c in got.sources())
    assert len(got.confluences()) >= 1 and len(got.mouths()) >= 1
    after = model_params(m)
    for k in before:
        for x, y in zip(before[k], after[k]):
            assert np.array_equal(x, y), k


# ---- 3. the world -----------------------------------------------------------------------------------------------------------------------
def test_the_worlds_rivers_are_the_rectangles_in_world_coordinates(small_model, dev, ops):
    from tests.gpu_common import ERO
    m = small_model
    net = RV.Network(8)
    with m.terrain_world(42, chunk_cells=2, erosion=ERO) as world:
        a = world.rivers(-20, 10, 70, 90, net)
        assert a.origin == (-20, 10) and a.shape == (70, 90) and len(a) >= 1
        hydro = world.hydrology(-20, 10, 70, 90)
        assert same_rivers(a, RV.rivers(ops, hydro, net, origin=(-20, 10)))
        _, want = reference(hydro, net, (-20, 10))
        assert same_rivers(a, want)
        p = a.points
        assert (p[:, 0] >= -20).all() and (p[:, 0] < 50).all() and (p[:, 1] >= 10).all() and (p[:, 1] < 100).all()
        assert same(a.height, hydro.filled[p[:, 0] + 20, p[:, 1] - 10])


# ---- 4. the command line ---------------------------------------------------------------------------------------------------------------
def test_command_line_writes_the_rivers(ops, tmp_path, capsys, plane_hydro):
    h, hydro = plane_hydro
    np.save(str(tmp_path / "h.npy"), h)
    tex = np.random.RandomState(3).randint(0, 256, h.shape + (3,)).astype(np.uint8)
    from gan_heightmaps_amd.util import read_image, save_png
    save_png(str(tmp_path / "t.png"), tex)
    args = [str(tmp_path / "h.npy"), str(tmp_path / "o.geojson"), "--river-threshold", "8", "--list",
            "--texture", str(tmp_path / "t.png"), "--painted", str(tmp_path / "p.png"), "--colour", "1,0,0", "--opacity", "1"]
    assert RV.main(args) == 0
    want = RV.rivers(ops, hydro, RV.Network(8))
    assert capsys.readouterr().out.startswith("%d reaches of order up to %d, %d rounds" % (len(want), int(want.order.max()), want.rounds))
    g = json.load(open(str(tmp_path / "o.geojson")))
    assert g["features"] == want.features() and len(want) > 20
    on = want.raster() >= 1
    painted = read_image(str(tmp_path / "p.png"))
    assert same(painted[~on], tex[~on]) and (painted[on] == [255, 0, 0]).all()
    assert RV.main(args[:1] + [str(tmp_path / "o.npz"), "--river-threshold", "8", "--min-order", "2", "--plain"]) == 0
    z = np.load(str(tmp_path / "o.npz"))
    want2 = RV.rivers(ops, hydro, RV.Network(8, 2))
    assert same(z["vertex"], want2.vertex) and same(z["downstream"], want2.downstream) and same(z["order"], want2.order)
    assert same(z["height"], want2.height) and same(z["lake"], want2.lake)


# ---- 5. refusals of the raw entry points ----------------------------------------------------------------------------------------------
def test_refusals_of_the_entry_points(dev, ops):
    from gan_heightmaps_amd._lib import GhmError
    want = R.expected("serpentine_t8")
    direction, A, T = R.planes("serpentine_t8")
    H, W = direction.shape
    n = H * W
    d_d, d_k = dev.alloc(n + 256), dev.alloc(n + 256)
    d_a, d_bad = dev.alloc(4 * n + 256), dev.alloc(4 * n + 256)
    d_w = dev.alloc(ops.rivers_workspace(H, W))
    outs = [np.full(4096, CANARY, np.uint8) for _ in range(3)]
    d_o = [dev.alloc(o.nbytes) for o in outs]
    d_l = None
    try:
        dev.h2d(d_d, direction)
        dev.h2d(d_a, A)
        for p, o in zip(d_o, outs):
            dev.h2d(p, o)
        assert ops.rivers_workspace(0, 5) == -1 and ops.rivers_workspace(1 << 16, 1 << 15) == -1 and ops.rivers_workspace(1, 9) > 0
        assert ops.rivers_workspace(4 * 65535 + 1, 1) == -1
        assert ops.rivers_list_bytes(-1) == -1 and ops.rivers_list_bytes(1 << 31) == -1 and ops.rivers_list_bytes(0) > 0

        def do_count(d=d_d, pd=W, a=d_a, pa=W, Hh=H, Ww=W, t=T, k=d_k, pk=W, w=d_w):
            return ops.rivers_count(d, pd, a, pa, Hh, Ww, t, k, pk, w)

        plane = ((dict(d=None), "null"), (dict(pd=W - 1), "pitch"), (dict(Hh=0), "out of range"), (dict(Hh=4 * 65535 + 1, Ww=1), "out of range"),
                 (dict(Hh=1 << 16, Ww=1 << 15, pd=1 << 15), "out of range"), (dict(Hh=1 << 15, pd=1 << 16), "pitch"))
        for kw, match in plane + ((dict(a=None), "null"), (dict(k=None), "null"), (dict(w=None), "null"), (dict(pa=W - 1), "pitch"),
                                  (dict(pk=W - 1), "pitch"), (dict(t=0), "threshold")):
            with pytest.raises(GhmError, match=match):
                do_count(**kw)
        # planes that are no drainage's: a direction out of range, a receiver outside, an accumulation that does not grow downstream
        for at, v, match in (((5, 5), 8, "direction"), ((5, 5), -2, "direction"), ((0, 7), 0, "outside the plane"),
                             ((H - 1, W - 1), 3, "outside the plane")):
            bad = direction.copy()
            bad[at] = v
            dev.h2d(d_k, bad)
            with pytest.raises(GhmError, match=match):
                do_count(d=d_k)
        stream = np.argwhere((want["kind"] & R.STREAM != 0) & (want["kind"] >> 4 == 1) & (want["kind"] & R.MOUTH == 0))[40]
        bad = A.copy()
        bad[tuple(stream)] = 0xffffffff
        dev.h2d(d_bad, bad)
        with pytest.raises(GhmError, match="accumulation"):
            do_count(a=d_bad)

        def do_trace(d=d_d, k=d_k, pk=W, form=0, w=d_w, lst=None, c=None, r=1, cap=32):
            return ops.rivers_trace(d, W, k, pk, H, W, form, w, lst, cells if c is None else c, r, cap)

        def do_extract(d=d_d, k=d_k, w=d_w, lst=None, c=None, r=1, v=506, o=tuple(d_o)):
            ops.rivers_extract(d, W, k, W, H, W, w, lst, cells if c is None else c, r, v, *o)

        cells = want["cells"]
        dev.h2d(d_w, np.full(ops.rivers_workspace(H, W), CANARY, np.uint8))
        with pytest.raises(GhmError, match="counted"):                    # a workspace nothing has counted in
            do_trace()
        with pytest.raises(GhmError, match="counted"):
            do_extract()
        counts = do_count()
        assert counts == tuple(want[k] for k in COUNTS[:6]) and counts[1] == 1
        d_l = dev.alloc(ops.rivers_list_bytes(cells))
        for kw, match in ((dict(d=None), "null"), (dict(k=None), "null"), (dict(w=None), "null"), (dict(pk=W - 1), "pitch"),
                          (dict(form=2), "form"), (dict(form=-1), "form"), (dict(form=1), "list buffer"), (dict(c=cells + 1), "counted"),
                          (dict(r=2), "counted"), (dict(cap=0), "max_rounds"), (dict(cap=33), "max_rounds"),
                          (dict(cap=5), "after 5 rounds"), (dict(form=1, lst=d_l, cap=5), "after 5 rounds"), (dict(cap=8), "after 8 rounds")):
            with pytest.raises(GhmError, match=match):
                do_trace(**kw)
        with pytest.raises(GhmError, match="no trace"):                   # the refused traces left none
            do_extract()
        assert do_trace(cap=9) == (506, 9)
        for kw, match in ((dict(d=None), "null"), (dict(k=None), "null"), (dict(w=None), "null"), (dict(o=(None,) + tuple(d_o[1:])), "null"),
                          (dict(o=(d_o[0], None, d_o[2])), "null"), (dict(o=tuple(d_o[:2]) + (None,)), "null"), (dict(r=2), "counted"),
                          (dict(c=cells - 1), "counted"), (dict(v=505), "vertices")):
            with pytest.raises(GhmError, match=match):
                do_extract(**kw)
        dev.sync()
        for p, o in zip(d_o, outs):                                        # no refusal has touched the outputs
            dev.d2h(o, p, o.nbytes)
            assert (o == CANARY).all()
        do_extract()
        dev.sync()
        dev.d2h(outs[0], d_o[0], outs[0].nbytes)
        assert same(outs[0][:4 * 506].view(np.int32), want["vertex"]) and (outs[0][4 * 506:] == CANARY).all()
        # a trace in the list form makes the extraction need the list
        assert do_trace(form=1, lst=d_l) == (506, 9)
        with pytest.raises(GhmError, match="list"):
            do_extract()
        do_extract(lst=d_l)
        dev.sync()
        dev.d2h(outs[1], d_o[1], outs[1].nbytes)
        assert outs[1][:16].view(np.int64).tolist() == [0, 506] and (outs[1][16:] == CANARY).all()
        # the orders refuse what is no forest
        assert [x.tolist() for x in ops.rivers_order(np.array([-1, 0, 1, 2, 2]), np.array([5, 4, 3, 1, 1]))] == [
            [2, 2, 2, 1, 1], [2, 2, 2, 1, 1], [1, 1, 1, 1, 0]]
        assert [len(x) for x in ops.rivers_order(np.zeros(0, np.int32), np.zeros(0, np.uint32))] == [0, 0, 0]
        for down, match in (([2, -1], "outside"), ([-2, -1], "outside"), ([0], "its own downstream"), ([1, 0], "cycle")):
            with pytest.raises(GhmError, match=match):
                ops.rivers_order(np.array(down, np.int32), np.ones(len(down), np.uint32))
        with pytest.raises(ValueError, match="areas"):
            ops.rivers_order(np.array([-1], np.int32), np.ones(2, np.uint32))
    finally:
        dev.sync()
        for b in [d_d, d_k, d_a, d_bad, d_w] + d_o + ([d_l] if d_l is not None else []):
            dev.free(b)
