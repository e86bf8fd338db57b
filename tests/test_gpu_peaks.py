"""The peaks on the MI355X (csrc/peaks.hip, gan_heightmaps_amd/peaks.py): the ascent, the labels and areas (the
hydrology's accumulation over the ascent), the count, the tree in both forms and the extraction through the raw entry points, and
the host's merge, against tests/peaks_ref.py bit for bit -- the definition is integer, so there are no tolerances.  The quantised
heights go in with a pitch of W + 3 whose padding is 2^30 high and must never win an ascent; the ascent, label, area and mask
planes lie in canary canvases with a pitch of W + 2; the dense outputs are followed by canary bytes.  Then ``peaks``, the paint,
the model's and the world's methods, peaks as observers and passes as route sources, and the refusals of the raw entry points."""
import numpy as np
import pytest

from oracle import step as ostep
from gan_heightmaps_amd import peaks as PK
from tests import peaks_ref as R
from tests.gpu_common import build_model, CANARY, Canvas, dev, model_params, ops, padded, same, SMALL      # noqa: F401  (dev, ops: the module-scoped fixtures)

pytestmark = pytest.mark.gpu

TAIL = 64                    # canary bytes behind every dense array


def raw_peaks(dev, ops, zq, form, max_rounds=32):
    """-> dict of the planes, the dense arrays, the merge's answer and the rounds through the raw entry points"""
    H, W = zq.shape
    bufs = []
    try:
        d_z, pz = padded(dev, zq, np.int32, 3, 1 << 30)
        bufs.append(d_z)
        asc, label, area, mask = (Canvas(dev, H, W, t) for t in (np.int8, np.int32, np.uint32, np.uint32))
        bufs += [c.base for c in (asc, label, area, mask)]
        d_hw = dev.alloc(ops.hydrology_workspace(H, W))
        bufs.append(d_hw)
        ops.peaks_ascent(d_z, pz, H, W, asc.ptr, asc.pitch)
        ops.hydrology_accumulate(asc.ptr, asc.pitch, H, W, area.ptr, area.pitch, label.ptr, label.pitch, d_hw)
        ws = np.full(ops.peaks_workspace(H, W) + TAIL, CANARY, np.uint8)
        d_w = dev.alloc(ws.nbytes)
        bufs.append(d_w)
        dev.h2d(d_w, ws)
        P, E = ops.peaks_count(d_z, pz, label.ptr, label.pitch, H, W, d_w)
        d_l, lst = None, None
        if form == 'list':
            lst = np.full(ops.peaks_list_bytes(E) + TAIL, CANARY, np.uint8)
            d_l = dev.alloc(lst.nbytes)
            bufs.append(d_l)
            dev.h2d(d_l, lst)
        rounds = ops.peaks_tree(d_z, pz, label.ptr, label.pitch, H, W, PK.FORMS.index(form), mask.ptr, mask.pitch, d_w, d_l, P, E,
                                max_rounds)
        host, ptrs = [], []
        for name, dtype, n in (("summit", np.int32, P), ("summit_area", np.uint32, P), ("tree", np.int32, 3 * (P - 1))):
            whole = np.full(4 * n + TAIL, CANARY, np.uint8)
            p = dev.alloc(whole.nbytes)
            bufs.append(p)
            dev.h2d(p, whole)
            host.append((name, dtype, 4 * n, whole))
            ptrs.append(p)
        ops.peaks_extract(label.ptr, label.pitch, area.ptr, area.pitch, mask.ptr, mask.pitch, H, W, d_w, P, *ptrs)
        dev.sync()
        got = dict(rounds=rounds, edges=E, ascent=asc.read(), label=label.read(), area=area.read(), mask=mask.read())
        for (name, dtype, n, whole), p in zip(host, ptrs):
            dev.d2h(whole, p, whole.nbytes)
            assert (whole[n:] == CANARY).all(), "bytes behind %s were written" % name
            got[name] = whole[:n].view(dtype).copy()
        got["tree"] = got["tree"].reshape(-1, 3)
        for what, whole, p in (("workspace", ws, d_w), ("list", lst, d_l)):
            if whole is not None:
                dev.d2h(whole, p, whole.nbytes)
                assert (whole[-TAIL:] == CANARY).all(), "bytes behind the %s were written" % what
        z = zq.ravel()
        got["col"], got["parent"], got["prominence_q"] = ops.peaks_merge(got["summit"], z[got["summit"]], got["tree"],
                                                                         z[got["tree"][:, 0]], int(z.min()))
        return got
    finally:
        dev.sync()
        for b in bufs:
            dev.free(b)


# ---- 1. the raw entry points, case by case, in both forms -----------------------------------------------------------------------------
@pytest.mark.parametrize("form", PK.FORMS)
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_every_array_equals_the_restatement(dev, ops, name, form):
    want = R.expected(name)
    if name == "ruler":
        assert want["rounds"] == 6 and len(want["summit"]) == 64
    if name == "staircase":
        assert want["rounds"] == 1 and len(want["summit"]) == 128
    if name == "spiral":
        assert want["hops"] > 1024 and len(want["summit"]) == 1
    got = raw_peaks(dev, ops, want["zq"], form)
    for k in ("ascent", "label", "area", "summit", "summit_area", "tree", "col", "parent", "prominence_q"):
        assert same(got[k], want[k]), (name, form, k)
    assert got["rounds"] == want["rounds"], (name, form)
    assert got["edges"] == len(R.edges(want["zq"], want["label"])), (name, form)
    bits = sum(bin(int(v)).count("1") for v in got["mask"].ravel())
    assert bits == len(want["tree"]) and set(np.flatnonzero(got["mask"].ravel()).tolist()) == set(want["tree"][:, 0].tolist())


# ---- 2. peaks, the paint, the model's methods -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_model(dev):
    m = build_model(ostep.default_cfg(**SMALL), 5, dev, dtype="f32", use_graph=False)
    cfg = ostep.default_cfg(**SMALL)
    for s in range(3):                       # non-trivial BatchNorm running statistics (the deterministic pass reads them)
        m.z_fn(ostep.synthetic_batch(4, cfg, seed=40 + s)[0])
    return m


def reference(h, rule, origin):
    """what ``peaks`` must give, by the definition"""
    zq = R.quantise(h, rule.height_scale)
    d = R.definition(zq)
    z = zq.ravel()
    _, area, _ = R.labels(R.ascent(zq))
    return zq, PK.report(d["summit"], z[d["summit"]], d["col"], z[np.maximum(d["col"], 0)], d["parent"], d["prominence_q"],
                         area.ravel()[d["summit"]], rule, origin, zq.shape)


def same_peaks(got, want):
    for k in ("cell", "height", "prominence", "col", "parent", "area", "on_edge"):
        assert same(getattr(got, k), getattr(want, k)), k
    assert np.array_equal(np.isnan(got.col_height), np.isnan(want.col_height))
    assert same(np.nan_to_num(got.col_height), np.nan_to_num(want.col_height)) and got.summits == want.summits
    assert all(p < i for i, p in enumerate(got.parent))
    return True


def test_peaks_equals_the_definition(dev, ops):
    h = R.heights(70, 90, 43, 5)
    rule = PK.Prominence(0.1, None, 20.0)
    zq, want = reference(h, rule, (100, -20))
    got = {form: PK.peaks(ops, h[None], rule, origin=(100, -20), form=form, keep=('zq', 'label')) for form in PK.FORMS}
    for form in PK.FORMS:
        assert same_peaks(got[form], want) and same(got[form].zq, zq) and got[form].form == form
        assert same(got[form].label, R.labels(R.ascent(zq))[0]) and got[form].rounds == got['plain'].rounds >= 1
    assert len(want) > 5 and want.summits > len(want) and PK.peaks(ops, h, rule).form == PK.DEFAULT_FORM
    top = PK.peaks(ops, h, PK.Prominence(0.1, 3, 20.0), origin=(100, -20))
    assert same(top.cell, want.cell[:3]) and same(top.parent, want.parent[:3])
    with pytest.raises(ValueError, match="%d summits" % want.summits):
        PK.peaks(ops, h, rule, max_summits=want.summits - 1)
    assert len(PK.peaks(ops, h, rule, max_summits=want.summits)) == len(want)
    u8 = (h * 255).astype(np.uint8)
    _, want8 = reference(u8.astype(np.float32) / np.float32(255), PK.Prominence(), (0, 0))
    assert same_peaks(PK.peaks(ops, u8), want8)
    for thin in (h[:1], h[:, :1], h[:1, :1]):
        _, w = reference(thin, rule, (0, 0))
        assert same_peaks(PK.peaks(ops, thin, rule), w)


def test_the_models_methods_the_paint_and_the_planes_that_fit(small_model, dev, ops):
    m = small_model
    before = model_params(m)
    h = R.heights(70, 90, 43, 5)
    rule = PK.Prominence(0.1, None, 20.0)
    want = PK.peaks(ops, h, rule)
    got = m.heightmap_peaks(h, rule, form='plain')
    assert same_peaks(got, want) and len(got) > 5
    tex = np.random.RandomState(3).randint(0, 256, (70, 90, 3)).astype(np.uint8)
    for cols in (False, True):
        at = np.array(got.passes() if cols else got.cell.tolist())
        near = np.zeros((70, 90), bool)
        for r, c in at:
            near[max(r - 1, 0):r + 2, max(c - 1, 0):c + 2] = True
        painted = m.paint_peaks(tex, got, (0.0, 1.0, 0.0), radius=1, cols=cols)
        assert painted.dtype == np.uint8 and same(painted[~near], tex[~near])              # unpainted pixels keep their bits
        assert (painted[near] == [0, 255, 0]).all() and near.sum() >= 4
    ftex = np.random.RandomState(4).rand(3, 70, 90).astype(np.float32) * 2 - 1
    dots = np.zeros((70, 90), bool)
    dots[got.cell[:, 0], got.cell[:, 1]] = True
    fp = m.paint_peaks(ftex, got, radius=0)
    assert same(fp[:, ~dots], ftex[:, ~dots]) and (fp[:, dots] != ftex[:, dots]).any()
    # watchtowers on the peaks, roads from the passes: the planes fit
    seen = m.heightmap_viewshed(h, got.observers(eye_height=2.0))
    assert seen.count.shape == (70, 90) and (seen.count[got.cell[:, 0], got.cell[:, 1]] >= 1).all()
    roads = m.heightmap_routes(h, got.passes())
    assert roads.cost.shape == (70, 90) and all(roads.cost[r, c] == 0 for r, c in got.passes())
    after = model_params(m)
    for k in before:
        for x, y in zip(before[k], after[k]):
            assert np.array_equal(x, y), k


# ---- 3. the world -----------------------------------------------------------------------------------------------------------------------
def test_the_worlds_peaks_are_the_rectangles_in_world_coordinates(small_model, dev, ops):
    from tests.gpu_common import ERO
    m = small_model
    rule = PK.Prominence(0.25, None, 24.0)
    with m.terrain_world(42, chunk_cells=2, erosion=ERO) as world:
        a = world.peaks(-20, 10, 70, 90, rule)
        assert a.origin == (-20, 10) and a.shape == (70, 90) and len(a) >= 1
        hm = world._unit_height(-20, 10, 70, 90)
        assert same_peaks(a, PK.peaks(ops, hm, rule, origin=(-20, 10)))
        _, want = reference(hm, rule, (-20, 10))
        assert same_peaks(a, want)
        assert (a.cell[:, 0] >= -20).all() and (a.cell[:, 0] < 50).all() and (a.cell[:, 1] >= 10).all() and (a.cell[:, 1] < 100).all()
        z = R.quantise(hm, 24.0)
        assert same(a.height, z[a.cell[:, 0] + 20, a.cell[:, 1] - 10] / 256.0)


# ---- 4. the command line ---------------------------------------------------------------------------------------------------------------
def test_command_line_writes_the_peaks(ops, tmp_path, capsys):
    import json
    h = R.heights(70, 90, 43, 5)
    np.save(str(tmp_path / "h.npy"), h)
    tex = np.random.RandomState(3).randint(0, 256, h.shape + (3,)).astype(np.uint8)
    from gan_heightmaps_amd.util import read_image, save_png
    save_png(str(tmp_path / "t.png"), tex)
    args = [str(tmp_path / "h.npy"), str(tmp_path / "o.geojson"), "--min-prominence", "0.1", "--height-scale", "20", "--plain",
            "--texture", str(tmp_path / "t.png"), "--painted", str(tmp_path / "p.png"), "--colour", "1,0,0", "--radius", "0"]
    assert PK.main(args) == 0
    want = PK.peaks(ops, h, PK.Prominence(0.1, None, 20.0))
    assert capsys.readouterr().out.startswith("%d peaks of %d summits, %d rounds" % (len(want), want.summits, want.rounds))
    g = json.load(open(str(tmp_path / "o.geojson")))
    assert g["features"] == want.features() and len(want) > 5
    dots = np.zeros(h.shape, bool)
    dots[want.cell[:, 0], want.cell[:, 1]] = True
    painted = read_image(str(tmp_path / "p.png"))
    assert same(painted[~dots], tex[~dots]) and (painted[dots] == [255, 0, 0]).all()
    assert PK.main(args[:1] + [str(tmp_path / "o.npz")] + args[2:6] + ["--top", "3", "--list"]) == 0
    z = np.load(str(tmp_path / "o.npz"))
    assert same(z["cell"], want.cell[:3]) and same(z["prominence"], want.prominence[:3]) and same(z["parent"], want.parent[:3])


# ---- 5. refusals of the raw entry points ----------------------------------------------------------------------------------------------
def test_refusals_of_the_entry_points(dev, ops):
    from gan_heightmaps_amd._lib import GhmError
    want = R.expected("ruler")
    zq = want["zq"]
    H, W = zq.shape
    n = H * W
    d_z, d_dir, d_a, d_b, d_m = (dev.alloc(4 * n + 256) for _ in range(5))
    d_hw, d_w = dev.alloc(ops.hydrology_workspace(H, W)), dev.alloc(ops.peaks_workspace(H, W))
    outs = [np.full(1024, CANARY, np.uint8) for _ in range(3)]
    d_o = [dev.alloc(o.nbytes) for o in outs]
    d_l = None
    try:
        dev.h2d(d_z, zq)
        for p, o in zip(d_o, outs):
            dev.h2d(p, o)
        assert ops.peaks_workspace(0, 5) == -1 and ops.peaks_workspace(1 << 16, 1 << 15) == -1 and ops.peaks_workspace(1, 9) > 0
        assert ops.peaks_list_bytes(-1) == -1 and ops.peaks_list_bytes(1 << 31) == -1 and ops.peaks_list_bytes(0) > 0

        def do_ascent(z=d_z, pz=W, Hh=H, Ww=W, a=d_dir, pa=W):
            ops.peaks_ascent(z, pz, Hh, Ww, a, pa)

        plane = ((dict(z=None), "null"), (dict(pz=W - 1), "pitch"), (dict(Hh=0), "out of range"), (dict(Hh=4 * 65535 + 1, Ww=1), "out of range"),
                 (dict(Hh=1 << 16, Ww=1 << 15, pz=1 << 15), "out of range"), (dict(Hh=1 << 15, pz=1 << 16), "pitch"))
        for kw, match in plane + ((dict(a=None), "null"), (dict(pa=W - 1), "pitch")):
            with pytest.raises(GhmError, match=match):
                do_ascent(**kw)
        do_ascent()
        ops.hydrology_accumulate(d_dir, W, H, W, d_a, W, d_b, W, d_hw)

        def do_count(z=d_z, pz=W, b=d_b, pl=W, Hh=H, Ww=W, w=d_w):
            return ops.peaks_count(z, pz, b, pl, Hh, Ww, w)

        for kw, match in plane + ((dict(b=None), "null"), (dict(w=None), "null"), (dict(pl=W - 1), "pitch")):
            with pytest.raises(GhmError, match=match):
                do_count(**kw)

        def do_tree(z=d_z, b=d_b, form=0, mk=d_m, pm=W, w=d_w, lst=None, s=64, e=None, cap=32):
            return ops.peaks_tree(z, W, b, W, H, W, form, mk, pm, w, lst, s, E if e is None else e, cap)

        # labels that lead to cells that are not their own label are no ascent's
        dev.h2d(d_m, ((np.arange(n, dtype=np.int32) + 1) % n).reshape(H, W))
        with pytest.raises(GhmError, match="no summit"):
            do_count(b=d_m)
        E = 0
        dev.h2d(d_w, np.full(ops.peaks_workspace(H, W), CANARY, np.uint8))
        with pytest.raises(GhmError, match="counted"):                    # a workspace nothing has counted in
            do_tree()
        P, E = do_count()
        assert (P, E) == (64, len(R.edges(zq, want["label"])))
        d_l = dev.alloc(ops.peaks_list_bytes(E))
        for kw, match in ((dict(z=None), "null"), (dict(b=None), "null"), (dict(mk=None), "null"), (dict(w=None), "null"),
                          (dict(pm=W - 1), "pitch"), (dict(form=2), "form"), (dict(form=-1), "form"), (dict(form=1), "list buffer"),
                          (dict(s=63), "counted"), (dict(e=E + 1), "edges"), (dict(cap=0), "max_rounds"), (dict(cap=33), "max_rounds"),
                          (dict(cap=5), "after 5 rounds"), (dict(form=1, lst=d_l, cap=5), "after 5 rounds")):
            with pytest.raises(GhmError, match=match):
                do_tree(**kw)

        def do_extract(b=d_b, a=d_a, mk=d_m, w=d_w, s=64, o=tuple(d_o)):
            ops.peaks_extract(b, W, a, W, mk, W, H, W, w, s, *o)

        with pytest.raises(GhmError, match="no tree"):                    # the refused trees left none
            do_extract()
        assert do_tree(cap=6) == 6
        for kw, match in ((dict(b=None), "null"), (dict(a=None), "null"), (dict(mk=None), "null"), (dict(w=None), "null"),
                          (dict(o=(None,) + tuple(d_o[1:])), "null"), (dict(o=tuple(d_o[:2]) + (None,)), "null"), (dict(s=65), "counted")):
            with pytest.raises(GhmError, match=match):
                do_extract(**kw)
        dev.sync()
        for p, o in zip(d_o, outs):
            dev.d2h(o, p, o.nbytes)
            assert (o == CANARY).all()
        do_extract()
        dev.sync()
        dev.d2h(outs[0], d_o[0], outs[0].nbytes)
        assert same(outs[0][:256].view(np.int32), want["summit"]) and (outs[0][256:] == CANARY).all()
        # a second tree needs a second count: the offsets of the edges are gone
        with pytest.raises(GhmError, match="edges"):
            do_tree(form=1, lst=d_l)
        # the merge refuses rows that are no tree of the summits
        z = zq.ravel()
        s, t = want["summit"], want["tree"]
        args = (s, z[s], t, z[t[:, 0]], int(z.min()))
        assert same(ops.peaks_merge(*args)[2], want["prominence_q"])
        bad = t.copy()
        bad[3, 2] = 1                                                       # cell 1 is no summit
        for rows, match in ((t[:-1], "summits - 1"), (bad, "no summit"), (np.concatenate([t[:1], t[:-1]]), "spanning tree")):
            with pytest.raises(GhmError, match=match):
                ops.peaks_merge(s, z[s], rows, z[rows[:, 0]], int(z.min()))
        with pytest.raises(GhmError, match="ascend"):
            ops.peaks_merge(s[::-1], z[s[::-1]], t, z[t[:, 0]], int(z.min()))
    finally:
        dev.sync()
        for b in [d_z, d_dir, d_a, d_b, d_m, d_hw, d_w] + d_o + ([d_l] if d_l is not None else []):
            dev.free(b)
