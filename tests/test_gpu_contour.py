"""The contours on the MI355X (csrc/contour.hip, gan_heightmaps_amd/contour.py): the count, the trace, the extraction
and the marks through the raw entry points against the restatement of tests/contour_ref.py, bit for bit on all five arrays -- the
definition is integer but for one correctly rounded division, so there are no tolerances.  The quantised heights go in with a
pitch of W + 3 whose padding is 2^30 high; the five arrays, which are dense, are followed by canary bytes; the marks lie in a
canary canvas with a pitch of W + 2.  Then ``contours``, the paint, the model's and the world's methods, the command line, and the
refusals of the raw entry points."""
import numpy as np
import pytest

from oracle import step as ostep
from gan_heightmaps_amd import contour as CT
from tests import contour_ref as R
from tests.gpu_common import build_model, CANARY, Canvas, dev, model_params, ops, padded, same, SMALL      # noqa: F401  (dev, ops: the module-scoped fixtures)

pytestmark = pytest.mark.gpu

TAIL = 64                    # canary bytes behind every dense array
ARRAYS = (("edge", np.int32, 3), ("t", np.float64, 1), ("offsets", np.int64, 1), ("level", np.int32, 1), ("closed", np.uint8, 1))


def ranking_rounds(longest):
    """the rounds of pointer doubling over a longest line of this many segments, the one that changes nothing included"""
    return 0 if longest == 0 else max(longest - 2, 0).bit_length() + 1


def raw_trace(dev, ops, zq, base_q, interval_q, count, index_every):
    """-> (dict of the five arrays, segments and rounds, marks) through the raw entry points"""
    H, W = zq.shape
    cnt = -1 if count is None else count
    bufs = []
    try:
        d_z, pz = padded(dev, zq, np.int32, 3, 1 << 30)
        bufs.append(d_z)
        d_c = dev.alloc(ops.contour_cells_bytes(H, W))
        bufs.append(d_c)
        S = ops.contour_count(d_z, pz, H, W, base_q, interval_q, cnt, d_c)
        d_w = dev.alloc(ops.contour_workspace(H, W, S))
        bufs.append(d_w)
        L, V, rounds = ops.contour_trace(d_z, pz, H, W, base_q, interval_q, cnt, d_c, d_w, S)
        host, ptrs = [], []
        for name, dtype, width in ARRAYS:
            n = (V if name in ("edge", "t") else L + 1 if name == "offsets" else L) * width * np.dtype(dtype).itemsize
            whole = np.full(n + TAIL, CANARY, np.uint8)
            p = dev.alloc(whole.nbytes)
            bufs.append(p)
            dev.h2d(p, whole)
            host.append((name, dtype, width, n, whole))
            ptrs.append(p)
        ops.contour_extract(d_z, pz, H, W, base_q, interval_q, cnt, d_c, d_w, S, L, V, *ptrs)
        marks = Canvas(dev, H, W, np.uint32)
        bufs.append(marks.base)
        ops.contour_marks(d_z, pz, H, W, base_q, interval_q, cnt, index_every, marks.ptr, marks.pitch)
        dev.sync()
        got = dict(segments=S, rounds=rounds)
        for (name, dtype, width, n, whole), p in zip(host, ptrs):
            dev.d2h(whole, p, whole.nbytes)
            assert (whole[n:] == CANARY).all(), "bytes behind %s were written" % name
            a = whole[:n].view(dtype).copy()
            got[name] = a.reshape(-1, 3) if width == 3 else a
        return got, marks.read()
    finally:
        dev.sync()
        for b in bufs:
            dev.free(b)


def same_lines(got, want):
    for name, dtype, _ in ARRAYS:
        if name == "t":
            assert np.array_equal(got["t"].view(np.int64), want["t"].view(np.int64)), "t"
        else:
            assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), name
    return True


# ---- 1. the raw entry points, case by case ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_the_five_arrays_and_the_marks_equal_the_restatement(dev, ops, name):
    c = R.case(name)
    want, want_marks = R.expected(name)
    # the case contains what it is for
    if name == "serpentine":
        assert want["segments"] == 4604 and want["closed"].tolist() == [1] and ranking_rounds(4604) >= 13
    if name == "serpentine_open":
        assert want["segments"] == 4606 and want["closed"].tolist() == [0] and np.diff(want["offsets"]).tolist() == [4607]
    if name == "noise37":
        assert (len(want["level"]), int(want["closed"].sum())) == (276, 55)
    if name == "noise96_512":
        assert (len(want["level"]), int(want["closed"].sum())) == (677, 393)
    if name in ("row", "column"):
        assert want["segments"] == 0 and want["offsets"].tolist() == [0]
    if name == "steep":
        assert want["segments"] == 64
    if name == "peak":
        assert want["closed"].tolist() == [1, 1, 1, 1]
    if name == "tie":
        assert np.diff(want["offsets"]).tolist() == [2, 2] and not want["closed"].any()
    if name == "clipped":
        assert set(want["level"].tolist()) == set(range(6))
    got, got_marks = raw_trace(dev, ops, c["zq"], c["base_q"], c["interval_q"], c["count"], c["index_every"])
    assert got["segments"] == want["segments"], name
    assert same_lines(got, want), name
    assert got["rounds"] == ranking_rounds(want["longest"]), name
    assert same(got_marks, want_marks), name


# ---- 2. contours, the paint, the model's methods ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_model(dev):
    m = build_model(ostep.default_cfg(**SMALL), 5, dev, dtype="f32", use_graph=False)
    cfg = ostep.default_cfg(**SMALL)
    for s in range(3):                       # non-trivial BatchNorm running statistics (the deterministic pass reads them)
        m.z_fn(ostep.synthetic_batch(4, cfg, seed=40 + s)[0])
    return m


def test_contours_equals_the_restatement(dev, ops):
    h = R.heights(70, 90, 43)
    levels = CT.Levels(interval=1.5, base=-0.75, count=None, index_every=3, height_scale=20.0)
    zq = R.quantise(h, 20.0)
    want = R.trace(zq, -192, 384)
    got = CT.contours(ops, h[None], levels, origin=(100, -20), keep='zq')
    assert same(got.zq, zq) and same_lines(dict((k, getattr(got, k)) for k, _, _ in ARRAYS), want)
    assert got.shape == (70, 90) and got.origin == (100, -20) and got.rounds == ranking_rounds(want["longest"]) and len(got) > 20
    along = want["edge"][:, 2] == 1
    assert same(got.points[:, 0], (100 + want["edge"][:, 0]) + np.where(along, want["t"], 0.0))
    assert same(got.points[:, 1], (-20 + want["edge"][:, 1]) + np.where(along, 0.0, want["t"]))
    assert len(got.segments()) == want["segments"] and got.height(0) == levels.height(want["level"][0])
    with pytest.raises(ValueError, match="%d contour segments" % want["segments"]):
        CT.contours(ops, h, levels, max_segments=want["segments"] - 1)
    assert len(CT.contours(ops, h, levels, max_segments=want["segments"])) == len(got)
    u8 = (h * 255).astype(np.uint8)
    coast = CT.contours(ops, u8, CT.Levels(base=32.0, count=1))
    want = R.trace(R.quantise(u8.astype(np.float32) / np.float32(255), 64.0), 32 * 256, 1024, 1)
    assert same_lines(dict((k, getattr(coast, k)) for k, _, _ in ARRAYS), want) and set(coast.level.tolist()) == {0}
    for flat in (h[:1], h[:, :1]):                                        # no cells: no lines, and not an error
        none = CT.contours(ops, flat)
        assert len(none) == 0 and none.offsets.tolist() == [0] and none.edge.shape == (0, 3)
    assert same(CT.marks(ops, h, levels), R.marks(zq, -192, 384, None, 3))


def test_the_models_methods_and_the_paint(small_model, dev, ops):
    m = small_model
    before = model_params(m)
    h = R.heights(70, 90, 43)
    levels = CT.Levels(interval=2.0, index_every=4, height_scale=20.0)
    want = CT.contours(ops, h, levels)
    got = m.heightmap_contours(h, levels, keep='zq')
    assert same_lines(dict((k, getattr(got, k)) for k, _, _ in ARRAYS), dict((k, getattr(want, k)) for k, _, _ in ARRAYS))
    mk = R.marks(got.zq, 0, 512, None, 4)
    line, index = mk >= 1, mk == 2
    assert 200 < line.sum() < line.size - 200 and 20 < index.sum() < line.sum()
    tex = np.random.RandomState(3).randint(0, 256, (70, 90, 3)).astype(np.uint8)
    painted = m.paint_contours(tex, h, levels, (0.0, 1.0, 0.0), opacity=1.0, index_opacity=1.0)
    assert painted.dtype == np.uint8 and same(painted[~line], tex[~line])                  # unpainted pixels keep their bits
    assert (painted[line] == [0, 255, 0]).all()
    soft = m.paint_contours(tex, h, levels)
    assert same(soft[~line], tex[~line]) and (soft[line] != tex[line]).any()
    assert same(soft, CT.paint(ops, tex, got, value_range=m.is_b_grayscale))               # from the Contours' kept heights
    only = m.paint_contours(tex, h, levels, (1.0, 0.0, 0.0), opacity=0.0, index_opacity=1.0)
    assert same(only[~line], tex[~line]) and (only[index] == [255, 0, 0]).all()            # the second pass is the index contours'
    ftex = np.random.RandomState(4).rand(3, 70, 90).astype(np.float32) * 2 - 1
    fp = m.paint_contours(ftex, h, levels)
    assert same(fp[:, ~line], ftex[:, ~line]) and (fp[:, line] != ftex[:, line]).any()
    after = model_params(m)
    for k in before:
        for x, y in zip(before[k], after[k]):
            assert np.array_equal(x, y), k


# ---- 3. the world: two rectangles agree on the cells both contain -------------------------------------------------------------------
@pytest.mark.parametrize("eroded", (False, True))
def test_two_rectangles_of_the_world_agree_bit_for_bit_on_their_common_cells(small_model, dev, ops, eroded):
    from tests.gpu_common import ERO
    m = small_model
    kw = dict(erosion=ERO) if eroded else {}
    levels = CT.Levels(interval=1.0, index_every=4, height_scale=24.0)
    with m.terrain_world(42, chunk_cells=2, **kw) as world:
        a = world.contours(-20, 10, 70, 90, levels)
        b = world.contours(-5, 30, 60, 100, levels)
        assert a.origin == (-20, 10) and b.origin == (-5, 30) and a.shape == (70, 90) and b.shape == (60, 100)
        common = (-5, 30, 55, 70)                                          # rows -5 .. 49, columns 30 .. 99
        sa, sb = a.segments(within=common), b.segments(within=common)
        assert len(sa) > 100 and sa.tobytes() == sb.tobytes()              # and there is something to agree on
        assert len(sa) < len(a.segments()) and len(sb) < len(b.segments())
        hm = world._unit_height(-20, 10, 70, 90)
        ref = CT.contours(ops, hm, levels, origin=(-20, 10))
        assert a.segments().tobytes() == ref.segments().tobytes() and same(a.offsets, ref.offsets) and same(a.closed, ref.closed)
        want = R.trace(R.quantise(hm, 24.0), 0, 256)
        assert same_lines(dict((k, getattr(a, k)) for k, _, _ in ARRAYS), want)


# ---- 4. the command line --------------------------------------------------------------------------------------------------------------
def test_command_line_writes_the_lines(ops, tmp_path, capsys):
    import json
    h = R.heights(70, 90, 43)
    np.save(str(tmp_path / "h.npy"), h)
    tex = np.random.RandomState(3).randint(0, 256, h.shape + (3,)).astype(np.uint8)
    from gan_heightmaps_amd.util import read_image, save_png
    save_png(str(tmp_path / "t.png"), tex)
    args = [str(tmp_path / "h.npy"), str(tmp_path / "o.geojson"), "--interval", "2", "--base", "-1", "--index-every", "4", "--height-scale",
            "20", "--texture", str(tmp_path / "t.png"), "--painted", str(tmp_path / "p.png"), "--opacity", "1", "--colour", "1,0,0"]
    assert CT.main(args) == 0
    levels = CT.Levels(2.0, -1.0, None, 4, 20.0)
    want = CT.contours(ops, h, levels, keep='zq')
    assert capsys.readouterr().out.startswith("%d lines (%d closed), %d vertices" % (len(want), want.closed.sum(), len(want.t)))
    g = json.load(open(str(tmp_path / "o.geojson")))
    assert len(g["features"]) == len(want) > 10
    for i in (0, len(want) - 1):
        assert g["features"][i]["geometry"]["coordinates"][0] == [want.line(i)[0][1], want.line(i)[0][0]]
        assert g["features"][i]["properties"]["height"] == want.height(i)
    line = R.marks(want.zq, -256, 512, None, 4) >= 1
    painted = read_image(str(tmp_path / "p.png"))
    assert same(painted[~line], tex[~line]) and (painted[line] == [255, 0, 0]).all()
    assert CT.main(args[:1] + [str(tmp_path / "o.npz")] + args[2:10]) == 0
    z = np.load(str(tmp_path / "o.npz"))
    assert same(z["edge"], want.edge) and same(z["t"], want.t) and same(z["offsets"], want.offsets)


# ---- 5. refusals of the raw entry points ------------------------------------------------------------------------------------------
def test_refusals_of_the_entry_points_leave_every_byte_alone(dev, ops):
    from gan_heightmaps_amd._lib import GhmError
    H, W = 4, 8
    zq = np.zeros((H, W), np.int32)
    zq[1:3, 2:6] = 1000
    src = dev.alloc(4096)
    dev.h2d(src, zq)
    cells = np.full(ops.contour_cells_bytes(H, W) + TAIL, CANARY, np.uint8)
    d_c = dev.alloc(cells.nbytes)
    dev.h2d(d_c, cells)
    marks = Canvas(dev, H, W, np.uint32)
    outs = [np.full(256, CANARY, np.uint8) for _ in range(5)]
    d_o = [dev.alloc(o.nbytes) for o in outs]
    for p, o in zip(d_o, outs):
        dev.h2d(p, o)
    d_w = None

    def do_count(z=src, pz=W, Hh=H, Ww=W, b=0, iq=256, cnt=-1, c=d_c):
        return ops.contour_count(z, pz, Hh, Ww, b, iq, cnt, c)

    def do_marks(z=src, pz=W, Hh=H, Ww=W, b=0, iq=256, cnt=-1, ie=5, mk=marks.ptr, pm=marks.pitch):
        ops.contour_marks(z, pz, Hh, Ww, b, iq, cnt, ie, mk, pm)

    try:
        plane = ((dict(z=None), "null"), (dict(pz=W - 1), "pitch"), (dict(Hh=0), "out of range"), (dict(Hh=4 * 65535 + 1, Ww=1), "out of range"),
                 (dict(Hh=1 << 16, Ww=1 << 15, pz=1 << 15), "out of range"), (dict(Hh=1 << 15, pz=1 << 16), "pitch"),
                 (dict(iq=0), "interval_q"), (dict(iq=-5), "interval_q"), (dict(cnt=0), "count"), (dict(cnt=-2), "count"),
                 (dict(b=(1 << 30) + 1), "base_q"))
        for kw, match in plane + ((dict(c=None), "null"),):
            with pytest.raises(GhmError, match=match):
                do_count(**kw)
        for kw, match in plane + ((dict(mk=None), "null"), (dict(pm=W - 1), "pitch"), (dict(ie=0), "index_every")):
            with pytest.raises(GhmError, match=match):
                do_marks(**kw)
        dev.sync()
        dev.d2h(cells, d_c, cells.nbytes)
        assert (cells == CANARY).all() and (marks.read().view(np.uint8) == CANARY).all()
        assert ops.contour_cells_bytes(0, 5) == -1 and ops.contour_cells_bytes(1 << 16, 1 << 15) == -1 and ops.contour_cells_bytes(1, 9) > 0
        assert ops.contour_workspace(H, W, -1) == -1 and ops.contour_workspace(H, W, 1 << 31) == -1 and ops.contour_workspace(0, W, 4) == -1
        assert ops.contour_workspace(H, W, 0) > 0
        # a counted plane: the trace and the extraction refuse totals that are not the cells' or the workspace's
        S = do_count()
        assert S == R.trace(zq, 0, 256)["segments"] == 4 * 12
        ws = np.full(ops.contour_workspace(H, W, S) + TAIL, CANARY, np.uint8)
        d_w = dev.alloc(ws.nbytes)
        dev.h2d(d_w, ws)

        def do_trace(z=src, pz=W, iq=256, c=d_c, w=d_w, s=S):
            return ops.contour_trace(z, pz, H, W, 0, iq, -1, c, w, s)

        for kw, match in ((dict(z=None), "null"), (dict(c=None), "null"), (dict(w=None), "null"), (dict(pz=W - 1), "pitch"),
                          (dict(iq=0), "interval_q"), (dict(s=S + 1), "segments"), (dict(s=S - 1), "segments"), (dict(s=-1), "segments"),
                          (dict(s=1 << 31), "segments")):
            with pytest.raises(GhmError, match=match):
                do_trace(**kw)
        dev.sync()
        dev.d2h(ws, d_w, ws.nbytes)
        assert (ws == CANARY).all()

        def do_extract(z=src, c=d_c, w=d_w, s=S, l=4, v=4 * 12, o=tuple(d_o)):
            ops.contour_extract(z, W, H, W, 0, 256, -1, c, w, s, l, v, *o)

        with pytest.raises(GhmError, match="traced"):                     # a workspace nothing has traced in
            do_extract()
        L, V, rounds = do_trace()
        assert (L, V) == (4, 4 * 12) and rounds == ranking_rounds(12)          # four loops round the block, twelve cells each
        for kw, match in ((dict(z=None), "null"), (dict(c=None), "null"), (dict(w=None), "null"), (dict(o=(None,) + tuple(d_o[1:])), "null"),
                          (dict(o=tuple(d_o[:2]) + (None,) + tuple(d_o[3:])), "null"), (dict(s=S - 1), "traced"), (dict(l=3), "traced"),
                          (dict(l=5), "traced"), (dict(v=4 * 12 + 1), "traced"), (dict(v=0), "traced")):
            with pytest.raises(GhmError, match=match):
                do_extract(**kw)
        dev.sync()
        for p, o in zip(d_o, outs):
            dev.d2h(o, p, o.nbytes)
            assert (o == CANARY).all()
        do_extract()
        dev.sync()
        dev.d2h(outs[2], d_o[2], outs[2].nbytes)
        assert outs[2][:40].view(np.int64).tolist() == [0, 12, 24, 36, 48] and (outs[2][40:] == CANARY).all()
        dev.d2h(ws, d_w, ws.nbytes)
        assert (ws[-TAIL:] == CANARY).all()
        dev.d2h(cells, d_c, cells.nbytes)
        assert (cells[-TAIL:] == CANARY).all()
    finally:
        dev.sync()
        for b in [src, d_c, marks.base] + d_o + ([d_w] if d_w is not None else []):
            dev.free(b)
