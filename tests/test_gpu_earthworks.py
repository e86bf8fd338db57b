"""Earthworks on the MI355X (csrc/earthworks.hip, gan_heightmaps_amd/earthworks.py): both forms of the nearest mark
and the shaping through the raw entry points against the restatement of tests/earthworks_ref.py and against each other, bit for
bit -- the transform is integer and the shaping's operations are rounded one by one, so there are no tolerances.  Every output
lies in a canary canvas with a pitch of W + 2; every input has a pitch of W + 3 whose padding is marked (0xFFFFFFFF) or NaN.  Then
``nearest``, ``carve``, ``cut_rivers`` and ``grade_roads``, the model's and the world's methods, the command line, and the
refusals of the raw entry points."""
import numpy as np
import pytest

from oracle import step as ostep
from gan_heightmaps_amd import earthworks as EW
from gan_heightmaps_amd import hydrology as HY
from gan_heightmaps_amd import route as RT
from tests import earthworks_ref as E
from tests import hydrology_ref as HR
from tests import route_ref as RR
from tests.gpu_common import build_model, CANARY, Canvas, dev, model_params, ops, padded, same, SMALL      # noqa: F401  (dev, ops: the module-scoped fixtures)

pytestmark = pytest.mark.gpu


def raw_nearest(dev, ops, marks, threshold, R, tiled):
    """-> (nearest, dist2) through the raw entry point; the canvases check their canaries when they are read"""
    H, W = marks.shape
    bufs = []
    try:
        d_m, pm = padded(dev, marks, np.uint32, 3, 0xFFFFFFFF)
        bufs.append(d_m)
        near, dist2 = Canvas(dev, H, W, np.int32), Canvas(dev, H, W, np.int32)
        bufs += [near.base, dist2.base]
        ops.earthworks_nearest(d_m, pm, H, W, threshold, R, tiled, near.ptr, near.pitch, dist2.ptr, dist2.pitch)
        dev.sync()
        return near.read(), dist2.read()
    finally:
        dev.sync()
        for b in bufs:
            dev.free(b)


def raw_shape(dev, ops, h, near, dist2, target, table, R, mode):
    H, W = h.shape
    bufs = []
    try:
        for plane, dtype, fill in ((h, np.float32, np.nan), (near, np.int32, 0), (dist2, np.int32, 0), (target, np.float32, np.nan)):
            bufs.append(padded(dev, plane, dtype, 3, fill))
        (d_h, ph), (d_n, pn), (d_d, pd), (d_t, pt) = bufs
        table = np.ascontiguousarray(table, np.float32)
        d_tab = dev.alloc(table.nbytes)
        dev.h2d(d_tab, table)
        out = Canvas(dev, H, W, np.float32)
        bufs += [(d_tab, 0), (out.base, 0)]
        ops.earthworks_shape(d_h, ph, d_n, pn, d_d, pd, d_t, pt, d_tab, R, mode, H, W, out.ptr, out.pitch)
        dev.sync()
        return out.read()
    finally:
        dev.sync()
        for b, _ in bufs:
            dev.free(b)


# ---- 1. the nearest mark, both forms ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", E.KINDS)
def test_both_forms_of_the_nearest_mark_equal_the_restatement(dev, ops, kind):
    seen = dict(ties=0, unfound=0, found=0, rim=0, below=0)
    for shape, R in E.nearest_cases():
        m, thr, near, dist2 = E.nearest_case(kind, shape, R)
        plain = raw_nearest(dev, ops, m, thr, R, False)
        tiled = raw_nearest(dev, ops, m, thr, R, True)
        for got, form in ((plain, "plain"), (tiled, "tiled")):
            assert same(got[0], near) and same(got[1], dist2), (kind, shape, R, form)
        assert same(plain[0], tiled[0]) and same(plain[1], tiled[1])
        seen['ties'] += E.ties(m, R, thr, dist2)
        seen['unfound'] += int((near == E.NONE).sum())
        seen['found'] += int((near != E.NONE).sum())
        seen['rim'] += int(((dist2 == R * R) & (R > 0)).sum())
        seen['below'] += int(((m > 0) & (m < thr)).sum())
    # the case contains what it is for
    if kind == 'none':
        assert seen['found'] == 0
    if kind == 'all':
        assert seen['unfound'] == 0 and seen['ties'] == 0
    if kind == 'corners':
        assert seen['unfound'] > 0 and seen['found'] > 0 and seen['rim'] > 0          # a hit at d2 = R^2
    if kind in ('checker', 'pairs'):
        assert seen['ties'] > 0 and seen['rim'] > 0
    if kind == 'scatter':
        assert seen['unfound'] > 0 and seen['found'] > 0 and seen['ties'] > 0 and seen['rim'] > 0
    if kind == 'values':
        assert seen['below'] > 0 and seen['found'] > 0


def test_the_window_larger_than_the_plane_and_the_marks_at_the_tile_corner(dev, ops):
    shape, R = E.BIG
    m, thr, near, dist2 = E.nearest_case('corners', shape, R)
    assert m[31, 31] and m[32, 32] and 2 * R + 1 > shape[0]
    for tiled in (False, True):
        n, d = raw_nearest(dev, ops, m, thr, R, tiled)
        assert same(n, near) and same(d, dist2)
        assert (n == E.NONE).sum() == 0 and d.max() == 31 * 31 + 1
    one = np.zeros(shape, np.uint32)                              # a mark at exactly R is found, one at (R, 1) is not
    one[0, 0] = one[0, 64] = 9
    near, dist2 = E.nearest(one, R, 9)
    assert near[0, 32] == 0 and dist2[0, 32] == R * R and near[1, 32] == E.NONE and E.ties(one, R, 9, dist2) == 1
    for tiled in (False, True):
        n, d = raw_nearest(dev, ops, one, 9, R, tiled)
        assert same(n, near) and same(d, dist2)
    assert ops.earthworks_lds_bytes(32) == 96 * 96 + 32 * 96 == 12288 and ops.earthworks_lds_bytes(0) == 1024 + 1024
    assert ops.earthworks_lds_bytes(5) == (42 * 42 + 15) // 16 * 16 + 32 * 42
    assert ops.earthworks_lds_bytes(-1) == -1 and ops.earthworks_lds_bytes(33) == -1


# ---- 2. the shaping ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", range(3))
def test_the_shaping_equals_the_restatement(dev, ops, mode):
    touched = cored = 0
    for shape, (core, reach) in (((1, 1), (0.0, 0.0)), ((1, 40), (1.0, 5.5)), ((40, 1), (0.0, 1.0)), ((31, 33), (2.0, 2.0)),
                                 ((33, 65), (0.0, 32.0)), ((64, 64), (0.0, 0.0)), ((70, 45), (1.0, 6.0))):
        R = int(reach)
        h, m, thr, target = E.shape_case(shape, R, 7 + mode)
        tab = E.table(core, reach)
        near, dist2 = E.nearest(m, R, thr)
        want = E.shape(h, near, dist2, target, tab, mode)
        got = raw_shape(dev, ops, h, near, dist2, target, tab, R, mode)
        assert same(got, want), (shape, core, reach, mode)
        on = m.astype(np.int64) >= thr
        assert shape == (1, 1) or (np.isnan(target[~on]).all() and (~on).any())            # NaN off the marks
        assert (h < 0).any() or shape == (1, 1)
        assert shape == (1, 1) or ((h != 0) & (np.abs(h) < np.float32(1e-38))).any()       # denormals
        same_bits = got.view(np.int32) == h.view(np.int32)
        untouched = (near == E.NONE) | (tab[np.maximum(dist2, 0), 1] == 0)
        assert same_bits[untouched].all()                                                  # untouched cells keep their bits
        if mode == 0:
            assert same(got[on], target[on])                                               # a core cell: its target's bits
        if mode == 1:
            assert (got <= h).all()
        if mode == 2:
            assert (got >= h).all()
        touched += int((~same_bits).sum())
        cored += int(on.sum())
    assert touched > 100 and cored > 30


# ---- 3. nearest and carve -----------------------------------------------------------------------------------------------------
def test_nearest_and_carve_in_every_form_and_with_every_keep(dev, ops):
    shape = (70, 45)
    h, m, thr, target = E.shape_case(shape, 6, 21)
    for R in (0, 5, 32):
        want = E.nearest(m, R, thr)
        for t in (None, False, True):
            got = EW.nearest(ops, m, R, threshold=thr, tiled=t)
            assert same(got[0], want[0]) and same(got[1], want[1]), (R, t)
    for mode in E.MODES:
        want, near, dist2 = E.carve(h, m, target, 1.0, 6.5, mode, thr)
        for t in (None, False, True):
            e = EW.carve(ops, h, m, target, EW.Profile(1.0, 6.5, mode), threshold=thr, tiled=t, keep=EW.KEEP, origin=(3, -4))
            assert same(e.height, want) and same(e.nearest, near) and same(e.dist2, dist2), (mode, t)
            assert e.tiled is (EW.DEFAULT_TILED if t is None else t) and e.shape == shape and e.origin == (3, -4)
            d = want.astype(np.float64) - h.astype(np.float64)
            assert e.cut == -d[d < 0].sum() and e.fill == d[d > 0].sum()
            assert (e.cut > 0 or mode == 'fill') and (e.fill > 0 or mode == 'cut')
            assert (e.fill == 0) == (mode == 'cut') and (e.cut == 0) == (mode == 'fill')
    for keep in EW.KEEP:
        e = EW.carve(ops, h[None], m, target.astype(np.float64), EW.Profile(1.0, 6.5), threshold=thr, keep=keep)
        assert same(getattr(e, keep), dict(height=E.carve(h, m, target, 1.0, 6.5, 'both', thr)[0], nearest=near, dist2=dist2)[keep])
        assert all(getattr(e, k) is None for k in EW.KEEP if k != keep)
    u8 = np.random.RandomState(4).randint(0, 256, shape).astype(np.uint8)                # uint8 is read as v / 255
    e = EW.carve(ops, u8, m, target, EW.Profile(0.0, 3.0), threshold=thr)
    assert same(e.height, E.carve(u8.astype(np.float32) / np.float32(255), m, target, 0.0, 3.0, 'both', thr)[0])


# ---- 4. rivers and roads -------------------------------------------------------------------------------------------------------
def test_cut_rivers_on_a_terrain_with_lakes_and_rivers(dev, ops):
    H, W, q, seed = HR.CASES[1]
    r = HR.analyse(HR.terrain(H, W, q, seed))
    hydro = HY.Hydrology((H, W), (1, 1), 1, False, filled=r.filled, depth=r.depth, accumulation=r.accumulation)
    ch = EW.Channel(river_threshold=40, lake_min_depth=1.0 / 64, depth=0.6, growth=0.3, max_depth=1.4, core=1.0, reach=3.5)
    marks, target = E.channel_targets(r.filled, r.depth, r.accumulation, 40, 1.0 / 64, 0.6, 0.3, 1.4, 64.0)
    lakes = r.depth > np.float32(1.0 / 64)
    assert lakes.any() and marks.any() and ((r.accumulation >= 40) & lakes).any()       # lakes, rivers, and rivers through lakes
    want, near, dist2 = E.carve(r.filled, marks, target, 1.0, 3.5, 'cut')
    for t in (False, True):
        e = EW.cut_rivers(ops, hydro, ch, tiled=t, keep=EW.KEEP)
        assert same(e.height, want) and same(e.nearest, near) and same(e.dist2, dist2), t
        assert e.fill == 0 and e.cut > 0 and (e.height <= r.filled).all()
    on = marks != 0
    assert same(want[on & (target < r.filled)], target[on & (target < r.filled)])          # the bed itself
    far = near == E.NONE
    assert far.any() and same(want[far], r.filled[far])


def test_grade_roads_along_paths_and_along_the_traffic_network(dev, ops):
    h, pen, sources = RR.case(3, 5)
    r = RR.field(h, sources, penalty=pen)
    cf = RT.CostField(h.shape, sources, cost=r.cost, parent=r.parent, territory=r.territory, traffic=r.traffic)
    cells = [tuple(int(v) for v in c) for c in np.argwhere(r.cost != RR.UNREACHED)[::173]]
    paths = [RR.walk(r.parent, c) for c in cells]
    bed = EW.Roadbed(core=1.0, reach=4.0, smooth=6)
    marks, target = E.road_targets(h, r.parent, RR.raster(h.shape, paths) != 0, 6)
    want = E.carve(h, marks, target, 1.0, 4.0, 'both')[0]
    e = EW.grade_roads(ops, h, cf, paths, bed)
    assert same(e.height, want) and e.cut > 0 and e.fill > 0 and int(marks.sum()) > 30
    assert same(EW.grade_roads(ops, h, cf, paths[::-1], bed, tiled=False).height, want)      # whatever the order of the paths
    moved = RT.CostField(h.shape, sources, origin=(7, -9), parent=r.parent)
    e = EW.grade_roads(ops, h, moved, [p + [7, -9] for p in paths], bed)
    assert same(e.height, want) and e.origin == (7, -9)
    for mode in ('cut', 'fill'):
        bed = EW.Roadbed(core=0.0, reach=3.0, smooth=20, mode=mode)
        marks, target = E.road_targets(h, r.parent, r.traffic >= 25, 20)
        assert 30 < int(marks.sum()) < h.size // 2
        e = EW.grade_roads(ops, h, cf, paths, bed, traffic_threshold=25)                     # the paths are not looked at
        assert same(e.height, E.carve(h, marks, target, 0.0, 3.0, mode)[0]) and (e.cut > 0) == (mode == 'cut')


# ---- 5. the model's and the world's methods -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_model(dev):
    m = build_model(ostep.default_cfg(**SMALL), 5, dev, dtype="f32", use_graph=False)
    cfg = ostep.default_cfg(**SMALL)
    for s in range(3):                       # non-trivial BatchNorm running statistics (the deterministic pass reads them)
        m.z_fn(ostep.synthetic_batch(4, cfg, seed=40 + s)[0])
    return m


def test_model_and_world_methods_equal_the_modules_functions(small_model, dev, ops):
    m = small_model
    before = model_params(m)
    H, W, q, seed = HR.CASES[3]
    h = HR.terrain(H, W, q, seed)
    hydro = HY.analyse(ops, h)
    ch = EW.Channel(river_threshold=20, lake_min_depth=1.0 / 64)
    want = EW.cut_rivers(ops, hydro, ch)
    got = m.cut_rivers(hydro, ch, tiled=False)
    assert same(got.height, want.height) and got.cut == want.cut > 0
    sources = [(3, 4), (28, 40)]
    cf = RT.field(ops, hydro.filled, sources, hydro=hydro)
    paths = cf.paths([(16, 20), (0, 46)])
    got = m.grade_roads(want.height, cf, paths, EW.Roadbed(smooth=4), keep=EW.KEEP)
    ref = EW.grade_roads(ops, want.height, cf, paths, EW.Roadbed(smooth=4), keep=EW.KEEP)
    for k in EW.KEEP:
        assert same(getattr(got, k), getattr(ref, k)), k
    assert got.cut + got.fill > 0
    net = m.grade_roads(h[None], cf, traffic_threshold=15)
    assert same(net.height, EW.grade_roads(ops, h, cf, traffic_threshold=15).height) and not same(net.height, h)
    marks, target = EW.road_targets(h, cf.parent, cf.traffic >= 15)
    prof = EW.Profile(1.0, 6.0)
    assert same(m.carve_heightmap(h, marks, target, prof, tiled=True).height, net.height)
    with m.terrain_world(42, chunk_cells=2) as world:
        y0, x0, hh, ww = rect = (-20, 10, 50, 70)
        towns, ends = [(-15, 20), (25, 75)], [(29, 79), (0, 40)]
        ch, travel = EW.Channel(river_threshold=30), RT.Travel(river_threshold=30)
        got = world.earthworks(*rect, sources=towns, targets=ends, channel=ch, travel=travel)
        wh = world.hydrology(*rect)
        cut = EW.cut_rivers(ops, wh, ch)
        assert cut.cut > 0
        cf = RT.field(ops, wh.filled, [(r - y0, c - x0) for r, c in towns], travel, hydro=wh)
        local = cf.paths([(r - y0, c - x0) for r, c in ends])
        ref = EW.grade_roads(ops, cut.height, cf, local)
        assert same(got.height, ref.height) and not same(got.height, cut.height) and got.height.shape == (hh, ww)
        assert len(got.paths) == 2 and all(np.array_equal(p, q + [y0, x0]) for p, q in zip(got.paths, local))   # world coordinates
        assert got.cost_field.origin == (y0, x0) and same(got.cost_field.cost, cf.cost) and same(got.hydro.filled, wh.filled)
        bare = world.earthworks(*rect, rivers=False)
        assert same(bare.height, wh.filled) and bare.cost_field is None and bare.paths == []
        assert same(world.earthworks(*rect, channel=ch, tiled=False).height, cut.height)
    after = model_params(m)
    for k in before:
        for x, y in zip(before[k], after[k]):
            assert np.array_equal(x, y), k


def test_command_line_writes_the_carved_heightmap(ops, tmp_path, capsys):
    H, W, q, seed = HR.CASES[3]
    h = HR.terrain(H, W, q, seed)
    np.save(str(tmp_path / "h.npy"), h)
    assert EW.main([str(tmp_path / "h.npy"), str(tmp_path / "o.npy"), "--rivers", "--river-threshold", "20", "--from", "3,4", "--to",
                    "16,20", "--road-smooth", "4", "--plain"]) == 0
    hydro = HY.analyse(ops, h)
    cut = EW.cut_rivers(ops, hydro, EW.Channel(river_threshold=20))
    cf = RT.field(ops, hydro.filled, [(3, 4)], RT.Travel(river_threshold=20), hydro=hydro)
    want = EW.grade_roads(ops, cut.height, cf, cf.paths([(16, 20)]), EW.Roadbed(smooth=4))
    assert same(np.load(str(tmp_path / "o.npy")), want.height)
    assert capsys.readouterr().out.startswith("cut %.6g, fill %.6g" % (cut.cut + want.cut, cut.fill + want.fill))


# ---- 6. refusals of the raw entry points ------------------------------------------------------------------------------------------
def test_refusals_of_the_entry_points_leave_every_byte_alone(dev, ops):
    from gan_heightmaps_amd._lib import GhmError
    H, W = 4, 8
    src = dev.alloc(4096)
    near, dist2, out = Canvas(dev, H, W, np.int32), Canvas(dev, H, W, np.int32), Canvas(dev, H, W, np.float32)
    p = near.pitch

    def nearest(marks=src, pm=W, Hh=H, Ww=W, threshold=1, reach=2, tiled=False, n=near.ptr, pn=p, d=dist2.ptr, pd=p):
        ops.earthworks_nearest(marks, pm, Hh, Ww, threshold, reach, tiled, n, pn, d, pd)

    def shape(h=src, ph=W, n=src, pn=W, d=src, pd=W, t=src, pt=W, table=src, reach=2, mode=0, Hh=H, Ww=W, o=out.ptr, po=p):
        ops.earthworks_shape(h, ph, n, pn, d, pd, t, pt, table, reach, mode, Hh, Ww, o, po)

    try:
        for kw, match in ((dict(marks=None), "null"), (dict(n=None), "null"), (dict(d=None), "null"), (dict(pm=W - 1), "pitch"),
                          (dict(pn=W - 1), "pitch"), (dict(pd=W - 1), "pitch"), (dict(Hh=0), "out of range"),
                          (dict(Hh=1 << 16, Ww=1 << 15, pm=1 << 15, pn=1 << 15, pd=1 << 15), "out of range"),
                          (dict(Hh=4 * 65535 + 1, Ww=1, pm=1, pn=1, pd=1), "out of range"), (dict(Hh=1 << 15, pm=1 << 16), "pitch"),
                          (dict(reach=-1), "reach"), (dict(reach=33), "reach"), (dict(reach=33, tiled=True), "reach"),
                          (dict(threshold=0), "threshold"), (dict(threshold=0, tiled=True), "threshold")):
            with pytest.raises(GhmError, match=match):
                nearest(**kw)
        for kw, match in ((dict(h=None), "null"), (dict(n=None), "null"), (dict(d=None), "null"), (dict(t=None), "null"),
                          (dict(table=None), "null"), (dict(o=None), "null"), (dict(ph=W - 1), "pitch"), (dict(pn=W - 1), "pitch"),
                          (dict(pd=W - 1), "pitch"), (dict(pt=W - 1), "pitch"), (dict(po=W - 1), "pitch"),
                          (dict(Ww=0), "out of range"), (dict(Hh=4 * 65535 + 1, Ww=1), "out of range"),
                          (dict(reach=-1), "reach"), (dict(reach=33), "reach"), (dict(mode=-1), "mode"), (dict(mode=3), "mode")):
            with pytest.raises(GhmError, match=match):
                shape(**kw)
        dev.sync()
        for cv in (near, dist2, out):                  # the canaries around the planes, and the planes themselves
            assert (cv.read().view(np.uint8) == CANARY).all()
    finally:
        dev.sync()
        for b in (src, near.base, dist2.base, out.base):
            dev.free(b)
