"""Least-cost travel on the MI355X (csrc/route.hip, gan_heightmaps_amd/route.py): every plane against the sequential
restatements of tests/route_ref.py -- a heap Dijkstra on Python integers -- exactly: costs are integers, so there are no
tolerances.  The tiled form against the plain one, resuming, degenerate and adversarial planes, pitches and canaries, the sweep
counts, ``field`` and ``paint``, the model's and the world's methods, and the refusals of the raw entry points."""
import numpy as np
import pytest

from oracle import step as ostep
from gan_heightmaps_amd import hydrology as HY
from gan_heightmaps_amd import route as RT
from tests import hydrology_ref as HR
from tests import route_ref as R
from tests.gpu_common import build_model, CANARY, Canvas, dev, model_params, ops, padded, same, scene_heights, SMALL      # noqa: F401  (dev, ops: the module-scoped fixtures)

pytestmark = pytest.mark.gpu

TILE = 32
PLANES = ('cost', 'parent', 'territory', 'traffic')
RAW = dict(cost=np.uint32, parent=np.int8, traffic=np.uint32, basin=np.int32)


def raw(dev, ops, h, sources, tiled, travel=R.TRAVEL, penalty=None, depth=None, acc=None, pad=2, src_pad=3, resume_with=None):
    """h, sources -> the four planes and the counts through the raw entry points; every output lies in a Canvas with a pitch of
    W + pad, the sources' planes have a pitch of W + src_pad with NaN (or a huge area) beyond their width.  resume_with: more
    sources, added to the finished field by a second call with resume"""
    h = np.ascontiguousarray(h, np.float32)
    H, W = h.shape
    bufs, cv = [], {}
    out = {}
    try:
        for plane, dtype, fill in ((h, np.float32, np.nan), (penalty, np.float32, np.nan), (depth, np.float32, np.nan),
                                   (acc, np.uint32, 0xFFFFFFFF)):
            bufs.append(padded(dev, plane, dtype, src_pad, fill))
        (d_h, ph), (d_pen, pp), (d_depth, pd), (d_acc, pa) = bufs
        ws, hws = dev.alloc(ops.route_workspace(H, W)), dev.alloc(ops.hydrology_workspace(H, W))
        bufs += [(ws, 0), (hws, 0)]
        for k in RAW:
            cv[k] = Canvas(dev, H, W, RAW[k], pad)
            bufs.append((cv[k].base, 0))
        p = cv['cost'].pitch
        ops.route_weights(d_h, H, W, ph, travel.height_scale, travel.grade, travel.lake, travel.ford, travel.river_threshold,
                          travel.lake_min_depth, ws, d_pen, pp, d_depth, pd, d_acc, pa)
        flat = R.flat_sources(sources, W)
        out['sweeps'], out['changed'] = ops.route_relax(H, W, flat, tiled, cv['cost'].ptr, p, ws)
        first = cv['cost'].read()
        out['again'] = ops.route_relax(H, W, flat, tiled, cv['cost'].ptr, p, ws, resume=True)
        assert np.array_equal(cv['cost'].read(), first)
        if resume_with:
            out['more'] = ops.route_relax(H, W, R.flat_sources(resume_with, W), tiled, cv['cost'].ptr, p, ws, resume=True)
        ops.route_parents(cv['cost'].ptr, p, H, W, cv['parent'].ptr, p, ws)
        out['rounds'] = ops.hydrology_accumulate(cv['parent'].ptr, p, H, W, cv['traffic'].ptr, p, cv['basin'].ptr, p, hws)
        dev.sync()
        got = {k: cv[k].read() for k in RAW}
    finally:
        dev.sync()
        for b, _ in bufs:
            if b is not None:
                dev.free(b)
    out['cost'], out['parent'] = got['cost'], got['parent']
    every = list(sources) + list(resume_with or ())
    out['territory'], out['traffic'] = RT.territory_traffic(got['basin'], got['traffic'], got['cost'], R.flat_sources(every, W))
    return out


def check_case(dev, ops, h, sources, label, **kw):
    """both forms through the raw entry points against the restatement"""
    want = R.field(h, sources, kw.get('travel', R.TRAVEL), kw.get('penalty'), kw.get('depth'), kw.get('acc'))
    H, W = h.shape
    jacobi_sweeps = R.jacobi(want.q, sources)[1]
    got = {}
    for tiled in (False, True):
        g = got[tiled] = raw(dev, ops, h, sources, tiled, **kw)
        for k in PLANES:
            assert same(g[k], getattr(want, k)), "%s: %s differs (tiled=%s)" % (label, k, tiled)
        assert 1 <= g['sweeps'] <= H * W
        assert g['changed'] == bool(((want.cost != 0) & (want.cost != R.UNREACHED)).any())
        # a second call with resume on the finished plane runs one group, changes nothing and says so
        assert g['again'][1] is False and 1 <= g['again'][0] <= (4 if tiled else 8)
        print("%s %d x %d tiled=%d: %d launches, jacobi %d" % (label, H, W, tiled, g['sweeps'], jacobi_sweeps))
    # the plain form's count does not depend on timing: the restated Jacobi count under the host's grouping rule
    assert got[False]['sweeps'] == R.host_sweeps(jacobi_sweeps, H * W)
    assert got[True]['sweeps'] <= got[False]['sweeps']
    return want, got


# ---- 1. exactness, both forms ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 5])
@pytest.mark.parametrize("case", range(len(R.TERRAINS)))
def test_every_plane_equals_the_restatement_and_tiled_equals_plain(dev, ops, case, count):
    h, pen, sources = R.case(case, count)
    want, _ = check_case(dev, ops, h, sources, "case %d, %d sources" % (case, count), penalty=pen)
    assert (want.cost == R.UNREACHED).any() and (want.parent >= 0).any()


def test_lakes_and_fords_of_a_hydrology_cost_what_travel_says(dev, ops):
    H, W, q, seed = R.TERRAINS[1]
    r = HR.analyse(R.terrain(H, W, q, seed))
    travel = R.TRAVEL._replace(river_threshold=40, lake_min_depth=1.0 / 64, lake=8.0, ford=3.0)
    assert (r.depth > 1.0 / 64).any() and (r.accumulation >= 40).any()
    sources = R.pick_sources(np.ones((H, W)), 3, 5)
    want, _ = check_case(dev, ops, r.filled, sources, "hydro", travel=travel, depth=r.depth, acc=r.accumulation)
    assert not same(want.cost, R.field(r.filled, sources, travel).cost)


# ---- 2. resume ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tiled", [False, True])
def test_resume_with_one_more_source_equals_all_sources_from_scratch(dev, ops, tiled):
    h, pen, sources = R.case(0, 5)
    want = R.field(h, sources, penalty=pen)
    g = raw(dev, ops, h, sources[:4], tiled, penalty=pen, resume_with=sources[4:])
    for k in PLANES:
        assert same(g[k], getattr(want, k)), k
    assert g['more'][1] is True and not same(want.cost, R.field(h, sources[:4], penalty=pen).cost)


# ---- 3. degenerate sizes and tile edges -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1), (2, 2)])
def test_degenerate_sizes(dev, ops, shape):
    H, W = shape
    h = R.terrain(H, W, None, 100 + H + W)
    _, got = check_case(dev, ops, h, [(0, 0)], "size")
    assert got[False]['sweeps'] == H * W               # the far cell needs every sweep the cap allows; the last goes out alone


@pytest.mark.parametrize("shape", [(TILE, TILE), (TILE + 1, TILE + 1), (TILE - 1, 2 * TILE + 1)])
def test_tile_edges_with_a_source_in_a_tile_corner(dev, ops, shape):
    H, W = shape
    h = R.terrain(H, W, 16, 200 + H + W)
    pen = R.sprinkled(H, W, 300 + H)
    corners = [(min(TILE - 1, H - 1), min(TILE - 1, W - 1)), (H - 1, W - 1), (0, min(TILE, W - 1))]
    for s in corners:
        pen[s] = 1
    check_case(dev, ops, h, corners[:1], "corner", penalty=pen)
    check_case(dev, ops, h, corners, "corners", penalty=pen)


def test_pitches_wider_than_the_plane(dev, ops):
    h, pen, sources = R.case(3, 5)
    want = R.field(h, sources, penalty=pen)
    for tiled in (False, True):
        g = raw(dev, ops, h, sources, tiled, penalty=pen, pad=9, src_pad=5)
        for k in PLANES:
            assert same(g[k], getattr(want, k)), (k, tiled)


# ---- 4. adversarial planes ------------------------------------------------------------------------------------------------------
def test_a_serpentine_corridor_crosses_every_tile_border_many_times(dev, ops):
    h, pen, source, end, units = R.serpentine()
    assert h.shape == (2 * TILE + 3, 2 * TILE + 3)      # 3 x 3 tiles
    want, got = check_case(dev, ops, h, [source], "serpentine", penalty=pen)
    assert int(got[True]['cost'][end]) == units == int(want.cost[end])
    # the plain form needs a sweep per cell of the corridor; the tiles shorten the way but still need many launches
    assert got[False]['sweeps'] > 30 * h.shape[0] and got[True]['sweeps'] > 30


def test_a_walled_in_source_and_a_source_on_impassable_ground_reach_themselves_alone(dev, ops):
    h, pen, at = R.walled_in()
    want, got = check_case(dev, ops, h, [at], "walled in", penalty=pen)
    for tiled in (False, True):
        g = got[tiled]
        rest = np.ones(h.shape, bool)
        rest[at] = False
        assert (g['cost'][rest] == R.UNREACHED).all() and (g['parent'][rest] == R.NO_PARENT).all()
        assert (g['territory'][rest] == -1).all() and (g['traffic'][rest] == 0).all()
        assert g['cost'][at] == 0 and g['parent'][at] == -1 and g['territory'][at] == 0 and g['traffic'][at] == 1
    pen = np.ones((TILE + 2, TILE + 3), np.float32)
    pen[TILE, TILE] = np.inf
    _, got = check_case(dev, ops, np.zeros(pen.shape, np.float32), [(TILE, TILE)], "impassable source", penalty=pen)
    assert int((got[True]['cost'] != R.UNREACHED).sum()) == 1 and got[True]['traffic'].sum() == 1


def test_two_sources_at_equal_cost_break_the_tie_by_the_lowest_k(dev, ops):
    h = np.zeros((5, 2 * TILE + 1), np.float32)
    sources = [(2, 0), (2, 2 * TILE)]
    _, got = check_case(dev, ops, h, sources, "tie")
    for tiled in (False, True):
        g = got[tiled]
        assert (g['cost'][:, TILE] == g['cost'][::-1, TILE]).all() and g['cost'][2, TILE] == 64 * TILE
        assert g['parent'][2, TILE] == 2 and g['territory'][2, TILE] == 1       # E (k = 2) before W (k = 6)
        assert g['parent'][2, TILE - 1] == 6 and g['parent'][2, TILE + 1] == 2


def test_an_impassable_lake_is_walked_around(dev, ops):
    h, depth = R.lake_plane()
    travel = R.TRAVEL._replace(lake=np.inf)
    want, got = check_case(dev, ops, h, [(18, 2)], "lake", travel=travel, depth=depth)
    assert (got[True]['cost'][depth > 0] == R.UNREACHED).all() and got[True]['cost'][18, 37] > 35 * 64


def test_saturation_every_edge_clamps_and_the_sum_does_not_wrap(dev, ops):
    h, pen, source = R.saturated_strip()
    want, got = check_case(dev, ops, h, [source], "saturation", penalty=pen)
    for tiled in (False, True):
        c = got[tiled]['cost'][0]
        assert np.array_equal(c[:256].astype(np.int64), np.arange(256, dtype=np.int64) << 24) and (c[256:] == R.UNREACHED).all()


# ---- 5. field ------------------------------------------------------------------------------------------------------------------
def test_field_in_every_form_and_with_every_keep(dev, ops):
    h, pen, sources = R.case(2, 5)
    want = R.field(h, sources, penalty=pen)
    plain_sweeps = R.host_sweeps(R.jacobi(want.q, sources)[1], h.size)
    for t in (None, False, True):
        f = RT.field(ops, h, sources, penalty=pen, tiled=t)
        for k in PLANES:
            assert same(getattr(f, k), getattr(want, k)), "field(tiled=%s).%s" % (t, k)
        assert f.tiled is (RT.DEFAULT_TILED if t is None else t) and f.shape == h.shape and f.origin == (0, 0)
        assert f.sources == tuple(sources) and f.unit == 64 and 1 <= f.sweeps <= h.size
        if not f.tiled:
            assert f.sweeps == plain_sweeps
    for keep in PLANES:
        f = RT.field(ops, h[None], sources, penalty=pen, keep=keep)
        assert same(getattr(f, keep), getattr(want, keep))
        assert all(getattr(f, k) is None for k in PLANES if k != keep)
    far = tuple(int(v) for v in np.argwhere(want.cost == want.cost[want.cost != R.UNREACHED].max())[0])
    f = RT.field(ops, h, sources, penalty=pen, keep=('cost', 'parent'))
    assert np.array_equal(f.path(far), R.walk(want.parent, far)) and f.travel_cost(far) == int(want.cost[far]) / 64.0
    u8 = np.rint(h * 255).astype(np.uint8)                                    # uint8 is read as v / 255
    assert same(RT.field(ops, u8, sources, keep='cost').cost, R.field(u8.astype(np.float32) / np.float32(255), sources).cost)
    moved = RT.field(ops, h, [(r + 7, c - 9) for r, c in sources], penalty=pen, origin=(7, -9), keep=('cost', 'parent'))
    assert same(moved.cost, want.cost) and np.array_equal(moved.path((far[0] + 7, far[1] - 9)), f.path(far) + [7, -9])


def test_field_on_a_hydrology_routes_round_its_lakes_and_fords(dev, ops):
    H, W, q, seed = R.TERRAINS[1]
    h = R.terrain(H, W, q, seed)
    hydro = HY.analyse(ops, h)
    travel = RT.Travel(river_threshold=40, lake_min_depth=1.0 / 64)
    sources = R.pick_sources(np.ones((H, W)), 3, 6)
    f = RT.field(ops, hydro.filled, sources, travel, hydro=hydro)
    want = R.field(hydro.filled, sources, R.Travel(*[getattr(travel, k) for k in R.Travel._fields]), depth=hydro.depth,
                   accumulation=hydro.accumulation)
    for k in PLANES:
        assert same(getattr(f, k), getattr(want, k)), k
    assert not same(f.cost, RT.field(ops, hydro.filled, sources, travel, keep='cost').cost)


# ---- 6. paint ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def road_case():
    h, pen, sources = R.case(1, 5)
    r = R.field(h, sources, penalty=pen)
    f = RT.CostField(h.shape, sources, cost=r.cost, parent=r.parent, territory=r.territory, traffic=r.traffic)
    cells = [tuple(int(v) for v in c) for c in np.argwhere(r.cost != R.UNREACHED)[::401]]
    return h, r, f, [R.walk(r.parent, c) for c in cells]


@pytest.mark.parametrize("width", [0, 2])
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("kind", ["uint8", "unit", "tanh"])
def test_paint_against_the_numpy_restatement(ops, road_case, kind, channels, width):
    h, r, f, paths = road_case
    H, W = h.shape
    road = RT.Road(width=width, colour=(0.4, 0.3, 0.1), opacity=0.7)
    marks = R.raster((H, W), paths)
    on = HR.wet_mask(np.zeros((H, W), np.float32), marks, 1, width, 0.0)
    assert on.any() and (~on).any() and int(marks.sum()) > 50
    rs = np.random.RandomState(5)
    colour = np.float32([0.4, 0.3, 0.1])
    if kind == "uint8":
        tex = rs.randint(0, 256, (H, W, channels)).astype(np.uint8)
        tex = tex[:, :, 0] if channels == 1 and width == 0 else tex               # (H, W) and (H, W, 1)
        planes = (tex.reshape(H, W, channels).astype(np.float32) / np.float32(255)).transpose(2, 0, 1)
        want = HR.paint_planes(planes, on, colour, 0.7)
        want = np.rint(np.clip(want, 0, 1).astype(np.float64) * 255).astype(np.uint8).transpose(1, 2, 0).reshape(tex.shape)
        value_range = None
    else:
        tex = rs.rand(channels, H, W).astype(np.float32)
        if kind == "tanh":
            tex = tex * 2 - 1
            colour = (colour * np.float32(255) - np.float32(127.5)) / np.float32(127.5)
        tex = tex[0] if channels == 1 and width == 0 else tex                     # (H, W) and (1, H, W)
        want = HR.paint_planes(tex.reshape(channels, H, W), on, colour, 0.7).reshape(tex.shape)
        value_range = kind == "unit"
    got = RT.paint(ops, tex, f, paths, road, value_range=value_range)
    assert got.shape == tex.shape and same(got, want)
    off = ~on if tex.ndim == 2 else (~on[:, :, None] if kind == "uint8" else ~on[None])
    off = np.broadcast_to(off, tex.shape)
    assert np.array_equal(got[off].view(np.uint8), tex[off].view(np.uint8))       # unpainted pixels: the input's bits
    assert (got != tex)[np.broadcast_to(~off, tex.shape)].any()


def test_paint_the_trails_that_traffic_makes(ops, road_case):
    h, r, f, paths = road_case
    H, W = h.shape
    road = RT.Road(width=0, traffic_threshold=25, colour=(0.4, 0.3, 0.1), opacity=0.7)
    on = r.traffic >= 25
    assert on.any() and (~on).any()
    tex = np.random.RandomState(6).rand(3, H, W).astype(np.float32)
    got = RT.paint(ops, tex, f, paths, road, value_range=True)                   # the paths are not looked at
    assert same(got, HR.paint_planes(tex, on, np.float32([0.4, 0.3, 0.1]), 0.7))
    off = np.broadcast_to(~on[None], tex.shape)
    assert np.array_equal(got[off].view(np.uint8), tex[off].view(np.uint8))       # unpainted pixels: the input's bits
    moved = RT.CostField(h.shape, f.sources, origin=(3, 4), cost=r.cost, parent=r.parent)
    assert same(RT.paint(ops, tex, moved, [p + [3, 4] for p in paths], RT.Road(width=0), value_range=True),
                RT.paint(ops, tex, f, paths, RT.Road(width=0), value_range=True))


# ---- 7. the model's and the world's methods --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_model(dev):
    m = build_model(ostep.default_cfg(**SMALL), 5, dev, dtype="f32", use_graph=False)
    cfg = ostep.default_cfg(**SMALL)
    for s in range(3):                       # non-trivial BatchNorm running statistics (the deterministic pass reads them)
        m.z_fn(ostep.synthetic_batch(4, cfg, seed=40 + s)[0])
    return m


def test_model_and_world_methods_equal_field_and_leave_the_training_state_untouched(small_model, dev, ops):
    m = small_model
    before = model_params(m)
    h, pen, sources = R.case(3, 5)
    H, W = h.shape
    want = RT.field(ops, h, sources, penalty=pen)
    got = m.heightmap_routes(h[None], sources, penalty=pen, tiled=True)
    for k in RT.KEEP:
        assert same(getattr(got, k), getattr(want, k)), k
    tex = np.random.RandomState(3).randint(0, 256, (H, W, 3)).astype(np.uint8)
    far = tuple(int(v) for v in np.argwhere(want.cost == want.cost[want.cost != R.UNREACHED].max())[0])
    paths = got.paths([far])
    painted = m.paint_roads(tex, got, paths)
    assert same(painted, RT.paint(ops, tex, want, paths)) and (painted != tex).any()
    trails = m.paint_roads(tex, got, road=RT.Road(traffic_threshold=20))
    assert same(trails, RT.paint(ops, tex, want, road=RT.Road(traffic_threshold=20))) and (trails != tex).any()
    with m.terrain_world(42, chunk_cells=2) as world:
        y0, x0, hh, ww = rect = (-20, 10, 50, 70)
        towns = [(-15, 20), (25, 75), (0, 40)]
        wr = world.routes(*rect, towns)
        hm = scene_heights(m, world.heightmap(*rect))
        local = [(r - y0, c - x0) for r, c in towns]
        ref = RT.field(ops, hm, local)
        for k in RT.KEEP:
            assert same(getattr(wr, k), getattr(ref, k)), k
        assert wr.origin == (y0, x0) and wr.sources == tuple(towns) and wr.shape == (hh, ww)
        p = wr.path((29, 79))                                                    # world coordinates in, world coordinates out
        assert np.array_equal(p, ref.path((29 - y0, 79 - x0)) + [y0, x0]) and tuple(p[0]) == (29, 79) and tuple(p[-1]) in towns
        assert wr.travel_cost((29, 79)) == ref.travel_cost((29 - y0, 79 - x0)) > 0
        hydro = world.hydrology(*rect)
        wh = world.routes(*rect, towns, hydrology=True, keep=('cost', 'territory'))
        rh = RT.field(ops, hydro.filled, local, hydro=hydro)
        assert same(wh.cost, rh.cost) and same(wh.territory, rh.territory) and wh.parent is None and wh.origin == (y0, x0)
        # routes belong to the rectangle: a sub-rectangle does not see the ways round its outside
        sub = world.routes(-10, 20, 30, 40, [(0, 40)], keep=('cost',))
        assert sub.cost[10, 20] == 0 and (sub.cost >= world.routes(*rect, [(0, 40)], keep=('cost',)).cost[10:40, 10:50]).all()
    after = model_params(m)
    for k in before:
        for x, y in zip(before[k], after[k]):
            assert np.array_equal(x, y), k


def test_command_line_writes_the_planes_the_paths_and_the_painted_texture(ops, tmp_path):
    from PIL import Image
    H, W, q, seed = R.TERRAINS[3]
    u8 = np.rint(R.terrain(H, W, q, seed) * 255).astype(np.uint8)
    tex = np.random.RandomState(9).randint(0, 256, (H, W, 3)).astype(np.uint8)
    Image.fromarray(u8).save(str(tmp_path / "h.png"))
    Image.fromarray(tex).save(str(tmp_path / "t.png"))
    prefix = str(tmp_path / "out")
    assert RT.main([str(tmp_path / "h.png"), prefix, "--from", "3,4", "--from", "30,40", "--to", "16,20", "--to", "0,46", "--hydrology",
                    "--texture", str(tmp_path / "t.png"), "--painted", str(tmp_path / "p.png"), "--road-width", "0", "--grade",
                    "0.3", "--plain"]) == 0
    hydro = HY.analyse(ops, u8)
    want = RT.field(ops, hydro.filled, [(3, 4), (30, 40)], RT.Travel(grade=0.3), hydro=hydro)
    for k in RT.KEEP:
        assert same(np.load("%s.%s.npy" % (prefix, k)), getattr(want, k)), k
    paths = want.paths([(16, 20), (0, 46)])
    for i, p in enumerate(paths):
        assert same(np.load("%s.path%d.npy" % (prefix, i)), p)
    painted = np.asarray(Image.open(str(tmp_path / "p.png")))
    assert same(painted, RT.paint(ops, tex, want, paths, RT.Road(width=0))) and (painted != tex).any()


# ---- 8. refusals of the raw entry points -------------------------------------------------------------------------------------------
def test_refusals_of_the_entry_points_leave_every_byte_alone(dev, ops):
    from gan_heightmaps_amd._lib import GhmError
    assert ops.route_workspace(0, 5) == -1 and ops.route_workspace(1 << 16, 1 << 15) == -1
    assert ops.route_workspace(3, 5) == 256 + 4 * RT.MAX_SOURCES + 5 * 4 * 15
    H, W = 4, 8
    good = dict(height_scale=64.0, grade=0.15, lake=16.0, ford=4.0, river_threshold=256, lake_min_depth=0.0)
    src = dev.alloc(4096)
    wsize = ops.route_workspace(H, W)
    ws = dev.alloc(wsize)
    canary = np.full(wsize, CANARY, np.uint8)
    dev.h2d(ws, canary)
    cost, parent = Canvas(dev, H, W, np.uint32), Canvas(dev, H, W, np.int8)
    p = cost.pitch

    def weights(h=src, Hh=H, Ww=W, pitch=W, w=ws, pen=None, pp=0, depth=None, dp=0, acc=None, ap=0, **kw):
        t = dict(good, **kw)
        ops.route_weights(h, Hh, Ww, pitch, t['height_scale'], t['grade'], t['lake'], t['ford'], t['river_threshold'],
                          t['lake_min_depth'], w, pen, pp, depth, dp, acc, ap)

    try:
        for kw, match in ((dict(h=None), "null"), (dict(w=None), "null"), (dict(pitch=W - 1), "pitch"),
                          (dict(Hh=0), "out of range"), (dict(Hh=1 << 16, Ww=1 << 15, pitch=1 << 15), "out of range"),
                          (dict(Hh=4 * 65535 + 1, Ww=1, pitch=1), "out of range"), (dict(Hh=1 << 15, pitch=1 << 16), "pitch"),
                          (dict(pen=src, pp=W - 1), "pitch"), (dict(depth=src, dp=W - 1), "pitch"),
                          (dict(acc=src, ap=W - 1), "pitch"),
                          (dict(grade=0.0), "grade"), (dict(grade=-1.0), "grade"), (dict(grade=float("inf")), "grade"),
                          (dict(grade=float("nan")), "grade"), (dict(grade=1e-40), "grade"),
                          (dict(height_scale=0.0), "height_scale"), (dict(height_scale=float("inf")), "height_scale"),
                          (dict(height_scale=float("nan")), "height_scale"), (dict(lake=0.5), "lake"),
                          (dict(lake=float("nan")), "lake"), (dict(ford=0.5), "ford"), (dict(ford=float("inf")), "ford"),
                          (dict(lake_min_depth=-1.0), "lake_min_depth")):
            with pytest.raises(GhmError, match=match):
                weights(**kw)
        for args, kw, match in (((H, W, [0], False, None, p, ws), {}, "null"), ((H, W, [0], False, cost.ptr, p, None), {}, "null"),
                                ((H, W, [], False, cost.ptr, p, ws), {}, "null|sources"),
                                ((H, W, [0], True, cost.ptr, W - 1, ws), {}, "pitch"),
                                ((H, W, [H * W], False, cost.ptr, p, ws), {}, "outside"),
                                ((H, W, [3, -1], True, cost.ptr, p, ws), {}, "outside"),
                                ((H, W, [0] * (RT.MAX_SOURCES + 1), False, cost.ptr, p, ws), dict(resume=True), "sources"),
                                ((0, W, [0], False, cost.ptr, p, ws), {}, "out of range"),
                                ((1 << 16, 1 << 15, [0], False, cost.ptr, 1 << 15, ws), {}, "out of range"),
                                ((4 * 65535 + 1, 1, [0], True, cost.ptr, 1, ws), {}, "out of range")):
            with pytest.raises(GhmError, match=match):
                ops.route_relax(*args, **kw)
        for args, match in (((None, p, H, W, parent.ptr, parent.pitch, ws), "null"), ((cost.ptr, p, H, W, None, p, ws), "null"),
                            ((cost.ptr, p, H, W, parent.ptr, parent.pitch, None), "null"),
                            ((cost.ptr, W - 1, H, W, parent.ptr, parent.pitch, ws), "pitch"),
                            ((cost.ptr, p, H, W, parent.ptr, W - 1, ws), "pitch"),
                            ((cost.ptr, p, H, 0, parent.ptr, parent.pitch, ws), "out of range")):
            with pytest.raises(GhmError, match=match):
                ops.route_parents(*args)
        dev.sync()
        back = np.empty_like(canary)
        dev.d2h(back, ws, wsize)
        assert (back == CANARY).all(), "a refused call wrote to the workspace"
        for cv in (cost, parent):                      # the canaries around the planes, and the planes themselves
            assert (cv.read().view(np.uint8) == CANARY).all()
        weights(lake=float("inf"))                     # +inf is a lake's way of being impassable, not a refusal
        dev.sync()
    finally:
        dev.sync()
        for b in (src, ws, cost.base, parent.base):
            dev.free(b)
