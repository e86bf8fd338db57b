"""The scatter on the MI355X (csrc/scatter.hip, gan_heightmaps_amd/scatter.py): the chance, the candidates and both
forms of the thinning through the raw entry points against the restatement of tests/scatter_ref.py and against each other, bit for
bit -- the sampler is integer and the chance's operations are rounded one by one, so there are no tolerances.  The thinning is
driven with explicit priority planes, so that the cases can be adversarial.  Every output lies in a canary canvas with a pitch of
W + 2; every input has a pitch of W + 3 whose padding is NaN, blocked, or a candidate of priority 0; the state plane, which is
thinned in place, lies with a pitch of W + 3 inside a frame of such candidates that must come back untouched.  Then ``chance``,
``thin`` and ``scatter``, the model's and the world's methods, the command line, and the refusals of the raw entry points."""
import numpy as np
import pytest

from oracle import step as ostep
from gan_heightmaps_amd import hydrology as HY
from gan_heightmaps_amd import scatter as SC
from tests import hydrology_ref as HR
from tests import scatter_ref as S
from tests.gpu_common import build_model, CANARY, Canvas, dev, model_params, ops, padded, same, SMALL      # noqa: F401  (dev, ops: the module-scoped fixtures)
from tests.test_scatter_host import chance_cases

pytestmark = pytest.mark.gpu


def raw_thin(dev, ops, state, prio, s2, tiled):
    """-> (the thinned states, the launches) through the raw entry point"""
    H, W = state.shape
    p = W + 3
    frame = np.full((H + 2, p), S.UNDECIDED, np.uint8)              # a row above and below, two cells left, one right: candidates
    frame[1:H + 1, 2:W + 2] = state
    bufs = []
    try:
        d_p, pp = padded(dev, prio, np.uint32, 3, 0)
        bufs.append(d_p)
        d_s = dev.alloc(frame.nbytes)
        bufs.append(d_s)
        dev.h2d(d_s, frame)
        ws = dev.alloc(ops.scatter_workspace(H, W))
        bufs.append(ws)
        sweeps = ops.scatter_thin(d_p, pp, d_s + p + 2, p, H, W, s2, tiled, ws)
        dev.sync()
        back = np.empty_like(frame)
        dev.d2h(back, d_s, back.nbytes)
    finally:
        dev.sync()
        for b in bufs:
            dev.free(b)
    out = back[1:H + 1, 2:W + 2].copy()
    back[1:H + 1, 2:W + 2] = S.UNDECIDED
    assert (back == S.UNDECIDED).all(), "states around the plane were written"
    return out, sweeps


def raw_chance(dev, ops, h, tab, height_scale, density, seed, origin, dist2=None, water=None, blocked=None, threshold=0):
    """-> (chance, priority, state) through the raw entry points"""
    H, W = h.shape
    bufs = []
    try:
        d_h, ph = padded(dev, h, np.float32, 3, np.nan)
        bufs.append(d_h)
        d_d, pd = padded(dev, dist2 if water is not None else None, np.int32, 3, 0)
        d_b, pb = padded(dev, blocked if threshold else None, np.uint32, 3, 0xFFFFFFFF)
        bufs += [b for b in (d_d, d_b) if b is not None]
        d_t = dev.alloc(4 * S.TABLE_FLOATS)
        bufs.append(d_t)
        dev.h2d(d_t, np.ascontiguousarray(tab, np.float32))
        d_w = None
        if water is not None:
            water = np.ascontiguousarray(water, np.float32)
            d_w = dev.alloc(water.nbytes)
            bufs.append(d_w)
            dev.h2d(d_w, water)
        chance, prio, state = Canvas(dev, H, W, np.uint32), Canvas(dev, H, W, np.uint32), Canvas(dev, H, W, np.uint8)
        bufs += [chance.base, prio.base, state.base]
        ops.scatter_chance(d_h, ph, H, W, d_t, height_scale, density, chance.ptr, chance.pitch, d_d, pd, d_w,
                           0 if water is None else water.size - 1, d_b, pb, max(threshold, 1))
        ops.scatter_candidates(chance.ptr, chance.pitch, H, W, seed, origin, state.ptr, state.pitch, prio.ptr, prio.pitch)
        dev.sync()
        return chance.read(), prio.read(), state.read()
    finally:
        dev.sync()
        for b in bufs:
            dev.free(b)


# ---- 1. the thinning, both forms ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", S.KINDS)
def test_both_forms_of_the_thinning_equal_the_restatement(dev, ops, kind):
    kept = rejected = 0
    for shape in S.SHAPES:
        for s2 in S.S2S:
            state, prio = S.thin_case(kind, shape)
            want = S.thin_expected(kind, shape, s2)
            plain, sweeps = raw_thin(dev, ops, state, prio, s2, False)
            tiled, launches = raw_thin(dev, ops, state, prio, s2, True)
            assert same(plain, want), (kind, shape, s2, "plain")
            assert same(tiled, want), (kind, shape, s2, "tiled")
            assert same(plain, tiled)
            assert S.invariants(state, prio, s2, plain) is None and S.invariants(state, prio, s2, tiled) is None
            assert 1 <= launches <= sweeps <= shape[0] * shape[1] + 1
            if s2 == 1:
                assert np.array_equal(plain == S.KEPT, state == 1)                    # every candidate is kept
            kept += int((want == S.KEPT).sum())
            rejected += int((want == S.REJECTED).sum())
    # the case contains what it is for
    if kind == 'none':
        assert kept == rejected == 0
    elif kind == 'corner':
        assert kept == len(S.SHAPES) * len(S.S2S) and rejected == 0
    else:
        assert kept > 1000 and rejected > 1000
    if kind == 'equal':                                                               # ties go to the row, then the column
        state, prio = S.thin_case(kind, (33, 65))
        assert (prio == prio[0, 0]).all()
        first = np.argwhere(state == 1)[0]
        assert S.thin_expected(kind, (33, 65), 16)[tuple(first)] == S.KEPT


@pytest.mark.parametrize("rising", (True, False))
def test_the_staircases_cost_the_plain_form_a_sweep_per_cell_and_the_tiled_one_a_launch_per_tile(dev, ops, rising):
    for shape in ((1, 300), (300, 1)):
        state, prio = S.staircase(shape, rising)
        want = S.thin(state, prio, 2)
        plain, sweeps = raw_thin(dev, ops, state, prio, 2, False)
        tiled, launches = raw_thin(dev, ops, state, prio, 2, True)
        assert same(plain, want) and same(tiled, want)
        assert S.invariants(state, prio, 2, plain) is None
        assert sweeps == 300 + 1                       # one decision per sweep and the sweep that changes nothing: 38 groups
        assert 2 <= launches <= 10 + 1                 # the tiles along the chain, and the launch that changes nothing


def test_lds_and_workspace_sizes(ops):
    assert ops.scatter_lds_bytes(1024) == 4 * 94 * 94 + (94 * 94 + 15) // 16 * 16 == 44192
    assert ops.scatter_lds_bytes(1) == 4096 + 1024 and ops.scatter_lds_bytes(2) == 5 * 34 * 34 + 12
    assert ops.scatter_lds_bytes(0) == -1 and ops.scatter_lds_bytes(1025) == -1
    assert ops.scatter_workspace(3, 5) == 256 + 15 and ops.scatter_workspace(0, 5) == -1 and ops.scatter_workspace(1 << 16, 1 << 15) == -1


# ---- 2. the chance and the candidates -------------------------------------------------------------------------------------------
def test_the_chance_and_the_candidates_equal_the_restatement(dev, ops):
    labels = set()
    for label, h, tab, hs, dens, seed, origin, d2, water, blocked, thr in chance_cases():
        want = S.chance(h, tab, hs, dens, d2, water, blocked, thr)
        ws, wp = S.candidates(want, seed, origin)
        c, p, s = raw_chance(dev, ops, h, tab, hs, dens, seed, origin, d2, water, blocked, thr)
        assert same(c, want) and same(p, wp) and same(s, ws), (label, h.shape)
        assert c.max() <= S.ONE
        labels.add(label)
        if label == 'wild' and h.size > 1:
            assert h.min() < 0 or h.max() > 1
        if label == 'level':
            assert (h == h[0, 0]).all() and len(set(c[blocked == 0].tolist())) <= 1 and (c[blocked >= 1] == 0).all()
        if label in ('all', 'wild', 'level'):
            assert origin[0] < 0 or origin[1] < 0
    assert labels == {'plain', 'all', 'wild', 'level'}


def test_candidates_are_functions_of_the_seed_and_the_world_position(dev, ops):
    half = S.tables(np.full(256, 0.5), np.ones(64))
    flat = np.full((70, 90), 0.5, np.float32)
    _, p0, s0 = raw_chance(dev, ops, flat, half, 64.0, 1.0, 11, (-40, -30))
    _, p1, s1 = raw_chance(dev, ops, flat[:50, :60], half, 64.0, 1.0, 11, (-20, 0))
    assert same(p0[20:70, 30:90], p1) and same(s0[20:70, 30:90], s1) and 0.4 < s0.mean() < 0.6
    _, p2, s2 = raw_chance(dev, ops, flat, half, 64.0, 1.0, 12, (-40, -30))
    assert (p2 != p0).mean() > 0.99 and (s2 != s0).mean() > 0.4


# ---- 3. chance, thin and scatter ------------------------------------------------------------------------------------------------
def _terrain():
    H, W, q, seed = HR.CASES[3]
    return HR.terrain(H, W, q, seed)


def test_chance_thin_and_scatter_equal_the_restatement(dev, ops):
    h = _terrain()
    H, W = h.shape
    hab = SC.Habitat(altitude=(0.2, 0.9), altitude_fade=0.1, slope=(0, 40), slope_fade=20, density=0.6, road_clearance=2.0)
    roads = np.zeros((H, W), np.uint8)
    roads[H // 2, :] = 1
    blocked = np.zeros((H, W), bool)
    blocked[:4, :5] = True
    near = (np.abs(np.arange(H)[:, None] - H // 2) <= 2) & np.ones((1, W), bool)
    want = S.chance(h, hab.tables(), 16.0, 0.6, blocked=(blocked | near).astype(np.uint32), threshold=1)
    got = SC.chance(ops, h, hab, roads=roads, blocked=blocked, height_scale=16.0)
    assert same(got, want) and (got[near] == 0).all() and 100 < (got > 0).sum() < got.size and (got > 0)[~near & ~blocked].any()
    assert same(SC.chance(ops, (h * 255).astype(np.uint8), hab), S.chance((h * 255).astype(np.uint8).astype(np.float32) / np.float32(255),
                                                                           hab.tables(), 64.0, 0.6))
    state, prio = S.candidates(want, 5, (3, -4))
    for t in (None, False, True):
        out, sweeps = SC.thin(ops, state, prio, 10, tiled=t)
        assert same(out, S.thin(state, prio, 10)) and sweeps >= 2
    sp = SC.Species("pine", 3.2, hab, scale=(0.5, 2.0))
    for t in (None, False, True):
        placed = SC.scatter(ops, h[None], sp, seed=5, origin=(3, -4), roads=roads, blocked=blocked, height_scale=16.0, tiled=t, keep=SC.KEEP)
        layer = placed["pine"]
        wst, wpr = S.candidates(want, sp.seed(5), (3, -4))
        wout = S.thin(wst, wpr, sp.s2)
        assert same(layer.chance, want) and same(layer.priority, wpr) and same(layer.state, wout), t
        assert same(layer.points, S.points(wout) + np.array([3, -4], np.int32)) and layer.points.dtype == np.int32
        assert len(layer) > 20 and layer.candidates == int(wst.sum()) and layer.sweeps >= 2 and placed.sweeps == (layer.sweeps,)
        assert placed.tiled is (SC.DEFAULT_TILED if t is None else t) and placed.origin == (3, -4) and placed.shape == (H, W)
        local = layer.points - [3, -4]
        assert same(layer.height, h[local[:, 0], local[:, 1]])
        yaw, scale = SC._instances(sp, sp.seed(5), layer.points)
        assert same(layer.yaw, yaw) and same(layer.scale, scale) and ((scale >= 0.5) & (scale <= 2.0)).all()
        assert same(placed.raster() != 0, wout == S.KEPT)
        d = local[:, None, :].astype(np.int64) - local[None, :, :]
        d2 = (d * d).sum(2) + np.eye(len(local), dtype=np.int64) * 10000
        assert d2.min() >= sp.s2                                                      # no two points within the spacing
    assert SC.scatter(ops, h, sp, seed=5).layers[0].state is None


def test_hydrology_keeps_the_points_dry_and_a_second_species_keeps_its_distance(dev, ops):
    h = _terrain()
    hydro = HY.analyse(ops, h)
    wet_hab = SC.Habitat(slope=(0, 90), water=(0.9, 6.5), lake_clearance=1.5, river_clearance=1.0, river_threshold=20, lake_min_depth=1.0 / 64)
    lakes = hydro.depth > np.float32(1.0 / 64)
    rivers = (hydro.accumulation >= 20) & ~lakes
    assert lakes.any() and rivers.any()
    from tests import earthworks_ref as E
    off = np.zeros(h.shape, bool)
    for marks, c in ((lakes, 1.5), (rivers, 1.0)):
        d2 = E.nearest(marks.astype(np.uint32), int(np.ceil(c)), 1)[1]
        off |= (d2 >= 0) & (d2 <= c * c)
    wd2 = E.nearest((lakes | rivers).astype(np.uint32), 7, 1)[1]
    want = S.chance(hydro.filled, wet_hab.tables(), 64.0, 1.0, wd2, wet_hab.water_table(), off.astype(np.uint32), 1)
    got = SC.chance(ops, hydro.filled, wet_hab, hydro=hydro)
    assert same(got, want) and (got[lakes | rivers] == 0).all() and (got > 0).any()
    far, close = (wd2 == -1) & ~off, (wd2 >= 0) & (wd2 <= 9) & ~off
    assert far.any() and close.any() and got[far].max() < got[close].max()             # the water preference shows
    a = SC.Species("oak", 4.0, SC.Habitat(slope=(0, 90), river_threshold=20, lake_min_depth=1.0 / 64))
    b = SC.Species("fern", 2.0, SC.Habitat(slope=(0, 90), river_threshold=20, lake_min_depth=1.0 / 64), seed_stream=1)
    placed = SC.scatter(ops, hydro.filled, [a, b], seed=77, hydro=hydro, keep=('chance', 'state'))
    oak, fern = placed.layers
    assert len(oak) > 10 and len(fern) > 10 and not (lakes | rivers)[oak.points[:, 0], oak.points[:, 1]].any()
    alone = SC.scatter(ops, hydro.filled, b, seed=77, hydro=hydro)
    assert len(alone.layers[0]) > len(fern)                                            # the oaks took some of the ferns' ground
    d = fern.points[:, None, :].astype(np.int64) - oak.points[None, :, :]
    assert (d * d).sum(2).min() >= b.s2                                                # at the ferns' own spacing, no closer
    oaks = np.zeros(h.shape, np.uint32)
    oaks[oak.points[:, 0], oak.points[:, 1]] = 1
    nd2 = E.nearest(oaks, 2, 1)[1]                             # reach 2 sees the diagonal, d2 = 2 < s2 = 4
    wet = (lakes | rivers)
    wantb = S.chance(hydro.filled, b.habitat.tables(), 64.0, 1.0, blocked=(wet | ((nd2 >= 0) & (nd2 < 4))).astype(np.uint32), threshold=1)
    assert same(fern.chance, wantb)
    st, pr = S.candidates(wantb, b.seed(77))
    assert same(fern.state, S.thin(st, pr, 4))
    m = placed.raster()
    assert (m == 1).sum() == len(oak) and (m == 2).sum() == len(fern)


# ---- 4. the model's and the world's methods, the command line ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_model(dev):
    m = build_model(ostep.default_cfg(**SMALL), 5, dev, dtype="f32", use_graph=False)
    cfg = ostep.default_cfg(**SMALL)
    for s in range(3):                       # non-trivial BatchNorm running statistics (the deterministic pass reads them)
        m.z_fn(ostep.synthetic_batch(4, cfg, seed=40 + s)[0])
    return m


def test_model_and_world_methods_equal_the_modules_functions(small_model, dev, ops, tmp_path):
    m = small_model
    before = model_params(m)
    h = _terrain()
    H, W = h.shape
    # (the wider spacing first: a later species keeps its own spacing from the points placed before it)
    sp = [SC.Species("rock", 6.0, SC.Habitat(slope=(0, 90), density=0.5), seed_stream=3), SC.Species("pine", 3.0, SC.Habitat(slope=(0, 90)))]
    want = SC.scatter(ops, h, sp, seed=9, origin=(-7, 5))
    got = m.scatter_heightmap(h, sp, seed=9, origin=(-7, 5), tiled=False)
    for a, b in zip(got.layers, want.layers):
        assert same(a.points, b.points) and same(a.yaw, b.yaw) and same(a.scale, b.scale) and same(a.height, b.height) and len(a) > 5
    tex = np.random.RandomState(3).randint(0, 256, (H, W, 3)).astype(np.uint8)
    painted = m.paint_scatter(tex, got, [(0.0, 1.0, 0.0), (1.0, 0.0, 0.0)], radius=0, opacity=1.0)
    marks = got.raster()
    assert painted.dtype == np.uint8 and same(painted[marks == 0], tex[marks == 0])        # unpainted pixels keep their bits
    assert (painted[marks == 1] == [0, 255, 0]).all() and (painted[marks == 2] == [255, 0, 0]).all()
    wide = m.paint_scatter(tex, got, (0.2, 0.4, 0.2), radius=2)
    assert (wide != tex).any(axis=2).sum() > (marks != 0).sum() and same(wide, SC.paint(ops, tex, got, (0.2, 0.4, 0.2), 2, value_range=m.is_b_grayscale))
    nothing = SC.scatter(ops, h, SC.Species("none", 3.0, SC.Habitat(density=0.0)), tiled=True)
    assert len(nothing.layers[0]) == 0 and nothing.layers[0].candidates == 0 and nothing.layers[0].sweeps == 1
    assert same(m.paint_scatter(tex, nothing), tex)                                         # painted with no points: the same bits
    ftex = np.random.RandomState(4).rand(3, H, W).astype(np.float32) * 2 - 1
    assert same(m.paint_scatter(ftex, nothing), ftex)
    with m.terrain_world(42, chunk_cells=2) as world:
        one = SC.Species("tree", 2.5, SC.Habitat(slope=(0, 90), density=0.8))
        a = world.scatter(-20, 10, 50, 70, one, keep=SC.KEEP)
        b = world.scatter(-5, 30, 40, 60, one, keep=SC.KEEP)
        la, lb = a.layers[0], b.layers[0]
        assert a.origin == (-20, 10) and la.points[:, 0].min() >= -20 and la.points[:, 1].max() < 80 and len(la) > 30
        ref = SC.scatter(ops, world._unit_height(-20, 10, 50, 70), one, seed=world.seed, origin=(-20, 10))
        assert same(la.points, ref.layers[0].points)
        # where the rectangles overlap, one cell inside their edges: the same chance, candidates and priorities
        ia, ib = (slice(16, 49), slice(21, 69)), (slice(1, 34), slice(1, 49))
        assert same(la.chance[ia], lb.chance[ib]) and same(la.priority[ia], lb.priority[ib])
        assert same(la.state[ia] != 0, lb.state[ib] != 0) and (la.state[ia] != 0).sum() > 100
        wet = world.scatter(-20, 10, 50, 70, one, hydrology=True, seed=3, tiled=False)
        hyd = world.hydrology(-20, 10, 50, 70)
        assert same(wet.layers[0].points, SC.scatter(ops, hyd.filled, one, seed=3, origin=(-20, 10), hydro=hyd).layers[0].points)
    after = model_params(m)
    for k in before:
        for x, y in zip(before[k], after[k]):
            assert np.array_equal(x, y), k
    # and into a mesh file
    from tests.test_scatter_host import _chunks
    mesh = m.heightmap_mesh(h, 0.02)
    doc, _ = _chunks(open(mesh.save(str(tmp_path / "land.glb"), None, 64.0, instances=want), "rb").read())
    assert [n["name"] for n in doc["nodes"]] == ["terrain", "rock", "pine"]
    counts = [doc["accessors"][n["extensions"]["EXT_mesh_gpu_instancing"]["attributes"]["TRANSLATION"]]["count"] for n in doc["nodes"][1:]]
    assert counts == [len(l) for l in want.layers]


def test_command_line_writes_the_points(ops, tmp_path, capsys):
    h = _terrain()
    np.save(str(tmp_path / "h.npy"), h)
    tex = np.random.RandomState(3).randint(0, 256, h.shape + (3,)).astype(np.uint8)
    from gan_heightmaps_amd.util import save_png
    save_png(str(tmp_path / "t.png"), tex)
    args = [str(tmp_path / "h.npy"), str(tmp_path / "o.npz"), "--spacing", "3", "--slope", "0,90", "--density", "0.7", "--seed", "4",
            "--hydrology", "--river-threshold", "20", "--texture", str(tmp_path / "t.png"), "--painted", str(tmp_path / "p.png"),
            "--radius", "0", "--plain"]
    assert SC.main(args) == 0
    hydro = HY.analyse(ops, h)
    sp = SC.Species("tree", 3.0, SC.Habitat(slope=(0, 90), density=0.7, river_threshold=20))
    want = SC.scatter(ops, h, sp, seed=4, hydro=hydro).layers[0]
    z = np.load(str(tmp_path / "o.npz"))
    assert same(z["points_0"], want.points) and same(z["yaw_0"], want.yaw) and z["names"].tolist() == ["tree"] and len(want) > 10
    assert capsys.readouterr().out.startswith("%d points of %d candidates" % (len(want), want.candidates))
    from gan_heightmaps_amd.util import read_image
    painted = read_image(str(tmp_path / "p.png"))
    on = np.zeros(h.shape, bool)
    on[want.points[:, 0], want.points[:, 1]] = True
    assert same(painted[~on], tex[~on]) and (painted[on] != tex[on]).any()
    assert SC.main(args[:1] + [str(tmp_path / "o.csv")] + args[2:10]) == 0
    assert len(open(str(tmp_path / "o.csv")).read().splitlines()) == 1 + len(SC.scatter(ops, h, SC.Species(
        "tree", 3.0, SC.Habitat(slope=(0, 90), density=0.7)), seed=4).layers[0])


# ---- 5. refusals of the raw entry points ------------------------------------------------------------------------------------------
def test_refusals_of_the_entry_points_leave_every_byte_alone(dev, ops):
    from gan_heightmaps_amd._lib import GhmError
    H, W = 4, 8
    src = dev.alloc(4096)
    dev.memset_zero(src, 4096)
    chance, prio, state = Canvas(dev, H, W, np.uint32), Canvas(dev, H, W, np.uint32), Canvas(dev, H, W, np.uint8)
    p = chance.pitch

    def do_chance(h=src, ph=W, Hh=H, Ww=W, tab=src, hs=64.0, dens=1.0, c=chance.ptr, pc=p, d=None, pd=0, w=None, wn=0, b=None, pb=0, thr=1):
        ops.scatter_chance(h, ph, Hh, Ww, tab, hs, dens, c, pc, d, pd, w, wn, b, pb, thr)

    def do_cand(c=src, pc=W, Hh=H, Ww=W, s=state.ptr, ps=p, pr=prio.ptr, pp=p):
        ops.scatter_candidates(c, pc, Hh, Ww, 1, (0, 0), s, ps, pr, pp)

    def do_thin(pr=src, pp=W, s=state.ptr, ps=p, Hh=H, Ww=W, s2=4, tiled=False, ws=src):
        ops.scatter_thin(pr, pp, s, ps, Hh, Ww, s2, tiled, ws)

    try:
        for kw, match in ((dict(h=None), "null"), (dict(tab=None), "null"), (dict(c=None), "null"), (dict(ph=W - 1), "pitch"),
                          (dict(pc=W - 1), "pitch"), (dict(Hh=0), "out of range"), (dict(Hh=4 * 65535 + 1, Ww=1), "out of range"),
                          (dict(Hh=1 << 16, Ww=1 << 15, ph=1 << 15, pc=1 << 15), "out of range"), (dict(hs=0.0), "height_scale"),
                          (dict(hs=float("inf")), "height_scale"), (dict(hs=float("nan")), "height_scale"), (dict(dens=1.5), "density"),
                          (dict(dens=-0.5), "density"), (dict(dens=float("nan")), "density"), (dict(w=src, wn=4), "null"),
                          (dict(w=src, wn=4, d=src, pd=W - 1), "pitch"), (dict(w=src, wn=0, d=src, pd=W), "water_n"),
                          (dict(w=src, wn=1026, d=src, pd=W), "water_n"), (dict(b=src, pb=W - 1), "pitch"),
                          (dict(b=src, pb=W, thr=0), "threshold")):
            with pytest.raises(GhmError, match=match):
                do_chance(**kw)
        for kw, match in ((dict(c=None), "null"), (dict(s=None), "null"), (dict(pr=None), "null"), (dict(pc=W - 1), "pitch"),
                          (dict(ps=W - 1), "pitch"), (dict(pp=W - 1), "pitch"), (dict(Ww=0), "out of range")):
            with pytest.raises(GhmError, match=match):
                do_cand(**kw)
        for kw, match in ((dict(pr=None), "null"), (dict(s=None), "null"), (dict(ws=None), "null"), (dict(pp=W - 1), "pitch"),
                          (dict(ps=W - 1), "pitch"), (dict(Hh=0), "out of range"), (dict(s2=0), "s2"), (dict(s2=1025), "s2"),
                          (dict(s2=1025, tiled=True), "s2"), (dict(s2=-4, tiled=True), "s2")):
            with pytest.raises(GhmError, match=match):
                do_thin(**kw)
        st = dev.step_record_begin([dev])                 # a recording context: the thinning waits for the device, and says so
        try:
            for tiled in (False, True):
                with pytest.raises(GhmError, match="cannot be recorded"):
                    do_thin(tiled=tiled)
        finally:
            dev.step_record_end(st)
            dev.step_destroy(st)
        dev.sync()
        for cv in (chance, prio, state):                  # the canaries around the planes, and the planes themselves
            assert (cv.read().view(np.uint8) == CANARY).all()
    finally:
        dev.sync()
        for b in (src, chance.base, prio.base, state.base):
            dev.free(b)
