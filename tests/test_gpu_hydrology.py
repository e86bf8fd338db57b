"""Hydrology on the MI355X (csrc/hydrology.hip, gan_heightmaps_amd/hydrology.py): every plane against the
sequential restatements of tests/hydrology_ref.py, exactly -- nothing here rounds differently, so there are no tolerances --
the tiled form against the plain one, degenerate and adversarial planes, pitches and canaries, the convergence counts, the
paint kernel against its numpy restatement, and the model's and the world's methods."""
import numpy as np
import pytest

from oracle import step as ostep
from gan_heightmaps_amd import hydrology as HY
from gan_heightmaps_amd import render as RN
from tests import hydrology_ref as R
from tests.gpu_common import build_model, CANARY, Canvas, dev, model_params, ops, same, scene_heights, SMALL      # noqa: F401  (dev, ops: the module-scoped fixtures)

pytestmark = pytest.mark.gpu

TILE = 32
PLANES = ('filled', 'flat', 'direction', 'accumulation', 'basin')
DTYPES = dict(filled=np.float32, flat=np.int32, direction=np.int8, accumulation=np.uint32, basin=np.int32)


def raw(dev, ops, h, tiled, pad=2, src_pad=0):
    """h -> the five planes and the counts through the raw entry points; every output lies in a Canvas with a pitch of
    W + pad, the source has a pitch of W + src_pad with NaN beyond its width"""
    h = np.ascontiguousarray(h, np.float32)
    H, W = h.shape
    src = np.full((H, W + src_pad), np.nan, np.float32)
    src[:, :W] = h
    bufs = [dev.alloc(src.nbytes), dev.alloc(ops.hydrology_workspace(H, W))]
    cv = {}
    try:
        for k in PLANES:
            cv[k] = Canvas(dev, H, W, DTYPES[k], pad)
            bufs.append(cv[k].base)
        dev.h2d(bufs[0], src)
        p = cv['filled'].pitch
        fill_sweeps, changed = ops.hydrology_fill(bufs[0], H, W, W + src_pad, tiled, cv['filled'].ptr, p, bufs[1])
        F = cv['filled'].read()
        again = ops.hydrology_fill(bufs[0], H, W, W + src_pad, tiled, cv['filled'].ptr, p, bufs[1], resume=True)
        assert np.array_equal(cv['filled'].read().view(np.int32), F.view(np.int32))
        flat_sweeps = ops.hydrology_flats(cv['filled'].ptr, H, W, p, tiled, cv['flat'].ptr, p, bufs[1])
        ops.hydrology_directions(cv['filled'].ptr, p, cv['flat'].ptr, p, H, W, cv['direction'].ptr, p)
        rounds = ops.hydrology_accumulate(cv['direction'].ptr, p, H, W, cv['accumulation'].ptr, p, cv['basin'].ptr, p, bufs[1])
        dev.sync()
        out = {k: cv[k].read() for k in PLANES}
    finally:
        dev.sync()
        for b in bufs:
            dev.free(b)
    out.update(sweeps=(fill_sweeps, flat_sweeps), rounds=rounds, changed=changed, again=again)
    return out


def check_plane(dev, ops, h, label, through_analyse=True):
    """both forms through the raw entry points against the restatement, and ``analyse`` in every form"""
    want = R.analyse(h)
    H, W = h.shape
    got = {}
    for tiled in (False, True):
        g = got[tiled] = raw(dev, ops, h, tiled)
        for k in PLANES:
            assert same(g[k], getattr(want, k)), "%s: %s differs (tiled=%s)" % (label, k, tiled)
        fill_sweeps, flat_sweeps = g['sweeps']
        assert 1 <= fill_sweeps <= H * W and 1 <= flat_sweeps <= H * W, g['sweeps']
        assert g['rounds'] == R.doubling(want.direction)[2]
        # a second call on the converged surface runs one group, changes nothing and says so
        assert g['again'][1] is False and g['again'][0] <= 8
        assert g['changed'] == bool((H > 2 and W > 2))
        print("%s %d x %d tiled=%d: sweeps %s, rounds %d" % (label, H, W, tiled, g['sweeps'], g['rounds']))
    if through_analyse:
        for t in (None, False, True):
            a = HY.analyse(ops, h, tiled=t)
            for k in ('filled', 'depth', 'direction', 'accumulation', 'basin'):
                assert same(getattr(a, k), getattr(want, k)), "%s: analyse(tiled=%s).%s" % (label, t, k)
            assert a.rounds == got[False]['rounds'] and a.tiled is (HY.DEFAULT_TILED if t is None else t)
            if not a.tiled:                            # the plain form's count does not depend on timing
                assert a.sweeps == got[False]['sweeps']
    return want, got


# ---- 1. exactness, both forms ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(R.CASES)))
def test_every_plane_equals_the_restatement_and_tiled_equals_plain(dev, ops, case):
    H, W, q, seed = R.CASES[case]
    check_plane(dev, ops, R.terrain(H, W, q, seed), "case %d" % case)


# ---- 2. degenerate and adversarial planes ----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 7), (9, 1), (1, 1), (2, 2), (3, 3), (2, 40), (TILE + 1, TILE + 1), (TILE - 1, TILE - 1),
                                   (TILE, 2 * TILE), (2 * TILE + 1, TILE - 1)])
def test_degenerate_sizes_and_sizes_round_the_tile(dev, ops, shape):
    H, W = shape
    h = R.terrain(H, W, 16, 100 + H + W)
    if H >= 3 and W >= 3:
        h[H // 2, W // 2] = -1.0                       # a pit, whatever the noise gives
    check_plane(dev, ops, h, "size", through_analyse=False)


def test_a_serpentine_lake_drains_along_a_path_far_longer_than_the_side(dev, ops):
    h = R.serpentine()
    want, got = check_plane(dev, ops, h, "serpentine")
    assert want.flat.max() > 10 * max(h.shape)
    # the plain form needs a sweep per cell of the channel; the tiles shorten the way but still need many launches
    assert got[False]['sweeps'][0] > want.flat.max() and got[True]['sweeps'][0] > 4


def test_pits_on_the_corners_where_four_tiles_meet(dev, ops):
    h = R.corner_pits(TILE, 3)
    want, _ = check_plane(dev, ops, h, "corner pits")
    for y in (TILE, 2 * TILE):
        for x in (TILE, 2 * TILE):
            assert (want.depth[y - 1:y + 1, x - 1:x + 1] > 0).all()


def test_minus_zero_reads_as_zero_and_a_constant_plane_is_one_flat(dev, ops):
    h = np.zeros((TILE + 3, TILE + 5), np.float32)
    h[::2, ::3] = -0.0
    want, got = check_plane(dev, ops, h, "zeros")
    assert not np.signbit(got[True]['filled']).any() and want.flat.max() == (TILE + 3 - 1) // 2


# ---- 3. pitches and canaries ---------------------------------------------------------------------------------------------------
def test_pitches_wider_than_the_plane(dev, ops):
    H, W, q, seed = R.CASES[3]
    h = R.terrain(H, W, q, seed)
    want = R.analyse(h)
    for tiled in (False, True):
        g = raw(dev, ops, h, tiled, pad=9, src_pad=5)
        for k in PLANES:
            assert same(g[k], getattr(want, k)), (k, tiled)


# ---- 4. convergence counts -------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits_and_counts(dev, ops):
    H, W, q, seed = R.CASES[1]
    h = R.terrain(H, W, q, seed)
    for tiled in (False, True):
        a, b = HY.analyse(ops, h, tiled=tiled), HY.analyse(ops, h, tiled=tiled)
        for k in HY.KEEP:
            assert same(getattr(a, k), getattr(b, k))
        assert a.rounds == b.rounds and max(a.sweeps) <= H * W and a.tiled is tiled
        if not tiled:
            assert a.sweeps == b.sweeps                # the plain form's count does not depend on timing
    part = HY.analyse(ops, h, keep=('depth',))
    assert part.filled is None and part.accumulation is None and same(part.depth, a.depth)


def test_refusals_of_the_entry_points(dev, ops):
    from gan_heightmaps_amd._lib import GhmError
    assert ops.hydrology_workspace(0, 5) == -1 and ops.hydrology_workspace(1 << 16, 1 << 15) == -1
    assert ops.hydrology_workspace(3, 5) == 256 + 6 * 4 * 15
    buf = dev.alloc(4096)
    try:
        with pytest.raises(GhmError, match="pitch"):
            ops.hydrology_fill(buf, 4, 8, 7, False, buf, 8, buf)
        with pytest.raises(GhmError, match="null"):
            ops.hydrology_flats(buf, 4, 8, 8, False, None, 8, buf)
        with pytest.raises(GhmError, match="out of range"):
            ops.hydrology_directions(buf, 8, buf, 8, 0, 8, buf, 8)
        with pytest.raises(GhmError, match="river_width"):
            ops.hydrology_paint(buf, 8, buf, 8, 4, 8, buf, 8, 1, (0, 0, 0), 0.5, 0.0, 1, 5, False, buf, 8)
        with pytest.raises(GhmError, match="channels"):
            ops.hydrology_paint(buf, 8, buf, 8, 4, 8, buf, 8, 2, (0, 0, 0), 0.5, 0.0, 1, 1, False, buf, 8)
    finally:
        dev.free(buf)


# ---- 5. paint ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def painted_case():
    H, W, q, seed = R.CASES[1]
    h = R.terrain(H, W, q, seed)
    r = R.analyse(h)
    hydro = HY.Hydrology((H, W), (0, 0), 0, False, filled=r.filled, depth=r.depth, accumulation=r.accumulation)
    return h, r, hydro


@pytest.mark.parametrize("width", [0, 2])
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("kind", ["uint8", "unit", "tanh"])
def test_paint_against_the_numpy_restatement(ops, painted_case, kind, channels, width):
    h, r, hydro = painted_case
    H, W = h.shape
    water = HY.Water(river_threshold=40, river_width=width, lake_min_depth=1.0 / 64, colour=(0.1, 0.3, 0.6), opacity=0.7)
    wet = R.wet_mask(r.depth, r.accumulation, 40, width, 1.0 / 64)
    edge = R.is_outlet(H, W)
    assert wet[edge].any() and (~wet).any() and (r.depth > 1.0 / 64).any()       # rivers reach the edges, lakes exist
    rs = np.random.RandomState(5)
    colour = np.float32([0.1, 0.3, 0.6])
    if kind == "uint8":
        tex = rs.randint(0, 256, (H, W, channels)).astype(np.uint8)
        tex = tex[:, :, 0] if channels == 1 and width == 0 else tex               # (H, W) and (H, W, 1)
        planes = (tex.reshape(H, W, channels).astype(np.float32) / np.float32(255)).transpose(2, 0, 1)
        want = R.paint_planes(planes, wet, colour, 0.7)
        want = np.rint(np.clip(want, 0, 1).astype(np.float64) * 255).astype(np.uint8).transpose(1, 2, 0).reshape(tex.shape)
        value_range = None
    else:
        tex = rs.rand(channels, H, W).astype(np.float32)
        if kind == "tanh":
            tex = tex * 2 - 1
            colour = (colour * np.float32(255) - np.float32(127.5)) / np.float32(127.5)
        tex = tex[0] if channels == 1 and width == 0 else tex                     # (H, W) and (1, H, W)
        want = R.paint_planes(tex.reshape(channels, H, W), wet, colour, 0.7).reshape(tex.shape)
        value_range = kind == "unit"
    got = HY.paint(ops, tex, hydro, water, value_range=value_range)
    assert got.shape == tex.shape and same(got, want)
    dry = ~wet if tex.ndim == 2 else (~wet[:, :, None] if kind == "uint8" else ~wet[None])
    dry = np.broadcast_to(dry, tex.shape)
    assert np.array_equal(got[dry].view(np.uint8), tex[dry].view(np.uint8))       # dry pixels: the input's bits
    assert (got != tex)[np.broadcast_to(~dry, tex.shape)].any()


# ---- 6. the model's and the world's methods -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_model(dev):
    m = build_model(ostep.default_cfg(**SMALL), 5, dev, dtype="f32", use_graph=False)
    cfg = ostep.default_cfg(**SMALL)
    for s in range(3):                       # non-trivial BatchNorm running statistics (the deterministic pass reads them)
        m.z_fn(ostep.synthetic_batch(4, cfg, seed=40 + s)[0])
    return m


def test_model_methods_equal_analyse_and_leave_the_training_state_untouched(small_model, dev, ops):
    m = small_model
    before = model_params(m)
    H, W, q, seed = R.CASES[3]
    h = R.terrain(H, W, q, seed)
    want = HY.analyse(ops, h)
    got = m.heightmap_hydrology(h[None], tiled=True)
    for k in HY.KEEP:
        assert same(getattr(got, k), getattr(want, k)), k
    tex = np.random.RandomState(3).randint(0, 256, (H, W, 3)).astype(np.uint8)
    water = HY.Water(river_threshold=30)
    painted = m.paint_water(tex, got, water)
    assert same(painted, HY.paint(ops, tex, want, water)) and (painted != tex).any()
    cam = RN.Camera.look_at((-10.0, -10.0, 40.0), (H / 2.0, W / 2.0, 0.0), size=(24, 32))
    with RN.Scene(got.filled, painted, device=dev) as scene:
        img = scene.render(cam, max_dist=120.0)
    assert img.shape == (24, 32, 3) and img.dtype == np.uint8 and img.std() > 0
    with m.terrain_world(42, chunk_cells=2) as world:
        rect = (-20, 10, 50, 70)
        wh = world.hydrology(*rect, keep=('filled', 'accumulation'))
        ref = HY.analyse(ops, scene_heights(m, world.heightmap(*rect)))
        assert same(wh.filled, ref.filled) and same(wh.accumulation, ref.accumulation) and wh.basin is None
        assert int(wh.accumulation[R.is_outlet(50, 70)].sum()) == 50 * 70
        # drainage belongs to the rectangle: a sub-rectangle has outlets of its own
        sub = world.hydrology(-10, 20, 30, 40, keep=('accumulation',))
        assert not np.array_equal(sub.accumulation, wh.accumulation[10:40, 10:50])
    from tests.gpu_common import ERO
    with m.terrain_world(42, chunk_cells=2, erosion=ERO) as eroded:              # an eroded world: the eroded heights' drainage
        eh = eroded.hydrology(*rect, keep=('filled',))
        assert same(eh.filled, HY.analyse(ops, scene_heights(m, eroded.heightmap(*rect))).filled)
        assert not same(eh.filled, wh.filled)
    after = model_params(m)
    for k in before:
        for x, y in zip(before[k], after[k]):
            assert np.array_equal(x, y), k


# ---- 7. the command line ---------------------------------------------------------------------------------------------------------------
def test_command_line_writes_the_planes_and_the_painted_texture(ops, tmp_path):
    from PIL import Image
    H, W, q, seed = R.CASES[3]
    u8 = np.rint(R.terrain(H, W, q, seed) * 255).astype(np.uint8)
    tex = np.random.RandomState(9).randint(0, 256, (H, W, 3)).astype(np.uint8)
    Image.fromarray(u8).save(str(tmp_path / "h.png"))
    Image.fromarray(tex).save(str(tmp_path / "t.png"))
    prefix = str(tmp_path / "out")
    assert HY.main([str(tmp_path / "h.png"), prefix, "--texture", str(tmp_path / "t.png"), "--painted", str(tmp_path / "p.png"),
                    "--river-threshold", "30", "--plain"]) == 0
    want = HY.analyse(ops, u8)
    for k in HY.KEEP:
        assert same(np.load("%s.%s.npy" % (prefix, k)), getattr(want, k)), k
    painted = np.asarray(Image.open(str(tmp_path / "p.png")))
    assert same(painted, HY.paint(ops, tex, want, HY.Water(river_threshold=30))) and (painted != tex).any()
