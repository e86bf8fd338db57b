"""The viewshed on the MI355X (csrc/viewshed.hip, gan_heightmaps_amd/viewshed.py): the quantisation, the block maxima
and both forms of the sight lines through the raw entry points against the restatement of tests/viewshed_ref.py and against each
other, bit for bit -- the definition is integer, so there are no tolerances.  Every output lies in a canary canvas with a pitch of
W + 2; every input has a pitch of W + 3 whose padding is NaN (the heights) or 2^30 high (the quantised heights); the block
maxima, which are dense, are followed by canary words.  Then ``viewshed``, the model's and the world's methods, the paint, the
command line, and the refusals of the raw entry points."""
import numpy as np
import pytest

from oracle import step as ostep
from gan_heightmaps_amd import viewshed as VS
from tests import viewshed_ref as V
from tests.gpu_common import build_model, CANARY, Canvas, dev, model_params, ops, padded, same, SMALL      # noqa: F401  (dev, ops: the module-scoped fixtures)

pytestmark = pytest.mark.gpu

TAIL = 16                    # canary words behind the block maxima


def raw_quantise(dev, ops, h, height_scale):
    """-> zq through the raw entry point"""
    H, W = h.shape
    bufs = []
    try:
        d_h, ph = padded(dev, h, np.float32, 3, np.nan)
        bufs.append(d_h)
        zq = Canvas(dev, H, W, np.int32)
        bufs.append(zq.base)
        ops.viewshed_quantise(d_h, ph, H, W, height_scale, zq.ptr, zq.pitch)
        dev.sync()
        return zq.read()
    finally:
        dev.sync()
        for b in bufs:
            dev.free(b)


def raw_sight(dev, ops, zq, observers, target_q, accel, masked, steps=False):
    """-> (count, mask or None, top or None) through the raw entry points; steps: (the steps tested, None, top) instead"""
    H, W = zq.shape
    bufs = []
    try:
        d_z, pz = padded(dev, zq, np.int32, 3, 1 << 30)
        bufs.append(d_z)
        d_t = top = None
        if accel:
            elems = ops.viewshed_top_elems(H, W)
            whole = np.full(4 * (elems + TAIL), CANARY, np.uint8)
            d_t = dev.alloc(whole.nbytes)
            bufs.append(d_t)
            dev.h2d(d_t, whole)
            ops.viewshed_top(d_z, pz, H, W, d_t, elems)
        count = Canvas(dev, H, W, np.uint32)
        bufs.append(count.base)
        mask = None
        if masked:
            mask = Canvas(dev, H, W, np.uint32)
            bufs.append(mask.base)
        if steps:
            ops.viewshed_steps(d_z, pz, H, W, observers, target_q, accel, d_t, count.ptr, count.pitch)
        else:
            ops.viewshed_sight(d_z, pz, H, W, observers, target_q, accel, d_t, count.ptr, count.pitch,
                               None if mask is None else mask.ptr, 0 if mask is None else mask.pitch)
        dev.sync()
        if accel:
            dev.d2h(whole, d_t, whole.nbytes)
            assert (whole[4 * elems:] == CANARY).all(), "words behind the block maxima were written"
            top = whole[:4 * elems].view(np.int32).reshape((H + V.BLOCK - 1) // V.BLOCK, (W + V.BLOCK - 1) // V.BLOCK).copy()
        return count.read(), None if mask is None else mask.read(), top
    finally:
        dev.sync()
        for b in bufs:
            dev.free(b)


# ---- 1. the quantisation ----------------------------------------------------------------------------------------------------------
def test_the_quantisation_equals_the_restatement(dev, ops):
    for k, (H, W) in enumerate(V.SHAPES):
        for scale in (1.0, 64.0, 0.37, 65536.0):
            h = V.heights(H, W, 30 + k)
            h.flat[0], h.flat[-1] = 0.0, 1.0
            assert same(raw_quantise(dev, ops, h, scale), V.quantise(h, scale)), (H, W, scale)
    ties = (np.arange(64, dtype=np.float32) / np.float32(512)).reshape(4, 16)          # odd / 512 lies half way at height_scale 1
    assert same(raw_quantise(dev, ops, ties, 1.0), V.quantise(ties, 1.0))
    for name in V.CASES:                                                               # what the sight lines' cases start from
        c = V.case(name)
        assert same(raw_quantise(dev, ops, c["h"], c["height_scale"]), c["zq"]), name
    assert int(V.case("row4096")["zq"].max()) == 1 << 24


# ---- 2. the sight lines, both forms -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(V.CASES))
def test_both_forms_of_the_sight_lines_equal_the_restatement(dev, ops, name):
    c = V.case(name)
    want_count, want_mask = V.expected(name)
    masked = len(c["observers"]) <= 32
    assert (want_mask is not None) == masked
    plain, plain_mask, _ = raw_sight(dev, ops, c["zq"], c["observers"], c["target_q"], False, masked)
    fast, fast_mask, top = raw_sight(dev, ops, c["zq"], c["observers"], c["target_q"], True, masked)
    assert same(top, V.top(c["zq"])), name
    assert same(plain, want_count), (name, "plain")
    assert same(fast, want_count), (name, "accel")
    assert same(plain, fast)
    if masked:
        assert same(plain_mask, want_mask) and same(fast_mask, want_mask) and same(plain_mask, fast_mask)
        # a null mask changes nothing of the count
        assert same(raw_sight(dev, ops, c["zq"], c["observers"], c["target_q"], True, False)[0], want_count)
    else:
        from gan_heightmaps_amd._lib import GhmError
        with pytest.raises(GhmError, match="mask"):
            raw_sight(dev, ops, c["zq"], c["observers"], c["target_q"], False, True)
    # the case contains what it is for
    obs = c["observers"]
    if c["random"] and len(obs) == 8:
        H, W = c["zq"].shape
        assert {(int(o[0]), int(o[1])) for o in obs[:4]} == {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)}
        assert tuple(obs[6][:2]) == tuple(obs[7][:2]) and obs[6][2] != obs[7][2]                       # two in one cell
        assert {int(o[3]) for o in obs} >= {-1, 0, 1, 2500} and len({int(o[3]) for o in obs}) == 5      # and one that cuts the plane
        assert ((want_mask >> np.uint32(6)) & 1).sum() == 1 and ((want_mask >> np.uint32(4)) & 1).sum() in (2, 3, 4)
    if name == "graze":
        assert want_mask[2, 23] == 1 and (want_mask[2, 14:23] == 0).all()
    if name == "row4096":
        assert (want_mask[0, 3::2] == 1).all() and (want_mask[0, 2::2] == 0).all()
    if name == "many300":
        assert len(obs) > 2 * V.CHUNK                                                                  # three launches add up
    if name == "one":
        assert want_count[0, 0] == 2


def test_eye_and_target_heights_are_zero_and_not():
    pairs = {(int(V.case(n)["observers"][0][2]) > 0, V.case(n)["target_q"] > 0) for n in V.CASES if V.case(n)["random"]}
    assert {(False, False), (True, False), (True, True)} <= pairs


def test_the_accel_form_tests_a_subset_of_the_plain_forms_steps(dev, ops):
    for name in ("wide", "wide0", "row4096"):
        c = V.case(name)
        plain = raw_sight(dev, ops, c["zq"], c["observers"], c["target_q"], False, False, steps=True)[0].astype(np.int64)
        fast = raw_sight(dev, ops, c["zq"], c["observers"], c["target_q"], True, False, steps=True)[0].astype(np.int64)
        assert (fast <= plain).all() and 0 < fast.sum() < plain.sum(), name
    c = V.case("graze")                                   # a level plane below the eye: the line clears every block but the wall's
    o = c["observers"][:1]
    steps = raw_sight(dev, ops, c["zq"], o, 0, False, False, steps=True)[0]
    n = np.maximum(np.abs(np.arange(5)[:, None] - 2), np.abs(np.arange(64)[None, :] - 3))
    hidden = V.expected("graze")[1] & 1 == 0
    assert same(steps[~hidden], np.maximum(n - 1, 0).astype(np.uint32)[~hidden])          # a seen target costs n - 1 steps
    assert (steps[hidden] == 10).all()                                                   # a hidden one leaves at the wall, step 10


# ---- 3. viewshed, the model's methods, the paint ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_model(dev):
    m = build_model(ostep.default_cfg(**SMALL), 5, dev, dtype="f32", use_graph=False)
    cfg = ostep.default_cfg(**SMALL)
    for s in range(3):                       # non-trivial BatchNorm running statistics (the deterministic pass reads them)
        m.z_fn(ostep.synthetic_batch(4, cfg, seed=40 + s)[0])
    return m


def test_viewshed_equals_the_restatement(dev, ops):
    h = V.heights(97, 130, 41)
    sight = VS.Sight(eye_height=1.5, target_height=0.25, max_dist=70.0, height_scale=12.0)
    observers = [(110, -20), (150, 60, 3.0), (196, 109, None, 30.0), (100, -20, 0.0, 1000.0)]
    zq = V.quantise(h, 12.0)
    table = [(10, 0, 384, 4900), (50, 80, 768, 4900), (96, 129, 384, 900), (0, 0, 0, -1)]
    want_count, want_mask = V.viewshed(zq, table, 64)
    for accel in (None, False, True):
        got = VS.viewshed(ops, h[None], observers, sight, accel=accel, origin=(100, -20), keep='zq')
        assert same(got.count, want_count) and same(got.mask, want_mask) and same(got.zq, zq), accel
        assert got.accel is (VS.DEFAULT_ACCEL if accel is None else accel) and got.origin == (100, -20)
        assert got.observers.tolist() == [[110, -20, 384, 4900], [150, 60, 768, 4900], [196, 109, 384, 900], [100, -20, 0, -1]]
        for i in range(4):
            assert same(got.visible(i), V.visible_from(zq, table[i], 64))
        assert same(got.seen(), want_count > 0) and 0.05 < got.share() < 0.95
    u8 = (h * 255).astype(np.uint8)
    got = VS.viewshed(ops, u8, [(10, 0)])
    assert same(got.count, V.viewshed(V.quantise(u8.astype(np.float32) / np.float32(255), 64.0), [(10, 0, 512, -1)], 0)[0])
    many = [(int(r), int(c)) for r, c in zip(np.arange(40) * 2, np.arange(40) * 3)]
    got = VS.viewshed(ops, h, many, VS.Sight(height_scale=12.0))
    assert got.mask is None and same(got.count, V.viewshed(zq, [(r, c, 512, -1) for r, c in many], 0)[0])


def test_the_models_methods_and_the_paint(small_model, dev, ops):
    m = small_model
    before = model_params(m)
    h = V.heights(70, 90, 43)
    sight = VS.Sight(height_scale=10.0)
    observers = [(5, 5), (60, 80, 4.0)]
    want = VS.viewshed(ops, h, observers, sight)
    got = m.heightmap_viewshed(h, observers, sight, accel=False)
    assert same(got.count, want.count) and same(got.mask, want.mask) and got.accel is False
    seen = got.seen()
    assert 200 < seen.sum() < seen.size - 200
    tex = np.random.RandomState(3).randint(0, 256, (70, 90, 3)).astype(np.uint8)
    painted = m.paint_viewshed(tex, got, (0.0, 1.0, 0.0), opacity=1.0)
    assert painted.dtype == np.uint8 and same(painted[~seen], tex[~seen])                  # unpainted pixels keep their bits
    assert (painted[seen] == [0, 255, 0]).all()
    dark = m.paint_viewshed(tex, got, (1.0, 0.0, 0.0), opacity=1.0, hidden=True)
    assert same(dark[seen], tex[seen]) and (dark[~seen] == [255, 0, 0]).all()
    soft = m.paint_viewshed(tex, got)
    assert same(soft[~seen], tex[~seen]) and (soft[seen] != tex[seen]).any()
    assert same(soft, VS.paint(ops, tex, got, value_range=m.is_b_grayscale))
    ftex = np.random.RandomState(4).rand(3, 70, 90).astype(np.float32) * 2 - 1
    fp = m.paint_viewshed(ftex, got, hidden=True)
    assert same(fp[:, seen], ftex[:, seen]) and (fp[:, ~seen] != ftex[:, ~seen]).any()
    after = model_params(m)
    for k in before:
        for x, y in zip(before[k], after[k]):
            assert np.array_equal(x, y), k


# ---- 4. the world: two rectangles agree where they overlap ------------------------------------------------------------------------
@pytest.mark.parametrize("eroded", (False, True))
def test_two_rectangles_of_the_world_agree_bit_for_bit_on_their_overlap(small_model, dev, ops, eroded):
    from tests.gpu_common import ERO
    m = small_model
    kw = dict(erosion=ERO) if eroded else {}
    observers = [(2, 40), (20, 62, 6.0), (10, 75, 1.0, 25.0), (30, 45, None, 300.0)]        # inside both rectangles
    sight = VS.Sight(height_scale=24.0, target_height=0.5)
    with m.terrain_world(42, chunk_cells=2, **kw) as world:
        a = world.viewshed(-20, 10, 70, 90, observers, sight)
        b = world.viewshed(-5, 30, 60, 100, observers, sight, accel=False)
        assert a.origin == (-20, 10) and b.origin == (-5, 30) and same(a.observers, b.observers)
        assert a.observers[:, :2].tolist() == [list(o[:2]) for o in observers]
        ia, ib = (slice(15, 70), slice(20, 90)), (slice(0, 55), slice(0, 70))
        assert same(a.count[ia], b.count[ib]) and same(a.mask[ia], b.mask[ib])
        over = a.count[ia]
        assert (over > 0).sum() > 100 and (over < 4).sum() > 100                           # and there is something to agree on
        ref = VS.viewshed(ops, world._unit_height(-20, 10, 70, 90), observers, sight, origin=(-20, 10))
        assert same(a.count, ref.count) and same(a.mask, ref.mask)
        hm = world._unit_height(-20, 10, 70, 90)
        want = V.viewshed(V.quantise(hm, 24.0), a.observers - np.array([-20, 10, 0, 0], np.int32), sight.target_q)
        assert same(a.count, want[0]) and same(a.mask, want[1])
        with pytest.raises(ValueError, match="observer"):
            world.viewshed(-5, 30, 60, 100, [(-10, 40)])


# ---- 5. the command line ------------------------------------------------------------------------------------------------------------
def test_command_line_writes_the_viewshed(ops, tmp_path, capsys):
    h = V.heights(70, 90, 43)
    np.save(str(tmp_path / "h.npy"), h)
    tex = np.random.RandomState(3).randint(0, 256, h.shape + (3,)).astype(np.uint8)
    from gan_heightmaps_amd.util import read_image, save_png
    save_png(str(tmp_path / "t.png"), tex)
    args = [str(tmp_path / "h.npy"), str(tmp_path / "o.npz"), "--from", "5,5", "--from", "60,80,4,50", "--eye", "1.5", "--target", "0.5",
            "--height-scale", "10", "--texture", str(tmp_path / "t.png"), "--painted", str(tmp_path / "p.png"), "--hidden", "--opacity",
            "1", "--colour", "1,0,0", "--plain"]
    assert VS.main(args) == 0
    want = VS.viewshed(ops, h, [(5, 5), (60, 80, 4.0, 50.0)], VS.Sight(1.5, 0.5, None, 10.0))
    z = np.load(str(tmp_path / "o.npz"))
    assert same(z["count"], want.count) and same(z["mask"], want.mask) and same(z["observers"], want.observers)
    seen = want.seen()
    assert capsys.readouterr().out.startswith("2 observers see %d of %d cells" % (seen.sum(), seen.size)) and 100 < seen.sum() < seen.size - 100
    painted = read_image(str(tmp_path / "p.png"))
    assert same(painted[seen], tex[seen]) and (painted[~seen] == [255, 0, 0]).all()
    assert VS.main(args[:1] + [str(tmp_path / "o.png")] + args[2:12]) == 0
    assert same(read_image(str(tmp_path / "o.png")), seen.astype(np.uint8) * np.uint8(255))


# ---- 6. refusals of the raw entry points ------------------------------------------------------------------------------------------
def test_refusals_of_the_entry_points_leave_every_byte_alone(dev, ops):
    from gan_heightmaps_amd._lib import GhmError
    H, W = 4, 8
    src = dev.alloc(4096)
    dev.memset_zero(src, 4096)
    zq, count, mask = Canvas(dev, H, W, np.int32), Canvas(dev, H, W, np.uint32), Canvas(dev, H, W, np.uint32)
    top = Canvas(dev, 1, 1, np.int32)
    p = count.pitch
    one = [(1, 2, 0, -1)]

    def do_quantise(h=src, ph=W, Hh=H, Ww=W, hs=64.0, z=zq.ptr, pz=p):
        ops.viewshed_quantise(h, ph, Hh, Ww, hs, z, pz)

    def do_top(z=src, pz=W, Hh=H, Ww=W, t=top.ptr, elems=1):
        ops.viewshed_top(z, pz, Hh, Ww, t, elems)

    def do_sight(z=src, pz=W, Hh=H, Ww=W, obs=one, tq=0, accel=False, t=None, c=count.ptr, pc=p, m=mask.ptr, pm=p):
        ops.viewshed_sight(z, pz, Hh, Ww, obs, tq, accel, t, c, pc, m, pm)

    def do_steps(z=src, pz=W, Hh=H, Ww=W, obs=one, tq=0, accel=False, t=None, c=count.ptr, pc=p):
        ops.viewshed_steps(z, pz, Hh, Ww, obs, tq, accel, t, c, pc)

    try:
        for kw, match in ((dict(h=None), "null"), (dict(z=None), "null"), (dict(ph=W - 1), "pitch"), (dict(pz=W - 1), "pitch"),
                          (dict(Hh=0), "out of range"), (dict(Hh=4 * 65535 + 1, Ww=1), "out of range"),
                          (dict(Hh=1 << 16, Ww=1 << 15, ph=1 << 15, pz=1 << 15), "out of range"), (dict(Hh=1 << 15, pz=1 << 16), "pitch"),
                          (dict(hs=0.0), "height_scale"), (dict(hs=65537.0), "height_scale"), (dict(hs=float("nan")), "height_scale"),
                          (dict(hs=-1.0), "height_scale")):
            with pytest.raises(GhmError, match=match):
                do_quantise(**kw)
        for kw, match in ((dict(z=None), "null"), (dict(t=None), "null"), (dict(pz=W - 1), "pitch"), (dict(Ww=0), "out of range"),
                          (dict(elems=2), "elements"), (dict(elems=0), "elements")):
            with pytest.raises(GhmError, match=match):
                do_top(**kw)
        for do in (do_sight, do_steps):
            for kw, match in ((dict(z=None), "null"), (dict(c=None), "null"), (dict(pz=W - 1), "pitch"), (dict(pc=W - 1), "pitch"),
                              (dict(Hh=0), "out of range"), (dict(Hh=1 << 16, Ww=1 << 15, pz=1 << 15, pc=1 << 15), "out of range"),
                              (dict(obs=np.zeros((0, 4), np.int32)), "null"), (dict(obs=one * 4097), "observers"),
                              (dict(obs=[(4, 0, 0, -1)]), "outside"), (dict(obs=[(0, 8, 0, -1)]), "outside"),
                              (dict(obs=[(-1, 0, 0, -1)]), "outside"), (dict(obs=one + [(0, 0, -1, -1)]), "eye_q"),
                              (dict(tq=-1), "target_q"), (dict(accel=True), "accel")):
                with pytest.raises(GhmError, match=match):
                    do(**kw)
        with pytest.raises(GhmError, match="mask"):
            do_sight(obs=one * 33)
        with pytest.raises(GhmError, match="pitch"):
            do_sight(pm=W - 1)
        with pytest.raises(ValueError, match="table"):
            do_sight(obs=[(1, 2, 0)])
        with pytest.raises(ValueError, match="32 bits"):
            do_sight(obs=[(1, 2, 1 << 31, -1)])
        assert ops.viewshed_top_elems(33, 65) == 3 * 5 and ops.viewshed_top_elems(16, 16) == 1 and ops.viewshed_top_elems(17, 1) == 2
        assert ops.viewshed_top_elems(0, 5) == -1 and ops.viewshed_top_elems(1 << 16, 1 << 15) == -1
        assert ops.viewshed_top_elems(4 * 65535 + 1, 1) == -1 and ops.viewshed_top_elems(4 * 65535, 1) == 16384
        dev.sync()
        for cv in (zq, count, mask, top):                 # the canaries around the planes, and the planes themselves
            assert (cv.read().view(np.uint8) == CANARY).all()
    finally:
        dev.sync()
        for b in (src, zq.base, count.base, mask.base, top.base):
            dev.free(b)
