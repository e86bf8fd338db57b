"""The sunlight on the MI355X (csrc/sunlight.hip, gan_heightmaps_amd/sunlight.py): both forms of the sun kernel
through the raw entry points against the restatement of tests/sunlight_ref.py and against each other, bit for bit -- the definition
is integer, so there are no tolerances.  Every output lies in a canary canvas with a pitch of W + 2; the quantised heights have a
pitch of W + 3 whose padding holds a wall 2^24 high that would shade the plane if it were read; the block maxima and the zmax word
are followed by canary words.  Then ``sunlight``, the model's and the world's methods, the paint, the command line, and the
refusals of the raw entry points."""
import numpy as np
import pytest

from oracle import step as ostep
from gan_heightmaps_amd import sunlight as SL
from tests import sunlight_ref as R
from tests.gpu_common import build_model, CANARY, Canvas, dev, model_params, ops, padded, same, SMALL      # noqa: F401  (dev, ops: the module-scoped fixtures)

pytestmark = pytest.mark.gpu

TAIL = 16                    # canary words behind the block maxima and behind the zmax word


def raw_sun(dev, ops, zq, table, target_q, form, masked, steps=False):
    """-> dict(lit, mask or None, hours_q, energy, top, zmax) through the raw entry points; steps: lit holds the steps tested and
    the other planes come back as they went in"""
    H, W = zq.shape
    bufs = []
    try:
        d_z, pz = padded(dev, zq, np.int32, 3, 1 << 24)
        bufs.append(d_z)
        elems = ops.viewshed_top_elems(H, W)
        whole = np.full(4 * (elems + TAIL), CANARY, np.uint8)
        word = np.full(4 * (1 + TAIL), CANARY, np.uint8)
        d_t, d_x = dev.alloc(whole.nbytes), dev.alloc(word.nbytes)
        bufs += [d_t, d_x]
        dev.h2d(d_t, whole)
        dev.h2d(d_x, word)
        ops.viewshed_top(d_z, pz, H, W, d_t, elems)
        ops.sunlight_zmax(d_t, elems, d_x)
        cv = {k: Canvas(dev, H, W, np.uint32) for k in ("lit", "hours_q", "energy")}
        if masked:
            cv["mask"] = Canvas(dev, H, W, np.uint32)
        bufs += [c.base for c in cv.values()]
        accel = form == 'accel'
        if steps:
            ops.sunlight_steps(d_z, pz, H, W, table, target_q, accel, d_t if accel else None, d_x, cv["lit"].ptr, cv["lit"].pitch)
        else:
            m = cv.get("mask")
            ops.sunlight_sun(d_z, pz, H, W, table, target_q, accel, d_t if accel else None, d_x, cv["lit"].ptr, cv["lit"].pitch,
                             None if m is None else m.ptr, 0 if m is None else m.pitch, cv["hours_q"].ptr, cv["hours_q"].pitch,
                             cv["energy"].ptr, cv["energy"].pitch)
        dev.sync()
        dev.d2h(whole, d_t, whole.nbytes)
        dev.d2h(word, d_x, word.nbytes)
        assert (whole[4 * elems:] == CANARY).all(), "words behind the block maxima were written"
        assert (word[4:] == CANARY).all(), "words behind zmax were written"
        out = {k: c.read() for k, c in cv.items()}
        out.setdefault("mask", None)
        out["top"] = whole[:4 * elems].view(np.int32).reshape((H + R.BLOCK - 1) // R.BLOCK, (W + R.BLOCK - 1) // R.BLOCK).copy()
        out["zmax"] = int(word[:4].view(np.int32)[0])
        return out
    finally:
        dev.sync()
        for b in bufs:
            dev.free(b)


# ---- 1. the sun kernel, both forms ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_both_forms_of_the_sun_kernel_equal_the_restatement(dev, ops, name):
    c = R.case(name)
    want = R.expected(name)
    masked = len(c["table"]) <= 32
    assert (want["mask"] is not None) == masked
    got = {form: raw_sun(dev, ops, c["zq"], c["table"], c["target_q"], form, masked) for form in SL.FORMS}
    for form in SL.FORMS:
        assert same(got[form]["top"], R.top(c["zq"])) and got[form]["zmax"] == int(c["zq"].max()), (name, form)
        for k in R.PLANES:
            if want[k] is not None:
                assert same(got[form][k], want[k]), (name, form, k)
    assert R.same_planes(got['plain'], got['accel'])
    if masked:
        # a null mask changes nothing of the other planes
        bare = raw_sun(dev, ops, c["zq"], c["table"], c["target_q"], 'accel', False)
        assert all(same(bare[k], want[k]) for k in ("lit", "hours_q", "energy"))
    else:
        from gan_heightmaps_amd._lib import GhmError
        with pytest.raises(GhmError, match="mask"):
            raw_sun(dev, ops, c["zq"], c["table"], c["target_q"], 'plain', True)
    # the case contains what it is for
    if name == "wall":
        at = R.WALL_AT - R.WALL_STEPS
        assert want["mask"][1, at] & 1 == 1 and want["mask"][3, at] & 1 == 0
    if name == "row4096":
        assert int(c["zq"].max()) == 1 << 24 and len(np.unique(want["lit"])) >= 2
    if name == "many300":
        assert len(c["table"]) > 4 * R.CHUNK                               # five launches add up
    if name == "many33":
        assert len(c["table"]) == 33 and want["mask"] is None


def test_the_accel_form_tests_a_subset_of_the_plain_forms_steps(dev, ops):
    for name in ("1x9", "17x33", "37x70", "70x37", "65x130", "wall", "row4096", "many300"):
        c = R.case(name)
        plain = raw_sun(dev, ops, c["zq"], c["table"], c["target_q"], 'plain', False, steps=True)
        fast = raw_sun(dev, ops, c["zq"], c["table"], c["target_q"], 'accel', False, steps=True)
        for got in (plain, fast):                                          # nothing but the steps is written
            assert (got["hours_q"].view(np.uint8) == CANARY).all() and (got["energy"].view(np.uint8) == CANARY).all()
        p, f = plain["lit"].astype(np.int64), fast["lit"].astype(np.int64)
        assert np.array_equal(p, R.expected_steps(name)), name
        assert (f <= p).all(), name
        if name in ("37x70", "70x37", "65x130", "many300"):
            assert 0 < f.sum() < p.sum(), name


# ---- 2. sunlight, the model's methods, the paint ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_model(dev):
    m = build_model(ostep.default_cfg(**SMALL), 5, dev, dtype="f32", use_graph=False)
    cfg = ostep.default_cfg(**SMALL)
    for s in range(3):                       # non-trivial BatchNorm running statistics (the deterministic pass reads them)
        m.z_fn(ostep.synthetic_batch(4, cfg, seed=40 + s)[0])
    return m


def test_sunlight_equals_the_restatement(dev, ops):
    h = R.V.heights(70, 90, 41)
    sun = SL.Sun(((10, 12), (100, 20, 2.0), (250, 8, 0.5), (300, 40)), target_height=0.25, height_scale=12.0)
    zq = R.quantise(h, 12.0)
    want = R.sunlight(zq, R.table(sun.positions), 64)
    assert 0.2 < (want["lit"] < 4).mean() < 0.95
    for form in (None,) + SL.FORMS:
        got = SL.sunlight(ops, h[None], sun, form=form, origin=(100, -20), keep='zq')
        assert all(same(getattr(got, k), want[k]) for k in R.PLANES) and same(got.zq, zq), form
        assert got.form == (SL.DEFAULT_FORM if form is None else form) and got.origin == (100, -20) and got.exact and got.sun is sun
        for i in range(4):
            assert same(got.shaded(i), (want["mask"] >> np.uint32(i)) & 1 == 0)
        assert same(got.hours(), want["hours_q"] / 256.0) and 0 < got.share()["mean_exposure"] < 1.5
    u8 = (h * 255).astype(np.uint8)
    got = SL.sunlight(ops, u8, SL.Sun(((45, 15),)))
    assert same(got.lit, R.sunlight(R.quantise(u8.astype(np.float32) / np.float32(255), 64.0), R.table([(45, 15)]), 0)["lit"])
    day = SL.Day(step_minutes=20).sun(height_scale=12.0)                   # 34 positions: no mask
    got = SL.sunlight(ops, h, day)
    want = R.sunlight(zq, day.table(), 0)
    assert got.mask is None and len(day) > 32 and all(same(getattr(got, k), want[k]) for k in ("lit", "hours_q", "energy"))


def test_the_models_methods_and_the_paint(small_model, dev, ops):
    m = small_model
    before = model_params(m)
    h = R.V.heights(70, 90, 43)
    sun = SL.Sun(((90, 10, 3.0), (200, 15, 3.0)), height_scale=10.0)
    want = SL.sunlight(ops, h, sun)
    got = m.heightmap_sunlight(h, sun, form='plain')
    assert all(same(getattr(got, k), getattr(want, k)) for k in R.PLANES) and got.form == 'plain'
    assert m.heightmap_sunlight(h).sun == SL.Day().sun()
    dark = ~got.mask_hours(4)
    assert 200 < dark.sum() < dark.size - 200
    tex = np.random.RandomState(3).randint(0, 256, (70, 90, 3)).astype(np.uint8)
    painted = m.paint_sunlight(tex, got, 4, (0.0, 0.0, 1.0), opacity=1.0)
    assert painted.dtype == np.uint8 and same(painted[~dark], tex[~dark])                  # unpainted pixels keep their bits
    assert (painted[dark] == [0, 0, 255]).all()
    soft = m.paint_sunlight(tex, got, 4)
    assert same(soft[~dark], tex[~dark]) and (soft[dark] != tex[dark]).any()
    assert same(soft, SL.paint(ops, tex, got, 4, value_range=m.is_b_grayscale))
    ftex = np.random.RandomState(4).rand(3, 70, 90).astype(np.float32) * 2 - 1
    fp = m.paint_sunlight(ftex, got, 4)
    assert same(fp[:, ~dark], ftex[:, ~dark]) and (fp[:, dark] != ftex[:, dark]).any()
    after = model_params(m)
    for k in before:
        for x, y in zip(before[k], after[k]):
            assert np.array_equal(x, y), k


# ---- 3. the world: two rectangles agree where they overlap --------------------------------------------------------------------------
def test_two_rectangles_of_the_world_agree_bit_for_bit_on_their_overlap(small_model, dev, ops):
    m = small_model
    sun = SL.Sun(((90, 12), (200, 15, 0.5), (315, 20, 2.0), (10, 30)), height_scale=24.0)
    reach = sun.reach
    assert reach == R.reach(sun.table(), 24.0) and 100 < reach < 130
    with m.terrain_world(42, chunk_cells=2) as world:
        a = world.sunlight(-20, 10, 70, 90, sun)
        b = world.sunlight(-5, 30, 60, 100, sun, form='plain')
        assert a.exact and b.exact and a.origin == (-20, 10) and b.origin == (-5, 30) and a.shape == (70, 90) and b.shape == (60, 100)
        ia, ib = (slice(15, 70), slice(20, 90)), (slice(0, 55), slice(0, 70))
        for k in R.PLANES:
            assert same(getattr(a, k)[ia], getattr(b, k)[ib]), k
        over = a.lit[ia]
        assert len(np.unique(over)) >= 2                                   # and there is something to agree on
        hm = world._unit_height(-20 - reach, 10 - reach, 70 + 2 * reach, 90 + 2 * reach)
        want = R.sunlight(R.quantise(hm, 24.0), sun.table(), 0)
        for k in R.PLANES:
            assert same(getattr(a, k), want[k][reach:-reach, reach:-reach]), k
        # a capped margin: the planes belong to the rectangle grown by the cap
        c = world.sunlight(-20, 10, 70, 90, sun, max_margin=5)
        ref = SL.sunlight(ops, world._unit_height(-25, 5, 80, 100), sun)
        assert not c.exact and c.origin == (-20, 10) and all(same(getattr(c, k), getattr(ref, k)[5:-5, 5:-5]) for k in R.PLANES)
        with pytest.raises(ValueError, match="max_margin"):
            world.sunlight(-20, 10, 70, 90, sun, max_margin=-1)


# ---- 4. the command line --------------------------------------------------------------------------------------------------------------
def test_command_line_writes_the_sunlight(ops, tmp_path, capsys):
    h = R.V.heights(70, 90, 43)
    np.save(str(tmp_path / "h.npy"), h)
    tex = np.random.RandomState(3).randint(0, 256, h.shape + (3,)).astype(np.uint8)
    from gan_heightmaps_amd.util import read_image, save_png
    save_png(str(tmp_path / "t.png"), tex)
    args = [str(tmp_path / "h.npy"), str(tmp_path / "o.npz"), "--sun", "90,10,3", "--sun", "-160,15,3", "--target", "0.5",
            "--height-scale", "10", "--texture", str(tmp_path / "t.png"), "--painted", str(tmp_path / "p.png"), "--max-hours", "4",
            "--opacity", "1", "--colour", "1,0,0", "--plain"]
    assert SL.main(args) == 0
    want = SL.sunlight(ops, h, SL.Sun(((90, 10, 3), (-160, 15, 3)), 0.5, 10.0))
    z = np.load(str(tmp_path / "o.npz"))
    assert all(same(z[k], getattr(want, k)) for k in R.PLANES) and same(z["table"], want.sun.table())
    assert capsys.readouterr().out.startswith("2 positions light %d of %d cells" % ((want.lit > 0).sum(), want.lit.size))
    dark = ~want.mask_hours(4)
    assert 100 < dark.sum() < dark.size - 100
    painted = read_image(str(tmp_path / "p.png"))
    assert same(painted[~dark], tex[~dark]) and (painted[dark] == [255, 0, 0]).all()
    assert SL.main([args[0], str(tmp_path / "o.png"), "--day", "--latitude", "50", "--height-scale", "10", "--accel"]) == 0
    day = SL.sunlight(ops, h, SL.Day(latitude=50).sun(height_scale=10.0))
    total = int(day.sun.table()[:, 8].sum())
    assert same(read_image(str(tmp_path / "o.png")), np.rint(day.hours_q * (255.0 / total)).astype(np.uint8))


# ---- 5. refusals of the raw entry points ----------------------------------------------------------------------------------------------
def test_refusals_of_the_entry_points_leave_every_byte_alone(dev, ops):
    from gan_heightmaps_amd._lib import GhmError
    H, W = 4, 8
    src = dev.alloc(4096)
    dev.memset_zero(src, 4096)
    cv = [Canvas(dev, H, W, np.uint32) for _ in range(4)]
    lit, mask, hours, energy = cv
    word = Canvas(dev, 1, 1, np.int32)
    p = lit.pitch
    one = [list(R.position(30, 20))]

    def row(**kw):
        names = ("rows", "gmaj", "gmin", "m_q", "rise_q", "s_y", "s_x", "s_z", "w_q")
        r = list(one[0])
        for k, v in kw.items():
            r[names.index(k)] = v
        return [r]

    def do_sun(z=src, pz=W, Hh=H, Ww=W, tab=one, tq=0, accel=False, t=None, x=src, l=lit.ptr, pl=p, m=mask.ptr, pm=p, h=hours.ptr, ph=p,
               e=energy.ptr, pe=p):
        ops.sunlight_sun(z, pz, Hh, Ww, tab, tq, accel, t, x, l, pl, m, pm, h, ph, e, pe)

    def do_steps(z=src, pz=W, Hh=H, Ww=W, tab=one, tq=0, accel=False, t=None, x=src, l=lit.ptr, pl=p):
        ops.sunlight_steps(z, pz, Hh, Ww, tab, tq, accel, t, x, l, pl)

    try:
        for do in (do_sun, do_steps):
            for kw, match in ((dict(z=None), "null"), (dict(l=None), "null"), (dict(x=None), "null"), (dict(pz=W - 1), "pitch"),
                              (dict(pl=W - 1), "pitch"), (dict(Hh=0), "out of range"),
                              (dict(Hh=1 << 16, Ww=1 << 15, pz=1 << 15, pl=1 << 15), "out of range"),
                              (dict(tab=np.zeros((0, 9), np.int64)), "null"), (dict(tab=one * 4097), "positions"),
                              (dict(tab=row(rise_q=0)), "rise_q"), (dict(tab=row(rise_q=(1 << 40) + 1)), "rise_q"),
                              (dict(tab=row(m_q=-1)), "m_q"), (dict(tab=row(m_q=65537)), "m_q"), (dict(tab=row(gmin=0)), "minor sign"),
                              (dict(tab=row(m_q=0)), "minor sign"), (dict(tab=row(rows=2)), "axis"), (dict(tab=row(gmaj=0)), "axis"),
                              (dict(tab=row(gmin=2)), "axis"), (dict(tab=row(s_y=16385)), "unit vector"), (dict(tab=row(s_z=-1)), "unit vector"),
                              (dict(tab=row(w_q=-1)), "w_q"), (dict(tab=row(w_q=(1 << 17) + 1)), "w_q"),
                              (dict(tab=row(w_q=1 << 16) * 3), "sum to"), (dict(tq=-1), "target_q"), (dict(tq=(1 << 24) + 1), "target_q"),
                              (dict(accel=True), "accel")):
                with pytest.raises(GhmError, match=match):
                    do(**kw)
        for kw, match in ((dict(h=None), "null"), (dict(e=None), "null"), (dict(ph=W - 1), "pitch"), (dict(pe=W - 1), "pitch"),
                          (dict(pm=W - 1), "pitch"), (dict(tab=one * 33), "mask")):
            with pytest.raises(GhmError, match=match):
                do_sun(**kw)
        with pytest.raises(ValueError, match="table"):
            do_sun(tab=[[1, 1, 0, 0, 1, 0, 0, 0]])
        for args, match in (((None, 1, word.ptr), "null"), ((src, 1, None), "null"), ((src, 0, word.ptr), "block maxima"),
                            ((src, 1 << 31, word.ptr), "block maxima")):
            with pytest.raises(GhmError, match=match):
                ops.sunlight_zmax(*args)
        dev.sync()
        for c in cv + [word]:                             # the canaries around the planes, and the planes themselves
            assert (c.read().view(np.uint8) == CANARY).all()
    finally:
        dev.sync()
        for b in [src, word.base] + [c.base for c in cv]:
            dev.free(b)
