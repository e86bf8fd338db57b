"""The host side of the sunlight (gan_heightmaps_amd/sunlight.py) without a device: the validation of Sun and Day, the
Sunlight's methods and writers, the command lines, and -- over tests/fake_device.py -- that ``sunlight`` and ``paint`` send their
launches inside one scratch and free it, on success and on failure.  Last, the device source of both forms compiled for the CPU
(tests/sunlight_host/harness.cpp) as a stand-alone program under the address and undefined-behaviour sanitizers."""
import numpy as np
import pytest

from gan_heightmaps_amd import sunlight as SL
from tests import sunlight_ref as R


# ---- Sun and Day ----------------------------------------------------------------------------------------------------------------------
def test_sun_validation():
    s = SL.Sun(((0, 10), (90.0, 45, 2)))
    assert s == SL.Sun([(0.0, 10.0, 1.0), (90, 45.0, 2.0)]) and hash(s) == hash(SL.Sun(((0, 10), (90, 45, 2)))) and len(s) == 2
    assert s.positions == ((0.0, 10.0, 1.0), (90.0, 45.0, 2.0)) and s.target_height == 0.0 and s.height_scale == 64.0 and s.target_q == 0
    assert SL.Sun(((np.float32(30), np.int64(20)),), np.float32(0.5), np.int64(8)).target_q == 128
    with pytest.raises(Exception):
        s.height_scale = 2.0                                               # frozen
    for kw, match in ((dict(positions=()), "positions"), (dict(positions=None), "positions"), (dict(positions=((0, 10),) * 4097), "positions"),
                      (dict(positions=((0,),)), "positions"), (dict(positions=((0, 10, 1, 2),)), "positions"), (dict(positions=(5,)), "positions"),
                      (dict(positions=((0, 0),)), "elevation"), (dict(positions=((0, -5),)), "elevation"), (dict(positions=((0, 90.5),)), "elevation"),
                      (dict(positions=((0, float("nan")),)), "elevation"), (dict(positions=(("n", 10),)), "azimuth"),
                      (dict(positions=((float("inf"), 10),)), "azimuth"), (dict(positions=((0, 10, -1),)), "hours"),
                      (dict(positions=((0, 10, 513),)), "hours"), (dict(positions=((0, 10, 300), (5, 10, 300))), "hours"),
                      (dict(positions=((0, 10, "x"),)), "hours"), (dict(target_height=-1), "target_height"),
                      (dict(target_height=65537), "target_height"), (dict(height_scale=0), "height_scale"), (dict(height_scale=65537), "height_scale"),
                      (dict(height_scale="x"), "height_scale")):
        with pytest.raises(ValueError, match=match):
            SL.Sun(**dict(dict(positions=((0, 10),)), **kw))
    assert len(SL.Sun(((0, 10, 0.125),) * 4096)) == 4096 and SL.Sun(((0, 10, 512),)).table()[0, 8] == SL.MAX_WEIGHT
    assert SL.FORMS == ('plain', 'accel') and SL.DEFAULT_FORM in SL.FORMS and SL.MAX_POSITIONS == R.MAX_POSITIONS and SL.MAX_WEIGHT == R.MAX_WEIGHT


def test_the_table_is_the_restatements():
    s = SL.Sun(R.ALL_SUNS, 0.25, 8.0)
    t = s.table()
    assert t.dtype == np.int64 and t.shape == (len(R.ALL_SUNS), R.FIELDS) and np.array_equal(t, R.table(R.ALL_SUNS))
    assert s.reach == R.reach(t, 8.0) == 256 * 2048 + 1                    # the sun whose rise_q clamps to 1
    assert SL.Sun(((90, 20),), height_scale=4.0).reach == 12 and s.level == int((t[:, 8] * t[:, 7]).sum())
    rng = np.random.RandomState(5)
    many = [(float(rng.uniform(-720, 720)), float(rng.uniform(0.01, 90)), float(rng.uniform(0, 1))) for _ in range(200)]
    assert np.array_equal(SL.Sun(many).table(), R.table(many))


def test_day():
    d = SL.Day()
    assert (d.latitude, d.declination, d.step_minutes, d.min_elevation) == (45.0, 0.0, 30, 2.0) and d == SL.Day(45, 0, 30, 2)
    for lat in (0.0, 30.0, 45.0, 60.0):                                    # noon at the equinox: due south, 90 - latitude up
        az, el = SL.Day(latitude=lat).position(12)
        assert abs(el - (90 - lat)) < 1e-9 and (lat == 0 or min(az, 360 - az) < 1e-9), lat
    for lat in (0.0, 45.0, 60.0):                                          # sunrise and sunset at the equinox: due east and west
        az, el = SL.Day(latitude=lat).position(6)
        assert abs(el) < 1e-9 and abs(az - 90) < 1e-9
        az, el = SL.Day(latitude=lat).position(18)
        assert abs(el) < 1e-9 and abs(az - 270) < 1e-9
    # due south is down the rows (azimuth 0 points along +y), east along the columns (azimuth 90 along +x)
    assert R.position(*SL.Day().position(12))[:3] == (1, 1, 0) and R.position(*SL.Day().position(6.5))[:2] == (0, 1)
    at = d.positions()
    assert len(at) == 24 and all(h == 0.5 for _, _, h in at) and min(e for _, e, _ in at) >= 2.0 and max(e for _, e, _ in at) < 45.0
    assert [round(a, 6) for a, _, _ in at] == [round((360 - a) % 360, 6) for a, _, _ in at[::-1]]      # the afternoon mirrors the morning
    summer, winter = SL.Day(declination=23.44).positions(), SL.Day(declination=-23.44).positions()
    assert len(summer) > len(at) > len(winter) and abs(SL.Day(declination=23.44).position(12)[1] - 68.44) < 1e-9
    s = d.sun(height_scale=32.0, target_height=1.0)
    assert isinstance(s, SL.Sun) and s.positions == at and s.height_scale == 32.0 and s.target_q == 256 and s.table()[:, 8].sum() == 24 * 128
    for kw in (dict(latitude=91), dict(latitude="n"), dict(declination=-91), dict(step_minutes=0), dict(step_minutes=7), dict(step_minutes=1.5),
               dict(step_minutes=1440), dict(min_elevation=0), dict(min_elevation=91)):
        with pytest.raises(ValueError, match=list(kw)[0]):
            SL.Day(**kw)
    with pytest.raises(ValueError, match="min_elevation"):
        SL.Day(latitude=80, declination=-23.44).sun()                      # the polar night
    assert len(SL.Day(step_minutes=1).sun()) <= 1440


# ---- Sunlight ---------------------------------------------------------------------------------------------------------------------------
def hand_made(n=2, **kw):
    sun = SL.Sun(tuple((30.0 * i, 30.0, 1.5) for i in range(n)))
    planes = dict(lit=np.array([[0, 1, 2], [2, 2, 1]], np.uint32), mask=np.array([[0, 2, 3], [3, 3, 1]], np.uint32),
                  hours_q=np.array([[0, 384, 768], [768, 768, 384]], np.uint32), energy=np.array([[0, 1 << 22, 3 << 22], [1 << 21, 0, 7]], np.uint32))
    planes.update(kw)
    return SL.Sunlight(sun=sun, origin=(10, -20), form='plain', **planes)


def test_sunlight_methods():
    s = hand_made()
    assert s.shape == (2, 3) and s.origin == (10, -20) and len(s) == 2 and s.exact is True and s.zq is None and "2 positions" in repr(s)
    assert s.hours().dtype == np.float64 and s.hours().tolist() == [[0, 1.5, 3], [3, 3, 1.5]]
    assert s.insolation().tolist()[0] == [0.0, 1.0, 3.0] and s.insolation()[1, 0] == 0.5
    level = s.sun.level
    assert level == 2 * 384 * 8192 and np.array_equal(s.exposure(), s.energy / float(level))
    assert s.shaded(0).tolist() == [[True, True, False], [False, False, False]] and s.shaded(1).tolist() == [[True, False, False], [False, False, True]]
    assert s.shaded(0).dtype == bool and s.mask_hours(2).tolist() == [[False, False, True], [True, True, False]] and s.mask_hours(0).all()
    assert s.mask_hours(1.5).sum() == 5
    sh = s.share()
    assert sh["lit"] == 5 / 6 and sh["mean_hours"] == 2.0 and sh["max_hours"] == 3.0 and sh["mean_exposure"] > 0
    for bad in (2, -1, 0.5):
        with pytest.raises(ValueError, match="position"):
            s.shaded(bad)
    with pytest.raises(ValueError, match="no mask is kept"):
        hand_made(33, mask=None).shaded(0)
    with pytest.raises(ValueError, match="min_hours"):
        s.mask_hours(-1)
    c = s.crop(0, 1, 2, 2, exact=False)
    assert c.shape == (2, 2) and c.origin == (10, -19) and c.exact is False and c.lit.tolist() == [[1, 2], [2, 1]] and c.mask.flags.c_contiguous
    assert hand_made(33, mask=None).crop(0, 0, 1, 1).mask is None


def test_save_round_trips(tmp_path):
    s = hand_made()
    s.save(str(tmp_path / "s.npz"))
    z = np.load(str(tmp_path / "s.npz"))
    for k in ("lit", "mask", "hours_q", "energy"):
        assert np.array_equal(z[k], getattr(s, k)) and z[k].dtype == np.uint32, k
    assert z["origin"].tolist() == [10, -20] and np.array_equal(z["table"], s.sun.table()) and bool(z["exact"])
    hand_made(33, mask=None).save(str(tmp_path / "n.npz"))
    assert "mask" not in np.load(str(tmp_path / "n.npz")).files
    s.save(str(tmp_path / "s.png"))
    from gan_heightmaps_amd.util import read_image
    assert read_image(str(tmp_path / "s.png")).tolist() == [[0, 128, 255], [255, 255, 128]]
    with pytest.raises(ValueError, match="npz or .png"):
        s.save(str(tmp_path / "s.tif"))


# ---- sunlight and paint over the fake device -----------------------------------------------------------------------------------------------
def recording(fail=None):
    from tests.fake_device import RecordingOps
    from tests.test_contour_host import Counting

    class Ops(RecordingOps):
        def viewshed_top_elems(self, H, W):
            return ((H + 15) // 16) * ((W + 15) // 16)

        def __getattr__(self, name):
            rec = RecordingOps.__getattr__(self, name)
            if name == fail:
                def boom(*a, **k):
                    raise RuntimeError("the launch failed")
                return boom
            return rec

    return Ops(Counting())


def test_sunlight_sends_its_launches_inside_one_scratch():
    h = R.case("37x70")["h"]
    H, W = h.shape
    ops = recording()
    sun = SL.Sun(((10, 20), (200, 5, 0.5)), 0.5, 16.0)
    got = SL.sunlight(ops, h, sun, form='accel', origin=(-5, 9))
    assert ops.dev.live == 0 and ops.dev.sizes == [4 * H * W] * 6 + [4 * 3 * 5, 4]
    assert [c[0] for c in ops.calls] == ["viewshed_quantise", "viewshed_top", "sunlight_zmax", "sunlight_sun"]
    q, s = ops.calls[0][1], ops.calls[3][1]
    assert q[1:5] == (W, H, W, 16.0) and ops.calls[1][1][1:4] == (W, H, W) and ops.calls[2][1][1] == 15
    assert s[1:4] == (W, H, W) and np.array_equal(s[4], sun.table()) and s[5] == 128 and s[6] is True and s[7] is not None and s[10] == W
    assert got.shape == (H, W) and got.origin == (-5, 9) and got.form == 'accel' and got.sun is sun and got.exact and got.zq is None
    assert got.lit.dtype == got.mask.dtype == got.hours_q.dtype == got.energy.dtype == np.uint32
    ops = recording()
    got = SL.sunlight(ops, h[None], SL.Sun(((1.0 * i, 30) for i in range(33))), form='plain', keep='zq')
    assert got.mask is None and ops.dev.sizes == [4 * H * W] * 5 + [60, 4] and ops.calls[3][1][6] is False and ops.calls[3][1][11] is None
    assert got.zq.dtype == np.int32 and got.zq.shape == (H, W)
    got = SL.sunlight(recording(), (h * 255).astype(np.uint8))
    assert got.form == SL.DEFAULT_FORM and got.sun == SL.Day().sun() and got.mask is not None


@pytest.mark.parametrize("fail", ["viewshed_quantise", "viewshed_top", "sunlight_zmax", "sunlight_sun"])
def test_sunlight_frees_its_scratch_when_a_launch_fails(fail):
    ops = recording(fail)
    with pytest.raises(RuntimeError, match="the launch failed"):
        SL.sunlight(ops, R.case("9x1")["h"])
    assert ops.dev.live == 0 and len(ops.dev.sizes) == 8


def test_refusals_before_the_device_is_touched():
    ops = None
    h = R.case("15x17")["h"]
    for kw, match in ((dict(sun="noon"), "Sun"), (dict(sun=SL.Day()), "Sun"), (dict(origin=(1,)), "origin"), (dict(origin=(1.5, 0)), "origin"),
                      (dict(form='fast'), "form"), (dict(form=True), "form"), (dict(keep=('top',)), "keep")):
        with pytest.raises(ValueError, match=match):
            SL.sunlight(ops, h, **kw)
    for bad in (h * 3, h[0], np.zeros((2, 3, 4), np.float32), h.astype(np.int32), np.full((2, 2), np.nan, np.float32)):
        with pytest.raises(ValueError):
            SL.sunlight(ops, bad)
    s = hand_made()
    tex = np.zeros((2, 3, 3), np.uint8)
    for args, match in (((tex, "s", 1), "Sunlight"), ((tex, s, -1), "max_hours"), ((tex, s, 1, (1, 2, 3)), "colour"), ((tex, s, 1, (1, 1, 1), 1.5), "opacity"),
                        ((np.zeros((4, 4, 3), np.uint8), s, 1), "differ in size")):
        with pytest.raises(ValueError, match=match):
            SL.paint(ops, *args)


def test_the_paint_marks_the_cells_lit_fewer_hours():
    ops = recording()
    s = hand_made()
    out = SL.paint(ops, np.zeros((2, 3, 3), np.uint8), s, 2.0, (0.0, 0.0, 0.0), 0.25)
    assert out.shape == (2, 3, 3) and out.dtype == np.uint8 and ops.dev.live == 0 and len(ops.dev.sizes) == 4
    name, args, _ = ops.calls[0]
    assert [c[0] for c in ops.calls] == ["hydrology_paint"] and args[4:6] == (2, 3) and args[8] == 3
    assert args[9:15] == ((0.0, 0.0, 0.0), 0.25, 0.0, 1, 0, True)           # marks >= 1 within 0 pixels, no depth, a uint8 texture


# ---- the command lines -------------------------------------------------------------------------------------------------------------------
def test_command_line_parsing(capsys):
    a = SL.parse_args(["in.png", "out.npz", "--day"])
    assert (a.input, a.output, a.sun_, a.texture, a.painted, a.form) == ("in.png", "out.npz", SL.Day().sun(), None, None, None) and a.max_hours == 6.0
    a = SL.parse_args(["in.npy", "o.png", "--sun", "10,20", "--sun", "-30,5.5,2", "--sun=-0.5,90", "--target", "1.5", "--height-scale", "32",
                       "--texture", "t.png", "--painted", "p.png", "--max-hours", "1", "--colour", "1,0,0", "--opacity", "0.3", "--plain"])
    assert a.sun_ == SL.Sun(((10, 20), (-30, 5.5, 2), (-0.5, 90)), 1.5, 32.0)
    assert (a.texture, a.painted, a.max_hours, a.colour, a.opacity, a.form) == ("t.png", "p.png", 1.0, (1.0, 0.0, 0.0), 0.3, "plain")
    a = SL.parse_args(["i", "o.npz", "--day", "--latitude=-33", "--declination", "23.44", "--step-minutes", "60", "--min-elevation", "5", "--accel"])
    assert a.sun_ == SL.Day(-33, 23.44, 60, 5).sun() and a.form == "accel"
    for bad, match in ((["i"], "required"), (["i", "o.npz"], "one of --sun"), (["i", "o.npz", "--day", "--sun", "1,2"], "one of --sun"),
                       (["i", "o.npz", "--sun", "1"], "AZ,EL"), (["i", "o.npz", "--sun", "1,2,3,4"], "AZ,EL"), (["i", "o.npz", "--sun", "a,b"], "AZ,EL"),
                       (["i", "o.npz", "--sun", "1,0"], "elevation"), (["i", "o.npz", "--sun", "1,95"], "elevation"), (["i", "o.npz", "--sun", "1,5,-2"], "hours"),
                       (["i", "o.npz", "--sun", "1,5", "--latitude", "3"], "need --day"), (["i", "o.npz", "--day", "--latitude", "95"], "latitude"),
                       (["i", "o.npz", "--day", "--step-minutes", "7"], "step_minutes"), (["i", "o.npz", "--day", "--min-elevation", "0"], "min_elevation"),
                       (["i", "o.npz", "--day", "--latitude", "85", "--declination=-20"], "never stands"),
                       (["i", "o.npz", "--day", "--target", "-1"], "target_height"), (["i", "o.npz", "--day", "--height-scale", "0"], "height_scale"),
                       (["i", "o.tif", "--day"], "npz or .png"), (["i", "o.npz", "--day", "--texture", "t.png"], "go together"),
                       (["i", "o.npz", "--day", "--painted", "p.png"], "go together"), (["i", "o.npz", "--day", "--max-hours", "2"], "goes with --painted"),
                       (["i", "o.npz", "--day", "--texture", "t", "--painted", "p", "--opacity", "2"], "opacity"),
                       (["i", "o.npz", "--day", "--texture", "t", "--painted", "p", "--max-hours=-1"], "max_hours"),
                       (["i", "o.npz", "--day", "--plain", "--accel"], "not allowed with"), (["i", "o.npz", "--day", "--moon"], "unrecognized")):
        with pytest.raises(SystemExit):
            SL.parse_args(bad)
        assert match in capsys.readouterr().err, bad


def test_the_worlds_command_line_takes_the_sunlight(capsys):
    from gan_heightmaps_amd import world as WD
    base = ["exp", "model.npz", "out.png", "--seed", "3", "--region", "-70,33,150,97"]
    a = WD.parse_args(base)
    assert a.sunlight is None and a.latitude is None and a.declination is None
    a = WD.parse_args(base + ["--sunlight", "s.npz"])
    assert a.sunlight == "s.npz" and a.sun == SL.Day().sun()
    a = WD.parse_args(base + ["--sunlight", "s.png", "--latitude=-30", "--declination", "10"])
    assert a.sun == SL.Day(-30, 10).sun()
    for bad, match in ((["--latitude", "3"], "need --sunlight"), (["--declination", "3"], "need --sunlight"), (["--sunlight", "s.tif"], ".npz or .png"),
                       (["--sunlight", "s.npz", "--latitude", "100"], "latitude"), (["--sunlight", "s.npz", "--latitude", "89", "--declination=-20"], "never stands")):
        with pytest.raises(SystemExit):
            WD.parse_args(base + bad)
        assert match in capsys.readouterr().err, bad


def test_the_planes_table_lists_the_sunlight():
    from gan_heightmaps_amd import planes
    assert "sunlight" in planes.__doc__ and "sunlight    True   True        True   None" in planes.as_plane.__doc__


# ---- the sun kernel's source on the host ---------------------------------------------------------------------------------------------------
def _build(d, name, extra=()):
    import os
    import subprocess
    from tests.test_render_host import CSRC, ROOT, _compiler
    head, sep, _ = open(os.path.join(CSRC, "sunlight.hip")).read().partition("#define SUN_GRID")
    assert sep and '#include "common.h"' in head and '#include "relax.h"' in head
    inc = d / "sunlight.hip.inc"
    inc.write_text(head.replace('#include "common.h"', "").replace('#include "relax.h"', "") + "}  // namespace\n")
    exe = d / name
    cmd = [_compiler(), "-x", "c++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
           '-DSUNLIGHT_DEVICE_INC="%s"' % inc] + list(extra) + [os.path.join(ROOT, "tests", "sunlight_host", "harness.cpp"), "-o", str(exe)]
    return exe, subprocess.run(cmd, capture_output=True, text=True)


def run_host(d, exe, name, form, steps=False):
    """the planes of a case through the host build: the heights in rows of W + 3 cells with a wall in the padding, the planes in
    rows of W + 3 cells whose padding must come back untouched"""
    import subprocess
    c = R.case(name)
    zq, tab = c["zq"], c["table"]
    H, W = zq.shape
    wide = np.full((H, W + 3), 1 << 24, np.int32)
    wide[:, :W] = zq
    (d / "zq.bin").write_bytes(wide.tobytes())
    (d / "table.bin").write_bytes(np.ascontiguousarray(tab, np.int64).tobytes())
    args = [H, W, len(tab), c["target_q"], SL.FORMS.index(form), int(steps), d / "zq.bin", d / "table.bin", d / "out.bin"]
    r = subprocess.run([str(exe)] + [str(v) for v in args], capture_output=True, text=True)
    assert r.returncode == 0, (name, form, r.returncode, r.stderr[-3000:])
    got = np.frombuffer((d / "out.bin").read_bytes(), np.uint32).reshape(4, H, W + 3)
    assert (got[:, :, W:] == 0xABABABAB).all(), "cells beyond a row's width were written"
    written = [True, len(tab) <= 32 and not steps, not steps, not steps]
    for p, w in zip(got, written):
        assert w or (p == 0xABABABAB).all()
    return dict(lit=got[0, :, :W], mask=got[1, :, :W] if written[1] else None, hours_q=got[2, :, :W], energy=got[3, :, :W])


def test_both_forms_on_the_host_build_under_the_sanitizers(tmp_path):
    """the device source of both forms as a stand-alone program with -fsanitize=address,undefined, run as a child process against
    exact-size padded buffers: an index past a plane or the block maxima and signed overflow in a product end it.  Every case, both
    forms, against the restatement; the steps of the plain form equal the restatement's and the accel form's never exceed them"""
    import subprocess
    from tests.test_render_host import _compiler
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]
    # only a compiler that cannot build and run an empty program with the sanitizers is a reason to skip
    (tmp_path / "empty.cpp").write_text("int main() { return 0; }\n")
    probe = subprocess.run([_compiler(), "-x", "c++"] + flags + [str(tmp_path / "empty.cpp"), "-o", str(tmp_path / "empty")],
                           capture_output=True, text=True)
    if probe.returncode != 0 or subprocess.run([str(tmp_path / "empty")]).returncode != 0:
        pytest.skip("the host compiler cannot link the sanitizer runtimes: " + probe.stderr[-300:])
    exe, r = _build(tmp_path, "sunlight_host_san", flags)
    assert r.returncode == 0, r.stderr[-3000:]
    for name in sorted(R.CASES):
        want = R.expected(name)
        for form in SL.FORMS:
            assert R.same_planes(run_host(tmp_path, exe, name, form), want), (name, form)
        plain = run_host(tmp_path, exe, name, 'plain', steps=True)["lit"].astype(np.int64)
        fast = run_host(tmp_path, exe, name, 'accel', steps=True)["lit"].astype(np.int64)
        assert np.array_equal(plain, R.expected_steps(name)), name
        assert (fast <= plain).all(), name
        if name in ("33x65", "37x70", "70x37", "65x130", "many300"):
            assert fast.sum() < plain.sum(), name
