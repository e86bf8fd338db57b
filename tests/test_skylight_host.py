"""The sky light on the host.  The device code of csrc/skylight.hip, and csrc/render.hip's with its sky-lit
wrapper, compiled for the CPU (tests/skylight_host/harness.cpp): the same source text the GPU runs, the tiled form run phase
by phase.  And the host logic of gan_heightmaps_amd/skylight.py, render.py and world.py on tests/fake_device.py: the SkyLight
object and its refusals, bake's refusals, what a bake sends to the device, flight_plan(sky=)'s byte count, the command
lines.  No GPU."""
import dataclasses
import os
import subprocess

import numpy as np
import pytest

from gan_heightmaps_amd import render as RN
from gan_heightmaps_amd import skylight as SK
from gan_heightmaps_amd import world as WD
from tests import render_ref as R
from tests import skylight_ref as S
from tests.fake_device import FakeDevice, RecordingOps
from tests.test_flight_plan import _line
from tests.test_render_host import CSRC, ROOT, _compiler
from tests.test_skylight_ref import SKY_F32_DEV
from tests.test_world_plan import _world

TOL = 8 * SKY_F32_DEV


# ---- the kernels' source on the host ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("skylight_host")
    defs = []
    for name, macro in (("render.hip", "RENDER_DEVICE_INC"), ("skylight.hip", "SKY_DEVICE_INC")):
        head, sep, _ = open(os.path.join(CSRC, name)).read().partition('extern "C" {')
        assert sep and '#include "common.h"' in head
        inc = d / (name + ".inc")
        inc.write_text(head.replace('#include "common.h"', ""))
        defs.append('-D%s="%s"' % (macro, inc))
    exe = d / "skylight_host"
    cmd = [_compiler(), "-x", "c++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "include")] + defs + \
          [os.path.join(ROOT, "tests", "skylight_host", "harness.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return d, exe


def run_bake(harness, src, sky, hs, rect=None, out_pitch=None, uint8=False):
    """src [rows, pitch] float32 (cols = pitch unless rect says otherwise through ``cols``) -> (plain, tiled) [h, out_pitch]"""
    d, exe = harness
    rows, pitch = src.shape
    y0, x0, h, w, cols = rect if rect is not None else (0, 0, rows, pitch, pitch)
    out_pitch = w if out_pitch is None else out_pitch
    (d / "in.bin").write_bytes(np.ascontiguousarray(src, np.float32).tobytes() + sky.table().tobytes())
    args = ["bake", rows, cols, pitch, y0, x0, h, w, out_pitch, sky.directions, sky.steps, sky.reach, repr(float(hs)),
            repr(sky.strength), int(uint8)]
    r = subprocess.run([str(exe)] + [str(v) for v in args] + [str(d / "in.bin"), str(d / "out.bin")])
    assert r.returncode == 0, r.returncode
    raw = np.fromfile(d / "out.bin", np.uint8 if uint8 else np.float32)
    assert raw.size == 2 * h * out_pitch
    return raw[:h * out_pitch].reshape(h, out_pitch), raw[h * out_pitch:].reshape(h, out_pitch)


@pytest.mark.parametrize("case", range(len(S.CASES)))
def test_both_forms_on_the_host_build(harness, case):
    H, W, seed, hs, kw = S.CASES[case]
    sky = SK.SkyLight(**kw)
    plain, tiled = run_bake(harness, S.terrain(seed, H, W), sky, hs)
    assert plain.tobytes() == tiled.tobytes()                          # bit for bit, the tiled form phase by phase
    err = np.abs(plain.astype(np.float64) - S.reference(case, 'float64'))
    differ = int((plain != S.reference(case, 'float32')).sum())
    print("case %d %d x %d: max err %.3e, %d of %d elements differ from the float32 restatement"
          % (case, H, W, err.max(), differ, H * W))
    assert (err <= TOL).all(), err.max()


def test_pitches_a_sub_rectangle_and_uint8_on_the_host_build(harness):
    sky = SK.SkyLight(directions=8, steps=6, step=1.0)
    m, hs = sky.reach, 64.0
    big = S.terrain(7, 50 + 2 * m, 41 + 2 * m)
    rows, cols = big.shape
    whole, whole_t = run_bake(harness, big, sky, hs)
    assert whole.tobytes() == whole_t.tobytes()
    # a source pitch beyond its width (the cells beyond are NaN), an output pitch beyond its width, a rectangle inside
    wide = np.full((rows, cols + 5), np.nan, np.float32)
    wide[:, :cols] = big
    y0, x0, h, w = m + 3, m + 2, 37, 35
    for rect in ((0, 0, rows, cols, cols), (y0, x0, h, w, cols)):
        plain, tiled = run_bake(harness, wide, sky, hs, rect=rect, out_pitch=rect[3] + 3)
        assert plain.tobytes() == tiled.tobytes()
        assert np.isnan(plain[:, rect[3]:]).all()                      # the cells beyond the output's width are untouched
        assert np.array_equal(plain[:, :rect[3]], whole[rect[0]:rect[0] + rect[2], rect[1]:rect[1] + rect[3]])
    # the same rectangle from a window of its own with ``reach`` of halo: the larger map's interior
    win, _ = run_bake(harness, big[y0 - m:y0 + h + m, x0 - m:x0 + w + m], sky, hs, rect=(m, m, h, w, w + 2 * m))
    assert np.array_equal(win, whole[y0:y0 + h, x0:x0 + w])
    u8, u8t = run_bake(harness, big, sky, hs, uint8=True)
    assert u8.tobytes() == u8t.tobytes() and np.array_equal(u8, np.rint(whole.astype(np.float64) * 255).astype(np.uint8))


def run_view(harness, hm, tex, sky_plane, cam, size, hs, shadows, **kw):
    d, exe = harness
    a = dict(R.VIEW_KW)
    a.update(kw)
    H, W = hm.shape
    (d / "vin.bin").write_bytes(b"".join(np.ascontiguousarray(x, np.float32).tobytes() for x in (hm, tex, sky_plane)))
    args = ["view", H, W, size[0], size[1], a['step'], a['max_dist'], *cam['pos'], cam['yaw'], cam['pitch'], cam['fov'], hs,
            a['sun_azimuth'], a['sun_elevation'], a['softness'], a['ambient'], a['haze'], int(shadows)]
    r = subprocess.run([str(exe)] + [v if isinstance(v, str) else repr(v) for v in args] +
                       [str(d / "vin.bin"), str(d / "vout.bin")])
    assert r.returncode == 0, r.returncode
    raw = np.fromfile(d / "vout.bin", np.float32)
    n = 3 * size[0] * size[1]
    return raw[:n].reshape((3,) + tuple(size)), raw[n:].reshape((3,) + tuple(size))


def test_the_sky_kernel_with_a_plane_of_ones_is_the_plain_kernel(harness):
    hm, tex = R.terrain(0)
    for cam in (0, 1):
        plain, lit = run_view(harness, hm, tex, np.ones_like(hm), R.CAMERAS[cam], R.VIEW_SIZE, R.HEIGHT_SCALE, True)
        assert (plain >= 0).all() and plain.tobytes() == lit.tobytes()


def test_a_sky_lit_view_on_the_host_build_against_float64(harness):
    from tests.test_render_plan import F32_DEV
    hm, tex = R.terrain(1)
    plane = S.bake(hm, R.HEIGHT_SCALE, np.float32)
    plain, lit = run_view(harness, hm, tex, plane, R.CAMERAS[0], R.VIEW_SIZE, R.HEIGHT_SCALE, True)
    want, _ = S.render_sky(hm, tex, plane, size=R.VIEW_SIZE, height_scale=R.HEIGHT_SCALE, **R.CAMERAS[0], **R.VIEW_KW)
    err = np.abs(lit.astype(np.float64) - want).max(0)
    print("sky-lit view: max err %.3e; darkest plane value %.3f" % (err.max(), plane.min()))
    assert (err <= 8 * F32_DEV).all() and not np.array_equal(plain, lit) and (lit <= plain).all()


# ---- the SkyLight object ------------------------------------------------------------------------------------------------
def test_skylight_defaults_and_freezing():
    s = SK.SkyLight()
    assert (s.directions, s.steps, s.step, s.strength, s.reach) == (16, 24, 1.5, 1.0, 37)
    assert s == SK.SkyLight() and hash(s) == hash(SK.SkyLight()) and s != SK.SkyLight(strength=0.5)
    with pytest.raises(dataclasses.FrozenInstanceError):
        s.steps = 3
    t = SK.SkyLight(directions=np.int64(4), steps=np.int32(2), step=np.float32(2), strength=1)
    assert (type(t.directions), type(t.steps), type(t.step), type(t.strength)) == (int, int, float, float)
    assert SK.SkyLight(directions=64, steps=256).table().shape == (64, 256)
    assert (SK.MAX_DIRECTIONS, SK.MAX_STEPS) == (64, 256) and SK.DEFAULT_TILED in (False, True)


@pytest.mark.parametrize("kw,match", [
    (dict(directions=0), "directions"), (dict(directions=65), "directions"), (dict(directions=4.0), "directions"),
    (dict(directions=True), "directions"), (dict(steps=0), "steps"), (dict(steps=257), "steps"), (dict(steps="3"), "steps"),
    (dict(step=0.0), "step"), (dict(step=-1.0), "step"), (dict(step=float("inf")), "step"), (dict(step=float("nan")), "step"),
    (dict(step=1e-40), "step"), (dict(strength=-0.1), "strength"), (dict(strength=1.01), "strength"),
    (dict(strength=float("nan")), "strength"), (dict(strength="1"), "strength")])
def test_skylight_refusals(kw, match):
    with pytest.raises(ValueError, match=match):
        SK.SkyLight(**kw)


def test_bake_refuses_before_it_touches_a_device():
    ok = np.zeros((8, 8), np.float32)
    for bad in (np.zeros((1, 8, 8), np.float32), np.zeros(8, np.float32), np.zeros((0, 4), np.float32)):
        with pytest.raises(ValueError, match="must be \\(H, W\\)"):
            SK.bake(None, bad)
    with pytest.raises(ValueError, match="uint8 or floating"):
        SK.bake(None, np.zeros((4, 4), np.int32))
    with pytest.raises(ValueError, match="non-finite"):
        SK.bake(None, np.full((4, 4), np.nan))
    with pytest.raises(ValueError, match="must be a SkyLight"):
        SK.bake(None, ok, sky=dict(steps=3))
    for hs in (0.0, -1.0, float("inf"), float("nan"), "64", True):
        with pytest.raises(ValueError, match="height_scale"):
            SK.bake(None, ok, height_scale=hs)
    for m in (-1, 1.5, True):
        with pytest.raises(ValueError, match="margin"):
            SK.bake(None, ok, margin=m)
    with pytest.raises(ValueError, match="no interior"):
        SK.bake(None, ok, margin=4)
    for out in (np.zeros((8, 8), np.float64), np.zeros((7, 8), np.float32), np.zeros((8, 16), np.float32)[:, ::2]):
        with pytest.raises(ValueError, match="out must be"):
            SK.bake(None, ok, out=out)
    with pytest.raises(ValueError, match="out must be"):
        SK.bake(None, ok, out=np.zeros((8, 8), np.float32), uint8=True)


def test_what_a_bake_sends_to_the_device():
    dev = FakeDevice()
    ops = RecordingOps(dev)
    sky = SK.SkyLight(directions=8, steps=6, step=1.0)
    out = SK.bake(ops, np.zeros((20, 30), np.uint8), sky, height_scale=24, margin=3, tiled=False)
    assert out.shape == (14, 24) and out.dtype == np.float32
    (name, args, _), = [c for c in ops.calls if c[0] == "skylight_bake"]
    src, rows, cols, pitch, table, directions, steps, reach, y0, x0, h, w, hs, strength, tiled, u8, dst, out_pitch = args
    assert (rows, cols, pitch, directions, steps, reach) == (20, 30, 30, 8, 6, 7)
    assert (y0, x0, h, w, hs, strength, tiled, u8, out_pitch) == (3, 3, 14, 24, 24.0, 1.0, False, False, 24)
    assert [c[0] for c in ops.calls] == ["skylight_table", "skylight_bake"] and ops.calls[0][1] == (sky,)
    assert SK.bake(ops, np.zeros((9, 9), np.float32), uint8=True, tiled=False).dtype == np.uint8


def test_the_device_table_is_uploaded_once_per_skylight():
    from gan_heightmaps_amd.device import Ops
    dev = FakeDevice()
    ops = Ops.__new__(Ops)
    ops.dev = dev
    a, b = SK.SkyLight(), SK.SkyLight(steps=5)
    pa = ops.skylight_table(a)
    assert ops.skylight_table(SK.SkyLight()) == pa and dev.uploads == 1            # an equal SkyLight is the same table
    other = Ops.__new__(Ops)
    other.dev = dev
    assert other.skylight_table(a) == pa and dev.uploads == 1                      # the cache belongs to the context
    assert ops.skylight_table(b) != pa and dev.uploads == 2
    for n in range(1, Ops.SKY_TABLES + 1):
        ops.skylight_table(SK.SkyLight(steps=40 + n))
    assert len(dev._sky_tables) == Ops.SKY_TABLES and a not in dev._sky_tables     # the least recently used left


# ---- scenes and flights ----------------------------------------------------------------------------------------------
def test_flight_plan_counts_the_sky_plane():
    assert WD.SCENE_BYTES_PER_PIXEL == 22 and WD.SKY_SCENE_BYTES_PER_PIXEL == 26
    w = _world(chunk_cells=2)
    cams = _line(12, (-200.0, 11.25, 14.0), (200.0, 11.25, 14.0))
    fps = [c.footprint(40.0) for c in cams]
    mb = 128 * 128 * 22 / float(1 << 20)
    plain = w.flight_plan(cams, 40.0, window_mb=mb)
    assert w.flight_plan(cams, 40.0, window_mb=mb, sky=None) == plain              # without sky the plan is today's
    assert plain == WD.plan_windows(fps, w.geometry.out, int(mb * (1 << 20)) // 22)
    lit = w.flight_plan(cams, 40.0, window_mb=mb, sky=SK.SkyLight())
    assert lit == WD.plan_windows(fps, w.geometry.out, int(mb * (1 << 20)) // 26)
    assert all(r[2] * r[3] * 26 <= mb * (1 << 20) for r, _, _ in lit) and len(lit) >= len(plain)
    # the reach does not enter the plan: the grown height plane is transient and outside the budget
    assert w.flight_plan(cams, 40.0, window_mb=mb, sky=SK.SkyLight(steps=200, step=3.0)) == lit
    with pytest.raises(ValueError, match="must be a skylight.SkyLight"):
        w.flight_plan(cams, 40.0, sky=3)
    with pytest.raises(ValueError, match="must be a skylight.SkyLight"):
        w.flight(cams, 40.0, sky="yes")
    with pytest.raises(ValueError, match="must be a skylight.SkyLight"):
        w.scene(0, 0, 8, 8, sky=1.0)


def test_scene_refusals_before_a_device():
    hm, tex = np.zeros((12, 12), np.float32), np.zeros((3, 8, 8), np.float32)
    with pytest.raises(ValueError, match="must be a skylight.SkyLight"):
        RN.Scene(hm[:8, :8], tex, sky=True, device=FakeDevice())
    with pytest.raises(ValueError, match="margin"):
        RN.Scene(hm, tex, sky=SK.SkyLight(), margin=-2, device=FakeDevice())
    with pytest.raises(ValueError, match="differ in size"):
        RN.Scene(hm, tex, sky=SK.SkyLight(), margin=1, device=FakeDevice())
    with pytest.raises(ValueError, match="no interior"):
        RN.Scene(hm, tex, sky=SK.SkyLight(), margin=6, device=FakeDevice())


# ---- command lines --------------------------------------------------------------------------------------------------------
def test_skylight_cli_arguments():
    a = SK.parse_args(["in.png", "out.npy"])
    assert (a.input, a.output, a.plain, a.tiled, a.height_scale) == ("in.png", "out.npy", False, False, 64.0)
    assert a.sky == SK.SkyLight() and SK.parse_args(["a", "b", "--tiled"]).tiled
    a = SK.parse_args(["in.npy", "out.png", "--directions", "8", "--steps", "6", "--step", "1", "--strength", "0.5",
                       "--height-scale", "24", "--plain"])
    assert a.sky == SK.SkyLight(8, 6, 1.0, 0.5) and a.height_scale == 24.0 and a.plain
    for bad in (["in.npy"], ["a", "b", "--directions", "0"], ["a", "b", "--steps", "300"], ["a", "b", "--step", "0"],
                ["a", "b", "--strength", "2"], ["a", "b", "--height-scale", "0"], ["a", "b", "--plain", "--tiled"]):
        with pytest.raises(SystemExit):
            SK.parse_args(bad)


def test_render_cli_takes_sky():
    cam = ["--pos", "1,2,3", "--yaw", "0", "--pitch", "-10"]
    files = ["out.png", "--heightmap", "h.png", "--texture", "t.png"] + cam
    assert RN.parse_args(files).skylight is None and RN.parse_args(files + ["--sky"]).skylight == SK.SkyLight()
    a = RN.parse_args(files + ["--sky", "--sky-directions", "8", "--sky-steps", "6", "--sky-step", "1", "--sky-strength", "0.5"])
    assert a.skylight == SK.SkyLight(8, 6, 1.0, 0.5)
    for bad in (["--sky-steps", "6"], ["--sky", "--sky-steps", "0"], ["--sky", "--sky-strength", "3"]):
        with pytest.raises(SystemExit):
            RN.parse_args(files + bad)
    wa = ["out.png", "--world", "EXP", "m.model", "--seed", "1", "--max-dist", "50", "--sky"] + cam
    assert RN.parse_args(wa).skylight == SK.SkyLight()
