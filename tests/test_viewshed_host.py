"""The host side of the viewshed (gan_heightmaps_amd/viewshed.py): Sight's validation, the observer table, the
refusals that are made before the device is touched, the launch sequence on a recording device, the command lines' parsing, the
.npz / .png writers.  And the device code of csrc/viewshed.hip compiled for the CPU (tests/viewshed_host/harness.cpp): the same
source text the GPU runs, the quantisation, the block maxima and both forms of the sight lines bit for bit against
tests/viewshed_ref.py on the cases of the device tests, once more under the address and undefined-behaviour sanitizers.  No
device."""
import os
import subprocess

import numpy as np
import pytest

from gan_heightmaps_amd import viewshed as VS
from tests import viewshed_ref as V
from tests.test_render_host import CSRC, ROOT, _compiler


# ---- validation and the table ---------------------------------------------------------------------------------------------------
def test_sight_validation():
    s = VS.Sight()
    assert (s.eye_height, s.target_height, s.max_dist, s.height_scale, s.eye_q, s.target_q) == (2.0, 0.0, None, 64.0, 512, 0)
    assert VS.Sight(np.float32(1.5), 1, np.int64(7), 8) == VS.Sight(1.5, 1.0, 7.0, 8.0) and hash(s) == hash(VS.Sight())
    assert VS.Sight(eye_height=65536).eye_q == 1 << 24 and VS.Sight(target_height=0.001).target_q == 0
    assert VS.Sight(eye_height=1.5 / 256).eye_q == 2 and VS.Sight(eye_height=2.5 / 256).eye_q == 2          # half to even
    with pytest.raises(Exception):
        s.eye_height = 3                                                   # frozen
    for kw in (dict(eye_height=-1), dict(eye_height=65537), dict(eye_height=None), dict(eye_height=True), dict(eye_height=float("nan")),
               dict(target_height=-0.5), dict(target_height="1"), dict(max_dist=-1), dict(max_dist=float("inf")), dict(max_dist="3"),
               dict(height_scale=0), dict(height_scale=65537), dict(height_scale=None), dict(height_scale=float("nan"))):
        with pytest.raises(ValueError):
            VS.Sight(**kw)
    assert VS.DEFAULT_ACCEL in (True, False) and VS.KEEP == ('zq',)


def test_the_observer_table():
    s = VS.Sight(eye_height=1.0, max_dist=5.5)
    t = VS.observer_table([(3, 4), [5, 6, 2.5], (np.int64(7), 8, None, 3.0), (0, 0, 0, 0), (9, 19, 1, 1000)], s, (10, 20))
    assert t.dtype == np.int32 and t.tolist() == [[3, 4, 256, 30], [5, 6, 640, 30], [7, 8, 256, 9], [0, 0, 0, 0], [9, 19, 256, -1]]
    assert VS.observer_table([(103, -4)], VS.Sight(), (10, 20), origin=(100, -10)).tolist() == [[3, 6, 512, -1]]
    assert VS.observer_table([(0, 0, 2, 21.0)], s, (10, 20))[0, 3] == 441 and VS.observer_table([(0, 0, 2, 21.1)], s, (10, 20))[0, 3] == -1
    assert len(VS.observer_table([(1, 1)] * 4096, s, (3, 3))) == 4096
    for bad in (None, [], 5, [(1, 1)] * 4097, [(1,)], [(1, 2, 3, 4, 5)], [(1.0, 2)], [(1, True)], [(10, 0)], [(0, 20)], [(-1, 0)],
                [(1, 1, -1)], [(1, 1, 65537)], [(1, 1, "2")], [(1, 1, 2, -1)], [(1, 1, 2, float("nan"))]):
        with pytest.raises(ValueError, match="observer"):
            VS.observer_table(bad, s, (10, 20))
    # a radius that cuts a plane longer than 46340 cells beyond them does not fit the table
    with pytest.raises(ValueError, match="46340"):
        VS.observer_table([(0, 0, 1, 50000.0)], s, (262140, 8000))
    assert VS.observer_table([(0, 0, 1, 300000.0)], s, (262140, 8000))[0, 3] == -1


def test_refusals_before_the_device_is_touched():
    ops = None                                                            # nothing may reach for it
    h = V.heights(8, 9, 1)
    obs = [(1, 2)]
    for bad in (np.zeros((2, 8, 9), np.float32), np.zeros(8, np.float32), np.zeros((8, 9), np.int32), np.zeros((0, 9), np.float32)):
        with pytest.raises(ValueError):
            VS.viewshed(ops, bad, obs)
    x = h.copy()
    x[3, 4] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        VS.viewshed(ops, x, obs)
    for v in (-0.01, 1.5):
        x = h.copy()
        x[3, 4] = v
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            VS.viewshed(ops, x, obs)
    huge = np.lib.stride_tricks.as_strided(np.zeros(1, np.float32), shape=(1 << 16, 1 << 15), strides=(0, 0), writeable=False)
    with pytest.raises(ValueError, match="out of range"):
        VS.viewshed(ops, huge, obs)
    for bad in ([], [(8, 0)], [(0, 9)], None, [(1, 2, -3)]):
        with pytest.raises(ValueError, match="observer"):
            VS.viewshed(ops, h, bad)
    with pytest.raises(ValueError, match="observer"):
        VS.viewshed(ops, h, [(1, 2)], origin=(5, 5))
    with pytest.raises(ValueError, match="Sight"):
        VS.viewshed(ops, h, obs, dict(eye_height=2))
    for bad in (3, (1,), (1.5, 2), None):
        with pytest.raises(ValueError, match="origin"):
            VS.viewshed(ops, h, obs, origin=bad)
    with pytest.raises(ValueError, match="keep"):
        VS.viewshed(ops, h, obs, keep=('count',))
    seen = VS.Viewshed(np.zeros((8, 9), np.uint32), None, np.zeros((40, 4), np.int32), (0, 0), VS.Sight(), True)
    tex = np.zeros((8, 9, 3), np.uint8)
    with pytest.raises(ValueError, match="Viewshed"):
        VS.paint(ops, tex, None)
    for bad in ((1, 2), (1.5, 0, 0), None):
        with pytest.raises(ValueError, match="colour"):
            VS.paint(ops, tex, seen, bad)
    with pytest.raises(ValueError, match="opacity"):
        VS.paint(ops, tex, seen, opacity=2)
    with pytest.raises(ValueError, match="differ in size"):
        VS.paint(ops, np.zeros((9, 8, 3), np.uint8), seen)
    with pytest.raises(ValueError, match="npz or .png"):
        seen.save("seen.txt")
    with pytest.raises(ValueError, match="32 observers"):
        seen.visible(3)
    with pytest.raises(ValueError, match="observer"):
        seen.visible(40)


def test_viewshed_sends_its_launches_inside_one_scratch():
    from tests.fake_device import FakeDevice, RecordingOps

    class Ops(RecordingOps):
        def viewshed_top_elems(self, H, W):
            return ((H + 15) // 16) * ((W + 15) // 16)

    class Counting(FakeDevice):
        def __init__(self):
            super().__init__()
            self.live = 0

        def alloc(self, nbytes):
            self.live += 1
            return super().alloc(nbytes)

        def free(self, ptr):
            self.live -= 1

    h = V.heights(20, 33, 1)
    ops = Ops(Counting())
    got = VS.viewshed(ops, h[None], [(103, -4), (110, 0, 1.0, 5.0)], VS.Sight(target_height=0.5, height_scale=32), accel=True,
                      origin=(100, -10), keep='zq')
    assert [c[0] for c in ops.calls] == ["viewshed_quantise", "viewshed_top", "viewshed_sight"] and ops.dev.live == 0
    qu, tp, si = (c[1] for c in ops.calls)
    assert qu[1:5] == (33, 20, 33, 32.0) and qu[6] == 33
    assert tp[0] == qu[5] and tp[1:4] == (33, 20, 33) and tp[5] == 2 * 3
    assert si[0] == qu[5] and si[1:4] == (33, 20, 33) and si[4].tolist() == [[3, 6, 512, -1], [10, 10, 256, 25]]
    assert si[5:7] == (128, True) and si[7] == tp[4] and si[9] == 33 and si[10] is not None and si[11] == 33
    assert got.shape == (20, 33) and got.origin == (100, -10) and got.accel is True and len(got) == 2
    assert got.observers.tolist() == [[103, -4, 512, -1], [110, 0, 256, 25]] and got.mask is not None and got.zq.dtype == np.int32
    assert got.count.dtype == np.uint32 and got.share() == 0.0 and not got.seen().any() and not got.visible(1).any()
    assert "2 observers" in repr(got)
    ops = Ops(Counting())
    got = VS.viewshed(ops, (h * 255).astype(np.uint8), [(1, 1)] * 33, accel=False)
    assert [c[0] for c in ops.calls] == ["viewshed_quantise", "viewshed_sight"] and ops.dev.live == 0
    si = ops.calls[1][1]
    assert si[6] is False and si[7] is None and si[10] is None and got.mask is None and got.zq is None and len(si[4]) == 33
    ops = Ops(Counting())
    assert VS.viewshed(ops, h, [(1, 1)]).accel is VS.DEFAULT_ACCEL
    # the paint goes through the hydrology's kernel, with the seen or the unseen cells as its marks
    seen = VS.Viewshed(np.eye(8, 9, dtype=np.uint32), np.eye(8, 9, dtype=np.uint32), np.zeros((1, 4), np.int32), (0, 0), VS.Sight(), True)
    marks = []

    class Paint(RecordingOps):
        def hydrology_paint(self, *args):
            self.calls.append(("hydrology_paint", args, {}))

    class Dev(FakeDevice):
        def h2d(self, ptr, arr):
            marks.append(np.array(arr))

    for hidden in (False, True):
        del marks[:]
        ops = Paint(Dev())
        VS.paint(ops, np.zeros((8, 9, 3), np.uint8), seen, hidden=hidden)
        assert [c[0] for c in ops.calls] == ["hydrology_paint"] and ops.calls[0][1][12:14] == (1, 0)
        assert np.array_equal(marks[1], np.eye(8, 9) != hidden) and marks[1].dtype == np.uint32


def test_viewshed_methods_and_writers(tmp_path):
    count = np.array([[0, 1, 2], [3, 0, 1]], np.uint32)
    mask = np.array([[0, 1, 3], [7, 0, 4]], np.uint32)
    obs = np.array([[5, 5, 512, -1], [5, 6, 0, 9], [6, 7, 256, -1]], np.int32)
    seen = VS.Viewshed(count, mask, obs, (5, 5), VS.Sight(), False)
    assert seen.visible(0).tolist() == [[False, True, True], [True, False, False]]
    assert seen.visible(2).tolist() == [[False, False, False], [True, False, True]]
    assert seen.seen().tolist() == [[False, True, True], [True, False, True]] and seen.share() == 4 / 6 and len(seen) == 3
    seen.save(str(tmp_path / "v.npz"))
    z = np.load(str(tmp_path / "v.npz"))
    assert np.array_equal(z["count"], count) and np.array_equal(z["mask"], mask) and np.array_equal(z["observers"], obs)
    assert z["origin"].tolist() == [5, 5]
    seen.save(str(tmp_path / "v.png"))
    from gan_heightmaps_amd.util import read_image
    img = read_image(str(tmp_path / "v.png"))
    assert img.dtype == np.uint8 and img.tolist() == [[0, 255, 255], [255, 0, 255]]
    VS.Viewshed(count, None, obs, (0, 0), VS.Sight(), True).save(str(tmp_path / "w.npz"))
    assert "mask" not in np.load(str(tmp_path / "w.npz")).files


# ---- command lines ------------------------------------------------------------------------------------------------------------------
def test_command_line_parsing():
    a = VS.parse_args(["in.png", "out.npz", "--from", "3,4"])
    assert (a.input, a.output, a.observers, a.sight, a.texture, a.painted, a.hidden, a.form) == \
        ("in.png", "out.npz", [(3, 4)], VS.Sight(), None, None, False, None)
    a = VS.parse_args(["i.npy", "o.png", "--from", "1,2,3.5", "--from", " 30 , 40 , 1 , 100", "--from", "-5,6", "--eye", "1.5",
                       "--target", "0.25", "--max-dist", "64", "--height-scale", "32", "--texture", "t.png", "--painted", "p.png",
                       "--hidden", "--colour", "0.5,0.25,0", "--opacity", "0.75", "--plain"])
    assert a.observers == [(1, 2, 3.5), (30, 40, 1.0, 100.0), (-5, 6)] and a.sight == VS.Sight(1.5, 0.25, 64.0, 32.0)
    assert (a.texture, a.painted, a.hidden, a.colour, a.opacity, a.form) == ("t.png", "p.png", True, (0.5, 0.25, 0.0), 0.75, False)
    assert VS.parse_args(["i", "o.npz", "--from", "0,0", "--accel"]).form is True
    for bad in (["i", "o.npz"], ["i", "--from", "1,2"], ["i", "o.txt", "--from", "1,2"], ["i", "o.npz", "--from", "1"],
                ["i", "o.npz", "--from", "1,2,3,4,5"], ["i", "o.npz", "--from", "1.5,2"], ["i", "o.npz", "--from", "1,2,x"],
                ["i", "o.npz", "--from", "1,2,-1"], ["i", "o.npz", "--from", "1,2,1,-4"], ["i", "o.npz", "--from", "1,2", "--plain", "--accel"],
                ["i", "o.npz", "--from", "1,2", "--eye", "-1"], ["i", "o.npz", "--from", "1,2", "--target", "70000"],
                ["i", "o.npz", "--from", "1,2", "--max-dist", "-2"], ["i", "o.npz", "--from", "1,2", "--height-scale", "0"],
                ["i", "o.npz", "--from", "1,2", "--texture", "t.png"], ["i", "o.npz", "--from", "1,2", "--painted", "p.png"],
                ["i", "o.npz", "--from", "1,2", "--hidden"], ["i", "o.npz", "--from", "1,2", "--texture", "t", "--painted", "p",
                                                            "--colour", "2,0,0"],
                ["i", "o.npz", "--from", "1,2", "--texture", "t", "--painted", "p", "--opacity", "1.5"]):
        with pytest.raises(SystemExit):
            VS.parse_args(bad)


def test_the_worlds_command_line_takes_viewshed():
    from gan_heightmaps_amd import world as WD
    base = ["exp", "model.npz", "out.png", "--seed", "3", "--region", "-70,33,150,97"]
    assert WD.parse_args(base).viewshed is None
    a = WD.parse_args(base + ["--viewshed", "seen.npz", "--from", "-5,40", "--from", "3,50"])
    assert a.viewshed == "seen.npz" and a.sources == [(-5, 40), (3, 50)] and a.routes is None
    a = WD.parse_args(base + ["--viewshed", "seen.png", "--routes", "pre", "--from", "-5,40", "--to", "-60,35"])
    assert a.viewshed == "seen.png" and a.routes == "pre" and a.targets == [(-60, 35)]
    for bad in (["--viewshed", "seen.npz"], ["--viewshed", "seen.txt", "--from", "1,40"], ["--viewshed", "seen.npz", "--from", "80,40"],
                ["--viewshed", "seen.npz", "--from", "1,40", "--to", "2,40"], ["--from", "1,40"]):
        with pytest.raises(SystemExit):
            WD.parse_args(base + bad)


# ---- the kernels' source on the host ----------------------------------------------------------------------------------------------
def _build(d, name, extra=()):
    head, sep, _ = open(os.path.join(CSRC, "viewshed.hip")).read().partition('extern "C" {')
    assert sep and '#include "common.h"' in head and '#include "relax.h"' in head
    inc = d / "viewshed.hip.inc"
    inc.write_text(head.replace('#include "common.h"', "").replace('#include "relax.h"', ""))
    exe = d / name
    cmd = [_compiler(), "-x", "c++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
           '-DVIEWSHED_DEVICE_INC="%s"' % inc] + list(extra) + [os.path.join(ROOT, "tests", "viewshed_host", "harness.cpp"),
                                                               "-o", str(exe)]
    return exe, subprocess.run(cmd, capture_output=True, text=True)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("viewshed_host")
    exe, r = _build(d, "viewshed_host")
    assert r.returncode == 0, r.stderr[-3000:]
    return d, exe


def run_quantise(harness, h, height_scale):
    """-> zq; the heights go in with rows of W + 3 cells padded with NaN, the result lies in rows of W + 2 cells whose padding
    must come back untouched"""
    d, exe = harness
    H, W = h.shape
    wide = np.full((H, W + 3), np.nan, np.float32)
    wide[:, :W] = h
    (d / "in.bin").write_bytes(wide.tobytes())
    args = ["quantise", H, W, W + 3, W + 2, repr(float(height_scale)), d / "in.bin", d / "out.bin"]
    r = subprocess.run([str(exe)] + [str(v) for v in args], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    raw = np.frombuffer((d / "out.bin").read_bytes(), np.uint8).reshape(H, (W + 2) * 4)
    assert (raw[:, W * 4:] == 0xAB).all(), "cells beyond a row's width were written"
    return np.ascontiguousarray(raw[:, :W * 4]).view(np.int32).reshape(H, W)


def run_sight(harness, zq, observers, target_q):
    """-> (top, {accel: (count, mask or None, steps)}); zq goes in with rows of W + 3 cells whose padding is 2^30 high, the
    results lie in rows of W + 2 cells whose padding must come back untouched"""
    d, exe = harness
    H, W = zq.shape
    obs = V.table(observers)
    wide = np.full((H, W + 3), 1 << 30, np.int32)
    wide[:, :W] = zq
    (d / "in.bin").write_bytes(wide.tobytes() + obs.tobytes())
    args = ["sight", H, W, W + 3, W + 2, len(obs), target_q, d / "in.bin", d / "out.bin"]
    r = subprocess.run([str(exe)] + [str(v) for v in args], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    raw = (d / "out.bin").read_bytes()
    th, tw = (H + V.BLOCK - 1) // V.BLOCK, (W + V.BLOCK - 1) // V.BLOCK
    top = np.frombuffer(raw[:4 * th * tw], np.int32).reshape(th, tw)
    planes = np.frombuffer(raw[4 * th * tw:], np.uint8).reshape(2, 3, H, (W + 2) * 4)
    assert (planes[:, :, :, W * 4:] == 0xAB).all(), "cells beyond a row's width were written"
    body = np.ascontiguousarray(planes[:, :, :, :W * 4]).view(np.uint32).reshape(2, 3, H, W)
    out = {}
    for accel in (0, 1):
        mask = body[accel, 1] if len(obs) <= 32 else None
        if mask is None:
            assert (planes[accel, 1] == 0xAB).all(), "a mask was written beyond 32 observers"
        out[bool(accel)] = (body[accel, 0], mask, body[accel, 2])
    return top, out


def check_case(harness, name):
    c = V.case(name)
    count, mask = V.expected(name)
    top, out = run_sight(harness, c["zq"], c["observers"], c["target_q"])
    assert np.array_equal(top, V.top(c["zq"])), name
    for accel in (False, True):
        got_count, got_mask, _ = out[accel]
        assert np.array_equal(got_count, count), (name, accel)
        assert (mask is None and got_mask is None) or np.array_equal(got_mask, mask), (name, accel)
    plain, fast = out[False][2].astype(np.int64), out[True][2].astype(np.int64)
    assert (fast <= plain).all(), name                                    # the accel form tests a subset of the plain form's steps
    return int(plain.sum()), int(fast.sum())


def test_the_quantisation_on_the_host_build(harness):
    for k, (H, W) in enumerate(V.SHAPES):
        for scale in (1.0, 64.0, 0.37, 65536.0):
            h = V.heights(H, W, 30 + k)
            h.flat[0], h.flat[-1] = 0.0, 1.0
            assert np.array_equal(run_quantise(harness, h, scale), V.quantise(h, scale)), (H, W, scale)
    ties = (np.arange(64, dtype=np.float32) / np.float32(512)).reshape(4, 16)          # odd / 512 lies half way at height_scale 1
    assert np.array_equal(run_quantise(harness, ties, 1.0), V.quantise(ties, 1.0)) and V.quantise(ties, 1.0)[0, :4].tolist() == [0, 0, 1, 2]


@pytest.mark.parametrize("name", sorted(V.CASES))
def test_both_forms_of_the_sight_lines_on_the_host_build(harness, name):
    plain, fast = check_case(harness, name)
    if name == "one":
        assert plain == fast == 0
    else:
        assert plain > 0
    if name in ("wide", "wide0", "row4096"):
        assert fast < plain, "no run was jumped"


def test_the_harness_under_the_sanitizers(tmp_path):
    """the same stand-alone program with -fsanitize=address,undefined: out-of-bounds plane or block-maxima indices and signed
    overflow in the kernels' arithmetic end it"""
    exe, r = _build(tmp_path, "viewshed_host_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])
    if r.returncode != 0:
        pytest.skip("the host compiler cannot link the sanitizer runtimes: " + r.stderr[-300:])
    h = (tmp_path, exe)
    for name in ("one", "row", "column", "small", "steep", "wide", "many33", "many300", "graze", "row4096"):
        check_case(h, name)
    hh = V.heights(33, 65, 2)
    assert np.array_equal(run_quantise(h, hh, 65536.0), V.quantise(hh, 65536.0))
    # the largest heights and eyes the table can hold, corner to corner: the int64 arithmetic has room
    zq = np.zeros((40, 50), np.int32)
    zq[::3, ::2] = (1 << 31) - 1
    obs = [(0, 0, (1 << 31) - 1, -1), (39, 49, 0, -1), (20, 25, 5, 400)]
    top, out = run_sight(h, zq, obs, (1 << 31) - 1)
    want = V.viewshed(zq, obs, (1 << 31) - 1)
    for accel in (False, True):
        assert np.array_equal(out[accel][0], want[0]) and np.array_equal(out[accel][1], want[1])
