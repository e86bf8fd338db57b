"""The device code of csrc/render.hip compiled for the CPU (tests/render_host/harness.cpp): the same source text the GPU
runs, so the accelerated march's bit identity with the plain one and the kernel's agreement with the float64 restatement
are checked without a GPU too.  The CPU's libm stands in for the device's sqrt / exp, everything else is the kernel's own
arithmetic (no contraction, as on the device)."""
import importlib.util
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import render_ref as R
from tests.test_render_plan import F32_DEV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gan_heightmaps_amd", "csrc")
TOL = 8 * F32_DEV


def _compiler():
    spec = importlib.util.spec_from_file_location("ghm_build_for_host", os.path.join(CSRC, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    clang = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(mod.HIPCC))), "llvm", "bin", "clang++")
    for c in (clang, shutil.which("clang++"), shutil.which("g++")):
        if c and os.path.exists(c):
            return c
    pytest.fail("no host C++ compiler beside hipcc")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("render_host")
    src = open(os.path.join(CSRC, "render.hip")).read()
    head, sep, _ = src.partition('extern "C" {')
    assert sep and '#include "common.h"' in head
    inc = d / "render_device.inc"
    inc.write_text(head.replace('#include "common.h"', ""))
    exe = d / "render_host"
    cmd = [_compiler(), "-x", "c++", "-std=c++17", "-O2", "-ffp-contract=off", '-DRENDER_DEVICE_INC="%s"' % inc,
           os.path.join(ROOT, "tests", "render_host", "harness.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return d, exe


def run(harness, hm, tex, cam, size, hs, shadows, **kw):
    d, exe = harness
    a = dict(R.VIEW_KW)
    a.update(kw)
    H, W = hm.shape
    (d / "in.bin").write_bytes(np.ascontiguousarray(hm, np.float32).tobytes() + np.ascontiguousarray(tex, np.float32).tobytes())
    args = [H, W, size[0], size[1], a['step'], a['max_dist'], *cam['pos'], cam['yaw'], cam['pitch'], cam['fov'], hs,
            a['sun_azimuth'], a['sun_elevation'], a['softness'], a['ambient'], a['haze'], int(shadows)]
    r = subprocess.run([str(exe)] + [repr(v) for v in args] + [str(d / "in.bin"), str(d / "out.bin")])
    assert r.returncode == 0
    raw = np.fromfile(d / "out.bin", np.float32)
    n = size[0] * size[1]
    out = []
    for k in range(2):
        part = raw[4 * n * k:4 * n * (k + 1)]
        out.append((part[:3 * n].reshape((3,) + tuple(size)), part[3 * n:].reshape(size)))
    return out


@pytest.mark.parametrize("shadows", [False, True])
def test_nine_views_on_the_host_build(harness, shadows):
    for seed, cam in R.views():
        hm, tex = R.terrain(seed)
        (plain, pd), (acc, ad) = run(harness, hm, tex, R.CAMERAS[cam], R.VIEW_SIZE, R.HEIGHT_SCALE, shadows)
        assert plain.tobytes() == acc.tobytes() and pd.tobytes() == ad.tobytes(), (seed, cam)        # bit for bit
        want, want_t = R.reference(seed, cam, shadows, 'float64')
        err = np.abs(acc.astype(np.float64) - want).max(0)
        print("seed %d camera %d shadows %d: max err %.3e" % (seed, cam, shadows, err.max()))
        # with the CPU's libm the kernel's arithmetic is the float32 restatement's up to operation order: no pixel may fail
        assert (err <= TOL).all() and np.array_equal(np.isfinite(ad), np.isfinite(want_t)), (seed, cam, err.max())


def _odd_terrain(H, W, seed):
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    hm = 0.5 + 0.25 * np.sin(0.11 * yy + 0.3) * np.cos(0.09 * xx) + 0.2 * np.sin(0.05 * (yy + xx))
    hm += rng.uniform(0, 0.05, (H, W))
    return np.clip(hm, 0, 1).astype(np.float32), rng.uniform(0, 1, (3, H, W)).astype(np.float32)


@pytest.mark.parametrize("H,W,size,cam,hs,kw", [
    (97, 83, (33, 65), dict(pos=(8.2, 40.7, 35.0), yaw=0.2, pitch=-0.4, fov=1.0), 20.0, dict(max_dist=120.0, step=0.37)),
    (97, 83, (7, 5), dict(pos=(-40.3, 30.1, 30.0), yaw=0.15, pitch=-0.3, fov=1.0), 20.0, dict(max_dist=200.0)),
    (2, 2, (24, 24), dict(pos=(-3.1, 1.2, 4.0), yaw=0.1, pitch=-0.6, fov=0.9), 2.0, dict(max_dist=20.0, step=0.25)),
    (16, 300, (20, 30), dict(pos=(2.0, -50.0, 30.0), yaw=1.5, pitch=-0.1, fov=1.0), 10.0, dict(max_dist=400.0)),
    (600, 500, (40, 56), dict(pos=(-20.0, 250.0, 90.0), yaw=0.05, pitch=-0.08, fov=1.0), 80.0, dict(max_dist=900.0)),
])
def test_skipping_keeps_the_bits_on_odd_shapes(harness, H, W, size, cam, hs, kw):
    hm, tex = _odd_terrain(H, W, H + W)
    for shadows in (False, True):
        (plain, pd), (acc, ad) = run(harness, hm, tex, cam, size, hs, shadows, **kw)
        assert plain.tobytes() == acc.tobytes() and pd.tobytes() == ad.tobytes()
        assert np.isfinite(pd).any() and (plain >= 0).all()
