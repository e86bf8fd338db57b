"""Camera views of a heightmap and its texture: a heightfield ray caster on the GPU (csrc/render.hip).

    scene   hm [H, W] in [0, 1] and tex [3, H, W] in [0, 1]; axes (y, x, z): y down the rows, x along the columns, z up.
            Pixel (i, j) covers [i, i+1) x [j, j+1); the surface is h(y, x) = height_scale * bilinear(hm).
    camera  position (y, x, z), yaw, pitch (negative looks down), vertical field of view, image size.
            forward = (cos p cos w, cos p sin w, sin p), right = (sin w, -cos w, 0), up = (-sin p cos w, -sin p sin w, cos p).
    march   samples at t_k = k step; the first sample at or below the surface is the hit, refined by one secant step.
    colour  texture x (ambient + (1 - ambient) max(0, n.s) shadow), then haze towards the sky colour.  A scene built with
            ``sky=SkyLight(...)`` bakes the light of the sky once (skylight.py) and shades with
            ambient x bilinear(sky plane) in place of ambient.

A ``Scene`` uploads the two arrays once and builds the maximum pyramid once; every ``render`` after that is one launch and one
download.  ``Pix2Pix.render_terrain`` renders arrays the caller has, ``TerrainWorld.scene`` / ``TerrainWorld.view`` render the
unbounded world (the scene is assembled through the host: ``both`` -> upload; ``TerrainWorld.scene(resident=True)`` and
``TerrainWorld.flight`` assemble it on the device from the resident chunks).

    python -m gan_heightmaps_amd.render OUT.png (--heightmap F --texture F | --world EXPERIMENT MODEL --seed N
        [--chunk-cells C] [--blend B] [--dtype D] [--erode N]) --pos Y,X,Z (--look-at Y,X,Z | --yaw A --pitch A) [--fov DEG]
        [--size HxW] [--max-dist N] [--height-scale S] [--sun AZ,EL] [--no-shadows] [--haze V] [--step V]
        [--frames N --to Y,X,Z [--window-mb M]] [--sky [--sky-directions N] [--sky-steps N] [--sky-step X] [--sky-strength X]]
"""
import argparse
import math
import os
import re
import sys

import numpy as np

from . import util
from .util import is_int as _is_int

__all__ = ["DEFAULTS", "MAX_STEPS", "Camera", "Scene", "union_footprint", "parse_args", "main"]

# what gives a legible picture of a 512 x 512 generator output: relief an eighth of the tile's side, a low sun from the
# upper left of a north-up map, a quarter of ambient light, haze that takes a fifth of the contrast across one tile
FOV_DEG = 50.0
DEFAULTS = dict(height_scale=64.0, fov=math.radians(FOV_DEG), size=(480, 640), sun_azimuth=math.radians(225.0),
                sun_elevation=math.radians(28.0), softness=8.0, ambient=0.25, haze=0.0005, step=0.5,
                horizon=(0.80, 0.86, 0.92), zenith=(0.30, 0.50, 0.85))
MAX_STEPS = 1 << 20          # samples per ray the kernel accepts (REN_MAX_STEPS, csrc/render.hip)


def _num(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) and math.isfinite(v)


class Camera:
    """A pinhole camera in (y, x, z) coordinates: ``pos``, ``yaw`` (0 faces down the rows, pi/2 along the columns), ``pitch``
    (negative looks down), the vertical field of view ``fov`` (radians) and the image ``size`` (Hi, Wi)."""

    def __init__(self, pos, yaw, pitch, fov=DEFAULTS['fov'], size=DEFAULTS['size']):
        try:
            pos = tuple(pos)
        except TypeError:
            raise ValueError("pos must be (y, x, z), got %r" % (pos,))
        if len(pos) != 3 or not all(_num(v) for v in pos):
            raise ValueError("pos must be three finite numbers (y, x, z), got %r" % (pos,))
        if not _num(yaw) or not _num(pitch):
            raise ValueError("yaw and pitch must be finite numbers, got %r, %r" % (yaw, pitch))
        if abs(pitch) > math.pi / 2:
            raise ValueError("pitch must lie in [-pi/2, pi/2], got %r" % (pitch,))
        if not _num(fov) or not 0.0 < fov < math.pi:
            raise ValueError("fov must lie in (0, pi) radians, got %r" % (fov,))
        try:
            size = tuple(size)
        except TypeError:
            raise ValueError("size must be (Hi, Wi), got %r" % (size,))
        if len(size) != 2 or not all(_is_int(v) and v >= 1 for v in size) or size[0] * size[1] >= 1 << 31:
            raise ValueError("size must be two positive integers (Hi, Wi) with Hi Wi < 2^31, got %r" % (size,))
        self.pos = tuple(float(v) for v in pos)
        self.yaw, self.pitch, self.fov = float(yaw), float(pitch), float(fov)
        self.size = (int(size[0]), int(size[1]))

    @classmethod
    def look_at(cls, pos, target, fov=DEFAULTS['fov'], size=DEFAULTS['size']):
        """the camera at ``pos`` whose axis passes through ``target``"""
        p, t = np.asarray(pos, np.float64), np.asarray(target, np.float64)
        if p.shape != (3,) or t.shape != (3,) or not np.isfinite(p).all() or not np.isfinite(t).all():
            raise ValueError("pos and target must be three finite numbers each")
        d = t - p
        n = math.sqrt(float((d * d).sum()))
        if n == 0.0:
            raise ValueError("look_at: pos and target coincide")
        ground = math.hypot(d[0], d[1])
        yaw = math.atan2(d[1], d[0]) if ground > 0.0 else 0.0
        return cls(tuple(p), yaw, math.atan2(d[2], ground), fov=fov, size=size)

    def basis(self):
        """(forward, right, up) as float64 vectors"""
        cy, sy, cp, sp = math.cos(self.yaw), math.sin(self.yaw), math.cos(self.pitch), math.sin(self.pitch)
        return (np.array([cp * cy, cp * sy, sp]), np.array([sy, -cy, 0.0]), np.array([-sp * cy, -sp * sy, cp]))

    def moved(self, pos):
        return Camera(pos, self.yaw, self.pitch, self.fov, self.size)

    def footprint(self, max_dist):
        """the integer rectangle (y0, x0, h, w) that holds the (y, x) of every point any ray reaches within ``max_dist``,
        padded by 2 pixels.  The rays lie in the pyramid spanned by the image's four corners; a point within max_dist of the
        camera is at most max_dist deep along the axis, so the camera and the four corner rays cut at that DEPTH (not at that
        length: the far end of a bundle of unit rays is a spherical cap, which bulges beyond its corners) bound it."""
        if not _num(max_dist) or max_dist <= 0:
            raise ValueError("max_dist must be a positive number, got %r" % (max_dist,))
        fw, rt, up = self.basis()
        Hi, Wi = self.size
        f = (Hi / 2.0) / math.tan(self.fov / 2.0)
        pts = [np.asarray(self.pos[:2])]
        for a in (-Wi / 2.0, Wi / 2.0):
            for b in (-Hi / 2.0, Hi / 2.0):
                d = f * fw + a * rt - b * up
                pts.append(np.asarray(self.pos[:2]) + (max_dist / f) * d[:2])
        pts = np.array(pts)
        if not np.isfinite(pts).all() or np.abs(pts).max() >= 2.0 ** 40:
            raise ValueError("the footprint of this camera within %r is unbounded" % (max_dist,))
        y0, x0 = (int(math.floor(v)) - 2 for v in pts.min(0))
        y1, x1 = (int(math.ceil(v)) + 2 for v in pts.max(0))
        return y0, x0, y1 - y0, x1 - x0


def union_footprint(rects):
    """the smallest rectangle (y0, x0, h, w) around the given ones"""
    y0, x0 = min(r[0] for r in rects), min(r[1] for r in rects)
    y1, x1 = max(r[0] + r[2] for r in rects), max(r[1] + r[3] for r in rects)
    return y0, x0, y1 - y0, x1 - x0


def _unit_planes(a, grey, what):
    """an image as the generators / PNG readers give it -> float32 [C, H, W] in [0, 1], the way util.convert_to_rgb maps it:
    uint8 (H, W) / (H, W, C) by / 255; float32 (H, W) / (C, H, W) as it is (``grey``: already in [0, 1]) or from the tanh
    range by (127.5 v + 127.5) / 255; clipped to [0, 1]"""
    a = np.asarray(a)
    if a.dtype == np.uint8 and a.ndim in (2, 3):
        a = a[:, :, None] if a.ndim == 2 else a
        if a.shape[2] not in (1, 3):
            raise ValueError("%s: a uint8 image has 1 or 3 channels, got %d" % (what, a.shape[2]))
        return np.ascontiguousarray((a.astype(np.float32) / np.float32(255)).transpose(2, 0, 1))
    if a.dtype == np.float32 and a.ndim in (2, 3):
        a = a[None] if a.ndim == 2 else a
        if a.shape[0] not in (1, 3):
            raise ValueError("%s: a float32 image is (H, W), (1, H, W) or (3, H, W), got %s" % (what, a.shape))
        if not np.isfinite(a).all():
            raise ValueError("%s has non-finite values" % what)
        rgb = util.convert_to_rgb(a, is_grayscale=grey)                       # [H, W, 3], clipped
        return np.ascontiguousarray(rgb.transpose(2, 0, 1)[:a.shape[0]], np.float32)
    raise ValueError("%s must be uint8 (H, W) / (H, W, C) or float32 (H, W) / (C, H, W), got %s %s" % (what, a.dtype, a.shape))


def _check_sky(sky, margin):
    from .skylight import SkyLight
    if sky is not None and not isinstance(sky, SkyLight):
        raise ValueError("sky must be a skylight.SkyLight, got %r" % (sky,))
    if not _is_int(margin) or margin < 0:
        raise ValueError("margin must be an integer >= 0, got %r" % (margin,))
    return sky, int(margin)


class Scene:
    """A heightmap and its texture resident on the GPU, ready to be looked at.

    heightmap, texture: uint8 (H, W) / (H, W, C), or float32 (H, W) / (C, H, W) in the generators' output range.
    value_range: (heightmap_is_unit, texture_is_unit) -- the model's (is_a_grayscale, is_b_grayscale): True means the float
    values are already in [0, 1], False the tanh range; None takes one-channel arrays as unit and three-channel ones as tanh.
    A three-channel heightmap gives the mean of its channels as height; a one-channel texture is replicated.
    origin: the world coordinates (Y0, X0) of the scene's first pixel; cameras are given in world coordinates.
    sky: a skylight.SkyLight: the scene bakes the light of the sky once, after the pyramid, and every render shades with it
    (DESIGN §4r).  margin = m > 0: the heightmap is (H + 2m, W + 2m), the texture (H, W), and the scene is the interior; the
    apron feeds the bake alone (m = sky.reach makes the plane independent of the scene's borders) and is freed after it."""

    def __init__(self, heightmap, texture, origin=(0, 0), height_scale=DEFAULTS['height_scale'], value_range=None,
                 device=None, sky=None, margin=0):
        if len(tuple(origin)) != 2 or not all(_is_int(v) for v in origin):
            raise ValueError("origin must be two integers (Y0, X0), got %r" % (origin,))
        if not _num(height_scale) or height_scale <= 0:
            raise ValueError("height_scale must be a positive number, got %r" % (height_scale,))
        if value_range is None:
            value_range = (None, None)
        hg, tg = value_range

        def grey(a, g):
            a = np.asarray(a)
            return bool(g) if g is not None else (a.ndim == 2 or a.shape[0] == 1)
        hm = _unit_planes(heightmap, grey(heightmap, hg), "heightmap")
        tex = _unit_planes(texture, grey(texture, tg), "texture")
        hm = hm[0] if hm.shape[0] == 1 else hm.astype(np.float64).mean(0).astype(np.float32)
        tex = np.ascontiguousarray(np.broadcast_to(tex, (3,) + tex.shape[1:]))
        sky, margin = _check_sky(sky, margin)
        grown = hm
        if margin:
            if hm.shape[0] <= 2 * margin or hm.shape[1] <= 2 * margin:
                raise ValueError("a heightmap of %s has no interior inside a margin of %d" % (hm.shape, margin))
            hm = np.ascontiguousarray(hm[margin:-margin, margin:-margin])
        if hm.shape != tex.shape[1:]:
            raise ValueError("heightmap %s and texture %s differ in size" % (hm.shape, tex.shape[1:]))
        H, W = hm.shape
        if H < 2 or W < 2 or H * W >= 1 << 31:
            raise ValueError("a scene is at least 2 x 2 and below 2^31 pixels, got %d x %d" % (H, W))
        from .device import Device, Ops
        self.origin = (int(origin[0]), int(origin[1]))
        self.height_scale = float(height_scale)
        self.shape = (H, W)
        self._own = device is None
        self.dev = Device(int(os.environ.get("LOCAL_RANK", "0"))) if device is None else device
        self.ops = Ops(self.dev)
        self._hm = self._tex = self._mip = self._sky = None
        self._outbuf, self._outbytes = None, 0
        self.sky = sky
        src = None
        try:
            self._hm = self.dev.alloc(hm.nbytes)
            self.dev.h2d(self._hm, hm)
            self._tex = self.dev.alloc(tex.nbytes)
            self.dev.h2d(self._tex, tex)
            self._mip = self.ops.render_maxmip(self._hm, H, W)
            if sky is not None and margin:
                src = self.dev.alloc(grown.nbytes)
                self.dev.h2d(src, grown)
            src = self._bake_sky(src, margin)
        except Exception:
            if src:
                self.dev.free(src)
            self.close()
            raise

    @classmethod
    def from_device(cls, dev, hm_ptr, tex_ptr, H, W, origin=(0, 0), height_scale=DEFAULTS['height_scale'], sky=None,
                    sky_src=None, margin=0):
        """a Scene over two buffers that are already on ``dev`` and already hold what the constructor would upload: hm fp32
        [H, W] in [0, 1] and tex fp32 [3, H, W] in [0, 1], both allocated with dev.alloc.  The scene takes ownership of them
        (close() frees them, and so does a failure in here); nothing is uploaded, the pyramid is built as usual.
        sky: a skylight.SkyLight, baked after the pyramid from sky_src: the height plane grown by ``margin`` all round, fp32
        [H + 2 margin, W + 2 margin] from dev.alloc, owned in the same way and freed after the bake (None with margin = 0:
        the bake reads hm itself)."""
        self = cls.__new__(cls)
        self.dev, self._own = dev, False
        self._hm, self._tex, self._mip, self._sky = hm_ptr, tex_ptr, None, None
        self._outbuf, self._outbytes = None, 0
        self.sky = None
        try:
            self.sky, margin = _check_sky(sky, margin)
            if (sky_src is not None) != (self.sky is not None and margin > 0):
                raise ValueError("sky_src is the grown height plane of a scene with sky and margin > 0, and of no other")
            if len(tuple(origin)) != 2 or not all(_is_int(v) for v in origin):
                raise ValueError("origin must be two integers (Y0, X0), got %r" % (origin,))
            if not _num(height_scale) or height_scale <= 0:
                raise ValueError("height_scale must be a positive number, got %r" % (height_scale,))
            if not _is_int(H) or not _is_int(W) or H < 2 or W < 2 or H * W >= 1 << 31:
                raise ValueError("a scene is at least 2 x 2 and below 2^31 pixels, got %r x %r" % (H, W))
            if not hm_ptr or not tex_ptr:
                raise ValueError("from_device needs the two device buffers")
            from .device import Ops
            self.origin = (int(origin[0]), int(origin[1]))
            self.height_scale = float(height_scale)
            self.shape = (int(H), int(W))
            self.ops = Ops(dev)
            self._mip = self.ops.render_maxmip(self._hm, self.shape[0], self.shape[1])
            sky_src = self._bake_sky(sky_src, margin)
        except Exception:
            if sky_src:
                dev.sync()
                dev.free(sky_src)
            self.close()
            raise
        return self

    def _bake_sky(self, src, margin):
        """bake the scene's sky plane from ``src`` (the height plane grown by ``margin``, freed here; None: the scene's own
        plane); returns None, the pointer the caller still owns"""
        if self.sky is None:
            return None
        from .skylight import bake_device
        H, W = self.shape
        self._sky = self.dev.alloc(4 * H * W)
        bake_device(self.ops, src if src else self._hm, H + 2 * margin, W + 2 * margin, self.sky, self.height_scale,
                    self._sky, margin=margin)
        if src:
            self.dev.sync()
            self.dev.free(src)
        return None

    def sky_plane(self):
        """the baked light of the sky, downloaded: float32 [H, W] in [0, 1]"""
        if self.dev is None:
            raise ValueError("this Scene is closed")
        if self._sky is None:
            raise ValueError("this Scene was built without sky=")
        out = np.empty(self.shape, np.float32)
        self.dev.d2h(out, self._sky, out.nbytes)
        return out

    def arrays(self):
        """the scene's planes as the renderer reads them, downloaded: (hm [H, W], tex [3, H, W]), float32 in [0, 1]"""
        if self.dev is None:
            raise ValueError("this Scene is closed")
        H, W = self.shape
        hm, tex = np.empty((H, W), np.float32), np.empty((3, H, W), np.float32)
        self.dev.d2h(hm, self._hm, hm.nbytes)
        self.dev.d2h(tex, self._tex, tex.nbytes)
        return hm, tex

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def close(self):
        dev = self.dev
        if dev is None:
            return
        if dev.h is not None:
            dev.sync()
            for p in (self._hm, self._tex, self._mip.ptr if self._mip else None, self._sky, self._outbuf):
                if p:
                    dev.free(p)
            if self._own:
                dev.close()
        self._hm = self._tex = self._mip = self._sky = self._outbuf = None
        self.dev = None

    def default_max_dist(self, camera):
        """the distance from the camera to the farthest corner of the scene's box: no ray needs more"""
        H, W = self.shape
        py, px, pz = camera.pos[0] - self.origin[0], camera.pos[1] - self.origin[1], camera.pos[2]
        return math.sqrt(max(abs(py), abs(py - H)) ** 2 + max(abs(px), abs(px - W)) ** 2
                         + max(abs(pz), abs(pz - self.height_scale)) ** 2) + 1.0

    def render(self, camera, sun_azimuth=DEFAULTS['sun_azimuth'], sun_elevation=DEFAULTS['sun_elevation'], shadows=True,
               softness=DEFAULTS['softness'], ambient=DEFAULTS['ambient'], haze=DEFAULTS['haze'], step=DEFAULTS['step'],
               max_dist=None, uint8=True, out=None, accel=True, horizon=DEFAULTS['horizon'], zenith=DEFAULTS['zenith'],
               depth=None):
        """one image: uint8 (Hi, Wi, 3), or with uint8=False float32 (3, Hi, Wi); ``out`` (that shape and dtype,
        C-contiguous) is written in place of a new array.  One launch and one download.  ``depth``: a C-contiguous float32
        (Hi, Wi) array that receives t_hit per pixel, +inf for sky (a second download)."""
        from .device import render_params
        if self.dev is None:
            raise ValueError("this Scene is closed")
        if not isinstance(camera, Camera):
            raise ValueError("camera must be a Camera, got %r" % (camera,))
        for name, v in (("sun_azimuth", sun_azimuth), ("sun_elevation", sun_elevation), ("softness", softness),
                        ("ambient", ambient), ("haze", haze), ("step", step)):
            if not _num(v):
                raise ValueError("%s must be a finite number, got %r" % (name, v))
        if step <= 0 or softness < 0 or haze < 0 or not 0.0 <= ambient <= 1.0:
            raise ValueError("step > 0, softness >= 0, haze >= 0 and 0 <= ambient <= 1 are required")
        if max_dist is None:
            max_dist = self.default_max_dist(camera)
        if not _num(max_dist) or max_dist <= 0:
            raise ValueError("max_dist must be a positive number, got %r" % (max_dist,))
        if math.floor(max_dist / step) > MAX_STEPS:
            raise ValueError("max_dist / step = %d samples per ray; at most %d" % (math.floor(max_dist / step), MAX_STEPS))
        Hi, Wi = camera.size
        shape, dtype = ((Hi, Wi, 3), np.uint8) if uint8 else ((3, Hi, Wi), np.float32)
        if out is None:
            out = np.empty(shape, dtype)
        elif not isinstance(out, np.ndarray) or out.shape != shape or out.dtype != dtype or not out.flags['C_CONTIGUOUS']:
            raise ValueError("out must be a C-contiguous %s array of shape %s" % (np.dtype(dtype), shape))
        pos = (camera.pos[0] - self.origin[0], camera.pos[1] - self.origin[1], camera.pos[2])
        p = render_params(pos, camera.yaw, camera.pitch, camera.fov, camera.size, self.height_scale, step, max_dist,
                          sun_azimuth, sun_elevation, shadows, softness, ambient, haze, horizon, zenith, accel=accel,
                          out_u8=uint8)
        if depth is not None and (not isinstance(depth, np.ndarray) or depth.shape != (Hi, Wi) or depth.dtype != np.float32
                                  or not depth.flags['C_CONTIGUOUS']):
            raise ValueError("depth must be a C-contiguous float32 array of shape %s" % ((Hi, Wi),))
        need = out.nbytes + (4 * Hi * Wi + 16 if depth is not None else 0)
        if need > self._outbytes:
            if self._outbuf:
                self.dev.sync()
                self.dev.free(self._outbuf)
            self._outbuf, self._outbytes = self.dev.alloc(need), need
        H, W = self.shape
        dptr = self._outbuf + (out.nbytes + 15) // 16 * 16 if depth is not None else None
        if self._sky is None:
            self.ops.render_view(p, self._hm, self._tex, H, W, self._mip, self._outbuf, dptr)
        else:
            self.ops.render_view_sky(p, self._hm, self._tex, self._sky, H, W, self._mip, self._outbuf, dptr)
        self.dev.d2h(out, self._outbuf, out.nbytes)
        if depth is not None:
            self.dev.d2h(depth, dptr, depth.nbytes)
        return out


# ---- command line -------------------------------------------------------------------------------------------------------
def _triple(text):
    m = re.fullmatch(r"\s*([^,\s]+)\s*,\s*([^,\s]+)\s*,\s*([^,\s]+)\s*", text)
    try:
        v = tuple(float(g) for g in m.groups())
    except (AttributeError, ValueError):
        raise argparse.ArgumentTypeError("wants Y,X,Z, got %r" % (text,))
    if not all(math.isfinite(c) for c in v):
        raise argparse.ArgumentTypeError("wants three finite numbers, got %r" % (text,))
    return v


def _pair(text):
    m = re.fullmatch(r"\s*([^,\s]+)\s*,\s*([^,\s]+)\s*", text)
    try:
        v = tuple(float(g) for g in m.groups())
    except (AttributeError, ValueError):
        raise argparse.ArgumentTypeError("wants AZ,EL in degrees, got %r" % (text,))
    if not all(math.isfinite(c) for c in v):
        raise argparse.ArgumentTypeError("wants two finite numbers, got %r" % (text,))
    return v


def _size(text):
    m = re.fullmatch(r"\s*(\d+)\s*[xX]\s*(\d+)\s*", text)
    if not m or int(m.group(1)) < 1 or int(m.group(2)) < 1:
        raise argparse.ArgumentTypeError("--size wants HxW, got %r" % (text,))
    return int(m.group(1)), int(m.group(2))


_NEGATIVE_OK = ("--pos", "--look-at", "--to", "--sun", "--yaw", "--pitch")


def parse_args(argv):
    p = argparse.ArgumentParser(prog="python -m gan_heightmaps_amd.render",
                                description="Render a camera view of a heightmap and its texture, or of the unbounded world "
                                            "of a seed.  Angles are in degrees; coordinates are Y,X,Z in pixels.")
    p.add_argument("output", help="the image (.png); with --frames N the frames go to OUT_0000.png ...")
    p.add_argument("--heightmap", help="heightmap: 8-bit PNG, or .npy (uint8 (H, W) / (H, W, C), or float32 (C, H, W))")
    p.add_argument("--texture", help="texture of the same size: 8-bit PNG or .npy")
    p.add_argument("--world", nargs=2, metavar=("EXPERIMENT", "MODEL"), help="render the world of a trained model instead")
    p.add_argument("--seed", type=int, default=None, help="the world's seed (with --world)")
    p.add_argument("--chunk-cells", type=int, default=None, help="generator cells per chunk side (with --world)")
    p.add_argument("--blend", default=None, choices=["mosaic", "bilinear"], help="how cells meet (with --world)")
    p.add_argument("--dtype", default=None, choices=["f32", "bf16x3", "bf16x2", "bf16", "f16"],
                   help="arithmetic of the convolutions (with --world; default bf16x3)")
    p.add_argument("--erode", type=int, default=None, metavar="N",
                   help="erode the world with N iterations of the water simulation (with --world)")
    p.add_argument("--pos", type=_triple, required=True, metavar="Y,X,Z", help="the camera's position")
    p.add_argument("--look-at", type=_triple, default=None, metavar="Y,X,Z", help="a point on the camera's axis")
    p.add_argument("--yaw", type=float, default=None, help="degrees; 0 faces down the rows, 90 along the columns")
    p.add_argument("--pitch", type=float, default=None, help="degrees; negative looks down")
    p.add_argument("--fov", type=float, default=FOV_DEG, help="vertical field of view in degrees")
    p.add_argument("--size", type=_size, default=DEFAULTS['size'], metavar="HxW", help="image size (default 480x640)")
    p.add_argument("--max-dist", type=float, default=None, help="how far a ray goes (needed with --world)")
    p.add_argument("--height-scale", type=float, default=DEFAULTS['height_scale'], help="pixels per unit height")
    p.add_argument("--sun", type=_pair, default=None, metavar="AZ,EL", help="the sun's azimuth and elevation in degrees")
    p.add_argument("--no-shadows", action="store_true", help="leave out the shadow march")
    p.add_argument("--haze", type=float, default=DEFAULTS['haze'], help="haze density per pixel of distance")
    p.add_argument("--step", type=float, default=DEFAULTS['step'], help="distance between samples")
    p.add_argument("--frames", type=int, default=None, help="render N frames, moving the camera to --to")
    p.add_argument("--to", type=_triple, default=None, metavar="Y,X,Z", help="the camera's position in the last frame")
    p.add_argument("--window-mb", type=float, default=None, metavar="M",
                   help="with --world and --frames: render the path through TerrainWorld.flight, from scene windows of at "
                        "most M MiB built on the device one after the other (default: one scene over the whole path)")
    p.add_argument("--sky", action="store_true", help="light the ground from the sky: bake a horizon scan per scene "
                                                      "(gan_heightmaps_amd.skylight) and dim the ambient light by it")
    p.add_argument("--sky-directions", type=int, default=None, help="azimuths of the scan (with --sky)")
    p.add_argument("--sky-steps", type=int, default=None, help="samples per azimuth (with --sky)")
    p.add_argument("--sky-step", type=float, default=None, help="pixels between samples (with --sky)")
    p.add_argument("--sky-strength", type=float, default=None, help="how far the visibility dims the light, in [0, 1]")
    # a value that starts with a minus sign would read as an option: hand it over in the --opt=value form
    argv = list(argv)
    i = 0
    while i < len(argv) - 1:
        if argv[i] in _NEGATIVE_OK and re.match(r"\s*-[\d.]", argv[i + 1]):
            argv[i:i + 2] = [argv[i] + "=" + argv[i + 1]]
        i += 1
    a = p.parse_args(argv)
    files = a.heightmap is not None or a.texture is not None
    if files == (a.world is not None):
        p.error("give either --heightmap and --texture, or --world EXPERIMENT MODEL")
    if files and (a.heightmap is None or a.texture is None):
        p.error("--heightmap and --texture go together")
    if a.world is not None:
        if a.seed is None:
            p.error("--world needs --seed")
        if a.max_dist is None:
            p.error("--world needs --max-dist: an unbounded world has no farthest corner")
        if a.chunk_cells is not None and a.chunk_cells < 1:
            p.error("--chunk-cells must be >= 1")
        if a.erode is not None and a.erode < 1:
            p.error("--erode must be >= 1")
    elif a.seed is not None or a.chunk_cells is not None or a.blend is not None or a.dtype is not None \
            or a.erode is not None:
        p.error("--seed / --chunk-cells / --blend / --dtype / --erode need --world")
    if (a.look_at is not None) == (a.yaw is not None or a.pitch is not None):
        p.error("give either --look-at, or --yaw and --pitch")
    if a.look_at is None and (a.yaw is None or a.pitch is None):
        p.error("--yaw and --pitch go together")
    if a.look_at is not None and a.look_at == a.pos:
        p.error("--look-at equals --pos")
    if a.pitch is not None and abs(a.pitch) > 90:
        p.error("--pitch must lie in [-90, 90]")
    if not 0 < a.fov < 180:
        p.error("--fov must lie in (0, 180)")
    if a.max_dist is not None and not a.max_dist > 0:
        p.error("--max-dist must be > 0")
    if not a.height_scale > 0 or not a.step > 0 or not a.haze >= 0:
        p.error("--height-scale and --step must be > 0, --haze >= 0")
    if (a.frames is None) != (a.to is None):
        p.error("--frames and --to go together")
    if a.frames is not None and a.frames < 2:
        p.error("--frames must be >= 2")
    if a.window_mb is not None and (a.world is None or a.frames is None):
        p.error("--window-mb needs --world and --frames")
    if a.window_mb is not None and not a.window_mb > 0:
        p.error("--window-mb must be > 0")
    if not a.output.endswith(".png"):
        p.error("the output must be a .png")
    skw = {k: getattr(a, "sky_" + k) for k in ("directions", "steps", "step", "strength") if getattr(a, "sky_" + k) is not None}
    if skw and not a.sky:
        p.error("--sky-directions / --sky-steps / --sky-step / --sky-strength need --sky")
    a.skylight = None
    if a.sky:
        from .skylight import SkyLight
        try:
            a.skylight = SkyLight(**skw)
        except ValueError as e:
            p.error(str(e))
    return a


def cameras_of(a):
    """the cameras of the frames the parsed arguments ask for"""
    n = a.frames or 1
    out = []
    for i in range(n):
        s = i / (n - 1.0) if n > 1 else 0.0
        pos = tuple(p + s * (q - p) for p, q in zip(a.pos, a.to)) if a.to is not None else a.pos
        if a.look_at is not None:
            out.append(Camera.look_at(pos, a.look_at, fov=math.radians(a.fov), size=a.size))
        else:
            out.append(Camera(pos, math.radians(a.yaw), math.radians(a.pitch), fov=math.radians(a.fov), size=a.size))
    return out


def frame_names(a):
    if a.frames is None:
        return [a.output]
    return ["%s_%04d.png" % (a.output[:-4], i) for i in range(a.frames)]


def main(argv=None):
    a = parse_args(sys.argv[1:] if argv is None else argv)
    cams = cameras_of(a)
    kw = dict(shadows=not a.no_shadows, haze=a.haze, step=a.step, max_dist=a.max_dist)
    if a.sun is not None:
        kw.update(sun_azimuth=math.radians(a.sun[0]), sun_elevation=math.radians(a.sun[1]))
    model = world = scene = None
    try:
        if a.world is not None:
            from .experiments import make_model
            model = make_model(a.world[0], dtype=a.dtype or "bf16x3", verbose=False)
            model.load_model(a.world[1], mode='both')
            wkw = {k: v for k, v in (("chunk_cells", a.chunk_cells), ("blend", a.blend)) if v is not None}
            if a.erode is not None:
                from .erosion import Erosion
                wkw["erosion"] = Erosion(iterations=a.erode)
            world = model.terrain_world(a.seed, **wkw)
            if a.window_mb is not None:
                # a window after the other, each built on the device: memory does not grow with the path
                fkw = {k: v for k, v in kw.items() if k != "max_dist"}
                for name, img in zip(frame_names(a), world.flight(cams, a.max_dist, window_mb=a.window_mb,
                                                                  height_scale=a.height_scale, sky=a.skylight, **fkw)):
                    util.save_png(name, img)
                return 0
            # one scene over the union of the frames' footprints
            scene = world.scene(*union_footprint([c.footprint(a.max_dist) for c in cams]), height_scale=a.height_scale,
                                sky=a.skylight)
        else:
            scene = Scene(util.read_image(a.heightmap), util.read_image(a.texture), height_scale=a.height_scale,
                          sky=a.skylight)
        for cam, name in zip(cams, frame_names(a)):
            util.save_png(name, scene.render(cam, **kw))
    finally:
        if scene is not None:
            scene.close()
        if world is not None:
            world.close()
        if model is not None:
            model.device.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
