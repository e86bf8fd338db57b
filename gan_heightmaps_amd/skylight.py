"""The light of the sky on a heightmap: a horizon scan baked on the device (csrc/skylight.hip).

The renderer's ambient term is one constant; what the sun does not reach gets the same flat share of the texture.  ``bake``
computes, per texel, how much of a uniform sky a horizontal patch of ground there receives: in ``directions`` azimuths it
finds the horizon the surrounding heights raise within ``steps * step`` pixels, and averages the light each leaves.

The host builds, in float64, a table of directions x steps samples.  Direction d has azimuth phi = 2 pi d / directions and
unit vector (cos phi, sin phi) in (y, x); sample m = 1 .. steps lies at the offset o = m step (cos phi, sin phi) from the
texel's centre: iy = floor(o_y), ix = floor(o_x), wy = float32(o_y - iy), wx = float32(o_x - ix), inv_r = float32(1 / (m step)).
For the texel (i, j) of a height plane p in [0, 1], h0 = p[i, j], every index clamped to the plane, per direction:

    a, b, c, e = p[i+iy, j+ix], p[i+iy, j+ix+1], p[i+iy+1, j+ix], p[i+iy+1, j+ix+1]
    t = a + wx (b - a);  u = c + wx (e - c);  hv = t + wy (u - t)
    T = max(0, max_m (hv - h0) inv_r);  q = height_scale T;  vis = 1 / (1 + q q)

and V = (sum of vis in the order d = 0, 1, ...) / directions, sky = 1 - strength (1 - V).  vis = cos^2 of the horizon's
elevation is the share of a uniform sky's light a horizontal patch receives over that horizon.  Every operation is rounded on
its own in float32, in the order written.  Positions enter through the integer offsets and the table's weights alone, never
through an absolute coordinate: the value at a pixel is the same in whatever window it is baked, as long as the window
holds ``reach`` more pixels all round (``margin``); without them the plane is clamped at its edges.

    python -m gan_heightmaps_amd.skylight IN OUT [--directions N] [--steps N] [--step X] [--strength X] [--height-scale X]
        [--plain | --tiled]
"""
import argparse
import dataclasses
import functools
import sys

import numpy as np

from .planes import as_plane, check_size, scratch
from .util import form_choice, is_int as _is_int, is_number as _number, read_image

__all__ = ["DEFAULT_TILED", "MAX_DIRECTIONS", "MAX_STEPS", "SkyLight", "bake", "bake_device", "parse_args", "main"]

MAX_DIRECTIONS = 64          # GHM_SKYLIGHT_MAX_DIRECTIONS (include/ghm.h)
MAX_STEPS = 256              # GHM_SKYLIGHT_MAX_STEPS
# the form ``bake`` and the scenes run by default: the one tools/skylight_bench.py shows faster on the MI355X -- the tiled
# one, 2.61 against 7.37 ms for a 4096 x 4096 plane with the default SkyLight (DESIGN §4r has the line); both give the same bits
DEFAULT_TILED = True
# one table entry as the kernels read it: ghm_skylight_sample (include/ghm.h)
SAMPLE_DTYPE = np.dtype([("iy", np.int32), ("ix", np.int32), ("wy", np.float32), ("wx", np.float32), ("inv_r", np.float32)])


@dataclasses.dataclass(frozen=True)
class SkyLight:
    """The parameters of a sky-light bake, validated and frozen: ``directions`` azimuths (1 .. 64), ``steps`` samples per
    azimuth (1 .. 256) ``step`` pixels apart (> 0), and the ``strength`` in [0, 1] with which the sky's visibility dims the
    ambient light (0: not at all)."""
    directions: int = 16
    steps: int = 24
    step: float = 1.5
    strength: float = 1.0

    def __post_init__(self):
        for k, hi in (("directions", MAX_DIRECTIONS), ("steps", MAX_STEPS)):
            v = getattr(self, k)
            if not _is_int(v) or not 1 <= v <= hi:
                raise ValueError("%s must be an integer in [1, %d], got %r" % (k, hi, v))
            object.__setattr__(self, k, int(v))
        if not _number(self.step) or not self.step > 0:
            raise ValueError("step must be a finite number > 0, got %r" % (self.step,))
        if not _number(self.strength) or not 0.0 <= self.strength <= 1.0:
            raise ValueError("strength must lie in [0, 1], got %r" % (self.strength,))
        object.__setattr__(self, "step", float(self.step))
        object.__setattr__(self, "strength", float(self.strength))
        if self.steps * self.step >= 1 << 24 or not 1.0 / self.step < 3e38:
            raise ValueError("step = %r is out of range (steps * step < 2^24, 1 / step finite in float32)" % (self.step,))

    def table(self):
        """the directions x steps samples, direction-major, as a structured array of SAMPLE_DTYPE"""
        d = np.arange(self.directions, dtype=np.float64)[:, None]
        r = np.arange(1, self.steps + 1, dtype=np.float64)[None, :] * self.step
        phi = 2.0 * np.pi * d / self.directions
        oy, ox = r * np.cos(phi), r * np.sin(phi)
        iy, ix = np.floor(oy), np.floor(ox)
        t = np.empty((self.directions, self.steps), SAMPLE_DTYPE)
        t["iy"], t["ix"] = iy.astype(np.int32), ix.astype(np.int32)
        t["wy"], t["wx"] = (oy - iy).astype(np.float32), (ox - ix).astype(np.float32)
        t["inv_r"] = np.broadcast_to((1.0 / r).astype(np.float32), t.shape)
        return t

    @functools.cached_property
    def reach(self):
        """pixels the table reads away from a texel: the largest of max(-iy, iy + 1, -ix, ix + 1) over its entries (not
        ceil(steps step) + 1, which overshoots).  A texel this far from every edge does not feel the clamping."""
        t = self.table()
        return int(max((-t["iy"]).max(), (t["iy"] + 1).max(), (-t["ix"]).max(), (t["ix"] + 1).max()))


def _check_sky(sky):
    sky = SkyLight() if sky is None else sky
    if not isinstance(sky, SkyLight):
        raise ValueError("sky must be a SkyLight, got %r" % (sky,))
    return sky


def _check_scale(height_scale):
    if not _number(height_scale) or not height_scale > 0 or not np.float32(height_scale) < np.float32(3e38):
        raise ValueError("height_scale must be a finite number > 0, got %r" % (height_scale,))
    return float(height_scale)


_plane = functools.partial(as_plane, lead=False)


def use_tiled(ops, sky, tiled):
    """the form to run: ``tiled`` (None: DEFAULT_TILED), or the plain one where the tiled form's window does not fit in LDS"""
    tiled = DEFAULT_TILED if tiled is None else bool(tiled)
    return tiled and ops.skylight_lds_bytes(sky.reach) > 0


def bake_device(ops, src_ptr, rows, cols, sky, height_scale, out_ptr, margin=0, uint8=False, tiled=None):
    """the bake between two device planes: the interior (rows - 2 margin) x (cols - 2 margin) of the fp32 plane [rows, cols]
    at src_ptr -> out_ptr, fp32 or uint8.  One launch, asynchronous."""
    h, w = rows - 2 * margin, cols - 2 * margin
    ops.skylight_bake(src_ptr, rows, cols, cols, ops.skylight_table(sky), sky.directions, sky.steps, sky.reach, margin,
                      margin, h, w, height_scale, sky.strength, use_tiled(ops, sky, tiled), uint8, out_ptr, w)


def bake(ops, heightmap, sky=None, height_scale=64.0, margin=0, out=None, uint8=False, tiled=None):
    """The sky light of a heightmap, baked on the device: upload, one launch, download.
    ops: a device.Ops; heightmap: (H + 2 margin, W + 2 margin), floating point in [0, 1] or uint8; sky: a SkyLight (default
    SkyLight()); height_scale: pixels per unit height, the renderer's.  The plane is clamped at the array's edges; with
    margin = sky.reach the (H, W) interior is what any larger map gives there, bit for bit.  tiled: the LDS form (True) or
    the plain one (False): the same bits; default DEFAULT_TILED; where the tiled form's window exceeds its LDS budget the
    plain form runs.  Returns the (H, W) interior as float32 in [0, 1], or with uint8=True as uint8 (rint(255 v), half to
    even); ``out`` (that shape and dtype) is written in place of a new array."""
    sky = _check_sky(sky)
    height_scale = _check_scale(height_scale)
    if not _is_int(margin) or margin < 0:
        raise ValueError("margin must be an integer >= 0, got %r" % (margin,))
    margin = int(margin)
    a = _plane(heightmap)
    rows, cols = a.shape
    H, W = rows - 2 * margin, cols - 2 * margin
    if H < 1 or W < 1:
        raise ValueError("a heightmap of %d x %d has no interior inside a margin of %d" % (rows, cols, margin))
    check_size(H, W, plane=(rows, cols))
    dtype = np.uint8 if uint8 else np.float32
    if out is None:
        out = np.empty((H, W), dtype)
    elif not isinstance(out, np.ndarray) or out.shape != (H, W) or out.dtype != dtype or not out.flags['C_CONTIGUOUS']:
        raise ValueError("out must be a contiguous %s %s, got %s" % (np.dtype(dtype), (H, W), getattr(out, "shape", out)))
    dev = ops.dev
    with scratch(dev) as alloc:
        src, dst = alloc(a.nbytes), alloc(out.nbytes)
        dev.h2d(src, a)
        bake_device(ops, src, rows, cols, sky, height_scale, dst, margin=margin, uint8=uint8, tiled=tiled)
        dev.sync()
        dev.d2h(out, dst, out.nbytes)
    return out


# ---- command line -------------------------------------------------------------------------------------------------------
def parse_args(argv):
    p = argparse.ArgumentParser(prog="python -m gan_heightmaps_amd.skylight",
                                description="Bake the light of the sky on a heightmap (a horizon scan on the GPU).")
    p.add_argument("input", help="heightmap: 8-bit PNG (read as greyscale), or .npy (uint8 or float in [0, 1], (H, W))")
    p.add_argument("output", help="the sky-light map: .png (8-bit), or .npy (float32)")
    d = SkyLight()
    p.add_argument("--directions", type=int, default=d.directions, help="azimuths (default %d)" % d.directions)
    p.add_argument("--steps", type=int, default=d.steps, help="samples per azimuth (default %d)" % d.steps)
    p.add_argument("--step", type=float, default=d.step, help="pixels between samples (default %g)" % d.step)
    p.add_argument("--strength", type=float, default=d.strength, help="how far the visibility dims the light, in [0, 1]")
    p.add_argument("--height-scale", type=float, default=64.0, help="pixels per unit height (default 64, the renderer's)")
    g = p.add_mutually_exclusive_group()
    g.add_argument("--plain", action="store_true", help="gather from global memory")
    g.add_argument("--tiled", action="store_true", help="gather from tiles staged in LDS (the same bits)")
    a = p.parse_args(argv)
    try:
        a.sky = SkyLight(directions=a.directions, steps=a.steps, step=a.step, strength=a.strength)
        _check_scale(a.height_scale)
    except ValueError as e:
        p.error(str(e))
    return a


def main(argv=None):
    a = parse_args(sys.argv[1:] if argv is None else argv)
    from .device import Device, Ops
    x = read_image(a.input, "L", mmap=False)
    dev = Device(0)
    try:
        to_png = not a.output.endswith(".npy")
        res = bake(Ops(dev), x, a.sky, height_scale=a.height_scale, uint8=to_png, tiled=form_choice(a.tiled, a.plain))
    finally:
        dev.close()
    if to_png:
        from PIL import Image
        Image.fromarray(res).save(a.output)
    else:
        np.save(a.output, res)
    return 0


if __name__ == "__main__":
    sys.exit(main())
