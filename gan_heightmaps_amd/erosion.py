"""Hydraulic erosion of heightmaps: a pipe-model water simulation on the device (csrc/erosion.hip).

A DCGAN heightmap is a plausible surface without drainage.  ``erode`` rains on it, lets the water run downhill through
"virtual pipes" between neighbouring cells (Mei, Decaudin and Hu, 2007), and lets the flow pick up and drop sediment: valleys
are cut, hollows fill.  The model is restated so that every step is a gather -- no atomics, no particles, no randomness --
and every operation is continuous in its inputs.

State per cell: ground ``b = heightmap * height_scale``, water depth ``d``, suspended sediment ``s``, outflow ``fL fR fT
fB`` to the four neighbours; all 0 at the start except ``b``.  The array's edge is a closed wall.  One iteration (a name
with a neighbour in brackets reads that neighbour's value):

    1. rain         d1 = d + dt rain
    2. flux         h = b + d1;  gX = max(0, fX + dt pipe gravity (h - h[X])), 0 towards a wall;
                    S = ((gL + gR) + (gT + gB)) dt;  K = d1 / S if S > d1 else 1;  fX' = K gX
    3. water        in = (fR'[L] + fL'[R]) + (fB'[T] + fT'[B]);  d2 = max(0, d1 + dt (in - ((fL' + fR') + (fT' + fB'))))
       velocity     wx = ((fR'[L] - fL') + (fR' - fL'[R])) / 2, wy likewise;  dbar = max((d1 + d2) / 2, min_depth);
                    u = clamp(wx / dbar, +-max_speed), v likewise
    4. erosion      gx = (b[R] - b[L]) / 2, gy likewise (indices clamped);  g2 = gx^2 + gy^2;
                    tilt = max(sqrt(g2 / (1 + g2)), min_tilt);  C = capacity tilt sqrt(u^2 + v^2);  D = C - s;
                    e = dissolve D if D > 0 else deposit D;  b' = b - e;  s1 = s + e
    5. transport    s' = the bilinear sample of s1 at (i - clamp(v dt, +-1), j - clamp(u dt, +-1)), clamped to the array
    6. evaporation  d' = d2 (1 - evaporation dt)

The output is ``clamp(b / height_scale, 0, 1)``.  One iteration reaches RADIUS = 3 cells (s' reads s1 at 1, that reads u at
1, that reads f' at 2, that reads b and d at 3), N iterations reach ``halo = 3 N``: a cell at least that far from every wall
does not feel the wall, which is what lets a TerrainWorld erode an unbounded world window by window (world.py).

    python -m gan_heightmaps_amd.erosion IN OUT [--iterations N] [--water OUT_W] [--dt X] [--rain X] ... [--plain | --fused]
"""
import argparse
import dataclasses
import sys

import numpy as np

from .planes import as_plane, check_size, scratch
from .util import form_choice, is_int as _is_int, is_number as _is_number, read_image

__all__ = ["RADIUS", "PLANES", "PARAMS", "DEFAULT_FUSED", "Erosion", "erode", "workspace_planes", "parse_args", "main"]

RADIUS = 3                  # cells one iteration reaches (DESIGN §4p has the derivation)
PLANES = 7                  # GHM_EROSION_PLANES: b, d, s, fL, fR, fT, fB
# the kernels' parameters, in the order of ghm_erosion_params (include/ghm.h)
PARAMS = ("dt", "rain", "evaporation", "gravity", "pipe", "capacity", "dissolve", "deposit", "min_tilt", "max_speed",
          "min_depth", "height_scale")
# the form ``erode`` and the eroded world run by default: the one tools/erosion_bench.py shows faster on the MI355X -- the
# plain one, 0.130 against 0.144 ms per iteration of a 2304 x 2304 window (DESIGN §4p has the table); both give the same bits
DEFAULT_FUSED = False


@dataclasses.dataclass(frozen=True)
class Erosion:
    """The parameters of an erosion, validated and frozen; part of an eroded world's identity.  ``min_depth > 0`` and a
    finite ``max_speed`` are part of the model: with a thin-film velocity it amplifies rounding into order-one differences
    within tens of iterations.  ``dt max_speed <= 1`` keeps the backtrace of step 5 inside one cell."""
    iterations: int = 32
    dt: float = 0.05
    rain: float = 0.02
    evaporation: float = 0.05
    gravity: float = 9.81
    pipe: float = 1.0
    capacity: float = 0.1
    dissolve: float = 0.05
    deposit: float = 0.05
    min_tilt: float = 0.01
    max_speed: float = 4.0
    min_depth: float = 0.05
    height_scale: float = 64.0      # render.DEFAULTS['height_scale']: the slopes the water sees are the ones rendered

    def __post_init__(self):
        if not _is_int(self.iterations) or self.iterations < 0:
            raise ValueError("iterations must be an integer >= 0, got %r" % (self.iterations,))
        object.__setattr__(self, "iterations", int(self.iterations))
        for k in PARAMS:
            v = getattr(self, k)
            if not _is_number(v) or v < 0 or np.float32(v) > np.float32(3e38):
                raise ValueError("%s must be a finite number >= 0, got %r" % (k, v))
            object.__setattr__(self, k, float(v))
        if not self.dt > 0:
            raise ValueError("dt must be > 0, got %r" % (self.dt,))
        if not self.min_depth > 0:
            raise ValueError("min_depth must be > 0 (the velocity is the flow over max(depth, min_depth)), got %r"
                             % (self.min_depth,))
        if not self.max_speed > 0:
            raise ValueError("max_speed must be > 0, got %r" % (self.max_speed,))
        if np.float32(self.dt) * np.float32(self.max_speed) > np.float32(1):
            raise ValueError("dt * max_speed must be <= 1 (the backtrace stays inside one cell), got %g * %g"
                             % (self.dt, self.max_speed))
        if not self.height_scale > 0:
            raise ValueError("height_scale must be > 0, got %r" % (self.height_scale,))
        if self.evaporation * self.dt > 1:
            raise ValueError("evaporation * dt must be <= 1, got %g * %g" % (self.evaporation, self.dt))

    @property
    def halo(self):
        """cells N iterations reach: a cell this far from every wall does not feel the wall"""
        return RADIUS * self.iterations

    def as_dict(self):
        """the kernels' parameters by name (without ``iterations``)"""
        return {k: getattr(self, k) for k in PARAMS}


def workspace_planes(fused):
    """fp32 planes of device memory one window needs: the ping-pong pair of states, and the plain form's u, v, s1"""
    return 2 * PLANES + (0 if fused else 3)


def _plane(heightmap):
    """-> (float32 [H, W] in [0, 1], whether the input had a leading channel axis)"""
    return as_plane(heightmap, what="erosion"), np.ndim(heightmap) == 3


def erode(device_ops, heightmap, erosion=None, fused=None, water=False, out=None, uint8=False):
    """Erode a heightmap on the device: upload, ``erosion.iterations`` steps, download.
    device_ops: a device.Ops; heightmap: (H, W) or (1, H, W), floating point in [0, 1] or uint8; the array's edge is a
    wall.  fused: the one-launch LDS form (True) or the three-launch form (False): the same bits; default DEFAULT_FUSED.
    Returns clamp(b / height_scale, 0, 1) in the input's shape as float32, or with uint8=True as uint8
    (rint(255 v), half to even); ``out`` (that shape and dtype) is written in place of a new array.  water=True returns
    (heightmap, water depth float32 in height units)."""
    from .device import erosion_params
    erosion = Erosion() if erosion is None else erosion
    if not isinstance(erosion, Erosion):
        raise ValueError("erosion must be an Erosion, got %r" % (erosion,))
    fused = DEFAULT_FUSED if fused is None else bool(fused)
    a, lead = _plane(heightmap)
    H, W = a.shape
    check_size(H, W)
    shape = (1, H, W) if lead else (H, W)
    dtype = np.uint8 if uint8 else np.float32
    if out is None:
        out = np.empty(shape, dtype)
    elif tuple(out.shape) != shape or out.dtype != dtype or not out.flags['C_CONTIGUOUS']:
        raise ValueError("out must be a contiguous %s %s, got %s %s" % (np.dtype(dtype), shape, out.dtype, tuple(out.shape)))
    ops, dev = device_ops, device_ops.dev
    plane = 4 * H * W
    with scratch(dev) as alloc:
        hm, s0, s1 = alloc(plane), alloc(PLANES * plane), alloc(PLANES * plane)
        uvs = None if fused else alloc(3 * plane)
        dev.h2d(hm, a)
        ops.erosion_init(hm, H, W, W, erosion.height_scale, s0, W)
        fin = ops.erosion_iterate(erosion_params(**erosion.as_dict()), s0, s1, uvs, H, W, W, erosion.iterations, fused)
        ops.erosion_emit(fin, H, W, W, erosion.height_scale, 0, 0, H, W, uint8, hm, H, W)
        dev.sync()
        dev.d2h(out, hm, H * W * (1 if uint8 else 4))
        depth = None
        if water:
            depth = np.empty(shape, np.float32)
            dev.d2h(depth, fin + plane, plane)
    return (out, depth) if water else out


# ---- command line -------------------------------------------------------------------------------------------------------
def parse_args(argv):
    p = argparse.ArgumentParser(prog="python -m gan_heightmaps_amd.erosion",
                                description="Erode a heightmap with a pipe-model water simulation on the GPU.")
    p.add_argument("input", help="heightmap: 8-bit PNG (read as greyscale), or .npy (uint8 or float in [0, 1]; (H, W) or "
                                 "(1, H, W))")
    p.add_argument("output", help="eroded heightmap: .png (8-bit), or .npy (float32, the input's shape)")
    d = Erosion()
    p.add_argument("--iterations", type=int, default=d.iterations, help="simulation steps (default %d)" % d.iterations)
    p.add_argument("--water", default=None, metavar="OUT_W", help="also write the water depth: .npy (float32, height "
                                                                  "units), or .png (8-bit, scaled to its maximum)")
    for k in PARAMS:
        p.add_argument("--" + k.replace("_", "-"), type=float, default=getattr(d, k), help="default %g" % getattr(d, k))
    g = p.add_mutually_exclusive_group()
    g.add_argument("--plain", action="store_true", help="run the three-launch form (the default: DEFAULT_FUSED)")
    g.add_argument("--fused", action="store_true", help="run the one-launch LDS form (the same bits)")
    a = p.parse_args(argv)
    try:
        a.erosion = Erosion(iterations=a.iterations, **{k: getattr(a, k) for k in PARAMS})
    except ValueError as e:
        p.error(str(e))
    return a


def _write(path, arr, scale_to_max=False):
    if path.endswith(".npy"):
        np.save(path, arr)
        return
    from PIL import Image
    a = np.asarray(arr, np.float32).reshape(arr.shape[-2:])
    if scale_to_max:
        a = a / max(float(a.max()), 1e-30)
    Image.fromarray(np.rint(np.clip(a, 0, 1).astype(np.float64) * 255).astype(np.uint8)).save(path)


def main(argv=None):
    a = parse_args(sys.argv[1:] if argv is None else argv)
    from .device import Device, Ops
    x = read_image(a.input, "L", mmap=False)
    dev = Device(0)
    try:
        res = erode(Ops(dev), x, a.erosion, fused=form_choice(a.fused, a.plain), water=a.water is not None)
    finally:
        dev.close()
    hm, depth = res if a.water is not None else (res, None)
    _write(a.output, hm)
    if depth is not None:
        _write(a.water, depth, scale_to_max=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
