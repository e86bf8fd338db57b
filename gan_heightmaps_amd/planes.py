"""What the one-shot terrain tools -- erosion, skylight, mesh, hydrology, route, earthworks, viewshed, contour, peaks, rivers, regions, climate, sunlight, and the world's calls
of them -- share on the host: the heightmap intake, the size limit of the plane kernels, the ``keep`` check and call-scoped device scratch.
Nothing here touches the library: a device is whatever has ``alloc``, ``free`` and ``sync``."""
import numpy as np

__all__ = ["MAX_CELLS", "MAX_ROWS", "as_plane", "check_size", "check_keep", "scratch"]

MAX_CELLS = 1 << 31          # flat indices are int32
MAX_ROWS = 4 * 65535         # = 262140


def check_size(H, W, plane=None, limits=False):
    """ValueError unless the plane kernels can index H x W cells: H W < 2^31 and H <= 262140.  plane: the (rows, cols) that
    are counted and named where they are more than the H rows the launch covers (skylight's plane with its margin);
    limits: the refusal states the limits."""
    rows, cols = (H, W) if plane is None else plane
    if H < 1 or W < 1 or rows * cols >= MAX_CELLS or H > MAX_ROWS:
        raise ValueError("heightmap size %d x %d out of range%s" % (rows, cols, " (H W < 2^31, H <= 262140)" if limits else ""))


def as_plane(heightmap, *, lead=True, unit_range=False, raw=False, what=None):
    """The one heightmap intake: uint8 (read as v / 255) or floating point, (H, W) or (1, H, W) -> a finite, contiguous
    float32 plane [H, W].  The refusals fire in the order of the text below; the tools differ in four ways:

        lead        (1, H, W) is taken and its axis dropped; False: (H, W) alone, and the refusal says so
        unit_range  floats outside [0, 1] are refused, and before the non-finite ones
        raw         heights are any finite numbers, read as the kernels read them: the size is checked (``check_size``, its
                    limits stated) from the shape alone, before an element is read -- an empty plane is a size out of range,
                    not a wrong shape --, the dtype's refusal names no range, and -0 becomes +0
        what        the tool's name: (C, H, W) with C > 1 is refused in its name, as one height per pixel too many

                    lead   unit_range  raw    what
        erosion     True   False       False  "erosion"
        skylight    False  False       False  None
        mesh        True   True        False  None
        hydrology   True   False       True   None            (route takes the hydrology's)
        earthworks  True   False       True   None            (scatter takes the same)
        viewshed    True   True        True   None
        contour     True   True        True   None            (it takes the viewshed's; peaks takes the same)
        climate     True   True        True   None            (the viewshed's too)
        sunlight    True   True        True   None            (the viewshed's too)
    """
    a = heightmap if hasattr(heightmap, "dtype") and hasattr(heightmap, "shape") else np.asarray(heightmap)
    shape = tuple(a.shape)
    if what is not None and a.ndim == 3 and a.shape[0] != 1:
        raise ValueError("%s needs one height per pixel: a (H, W) or (1, H, W) heightmap, got %s" % (what, shape))
    if lead and a.ndim == 3 and a.shape[0] == 1:
        a = a[0]
    if a.ndim != 2 or not (raw or (a.shape[0] >= 1 and a.shape[1] >= 1)):
        raise ValueError("heightmap must be %s, got %s" % ("(H, W) or (1, H, W)" if lead else "(H, W)", shape))
    if raw:
        check_size(a.shape[0], a.shape[1], limits=True)
    if a.dtype == np.uint8:
        a = np.asarray(a).astype(np.float32) / np.float32(255)
    elif a.dtype.kind == "f":
        a = np.ascontiguousarray(a, np.float32)
        if unit_range and (a.min() < 0 or a.max() > 1):
            raise ValueError("a floating-point heightmap must lie in [0, 1]")
    else:
        raise ValueError("heightmap must be uint8 or floating point%s, got %s" % ("" if raw else " in [0, 1]", a.dtype))
    if not np.isfinite(a).all():
        raise ValueError("the heightmap has non-finite values")
    return np.ascontiguousarray(a + np.float32(0) if raw else a)


def check_keep(keep, planes):
    """``keep``, one name or several, as a tuple of names out of ``planes``"""
    keep = (keep,) if isinstance(keep, str) else tuple(keep)
    for k in keep:
        if k not in planes:
            raise ValueError("keep holds %r: the planes are %s" % (k, ", ".join(planes)))
    return keep


class scratch:
    """Device memory that lives as long as a ``with`` block: ``with scratch(dev) as alloc: p = alloc(nbytes)``.
    Allocations are made one at a time, so one that fails leaves the earlier ones to be freed.  When the block ends, or
    fails, the device is made idle (``sync``; False where the body has already waited for all it launched) and everything
    handed out is freed -- but for what ``alloc.keep(*ptrs)`` gave to the caller for good."""

    def __init__(self, dev, sync=True):
        self._dev, self._sync, self._held = dev, sync, []

    def __enter__(self):
        return self

    def __call__(self, nbytes):
        self._held.append(self._dev.alloc(nbytes))
        return self._held[-1]

    def keep(self, *ptrs):
        for p in ptrs:
            self._held.remove(p)

    def __exit__(self, *exc):
        if self._sync:
            self._dev.sync()
        for p in self._held:
            self._dev.free(p)
        self._held = []
