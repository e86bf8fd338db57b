"""Score generators with a sliced Wasserstein distance on Laplacian-pyramid patches (csrc/swd.hip).

The metric of Karras et al. 2018, "Progressive Growing of GANs", §5: no pretrained network, one number per spatial scale
(coarse landforms against fine texture), any channel count.  Two sets of ``n`` images [n, C, H, W] are compared:

    1. Gaussian pyramid   G_0 = x, G_{i+1} = down(G_i): the separable binomial [1 4 6 4 1] / 16, even rows and columns kept
    2. Laplacian pyramid  Lap_i = G_i - up(G_{i+1}) for i < L - 1, Lap_{L-1} = G_{L-1}; up: the image on the even positions
                          of a zero image of twice the size, [1 4 6 4 1] / 8 per axis.  Both filters reflect without repeating
                          the edge (index -1 -> 1, n -> n - 2).  L defaults to the halvings that take min(H, W) to 16, plus one
    3. descriptors        per level and image ``patches_per_image`` windows of C x 7 x 7: N = n patches_per_image rows of
                          K = 49 C values (row image * patches_per_image + p, column c * 49 + dy * 7 + dx)
    4. normalisation      per level, channel and set: subtract the mean, divide by the population standard deviation of all
                          N x 49 values (a standard deviation of 0 is a ValueError naming level and channel)
    5. distance           ``repeats`` draws of ``directions`` unit vectors of R^K, the same for both sets; project both sets,
                          sort every column, take the mean of |sorted_A - sorted_B|; reported 1e3 x, per level and averaged

The draws, all from ``numpy.random.RandomState`` on the host: the corners of set ``s`` (0 or 1) at level ``i`` are
``RandomState([seed, s, i])``'s ``randint(0, H_i - 6, (n, P))`` (rows) and then ``randint(0, W_i - 6, (n, P))`` (columns), made
for the whole set at once, so they do not depend on how the set is fed; the directions of level ``i`` and repeat ``r`` are
``RandomState([seed, 2, i, r]).randn(K, directions)``, every column normalised in float64 and cast to float32.
tests/swd_ref.py restates all of it in float64.

    python -m gan_heightmaps_amd.swd EXPERIMENT MODEL [--images N] [--batch-size B] [--which W] [--seed S] [--dtype D] [--ema]
    python -m gan_heightmaps_amd.swd --real DIR_OR_NPY --fake DIR_OR_NPY [--seed S]
"""
import argparse
import dataclasses
import os
import sys

import numpy as np

from .planes import scratch
from .util import is_int as _is_int

__all__ = ["PATCH", "MAX_CHANNELS", "SWD", "Descriptors", "distance", "compare", "corners", "directions", "header", "row",
           "parse_args", "main"]

PATCH = 7                   # GHM_SWD_PATCH
MAX_CHANNELS = 4            # GHM_SWD_MAX_K / 49
MIN_SIZE = 16               # the short side of the coarsest level is at least this


@dataclasses.dataclass(frozen=True)
class SWD:
    """The parameters of the metric, validated and frozen.  levels=None: the halvings that take min(H, W) to 16, plus one."""
    levels: int = None
    patches_per_image: int = 128
    patch: int = PATCH
    directions: int = 128
    repeats: int = 4
    seed: int = 0

    def __post_init__(self):
        if self.patch != PATCH:
            raise ValueError("only patch=%d is supported, got %r" % (PATCH, self.patch))
        for k in ("patches_per_image", "directions", "repeats"):
            v = getattr(self, k)
            if not _is_int(v) or v < 1:
                raise ValueError("%s must be an integer >= 1, got %r" % (k, v))
            object.__setattr__(self, k, int(v))
        if self.levels is not None and (not _is_int(self.levels) or self.levels < 1):
            raise ValueError("levels must be None or an integer >= 1, got %r" % (self.levels,))
        if not _is_int(self.seed) or not 0 <= self.seed < 2 ** 32:
            raise ValueError("seed must be an integer in [0, 2^32), got %r" % (self.seed,))

    def num_levels(self, H, W):
        """the levels of an H x W image, checked: H and W divisible by 2^(L-1), the coarsest level at least 16 a side"""
        L = self.levels
        if L is None:
            L, m = 1, min(H, W)
            while m >= 2 * MIN_SIZE and m % 2 == 0:
                m //= 2
                L += 1
        f = 1 << (L - 1)
        if H % f or W % f or min(H, W) // f < MIN_SIZE:
            raise ValueError("%d levels need H and W divisible by %d and a coarsest level of at least %d pixels a side, got "
                             "%d x %d" % (L, f, MIN_SIZE, H, W))
        return L

    def sizes(self, H, W):
        """[(H_i, W_i)] per level"""
        return [(H >> i, W >> i) for i in range(self.num_levels(H, W))]


def corners(metric, set_index, level, n, H, W):
    """int32 [n, patches_per_image, 2]: the (row, column) corners of every window of a set of ``n`` images at a level of
    H x W pixels"""
    rs = np.random.RandomState([metric.seed, set_index, level])
    ys = rs.randint(0, H - (PATCH - 1), (n, metric.patches_per_image))
    xs = rs.randint(0, W - (PATCH - 1), (n, metric.patches_per_image))
    return np.ascontiguousarray(np.stack([ys, xs], axis=-1), np.int32)


def directions(metric, level, repeat, K):
    """float32 [K, directions]: unit columns"""
    d = np.random.RandomState([metric.seed, 2, level, repeat]).randn(K, metric.directions)
    return np.ascontiguousarray((d / np.sqrt((d * d).sum(axis=0, keepdims=True))).astype(np.float32))


class Descriptors:
    """The descriptor matrices of one image set, per level [N, 49 C] float32 in device memory, filled batch by batch.

    ops: a device.Ops (everything runs on its stream); set_index: 0 or 1 -- which corner table the set draws; max_batch:
    images per pyramid pass (a larger batch is fed in slices).  The device memory needed -- the matrices, the corner tables
    and the pyramid workspace of max_batch images -- is computed before anything is allocated: ``Descriptors.need(...)``,
    and a need above ``max_mb`` raises ValueError.  Use it as a context manager, or close() it."""

    @staticmethod
    def need(metric, n_images, C, H, W, max_batch=16):
        """bytes of device memory a Descriptors of these sizes allocates"""
        L = metric.num_levels(H, W)
        N = n_images * metric.patches_per_image
        img = max_batch * C * H * W
        work = img + img + img // 4 + (img // 16 if L > 2 else 0)          # staging, Lap, the two G buffers
        return 4 * (L * N * PATCH * PATCH * C + L * N * 2 + work)

    def __init__(self, ops, metric, set_index, n_images, C, H, W, max_mb=None, max_batch=16):
        if not isinstance(metric, SWD):
            raise ValueError("metric must be an SWD, got %r" % (metric,))
        if set_index not in (0, 1):
            raise ValueError("set_index must be 0 or 1, got %r" % (set_index,))
        if not all(_is_int(v) and v >= 1 for v in (n_images, C, H, W, max_batch)):
            raise ValueError("n_images, C, H, W and max_batch must be integers >= 1, got %r"
                             % ((n_images, C, H, W, max_batch),))
        if C > MAX_CHANNELS:
            raise ValueError("at most %d channels, got %d" % (MAX_CHANNELS, C))
        self.ops, self.dev, self.metric, self.set_index = ops, ops.dev, metric, set_index
        self.n_images, self.C, self.H, self.W = int(n_images), int(C), int(H), int(W)
        self.sizes = metric.sizes(H, W)
        self.L = len(self.sizes)
        self.P = metric.patches_per_image
        self.N, self.K = self.n_images * self.P, PATCH * PATCH * self.C
        self.max_batch = int(max_batch)
        self.bytes = self.need(metric, self.n_images, self.C, self.H, self.W, self.max_batch)
        if max_mb is not None and self.bytes > max_mb * 2 ** 20:
            raise ValueError("the descriptors of %d images of %d x %d x %d need %.1f MB of device memory, over max_mb=%g"
                             % (self.n_images, self.C, self.H, self.W, self.bytes / 2 ** 20, max_mb))
        self.count = 0
        self._stats = {}
        self._bufs = []
        img = 4 * self.max_batch * self.C * self.H * self.W
        try:
            self.desc = [self._alloc(4 * self.N * self.K) for _ in range(self.L)]
            self._corners = []
            for i, (h, w) in enumerate(self.sizes):
                p = self._alloc(4 * self.N * 2)
                self.dev.h2d(p, corners(metric, set_index, i, self.n_images, h, w))
                self._corners.append(p)
            self._stage, self._lap = self._alloc(img), self._alloc(img)
            self._g = [self._alloc(img // 4), self._alloc(img // 16) if self.L > 2 else None]
        except BaseException:
            self.close()
            raise

    def _alloc(self, nbytes):
        p = self.dev.alloc(nbytes)
        self._bufs.append(p)
        return p

    full = property(lambda s: s.count == s.n_images)

    def add(self, batch):
        """append a batch [b, C, H, W]: a device.DevTensor (read where it lies, no host round trip; its rows and channels
        are contiguous, its sample stride is free) or a host array (uploaded)"""
        from .device import DevTensor
        if self._bufs is None:
            raise ValueError("these descriptors are closed")
        shape = tuple(batch.shape)
        if len(shape) != 4 or shape[1:] != (self.C, self.H, self.W) or shape[0] < 1:
            raise ValueError("a batch must be [b, %d, %d, %d], got %s" % (self.C, self.H, self.W, shape))
        if self.count + shape[0] > self.n_images:
            raise ValueError("%d images more than the %d the set was made for (%d are in)"
                             % (shape[0], self.n_images, self.count))
        self._stats = {}
        for b0 in range(0, shape[0], self.max_batch):
            b = min(self.max_batch, shape[0] - b0)
            if isinstance(batch, DevTensor):
                g = batch.samples(b0, b0 + b)
            else:
                self.dev.h2d(self._stage, np.ascontiguousarray(batch[b0:b0 + b], np.float32))
                g = DevTensor(self.dev, self._stage, (b, self.C, self.H, self.W))
            self._add(g, b)

    def _add(self, g, b):
        from .device import DevTensor
        for i, (h, w) in enumerate(self.sizes):
            nxt = self._g[i % 2] if i < self.L - 1 else None
            self.ops.swd_pyramid_level(g, None, nxt, w // 2, self._lap, w)
            self.ops.swd_gather(self._lap, b, self.C, h, w, w, self._corners[i] + 8 * self.count * self.P, self.P,
                                self.desc[i], self.count * self.P, self.N)
            if nxt is not None:
                g = DevTensor(self.dev, nxt, (b, self.C, h // 2, w // 2))
        self.count += b

    def stats(self, level, workspace):
        """float32 [C, 2] (mean, population standard deviation) of a level's channels; ValueError on a deviation of 0"""
        if level not in self._stats:
            with scratch(self.dev, sync=False) as alloc:
                st = alloc(8 * self.C)
                self.ops.swd_stats(self.desc[level], self.N, self.C, st, workspace)
                self.dev.sync()
                out = np.zeros((self.C, 2), np.float32)
                self.dev.d2h(out, st, out.nbytes)
            for c in range(self.C):
                if not out[c, 1] > 0:
                    raise ValueError("set %d, level %d, channel %d: the standard deviation of the descriptors is 0 (a constant "
                                     "channel cannot be normalised)" % (self.set_index, level, c))
            self._stats[level] = out
        return self._stats[level]

    def numpy(self, level):
        """the level's [N, K] matrix on the host"""
        self.dev.sync()
        out = np.empty((self.N, self.K), np.float32)
        self.dev.d2h(out, self.desc[level], out.nbytes)
        return out

    def close(self):
        if self._bufs is not None:
            self.dev.sync()
            for p in self._bufs:
                self.dev.free(p)
            self._bufs = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def distance(ops, a, b, max_mb=None, sort_chunk=0):
    """The sliced Wasserstein distance of two full Descriptors -> {'levels': [sizes], 'swd': [per level], 'mean': float}
    (1e3 x the mean |sorted_A - sorted_B|; 'levels' names a level by the short side of its images).  One repeat is in device
    memory at a time: 2 x directions x N floats, refused with ValueError above ``max_mb``.  sort_chunk: ghm_swd_sort_columns'
    chunk (0: the library's default)."""
    for d in (a, b):
        if not isinstance(d, Descriptors) or d._bufs is None:
            raise ValueError("distance needs two open Descriptors")
        if not d.full:
            raise ValueError("set %d is not full: %d of %d images" % (d.set_index, d.count, d.n_images))
    if (a.n_images, a.C, a.H, a.W) != (b.n_images, b.C, b.H, b.W) or a.metric != b.metric:
        raise ValueError("the sets differ: %d x %s under %r against %d x %s under %r"
                         % (a.n_images, (a.C, a.H, a.W), a.metric, b.n_images, (b.C, b.H, b.W), b.metric))
    metric, N, K, C, D = a.metric, a.N, a.K, a.C, a.metric.directions
    need = 4 * (2 * D * N + K * D + 2 * C) + ops.swd_workspace()
    if max_mb is not None and need > max_mb * 2 ** 20:
        raise ValueError("the projections of %d descriptors on %d directions need %.1f MB of device memory, over max_mb=%g"
                         % (N, D, need / 2 ** 20, max_mb))
    dev = ops.dev
    for d in {id(x): x for x in (a.dev, b.dev, dev)}.values():
        d.sync()                                                # the sets may have been filled on other streams
    vals = []
    with scratch(dev) as alloc:
        pa, pb, dirs, sa, sb, ws = [alloc(n) for n in (4 * D * N, 4 * D * N, 4 * K * D, 8 * C, 8 * C, ops.swd_workspace())]
        for level in range(a.L):
            dev.h2d(sa, a.stats(level, ws))
            dev.h2d(sb, b.stats(level, ws))
            per = []
            for r in range(metric.repeats):
                dev.h2d(dirs, directions(metric, level, r, K))
                for desc, st, out in ((a.desc[level], sa, pa), (b.desc[level], sb, pb)):
                    ops.swd_project(desc, N, C, dirs, D, st, out)
                    ops.swd_sort_columns(out, N, D, sort_chunk)
                per.append(ops.swd_l1(pa, pb, D * N, ws))      # (waits for the stream: dirs may be overwritten)
            vals.append(1e3 * (sum(per) / len(per)))
    return {"levels": [min(h, w) for h, w in a.sizes], "swd": vals, "mean": float(np.mean(vals))}


def compare(ops, real, fake, metric=None, batch_size=16, max_mb=None):
    """the distance of two host image sets [n, C, H, W] (set 0: real, set 1: fake)"""
    metric = SWD() if metric is None else metric
    real, fake = np.asarray(real), np.asarray(fake)
    if real.ndim != 4 or real.shape != fake.shape:
        raise ValueError("two image sets of one shape [n, C, H, W] are needed, got %s and %s" % (real.shape, fake.shape))
    n, C, H, W = real.shape
    with Descriptors(ops, metric, 0, n, C, H, W, max_mb=max_mb, max_batch=batch_size) as a, \
            Descriptors(ops, metric, 1, n, C, H, W, max_mb=max_mb, max_batch=batch_size) as b:
        for i in range(0, n, batch_size):
            a.add(real[i:i + batch_size])
            b.add(fake[i:i + batch_size])
        return distance(ops, a, b, max_mb=max_mb)


# ---- swd.txt of Pix2Pix.train ---------------------------------------------------------------------------------------------
def header(levels):
    """the columns of swd.txt for a result's 'levels'"""
    return ["epoch", "weights", "net"] + ["swd_%d" % s for s in levels] + ["mean"]


def row(epoch, weights, net, result):
    return [str(epoch), weights, net] + [repr(float(v)) for v in result["swd"]] + [repr(float(result["mean"]))]


# ---- command line -------------------------------------------------------------------------------------------------------
def parse_args(argv):
    p = argparse.ArgumentParser(prog="python -m gan_heightmaps_amd.swd",
                                description="Sliced Wasserstein distance on Laplacian-pyramid patches: a model's generators "
                                            "against its dataset, or any two image sets.")
    p.add_argument("experiment", nargs="?", help="experiment name (gan_heightmaps_amd.experiments)")
    p.add_argument("model", nargs="?", help="checkpoint written by save_model / save_checkpoint")
    p.add_argument("--real", metavar="DIR_OR_NPY", help="a folder of PNGs of one size, or an .npy [n, C, H, W] / [n, H, W]")
    p.add_argument("--fake", metavar="DIR_OR_NPY", help="the set to compare with --real (the same number and shape)")
    p.add_argument("--images", type=int, default=1024, help="images per set (default 1024)")
    p.add_argument("--batch-size", type=int, default=4, help="images per forward pass (default 4)")
    p.add_argument("--which", choices=["both", "dcgan", "p2p"], default="both")
    p.add_argument("--seed", type=int, default=0, help="seed of the latent draws and of the metric (default 0)")
    p.add_argument("--dtype", default="bf16x3", help="arithmetic of the convolutions (default bf16x3)")
    p.add_argument("--ema", action="store_true", help="read the averaged generators: MODEL's N.model becomes N.ema.model")
    d = SWD()
    p.add_argument("--levels", type=int, default=None)
    p.add_argument("--patches", type=int, default=d.patches_per_image, help="windows per image and level (default 128)")
    p.add_argument("--directions", type=int, default=d.directions)
    p.add_argument("--repeats", type=int, default=d.repeats)
    a = p.parse_args(argv)
    sets = a.real is not None or a.fake is not None
    if sets and (a.real is None or a.fake is None):
        p.error("--real and --fake go together")
    if sets and (a.experiment is not None or a.ema):
        p.error("--real / --fake compare two image sets without a model")
    if not sets and (a.experiment is None or a.model is None):
        p.error("give EXPERIMENT MODEL, or --real and --fake")
    if a.images < 1 or a.batch_size < 1 or a.batch_size > a.images:
        p.error("--images and --batch-size must be >= 1, and a batch no larger than the set")
    try:
        a.metric = SWD(levels=a.levels, patches_per_image=a.patches, directions=a.directions, repeats=a.repeats, seed=a.seed)
    except ValueError as e:
        p.error(str(e))
    if a.ema:
        a.model = ema_path(a.model)
    return a


def ema_path(model):
    """N.model -> N.ema.model, the file Pix2Pix.train writes beside every checkpoint of a model with an average"""
    return model[:-len(".model")] + ".ema.model" if model.endswith(".model") and not model.endswith(".ema.model") \
        else model


def read_set(path):
    """a folder of PNGs (sorted by name, RGB kept only where a file has colour) or an .npy -> float32 [n, C, H, W]"""
    if path.endswith(".npy"):
        x = np.load(path)
        if x.ndim == 3:
            x = x[:, None]
        if x.ndim != 4:
            raise ValueError("%s: an array [n, C, H, W] or [n, H, W] is needed, got %s" % (path, x.shape))
        return x.astype(np.float32) / np.float32(255) if x.dtype == np.uint8 else np.ascontiguousarray(x, np.float32)
    from PIL import Image
    names = sorted(f for f in os.listdir(path) if f.lower().endswith(".png"))
    if not names:
        raise ValueError("%s: no PNG files" % path)
    imgs = [np.asarray(Image.open(os.path.join(path, f))) for f in names]
    grey = all(im.ndim == 2 for im in imgs)
    out = []
    for f, im in zip(names, imgs):
        if not grey:
            im = np.asarray(Image.open(os.path.join(path, f)).convert("RGB"))
        out.append(im[None] if grey else im.transpose(2, 0, 1))
    if len({o.shape for o in out}) != 1:
        raise ValueError("%s: the images differ in size" % path)
    return np.stack(out).astype(np.float32) / np.float32(255)


def _print(name, res):
    print("%-6s %s  mean %.4f" % (name, "  ".join("%d: %.4f" % (s, v) for s, v in zip(res["levels"], res["swd"])), res["mean"]))


def main(argv=None):
    a = parse_args(sys.argv[1:] if argv is None else argv)
    if a.real is not None:
        from .device import Device, Ops
        real, fake = read_set(a.real), read_set(a.fake)
        dev = Device(0)
        try:
            _print("swd", compare(Ops(dev), real, fake, a.metric))
        finally:
            dev.close()
        return 0
    from .experiments import DATASET, get_iterators, make_model
    model = make_model(a.experiment, dtype=a.dtype, verbose=False)
    model.load_model(a.model, mode="both" if a.which != "dcgan" else "dcgan")
    # the real images: the dataset's validation split, not augmented
    _, it_val = get_iterators(DATASET, a.batch_size, model.is_a_grayscale, model.is_b_grayscale, False, in_shp=model.in_shp,
                               device=model.device)
    res = model.swd(it_val, num_images=a.images, batch_size=a.batch_size, which=a.which,
                    metric=a.metric, seed=a.seed)
    for k in ("dcgan", "p2p"):
        if k in res:
            _print(k, res[k])
    model.device.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
