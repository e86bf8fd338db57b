"""Host restatement of the sliced Wasserstein distance on Laplacian-pyramid patches (gan_heightmaps_amd/swd.py,
csrc/swd.hip; Karras et al. 2018, "Progressive Growing of GANs", §5) in numpy float64.  It shares no code with
the package: the corner tables and directions are drawn here again, from the documented seeds, so a change of the draw
order on either side shows.

    G_0 = x, G_{i+1} = down(G_i);  Lap_i = G_i - up(G_{i+1}) for i < L - 1, Lap_{L-1} = G_{L-1}
    down: the separable binomial [1, 4, 6, 4, 1] / 16, even rows and columns kept;  up: the image on the even positions of a
    zero image of twice the size, filtered with [1, 4, 6, 4, 1] / 8 per axis;  both reflect without repeating the edge
    (index -1 -> 1, n -> n - 2).

Descriptors: per level and image ``patches_per_image`` windows of C x 7 x 7, row ``image * patches_per_image + p`` of an
[N, 49 C] matrix, column ``c * 49 + dy * 7 + dx``.  The corners of set ``s`` at level ``i`` are two draws from
``RandomState([seed, s, i])``: ``randint(0, H_i - 6, (n, P))`` (rows), then ``randint(0, W_i - 6, (n, P))`` (columns), for
all ``n`` images of the set at once -- so they do not depend on how the set is fed.  The directions of level ``i`` and repeat
``r`` are ``RandomState([seed, 2, i, r]).randn(K, directions)``, every column normalised in float64 and cast to float32.
"""
import numpy as np

PATCH = 7
W5 = np.array([1.0, 4.0, 6.0, 4.0, 1.0])


def default_levels(H, W):
    """halvings that take min(H, W) to 16, plus one"""
    n, m = 1, min(H, W)
    while m >= 32 and m % 2 == 0:
        m //= 2
        n += 1
    return n


def _filter(x, axis, w):
    """the 5-tap filter ``w`` along ``axis`` with the reflection -1 -> 1, n -> n - 2"""
    pad = [(0, 0)] * x.ndim
    pad[axis] = (2, 2)
    p = np.pad(x, pad, mode="reflect")
    n = x.shape[axis]
    out = np.zeros_like(x)
    for t in range(5):
        out += w[t] * np.take(p, np.arange(t, t + n), axis=axis)
    return out


def down(x):
    x = np.asarray(x, np.float64)
    y = _filter(_filter(x, -1, W5 / 16), -2, W5 / 16)
    return y[..., ::2, ::2]


def up(y):
    y = np.asarray(y, np.float64)
    z = np.zeros(y.shape[:-2] + (2 * y.shape[-2], 2 * y.shape[-1]))
    z[..., ::2, ::2] = y
    return _filter(_filter(z, -1, W5 / 8), -2, W5 / 8)


def gaussian_pyramid(x, levels):
    g = [np.asarray(x, np.float64)]
    for _ in range(levels - 1):
        g.append(down(g[-1]))
    return g


def laplacian_pyramid(x, levels):
    g = gaussian_pyramid(x, levels)
    return [g[i] - up(g[i + 1]) for i in range(levels - 1)] + [g[-1]]


def reconstruct(lap):
    x = lap[-1]
    for l in lap[-2::-1]:
        x = l + up(x)
    return x


def corners(seed, set_index, level, n, P, H, W):
    """-> int [n, P, 2]: (row, column) of every window's top-left corner"""
    rs = np.random.RandomState([seed, set_index, level])
    ys = rs.randint(0, H - (PATCH - 1), (n, P))
    xs = rs.randint(0, W - (PATCH - 1), (n, P))
    return np.stack([ys, xs], axis=-1)


def directions(seed, level, repeat, K, D):
    """-> float32 [K, D] unit columns"""
    d = np.random.RandomState([seed, 2, level, repeat]).randn(K, D)
    return (d / np.sqrt((d * d).sum(axis=0, keepdims=True))).astype(np.float32)


def gather(img, cor):
    """img [n, C, H, W], cor [n, P, 2] -> [n P, 49 C] in img's dtype"""
    n, C = img.shape[:2]
    P = cor.shape[1]
    out = np.empty((n * P, C * PATCH * PATCH), img.dtype)
    for i in range(n):
        for p in range(P):
            y, x = cor[i, p]
            out[i * P + p] = img[i, :, y:y + PATCH, x:x + PATCH].reshape(-1)
    return out


def descriptors(x, set_index, levels=None, patches_per_image=128, seed=0):
    """x [n, C, H, W] -> per level the float64 [N, K] matrix of raw (not normalised) descriptors"""
    x = np.asarray(x, np.float64)
    n, C, H, W = x.shape
    levels = default_levels(H, W) if levels is None else levels
    lap = laplacian_pyramid(x, levels)
    return [gather(l, corners(seed, set_index, i, n, patches_per_image, l.shape[2], l.shape[3])) for i, l in enumerate(lap)]


def normalise(desc, C, level=0):
    """per channel: subtract the mean, divide by the population standard deviation of all N x 49 values"""
    d = np.asarray(desc, np.float64).reshape(desc.shape[0], C, PATCH * PATCH)
    mu = d.mean(axis=(0, 2), keepdims=True)
    sd = d.std(axis=(0, 2), keepdims=True)
    if (sd == 0).any():
        raise ValueError("level %d, channel %d: the standard deviation is 0" % (level, int(np.argmax(sd.ravel() == 0))))
    return ((d - mu) / sd).reshape(desc.shape)


def sorted_l1(a, b):
    """a, b [N, M] -> the mean of |sort(a) - sort(b)| over all entries, columns sorted apart"""
    return float(np.abs(np.sort(a, axis=0) - np.sort(b, axis=0)).mean())


def level_distance(da, db, C, level, directions_=128, repeats=4, seed=0):
    """raw descriptors of one level of both sets -> 1e3 x the sliced Wasserstein distance"""
    na, nb = normalise(da, C, level), normalise(db, C, level)
    K = na.shape[1]
    D = np.concatenate([directions(seed, level, r, K, directions_) for r in range(repeats)], axis=1).astype(np.float64)
    return 1e3 * sorted_l1(na @ D, nb @ D)


def swd(xa, xb, levels=None, patches_per_image=128, directions_=128, repeats=4, seed=0, sets=(0, 1)):
    """two image sets [n, C, H, W] -> {'levels': [sizes], 'swd': [per level], 'mean': float}.  ``sets``: the set index each
    side draws its corners with; (0, 0) gives both sides the same windows, so swd(X, X, sets=(0, 0)) is exactly 0"""
    xa, xb = np.asarray(xa), np.asarray(xb)
    if xa.shape != xb.shape:
        raise ValueError("the sets differ in shape: %s, %s" % (xa.shape, xb.shape))
    n, C, H, W = xa.shape
    levels = default_levels(H, W) if levels is None else levels
    da = descriptors(xa, sets[0], levels, patches_per_image, seed)
    db = descriptors(xb, sets[1], levels, patches_per_image, seed)
    vals = [level_distance(da[i], db[i], C, i, directions_, repeats, seed) for i in range(levels)]
    return {"levels": [min(H, W) >> i for i in range(levels)], "swd": vals, "mean": float(np.mean(vals))}


def power_law_images(seed, n, size, C=1, beta=2.0):
    """[n, C, size, size] float64 noise with spectrum 1 / f^beta, scaled to unit standard deviation per image"""
    rs = np.random.RandomState(seed)
    f = np.fft.fftfreq(size)
    r = np.sqrt(f[:, None] ** 2 + f[None, :] ** 2)
    r[0, 0] = 1.0
    amp = r ** (-beta / 2)
    amp[0, 0] = 0.0
    x = np.fft.ifft2(np.fft.fft2(rs.randn(n, C, size, size)) * amp).real
    return x / x.std(axis=(2, 3), keepdims=True)
