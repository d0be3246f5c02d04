"""The checker of the line distortion: numpy only, float64, the formulas of the specification
stated directly -- Philox4x32-10 noise, Box-Muller, a separable gaussian with reflected borders (axis 0, then axis 1),
scaling to a maximal displacement, bilinear resampling with the strip's maximum outside, floor(v + 0.5).
tests/test_distort.py holds it against scipy.ndimage; tests/test_distort_gpu.py holds the kernels against it."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """ten rounds over arrays (or scalars) of counter words and key words; returns the four output words as uint64
    arrays holding 32-bit values"""
    c0, c1, c2, c3, k0, k1 = (np.asarray(v, dtype=np.uint64) & MASK for v in (c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        p0 = np.uint64(M0) * c0
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK)
        k0 = (k0 + np.uint64(W0)) & MASK
        k1 = (k1 + np.uint64(W1)) & MASK
    return c0, c1, c2, c3


def noise(h, w, seed, counter):
    """(2, h, w) standard normal fields: row displacement, column displacement"""
    seed, counter = int(seed) & (2 ** 64 - 1), int(counter) & (2 ** 64 - 1)
    p = np.arange(h * w, dtype=np.uint64)
    r = philox4x32_10(p, 0, counter & 0xFFFFFFFF, counter >> 32, seed & 0xFFFFFFFF, seed >> 32)
    u = [(v.astype(np.float64) + 0.5) * 2.0 ** -32 for v in r]
    n0 = np.sqrt(-2.0 * np.log(u[0])) * np.cos(2.0 * np.pi * u[1])
    n1 = np.sqrt(-2.0 * np.log(u[2])) * np.cos(2.0 * np.pi * u[3])
    return np.stack([n0.reshape(h, w), n1.reshape(h, w)])


def gauss_weights(sigma):
    """scipy.ndimage's 1-D gaussian kernel at truncate = 4: (weights [2 radius + 1], radius)"""
    radius = int(4.0 * float(sigma) + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return phi / phi.sum(), radius


def reflect(k, n):
    """index into a line of n elements extended as d c b a | a b c d | d c b a (period 2 n)"""
    m = np.mod(k, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def smooth_axis(a, sigma, axis):
    wts, rad = gauss_weights(sigma)
    n = a.shape[axis]
    idx = np.arange(n)
    out = np.take(a, idx, axis=axis) * wts[rad]
    for k in range(rad, 0, -1):                             # the pairs from the outermost inwards
        out = out + (np.take(a, reflect(idx - k, n), axis=axis) + np.take(a, reflect(idx + k, n), axis=axis)) * wts[rad - k]
    return out


def smooth(a, sigma):
    return smooth_axis(smooth_axis(a, sigma, 0), sigma, 1)


def fields(h, w, distort, dsigma, seed, counter):
    """(2, h, w): the displacement fields in pixels, max |D| = distort each"""
    out = []
    for n in noise(h, w, seed, counter):
        f = smooth(n, dsigma)
        m = np.abs(f).max()
        out.append(f * (distort / m) if m > 0 else np.zeros_like(f))
    return np.stack(out)


def sample(img, d):
    """v (h, w) float64: img sampled bilinearly at (y + d[0], x + d[1]); max(img) where the point lies outside"""
    h, w = img.shape
    a = img.astype(np.float64)
    sy = np.arange(h, dtype=np.float64)[:, None] + d[0]
    sx = np.arange(w, dtype=np.float64)[None, :] + d[1]
    inside = (sy >= 0) & (sy <= h - 1) & (sx >= 0) & (sx <= w - 1)
    sy, sx = np.where(inside, sy, 0.0), np.where(inside, sx, 0.0)
    y0, x0 = np.floor(sy).astype(np.int64), np.floor(sx).astype(np.int64)
    y1, x1 = np.minimum(y0 + 1, h - 1), np.minimum(x0 + 1, w - 1)
    ty, tx = sy - y0, sx - x0
    top = (1.0 - tx) * a[y0, x0] + tx * a[y0, x1]
    bot = (1.0 - tx) * a[y1, x0] + tx * a[y1, x1]
    return np.where(inside, (1.0 - ty) * top + ty * bot, float(img.max()))


def distort_strip(img, distort=3.0, dsigma=10.0, seed=0, counter=0):
    """(out uint8, v float64, d (2, h, w)) of one strip"""
    img = np.asarray(img)
    d = fields(img.shape[0], img.shape[1], distort, dsigma, seed, counter)
    v = sample(img, d)
    return np.floor(v + 0.5).astype(np.uint8), v, d
