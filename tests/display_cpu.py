"""numpy restatement of the display transform's definitions (include/neusky_hip.h, "A display transform"): the reference the kernels of
csrc/display.hip are tested against.  Luminance and bins in float32, exactly the header's rule (every product and sum rounded once,
the bin read off the bit pattern); everything else in float64."""
import math

import numpy as np

BINS = 3072
CURVES = ("clamp", "reinhard", "aces", "hable")
HABLE = dict(A=0.15, B=0.50, C=0.10, D=0.20, E=0.02, F=0.30, W=11.2, bias=2.0)


def luminance(lin):
    """float32 [..., 3] -> float32 [...]: (0.2126f r + 0.7152f g) + 0.0722f b, each operation rounded to float32"""
    lin = np.asarray(lin, dtype=np.float32)
    with np.errstate(all="ignore"):
        r, g, b = (np.float32(w) * lin[..., c] for c, w in enumerate((0.2126, 0.7152, 0.0722)))
        return ((r + g).astype(np.float32) + b).astype(np.float32)


def bins_of(Y):
    """the bin of each float32 luminance, -1 where it is not metered: not finite, or below 2^-24"""
    Y = np.ascontiguousarray(Y, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(Y) & (Y >= np.float32(2.0 ** -24))
    b = (Y.view(np.uint32).astype(np.int64) >> 17) - 6592
    return np.where(ok, np.minimum(b, BINS - 1), -1)


def histogram(lin, mask=None, threshold=None):
    """int64 [3072] of one image (any leading shape): the metered pixels of lin [..., 3], under mask [...] > threshold if both are given"""
    b = bins_of(luminance(lin)).reshape(-1)
    keep = b >= 0
    if mask is not None and threshold is not None:
        with np.errstate(invalid="ignore"):
            keep &= np.asarray(mask, dtype=np.float32).reshape(-1) > np.float32(threshold)
    return np.bincount(b[keep], minlength=BINS).astype(np.int64)


def exposure(hist, key=0.18, ev=0.0, percentiles=(0.05, 0.95)):
    """E of one histogram: float64 throughout, from the float32 key, ev and percentiles, j ascending; the caller rounds to float32"""
    hist = np.asarray(hist, dtype=np.int64)
    lo, hi = (float(np.float32(p)) for p in percentiles)
    n = int(hist.sum())
    a = math.floor(lo * n)
    b = n - math.floor((1.0 - hi) * n)
    if b <= a:
        return 1.0
    end = np.cumsum(hist)
    start = end - hist
    c = np.maximum(np.minimum(end, b) - np.maximum(start, a), 0)
    m = 0.0
    for j in np.nonzero(c)[0]:
        m += float(c[j]) * ((j + 0.5) / 64.0 - 24.0)
    m /= float(b - a)
    return float(np.float32(key)) * 2.0 ** (float(np.float32(ev)) - m)


def hable_partial(v):
    h = HABLE
    return (v * (h["A"] * v + h["C"] * h["B"]) + h["D"] * h["E"]) / (v * (h["A"] * v + h["B"]) + h["D"] * h["F"]) - h["E"] / h["F"]


def curve(x, name, white=4.0):
    """float64 tone curves on x >= 0"""
    x = np.asarray(x, dtype=np.float64)
    if name == "clamp":
        return x
    if name == "reinhard":
        return x * (1.0 + x / (white * white)) / (1.0 + x)
    if name == "aces":
        return x * (2.51 * x + 0.03) / (x * (2.43 * x + 0.59) + 0.14)
    if name == "hable":
        # the header's definition; its two constant terms D E / (D F) and E / F cancel on paper and to 1e-17 here
        return hable_partial(HABLE["bias"] * x) / hable_partial(HABLE["W"])
    raise ValueError(name)


def srgb(y):
    """clamp(linear_to_sRGB(y), 0, 1) in float64"""
    y = np.asarray(y, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        s = np.where(y <= 0.0031308, 12.92 * y, 1.055 * np.abs(y) ** (1.0 / 2.4) - 0.055)
    return np.clip(s, 0.0, 1.0)


def gaussian_weights(sigma):
    """float64 weights of radius ceil(3 sigma), normalised; the kernels take them rounded to float32"""
    r = int(math.ceil(3.0 * sigma))
    t = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-(t * t) / (2.0 * sigma * sigma))
    return w / w.sum()


def blur(src, weights):
    """float64 separable blur of src [H, W, C] with weights [2 r + 1], zero outside the frame: rows (along W) first, then columns"""
    src = np.asarray(src, dtype=np.float64)
    w = np.asarray(weights, dtype=np.float64)
    r = (len(w) - 1) // 2
    H, W, _ = src.shape
    pad = np.pad(src, ((0, 0), (r, r), (0, 0)))
    rows = sum(w[t] * pad[:, t:t + W] for t in range(2 * r + 1))
    pad = np.pad(rows, ((r, r), (0, 0), (0, 0)))
    return sum(w[t] * pad[t:t + H] for t in range(2 * r + 1))


def bloom_source(lin, E, threshold):
    """float32: max(E lin - threshold, 0), the product and the difference rounded once each, a NaN -> 0"""
    lin = np.asarray(lin, dtype=np.float32)
    with np.errstate(all="ignore"):
        s = ((np.float32(E) * lin).astype(np.float32) - np.float32(threshold)).astype(np.float32)
    return np.where(s > 0, s, np.float32(0)).astype(np.float32)


def display_map(lin, E, name, white=4.0, bloom=None, strength=0.0):
    """float64 rgb of float32 lin [..., 3] under the float32 exposure E (a scalar, or an array that broadcasts against lin)"""
    lin = np.asarray(lin, dtype=np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        v = np.asarray(E, dtype=np.float32).astype(np.float64) * lin
        if bloom is not None:
            v = v + float(np.float32(strength)) * np.asarray(bloom, dtype=np.float32).astype(np.float64)
    x = np.minimum(np.where(v > 0, v, 0.0), 2.0 ** 60)  # (a NaN becomes 0)
    return srgb(curve(x, name, float(np.float32(white))))
