"""numpy restatement of the antialiasing rules (include/neusky_hip.h, "Adaptive antialiasing of a frame"): the reference the kernels of
csrc/antialias.hip are tested against.  The edge mask in float32 with the header's order of operations (every product, sum and difference
rounded once), so that it is the kernel's mask to the bit; the sub-pixel rays in float32 (the same order) and in float64; the resolve in
float64; and the float64 pinhole the rays are measured against."""
import math

import numpy as np

F = np.float32
R2_G = 1.32471795724474602596


def r2_offsets(samples):
    """float64 [samples - 1, 2]: frac(0.5 + s (1 / g, 1 / g^2)) - 0.5, s = 1 .. samples - 1"""
    s = np.arange(1, samples, dtype=np.float64)[:, None]
    a = np.array([1.0 / R2_G, 1.0 / (R2_G * R2_G)])
    return np.mod(0.5 + s * a, 1.0) - 0.5


def luminance(lin):
    lin = np.asarray(lin, dtype=F)
    with np.errstate(all="ignore"):
        r, g, b = (F(w) * lin[..., c] for c, w in enumerate((0.2126, 0.7152, 0.0722)))
        return ((r + g).astype(F) + b).astype(F)


def _dot(a, b):
    """(x x' + y y') + z z' in float32"""
    with np.errstate(all="ignore"):
        x, y, z = ((a[..., c] * b[..., c]).astype(F) for c in range(3))
        return ((x + y).astype(F) + z).astype(F)


def _pairs(H, W):
    """the two slicings (p, q) of every horizontally and every vertically adjacent pair"""
    if W > 1:
        yield (slice(None), slice(0, W - 1)), (slice(None), slice(1, W))
    if H > 1:
        yield (slice(0, H - 1), slice(None)), (slice(1, H), slice(None))


def edge_mask(depth, normal, acc, lin, colour=0.1, depth_t=0.02, normal_deg=15.0, accumulation=0.1, covered=0.5, criteria=None):
    """uint8 [H, W] of depth [H, W], normal [H, W, 3], acc [H, W] and lin [K, H, W, 3] (or None).  criteria: a subset of ("accumulation",
    "depth", "normal", "colour") to apply (all by default): what marks a pixel can be told apart"""
    depth, normal, acc = np.asarray(depth, dtype=F), np.asarray(normal, dtype=F), np.asarray(acc, dtype=F)
    H, W = acc.shape
    lin = np.zeros((0, H, W, 3), F) if lin is None else np.asarray(lin, dtype=F).reshape(-1, H, W, 3)
    on = set(criteria or ("accumulation", "depth", "normal", "colour"))
    t_acc, t_depth, t_col, cov = F(accumulation), F(depth_t), F(colour), F(covered)
    cos2 = F(math.cos(math.radians(normal_deg)) ** 2)
    nn = _dot(normal, normal)
    Y = [luminance(img) for img in lin]
    mask = np.zeros((H, W), dtype=bool)
    with np.errstate(all="ignore"):
        for p, q in _pairs(H, W):
            differs = np.zeros(acc[p].shape, dtype=bool)
            if "accumulation" in on:
                differs |= np.abs((acc[p] - acc[q]).astype(F)) > t_acc
            both = (acc[p] > cov) & (acc[q] > cov)
            if "depth" in on:
                differs |= both & (np.abs((depth[p] - depth[q]).astype(F)) > (t_depth * np.fmin(depth[p], depth[q])).astype(F))
            if "normal" in on:
                d = _dot(normal[p], normal[q])
                bound = (cos2 * (nn[p] * nn[q]).astype(F)).astype(F)
                long_enough = (nn[p] >= F(1e-12)) & (nn[q] >= F(1e-12))
                differs |= both & long_enough & ((d <= 0) | ((d * d).astype(F) < bound))
            if "colour" in on:
                for y in Y:
                    top = np.fmax(np.fmax(y[p], y[q]), F(1e-4))
                    differs |= np.abs((y[p] - y[q]).astype(F)) > (t_col * top).astype(F)
            mask[p] |= differs
            mask[q] |= differs
    return mask.astype(np.uint8)


def synthetic_gbuffer(H, W, K, seed=0, cell=3):
    """a G-buffer of `cell` x `cell` blocks, each of one of 8 kinds, half of them kind 0; every value a small dyadic rational, so that under
    the default thresholds no comparison sits at its threshold:
      0 the base: accumulation 1, depth 2, normal +z, every image 0.5 grey     1 accumulation 0.875 (the accumulation test alone)
      2 depth 2.125 (depth alone)     3 normal (0, 0.5, 0.75) (normal alone)     4 the last image (0.5, 0.625, 0.5) (colour alone)
      5 uncovered: accumulation 0.25, depth 9, normal +x     6 uncovered: accumulation 0.3125, depth 5, normal +y (a pair of 5 and 6
      differs in depth and normal and must NOT be marked for it: 0.0625 of accumulation is below the threshold)     7 a zero normal
    -> dict(depth [H, W], normal [H, W, 3], acc [H, W], lin [K, H, W, 3]) and the kinds [H, W]"""
    rng = np.random.default_rng(seed)
    kinds = rng.choice(8, size=(-(-H // cell), -(-W // cell)), p=[0.5] + [0.5 / 7] * 7)
    kinds = np.repeat(np.repeat(kinds, cell, 0), cell, 1)[:H, :W]
    depth, acc = np.full((H, W), 2.0, F), np.ones((H, W), F)
    normal, lin = np.tile(F([0, 0, 1]), (H, W, 1)), np.full((K, H, W, 3), 0.5, F)
    acc[kinds == 1] = 0.875
    depth[kinds == 2] = 2.125
    normal[kinds == 3] = (0.0, 0.5, 0.75)
    if K:
        lin[K - 1][kinds == 4] = (0.5, 0.625, 0.5)
    acc[kinds == 5], depth[kinds == 5], normal[kinds == 5] = 0.25, 9.0, (1.0, 0.0, 0.0)
    acc[kinds == 6], depth[kinds == 6], normal[kinds == 6] = 0.3125, 5.0, (0.0, 1.0, 0.0)
    normal[kinds == 7] = 0.0
    return dict(depth=depth, normal=normal, acc=acc, lin=lin), kinds


def subpixel_rays(directions, norm, pixels, offsets, dtype=np.float32):
    """directions [H, W, 3], norm [H, W, 1] or None, pixels [E] (flat), offsets [S1, 2] -> (directions [E S1, 3], norm [E S1]) in `dtype`,
    pixel-major, the header's rule in its order of operations"""
    T = dtype
    d = np.asarray(directions, dtype=T)
    H, W, _ = d.shape
    D = d if norm is None else (d * np.asarray(norm, dtype=T).reshape(H, W, 1)).astype(T)
    gx, gy = np.zeros_like(D), np.zeros_like(D)
    if W > 1:
        gx[:, :-1] = (D[:, 1:] - D[:, :-1]).astype(T)
        gx[:, -1] = gx[:, -2]
    if H > 1:
        gy[:-1] = (D[1:] - D[:-1]).astype(T)
        gy[-1] = gy[-2]
    pixels = np.asarray(pixels, dtype=np.int64).reshape(-1)
    off = np.asarray(offsets, dtype=T).reshape(-1, 2)
    Dp, gxp, gyp = (a.reshape(-1, 3)[pixels][:, None, :] for a in (D, gx, gy))
    dx, dy = off[None, :, 0:1], off[None, :, 1:2]
    out = ((Dp + (dx * gxp).astype(T)).astype(T) + (dy * gyp).astype(T)).astype(T).reshape(-1, 3)
    x, y, z = ((out[:, c] * out[:, c]).astype(T) for c in range(3))
    length = np.sqrt(((x + y).astype(T) + z).astype(T)).astype(T)
    return (out / length[:, None]).astype(T), length


def pinhole(H, W, fov_deg, c2w, x, y):
    """float64: the un-normalised direction R ((x - W / 2) / f, -(y - H / 2) / f, -1) of relight.camera_rays' pinhole at the continuous
    pixel coordinate (x, y) (a pixel's centre is at its index + 0.5), normalised, and its length"""
    f = 0.5 * H / math.tan(math.radians(float(fov_deg)) / 2.0)
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    cam = np.stack([(x - 0.5 * W) / f, -(y - 0.5 * H) / f, -np.ones_like(x)], -1)
    d = cam @ np.asarray(c2w, dtype=np.float64)[:, :3].T
    n = np.linalg.norm(d, axis=-1)
    return d / n[..., None], n


def pinhole_subpixel(H, W, fov_deg, c2w, pixels, offsets):
    """float64 (directions [E S1, 3], norm [E S1]) of the pinhole at (x + 0.5 + dx, y + 0.5 + dy), pixel-major"""
    pixels = np.asarray(pixels, dtype=np.int64).reshape(-1)
    off = np.asarray(offsets, dtype=np.float64).reshape(-1, 2)
    x = (pixels % W)[:, None] + 0.5 + off[None, :, 0]
    y = (pixels // W)[:, None] + 0.5 + off[None, :, 1]
    d, n = pinhole(H, W, fov_deg, c2w, x.reshape(-1), y.reshape(-1))
    return d, n


def look_at(angle=0.3, radius=0.6, height=0.05):
    """a camera-to-world [3, 4] on a circle about the origin, looking at it (OpenGL: the camera looks down -z, +y up)"""
    c, s = math.cos(angle), math.sin(angle)
    eye = np.array([radius * c, radius * s, height])
    fwd = -eye / np.linalg.norm(eye)
    right = np.cross(fwd, [0.0, 0.0, 1.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    m = np.zeros((3, 4))
    m[:, 0], m[:, 1], m[:, 2], m[:, 3] = right, up, -fwd, eye
    return m


def resolve(frame, samples, pixels):
    """float64: frame [K, P, C], samples [K, E, S1, C], pixels [E] -> the frame with (frame + sum_s samples) / (S1 + 1) at the listed pixels"""
    out = np.asarray(frame, dtype=np.float64).copy()
    X = np.asarray(samples, dtype=np.float64)
    pixels = np.asarray(pixels, dtype=np.int64).reshape(-1)
    out[:, pixels] = (out[:, pixels] + X.sum(axis=2)) / (X.shape[2] + 1)
    return out


def srgb(y):
    """clamp(linear_to_sRGB(y), 0, 1) in float64"""
    y = np.asarray(y, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        s = np.where(y <= 0.0031308, 12.92 * y, 1.055 * np.abs(y) ** (1.0 / 2.4) - 0.055)
    return np.clip(s, 0.0, 1.0)
