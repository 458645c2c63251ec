"""numpy restatement of the depth-of-field rules (include/neusky_hip.h, "Depth of field of a frame"): the reference the kernels of csrc/dof.hip
are tested against.  The circle of confusion and the mark in float32 with the header's order of operations (every operation rounded once),
so that they are the kernels' to the bit; the sample table and the lens frame in float64; the lens rays in float64 and, the same rule in
the same order, in float32: how far those two lie apart is what rounding costs, and sets the bar the kernel is held to."""
import math

import numpy as np

F = np.float32
R4_G = 1.16730397826141868426  # the real root of g^5 = g + 1
TAU24 = 2.0 * math.pi * 2.0 ** -24


def lens_table(samples):
    """float64 [samples - 1, 4] = (dx, dy, u, v): the R2 sequence in four dimensions, its last two components through the concentric map"""
    s = np.arange(1, samples, dtype=np.float64)[:, None]
    t = np.mod(0.5 + s * np.array([R4_G ** -k for k in (1, 2, 3, 4)]), 1.0)
    out = np.zeros((samples - 1, 4))
    out[:, :2] = t[:, :2] - 0.5
    for i, (a, b) in enumerate(2.0 * t[:, 2:] - 1.0):
        if a == 0.0 and b == 0.0:
            continue
        if abs(a) > abs(b):
            r, phi = a, (math.pi / 4.0) * (b / a)
        else:
            r, phi = b, math.pi / 2.0 - (math.pi / 4.0) * (a / b)
        out[i, 2:] = r * math.cos(phi), r * math.sin(phi)
    return out


def hash32(x):
    """the header's 32-bit integer hash, on uint32 arrays"""
    x = np.asarray(x).astype(np.uint64) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x.astype(np.uint32)


def focus_of(depth, acc, pixel, covered=0.5):
    """float32 1 / z_f read at the flat pixel: 1 / depth of a covered pixel of positive depth, else 0"""
    d, a = F(np.asarray(depth).reshape(-1)[pixel]), F(np.asarray(acc).reshape(-1)[pixel])
    return F(1.0) / d if (a > F(covered) and d > 0) else F(0.0)


def coc(depth, acc, afpx, izf, covered=0.5):
    """float32 [H, W]: c = (a f_px) * |iz - 1 / z_f|, iz = 1 / depth where acc > covered and not depth <= 0, else 0"""
    depth, acc = np.asarray(depth, dtype=F), np.asarray(acc, dtype=F)
    with np.errstate(all="ignore"):
        near = (acc > F(covered)) & ~(depth <= 0)
        iz = np.where(near, (F(1.0) / np.where(near, depth, F(1.0))).astype(F), F(0.0)).astype(F)
        return (F(afpx) * np.abs((iz - F(izf)).astype(F))).astype(F)


def mark(c, threshold=0.5, reach=16):
    """uint8 [H, W]: the rule as stated, one shifted comparison per offset of the window"""
    c = np.asarray(c, dtype=F)
    H, W = c.shape
    with np.errstate(all="ignore"):
        blurred = c >= F(threshold)
        wide = (c + F(0.5)).astype(F)
        reaches = [blurred & (wide >= F(d)) for d in range(reach + 1)]  # of q, per distance
    mask = np.zeros((H, W), dtype=bool)
    for dy in range(-min(reach, H - 1), min(reach, H - 1) + 1):
        for dx in range(-min(reach, W - 1), min(reach, W - 1) + 1):
            ok = reaches[max(abs(dx), abs(dy))]
            # p = q - (dy, dx): p's rows [max(0, -dy), H - max(0, dy)) see q's rows shifted by dy
            py, px = slice(max(0, -dy), H - max(0, dy)), slice(max(0, -dx), W - max(0, dx))
            qy, qx = slice(max(0, dy), H - max(0, -dy)), slice(max(0, dx), W - max(0, -dx))
            mask[py, px] |= ok[qy, qx]
    return mask.astype(np.uint8)


def mark_pairs(c, threshold=0.5, reach=16):
    """the same rule as a plain double loop over all pairs of pixels"""
    c = np.asarray(c, dtype=F)
    H, W = c.shape
    mask = np.zeros((H, W), dtype=np.uint8)
    for qy in range(H):
        for qx in range(W):
            cq = c[qy, qx]
            if not cq >= F(threshold):
                continue
            wide = F(cq + F(0.5))
            for py in range(max(0, qy - reach), min(H, qy + reach + 1)):
                for px in range(max(0, qx - reach), min(W, qx + reach + 1)):
                    if wide >= F(max(abs(qx - px), abs(qy - py))):
                        mask[py, px] = 1
    return mask


def _unnormalised(directions, norm, T):
    d = np.asarray(directions, dtype=T)
    H, W, _ = d.shape
    return d if norm is None else (d * np.asarray(norm, dtype=T).reshape(H, W, 1)).astype(T)


def _differences(D, T):
    """g_x, g_y [H, W, 3]: forward differences, backward in the last column and row"""
    gx, gy = np.zeros_like(D), np.zeros_like(D)
    gx[:, :-1] = (D[:, 1:] - D[:, :-1]).astype(T)
    gx[:, -1] = gx[:, -2]
    gy[:-1] = (D[1:] - D[:-1]).astype(T)
    gy[-1] = gy[-2]
    return gx, gy


def lens_frame(directions, norm):
    """float64 (r^, s^, w^, f_px) of a bundle [H, W, 3]: the axes of the image plane from g_x, g_y at the centre pixel (W // 2, H // 2), the
    optical axis on D's side, f_px = 1 / |g_x|; and the largest |g - g_centre| / |g_centre| over the four corner pixels"""
    D = _unnormalised(directions, norm, np.float64)
    H, W, _ = D.shape
    gx, gy = _differences(D, np.float64)
    cy, cx = H // 2, W // 2
    lx, ly = np.linalg.norm(gx[cy, cx]), np.linalg.norm(gy[cy, cx])
    r, s = gx[cy, cx] / lx, gy[cy, cx] / ly
    w = np.cross(r, s)
    if D[cy, cx] @ w <= 0:
        w = -w
    bend = max(max(np.linalg.norm(gx[y, x] - gx[cy, cx]) / lx, np.linalg.norm(gy[y, x] - gy[cy, cx]) / ly)
               for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)))
    return r, s, w, 1.0 / lx, bend


def lens_block(directions, norm, aperture, izf):
    """float64 [12]: r^, s^, w^, a, 1 / z_f, a f_px"""
    r, s, w, f_px, _ = lens_frame(directions, norm)
    return np.concatenate([r, s, w, [aperture, izf, aperture * f_px]])


def lens_rays(origins, directions, norm, pixels, table, lens, rotate=True, dtype=np.float64):
    """origins, directions [H, W, 3], norm [H, W, 1] or None, pixels [E] (flat), table [S1, 4], lens [12] -> (origins [E S1, 3], directions
    [E S1, 3], norm [E S1]) in `dtype`, pixel-major, the header's rule in its order of operations.  In float32 the angle of the turn is
    (float) h * (float) tau and its sine and cosine are float32's; in float64, float64's."""
    T = dtype
    D = _unnormalised(directions, norm, T)
    H, W, _ = D.shape
    gx, gy = _differences(D, T)
    pixels = np.clip(np.asarray(pixels, dtype=np.int64).reshape(-1), 0, H * W - 1)
    tab = np.asarray(table, dtype=T).reshape(-1, 4)
    lens = np.asarray(lens, dtype=T)
    rh, sh, wh, a, izf = lens[0:3], lens[3:6], lens[6:9], lens[9], lens[10]
    E, S1 = pixels.shape[0], tab.shape[0]
    Dp, gxp, gyp, o = (x.reshape(-1, 3)[pixels][:, None, :] for x in (D, gx, gy, np.asarray(origins, dtype=T)))
    dx, dy = tab[None, :, 0:1], tab[None, :, 1:2]
    u, v = np.broadcast_to(tab[None, :, 2], (E, S1)), np.broadcast_to(tab[None, :, 3], (E, S1))
    d = ((Dp + (dx * gxp).astype(T)).astype(T) + (dy * gyp).astype(T)).astype(T)
    if rotate:
        h = (hash32(pixels.astype(np.uint64)) >> np.uint32(8)).astype(T)
        theta = ((h * T(TAU24)).astype(T))[:, None]
        sn, cs = np.sin(theta).astype(T), np.cos(theta).astype(T)
        u, v = ((u * cs).astype(T) - (v * sn).astype(T)).astype(T), ((u * sn).astype(T) + (v * cs).astype(T)).astype(T)
    lp = (a * ((u[..., None] * rh).astype(T) + (v[..., None] * sh).astype(T)).astype(T)).astype(T)

    def dot(p, q):
        x, y, z = ((p[..., c] * q[..., c]).astype(T) for c in range(3))
        return ((x + y).astype(T) + z).astype(T)

    k = dot(d, np.broadcast_to(wh, d.shape))
    t = (k * izf).astype(T)
    d = (d - (t[..., None] * lp).astype(T)).astype(T)
    length = np.sqrt(dot(d, d)).astype(T)
    with np.errstate(all="ignore"):
        return ((o + lp).astype(T).reshape(-1, 3), (d / length[..., None]).astype(T).reshape(-1, 3), (length / k).astype(T).reshape(-1))
