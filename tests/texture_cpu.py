"""An independent numpy float64 restatement of the texture-atlas definitions of include/neusky_hip.h (nsky_texture_*) for the
tests: layout, owner map, corner texels and UVs, the clamped barycentrics of a texel, the texel points in the kernel's order, and
the taps of a bilinear lookup.  Written from the definitions, not from the kernels.

P = px_per_uv_triangle, Q = P + 3 texels per side of a square, faces 2 s (lower) and 2 s + 1 (upper) in square s, S =
ceil(sqrt(ceil(F / 2))) squares per row, W = S Q; texel (i, j) of a square is column i, row j, and a texel's centre is its index."""
import math

import numpy as np


def layout(F, P):
    squares = -(-F // 2)
    S = 0
    while S * S < squares:
        S += 1
    Q = P + 3
    return S * Q, S, Q


def corner_texels(F, P):
    """[F, 3, 2] int64: the global texel index (x, y) of every face corner"""
    W, S, Q = layout(F, P)
    out = np.zeros((F, 3, 2), np.int64)
    for f in range(F):
        s = f // 2
        x0, y0 = (s % S) * Q, (s // S) * Q
        local = [(0, 0), (P, 0), (0, P)] if f % 2 == 0 else [(P + 2, P + 2), (2, P + 2), (P + 2, 2)]
        for k, (i, j) in enumerate(local):
            out[f, k] = (x0 + i, y0 + j)
    return out


def uvs(F, P):
    """[F, 3, 2] float64: u = (x + 0.5) / W, v = 1 - (y + 0.5) / W"""
    W, _, _ = layout(F, P)
    c = corner_texels(F, P).astype(np.float64)
    return np.stack([(c[..., 0] + 0.5) / max(W, 1), 1.0 - (c[..., 1] + 0.5) / max(W, 1)], -1)


def square_owner(F, P, s, i, j):
    """the face that owns texel (i, j) of square s, -1 for none"""
    f = 2 * s if i + j <= P + 2 else 2 * s + 1
    return f if f < F else -1


def owner_map(F, P):
    """[W, W] int64 (row y, column x): the owning face of every texel of the image, -1 for none"""
    W, S, Q = layout(F, P)
    out = np.full((W, W), -1, np.int64)
    for s in range(S * S):
        for j in range(Q):
            for i in range(Q):
                out[(s // S) * Q + j, (s % S) * Q + i] = square_owner(F, P, s, i, j)
    return out


def barycentrics(P, upper, i, j):
    """(b0, b1, b2) of texel (i, j) in the lower / upper face of its square: negative components 0, the rest divided by their sum"""
    if upper:
        b1, b2 = (P + 2 - i) / P, (P + 2 - j) / P
    else:
        b1, b2 = i / P, j / P
    b = np.maximum(np.array([1.0 - b1 - b2, b1, b2], np.float64), 0.0)
    return b / b.sum()


def texel_points(vertices, faces, P, s0=0, s1=None):
    """(owner [n] int64, offset [n] int64, points [n, 3] float64) of the texels of squares [s0, s1), square after square, row-major
    inside a square; points without an owner are 0"""
    F = len(faces)
    W, S, Q = layout(F, P)
    if s1 is None:
        s1 = -(-F // 2)
    v = np.asarray(vertices, np.float64)
    owner, offset, points = [], [], []
    for s in range(s0, s1):
        for j in range(Q):
            for i in range(Q):
                f = square_owner(F, P, s, i, j)
                owner.append(f)
                offset.append(((s // S) * Q + j) * W + (s % S) * Q + i)
                if f < 0:
                    points.append(np.zeros(3))
                    continue
                b = barycentrics(P, f % 2 == 1, i, j)
                a, bb, c = (int(t) for t in faces[f])
                points.append(b[0] * v[a] + b[1] * v[bb] + b[2] * v[c])
    return (np.array(owner, np.int64).reshape(-1), np.array(offset, np.int64).reshape(-1),
            np.array(points, np.float64).reshape(-1, 3))


def bilinear_taps(x, y):
    """the texels a bilinear lookup at the continuous texel position (x, y) reads with a non-zero weight: [(column, row, weight)]"""
    x0, y0 = math.floor(x), math.floor(y)
    fx, fy = x - x0, y - y0
    taps = [(x0, y0, (1 - fx) * (1 - fy)), (x0 + 1, y0, fx * (1 - fy)), (x0, y0 + 1, (1 - fx) * fy), (x0 + 1, y0 + 1, fx * fy)]
    return [t for t in taps if t[2] != 0.0]


def srgb_levels(linear):
    """float64: clamp(srgb(x), 0, 1) * 255, before rounding"""
    x = np.asarray(linear, np.float64)
    y = np.where(x <= 0.0031308, 12.92 * x, 1.055 * np.abs(x) ** (1 / 2.4) - 0.055)
    return np.clip(y, 0.0, 1.0) * 255.0
