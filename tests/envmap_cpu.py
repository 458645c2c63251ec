"""float64 numpy restatement of the environment-map definitions (include/neusky_hip.h, relight/envmap.py): texel directions, solid
angles, cell labels, the cell-average projection and the bilinear lookup; plus the tests' own Radiance RGBE and PFM writers."""
from __future__ import annotations

import numpy as np

CONVENTIONS = ("neusky", "blender")


def texel_angles(H: int, W: int, convention: str):
    """(theta [H], phi [W]) of the texel centres"""
    theta = np.pi * (np.arange(H) + 0.5) / H
    u = (np.arange(W) + 0.5) / W
    phi = 2 * np.pi * u if convention == "neusky" else np.pi - 2 * np.pi * u
    return theta, phi


def texel_directions(H: int, W: int, convention: str) -> np.ndarray:
    """[H, W, 3] unit directions of the texel centres"""
    theta, phi = texel_angles(H, W, convention)
    st, ct = np.sin(theta)[:, None], np.cos(theta)[:, None]
    return np.stack(np.broadcast_arrays(st * np.cos(phi)[None], st * np.sin(phi)[None], ct), -1)


def solid_angles(H: int, W: int) -> np.ndarray:
    """[H] solid angle of one texel of each row: (2 pi / W) (cos(pi i / H) - cos(pi (i + 1) / H))"""
    i = np.arange(H)
    return (2 * np.pi / W) * (np.cos(np.pi * i / H) - np.cos(np.pi * (i + 1) / H))


def direction_to_texel(v: np.ndarray, H: int, W: int, convention: str):
    """continuous texel coordinates (x, y) of directions v [..., 3]: texel centres at integers"""
    v = np.asarray(v, dtype=np.float64)
    theta = np.arctan2(np.hypot(v[..., 0], v[..., 1]), v[..., 2])
    phi = np.arctan2(v[..., 1], v[..., 0])
    u = phi / (2 * np.pi)
    if convention == "blender":
        u = 0.5 - u
    return u * W - 0.5, theta / np.pi * H - 0.5


def rotate(dirs: np.ndarray, rotation) -> np.ndarray:
    d = np.asarray(dirs, dtype=np.float64)
    return d if rotation is None else d @ np.asarray(rotation, dtype=np.float64).T


def labels_of(t: np.ndarray, dirs: np.ndarray, rotation=None, chunk: int = 1 << 16):
    """(label [N], margin [N]) of unit directions t [N, 3]: the arg-max of <t, R d_k> (ties to the lower k) and the gap between the
    best and the second-best dot product"""
    rd = rotate(dirs, rotation)
    t = np.asarray(t, dtype=np.float64).reshape(-1, 3)
    lab = np.empty(t.shape[0], dtype=np.int64)
    gap = np.empty(t.shape[0])
    for a in range(0, t.shape[0], chunk):
        dots = t[a:a + chunk] @ rd.T
        lab[a:a + chunk] = np.argmax(dots, axis=1)
        top2 = np.partition(dots, -2, axis=1)[:, -2:] if dots.shape[1] > 1 else np.concatenate([dots, dots - np.inf], 1)
        gap[a:a + chunk] = top2[:, 1] - top2[:, 0]
    return lab, np.abs(gap)


def lookup(envmap: np.ndarray, convention: str, v: np.ndarray, rotation=None, exposure: float = 1.0) -> np.ndarray:
    """[N, 3] bilinear lookup at R v: columns wrap modulo W, rows clamp to [0, H-1]"""
    m = np.asarray(envmap, dtype=np.float64)
    H, W = m.shape[:2]
    x, y = direction_to_texel(rotate(v, rotation), H, W, convention)
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = (x - x0)[:, None], (y - y0)[:, None]
    j0 = np.mod(x0.astype(np.int64), W)
    j1 = np.mod(j0 + 1, W)
    i0 = np.clip(y0.astype(np.int64), 0, H - 1)
    i1 = np.clip(y0.astype(np.int64) + 1, 0, H - 1)
    top = (1 - fx) * m[i0, j0] + fx * m[i0, j1]
    bot = (1 - fx) * m[i1, j0] + fx * m[i1, j1]
    return exposure * ((1 - fy) * top + fy * bot)


def project(envmap: np.ndarray, convention: str, dirs: np.ndarray, rotation=None, exposure: float = 1.0, labels=None):
    """(colours [D, 3], cell_weight [D]): the solid-angle-weighted mean of each direction's cell, the bilinear lookup at R d_k for a cell
    without a texel centre.  labels: [H, W] cells to reduce over (default: this restatement's own arg-max)"""
    m = np.asarray(envmap, dtype=np.float64)
    H, W = m.shape[:2]
    D = dirs.shape[0]
    if labels is None:
        labels = labels_of(texel_directions(H, W, convention).reshape(-1, 3), dirs, rotation)[0]
    lab = np.asarray(labels).reshape(-1).astype(np.int64)
    w = np.repeat(solid_angles(H, W), W)
    wsum = np.bincount(lab, weights=w, minlength=D)
    num = np.stack([np.bincount(lab, weights=w * m[..., c].reshape(-1), minlength=D) for c in range(3)], -1)
    cols = np.empty((D, 3))
    full = wsum > 0
    cols[full] = exposure * num[full] / wsum[full, None]
    if (~full).any():
        cols[~full] = lookup(m, convention, np.asarray(dirs, dtype=np.float64)[~full], rotation, exposure)
    return cols, wsum


# ---- writers used by the tests (the package only reads)
def float_to_rgbe(rgb: np.ndarray) -> np.ndarray:
    """float [..., 3] -> RGBE bytes [..., 4] (Radiance's float2rgbe)"""
    rgb = np.asarray(rgb, dtype=np.float64)
    v = rgb.max(-1)
    mant, ex = np.frexp(v)
    scale = np.where(v > 1e-32, mant * 256.0 / np.where(v > 1e-32, v, 1.0), 0.0)
    out = np.zeros(rgb.shape[:-1] + (4,), dtype=np.uint8)
    out[..., :3] = np.clip(np.floor(rgb * scale[..., None]), 0, 255).astype(np.uint8)
    out[..., 3] = np.where(v > 1e-32, ex + 128, 0).astype(np.uint8)
    return out


def rgbe_to_float(rgbe: np.ndarray) -> np.ndarray:
    e = rgbe[..., 3].astype(np.int64)
    f = np.where(e > 0, np.ldexp(1.0, e - 136), 0.0)
    return (rgbe[..., :3].astype(np.float64) * f[..., None]).astype(np.float32)


def _rle_component(vals: np.ndarray) -> bytes:
    """one component of a new-style RLE scanline: runs of >= 3 equal bytes as (128 + n, byte), the rest as literals (n <= 128)"""
    out = bytearray()
    i, n = 0, len(vals)
    lit = []
    while i < n:
        j = i
        while j < n and vals[j] == vals[i] and j - i < 127:
            j += 1
        if j - i >= 3:
            while lit:
                out += bytes([min(len(lit), 128)]) + bytes(lit[:128])
                lit = lit[128:]
            out += bytes([128 + (j - i), int(vals[i])])
            i = j
        else:
            lit.append(int(vals[i]))
            i += 1
    while lit:
        out += bytes([min(len(lit), 128)]) + bytes(lit[:128])
        lit = lit[128:]
    return bytes(out)


def write_hdr(path, rgbe: np.ndarray, rle: bool, orientation: str = None) -> None:
    """Radiance file of RGBE bytes [H, W, 4], flat or new-style RLE scanlines"""
    H, W = rgbe.shape[:2]
    with open(path, "wb") as f:
        f.write(b"#?RADIANCE\n# written by the relight tests\nFORMAT=32-bit_rle_rgbe\n\n")
        f.write((orientation or f"-Y {H} +X {W}").encode() + b"\n")
        for y in range(H):
            if rle:
                f.write(bytes([2, 2, W >> 8, W & 255]))
                for c in range(4):
                    f.write(_rle_component(rgbe[y, :, c]))
            else:
                f.write(rgbe[y].tobytes())


def write_pfm(path, rgb: np.ndarray, little_endian: bool = True) -> None:
    H, W = rgb.shape[:2]
    with open(path, "wb") as f:
        f.write(f"PF\n{W} {H}\n{-1.0 if little_endian else 1.0}\n".encode())
        f.write(np.ascontiguousarray(rgb[::-1], dtype="<f4" if little_endian else ">f4").tobytes())
