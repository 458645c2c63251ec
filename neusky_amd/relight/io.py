"""Readers of equirectangular environment maps, numpy and PIL only: Radiance RGBE (.hdr / .pic), .pfm, .npy, sRGB .png / .jpg and,
when pyexr imports, .exr.  Every reader returns float32 [H, W, 3] linear radiance with row 0 at the top."""
from __future__ import annotations

import os

import numpy as np

FORMATS = (".hdr", ".pic", ".pfm", ".npy", ".png", ".jpg", ".jpeg")


def srgb_to_linear(s: np.ndarray) -> np.ndarray:
    """the exact inverse of utils.linear_to_sRGB on [0, 1]: s <= 12.92 * 0.0031308 -> s / 12.92, else ((s + 0.055) / 1.055)^2.4"""
    s = np.asarray(s, dtype=np.float64)
    return np.where(s <= 12.92 * 0.0031308, s / 12.92, np.power((s + 0.055) / 1.055, 2.4))


def _rgbe_to_float(rgbe: np.ndarray) -> np.ndarray:
    """RGBE bytes [..., 4] -> float32 [..., 3]: mantissa * 2^(e - 136), 0 where e == 0 (stb_image's and FreeImage's decoding)"""
    e = rgbe[..., 3].astype(np.int32)
    out = np.ldexp(rgbe[..., :3].astype(np.float32), (e - 136)[..., None]).astype(np.float32)
    out[e == 0] = 0.0
    return out


def read_hdr(path) -> np.ndarray:
    """Radiance RGBE: flat scanlines and new-style run-length scanlines.  Only the standard orientation `-Y H +X W` is read."""
    with open(path, "rb") as f:
        buf = f.read()
    pos = 0

    def line():
        nonlocal pos
        end = buf.find(b"\n", pos)
        if end < 0:
            raise ValueError(f"{path}: truncated Radiance header")
        s = buf[pos:end].decode("latin-1")
        pos = end + 1
        return s

    magic = line()
    if not magic.startswith("#?"):
        raise ValueError(f"{path}: not a Radiance file (no #? signature)")
    while True:
        s = line().strip()
        if not s:
            break
        if s.startswith("FORMAT=") and s != "FORMAT=32-bit_rle_rgbe":
            raise ValueError(f"{path}: unsupported pixel format {s[7:]!r} (only 32-bit_rle_rgbe)")
    res = line().split()
    if len(res) != 4 or res[0] != "-Y" or res[2] != "+X":
        raise ValueError(f"{path}: unsupported orientation {' '.join(res)!r}: only '-Y H +X W' (row 0 at the top) is read")
    H, W = int(res[1]), int(res[3])
    data = np.frombuffer(buf, dtype=np.uint8, offset=pos)
    out = np.empty((H, W, 4), dtype=np.uint8)
    p = 0
    for y in range(H):
        if 8 <= W < 32768 and p + 4 <= data.size and data[p] == 2 and data[p + 1] == 2 and (int(data[p + 2]) << 8 | int(data[p + 3])) == W:
            p += 4
            for c in range(4):  # new-style RLE: each component on its own, runs (count > 128) or literals
                x = 0
                while x < W:
                    if p >= data.size:
                        raise ValueError(f"{path}: truncated scanline {y}")
                    n = int(data[p])
                    p += 1
                    if n > 128:
                        n -= 128
                        if x + n > W or p >= data.size:
                            raise ValueError(f"{path}: bad run in scanline {y}")
                        out[y, x:x + n, c] = data[p]
                        p += 1
                    else:
                        if n == 0 or x + n > W or p + n > data.size:
                            raise ValueError(f"{path}: bad literal in scanline {y}")
                        out[y, x:x + n, c] = data[p:p + n]
                        p += n
                    x += n
        else:  # flat scanline
            if p + 4 * W > data.size:
                raise ValueError(f"{path}: truncated scanline {y}")
            out[y] = data[p:p + 4 * W].reshape(W, 4)
            p += 4 * W
    return _rgbe_to_float(out)


def read_pfm(path) -> np.ndarray:
    """Portable float map: `PF` (RGB) or `Pf` (grey), rows stored bottom to top, the scale's sign giving the byte order"""
    with open(path, "rb") as f:
        tokens = []
        while len(tokens) < 4:
            s = f.readline()
            if not s:
                raise ValueError(f"{path}: truncated PFM header")
            tokens += s.split()
        kind, W, H, scale = tokens[0].decode(), int(tokens[1]), int(tokens[2]), float(tokens[3])
        if kind not in ("PF", "Pf"):
            raise ValueError(f"{path}: not a PFM file")
        C = 3 if kind == "PF" else 1
        raw = np.fromfile(f, dtype="<f4" if scale < 0 else ">f4", count=H * W * C)
    if raw.size != H * W * C:
        raise ValueError(f"{path}: truncated PFM data")
    img = raw.reshape(H, W, C)[::-1].astype(np.float32)
    return np.ascontiguousarray(np.repeat(img, 3, axis=2) if C == 1 else img)


def read_npy(path) -> np.ndarray:
    a = np.load(path)
    if a.ndim != 3 or a.shape[2] not in (3, 4):
        raise ValueError(f"{path}: expected an array [H, W, 3] or [H, W, 4], got {a.shape}")
    return np.ascontiguousarray(a[..., :3], dtype=np.float32)


def read_ldr(path) -> np.ndarray:
    """8-bit sRGB (NeRF-OSR's ENV_MAP_CC captures are JPEGs), linearised with the exact inverse of utils.linear_to_sRGB"""
    from PIL import Image
    with Image.open(path) as im:
        a = np.asarray(im.convert("RGB"), dtype=np.float64) / 255.0
    return srgb_to_linear(a).astype(np.float32)


def read_exr(path) -> np.ndarray:
    try:
        import pyexr
    except ImportError:
        raise ValueError(f"{path}: reading .exr needs pyexr, which is not installed; readable formats: {', '.join(FORMATS)}") from None
    a = np.asarray(pyexr.read(path), dtype=np.float32)
    if a.ndim == 2:
        a = a[..., None]
    return np.ascontiguousarray(np.repeat(a, 3, axis=2) if a.shape[2] == 1 else a[..., :3])


def read_envmap(path) -> np.ndarray:
    """float32 [H, W, 3] linear radiance of an equirectangular map file, row 0 at the top"""
    ext = os.path.splitext(str(path))[1].lower()
    if ext in (".hdr", ".pic"):
        return read_hdr(path)
    if ext == ".pfm":
        return read_pfm(path)
    if ext == ".npy":
        return read_npy(path)
    if ext in (".png", ".jpg", ".jpeg"):
        return read_ldr(path)
    if ext == ".exr":
        return read_exr(path)
    raise ValueError(f"{path}: unknown environment-map format {ext!r}; readable formats: {', '.join(FORMATS)} (.exr with pyexr)")
