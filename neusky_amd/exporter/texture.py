"""Texture baking for the mesh export: a per-triangle-pair atlas filled from the field, and a Wavefront OBJ writer
(include/neusky_hip.h, nsky_texture_*; csrc/texture.hip).

Layout (P = px_per_uv_triangle, nerfstudio's name and default): a square of Q = P + 3 texels per side holds faces 2 s (lower) and
2 s + 1 (upper); S = ceil(sqrt(ceil(F / 2))) squares per row; the image is W x W with W = S Q, row 0 at the top.  In texel indices
(column i, row j) of the square, a texel's centre being its index:
  lower  v0 (0, 0)      v1 (P, 0)    v2 (0, P)      owns i + j <= P + 2
  upper  v0 (P+2, P+2)  v1 (2, P+2)  v2 (P+2, 2)    owns i + j >= P + 3
so that each face has a gutter of about a texel and a half on the diagonal side, and a bilinear lookup anywhere in a face's UV
triangle reads only texels that face owns.  A texel samples the point of its face whose barycentrics it has at its centre, negative
components set to 0 and the rest divided by their sum: gutter texels repeat the nearest edge or corner of their own triangle.

Per chunk of whole squares: the texel-points kernel, the field's fused value chain (field.field_values) at those points, the
texel-store kernel (sRGB encoding as the vertex colours; optionally the unit gradient as an object-space normal map)."""
from __future__ import annotations

import math
import os
from dataclasses import dataclass
from typing import Callable, Optional, Tuple

import numpy as np
import torch

from .. import hip
from .mesh import Mesh, _field_device, refresh_field
from .simplify import _check_mesh

MAX_SIZE = hip.TEXTURE_MAX_SIZE
CHUNK = 1 << 20  # texels per field call (the chain's scratch grows with the rows of a call)


@dataclass
class TextureAtlas:
    image: torch.Tensor                   # [W, W, 3] uint8, sRGB, row 0 at the top
    normal_image: Optional[torch.Tensor]  # [W, W, 3] uint8, n * 0.5 + 0.5 of the unit SDF gradient (object space), or None
    uvs: torch.Tensor                     # [F, 3, 2] fp32, (u, v) of every face corner, v up
    px_per_uv_triangle: int


def _check_px(px_per_uv_triangle, who: str) -> int:
    if isinstance(px_per_uv_triangle, bool) or not isinstance(px_per_uv_triangle, int) or px_per_uv_triangle < 1:
        raise ValueError(f"{who}: px_per_uv_triangle must be an integer >= 1, got {px_per_uv_triangle!r}")
    return px_per_uv_triangle


def atlas_layout(num_faces: int, px_per_uv_triangle: int = 4) -> Tuple[int, int, int]:
    """(W, S, Q): the side of the texture in texels, the squares per row, the texels per side of a square.  (0, 0, Q) without faces."""
    P = _check_px(px_per_uv_triangle, "atlas_layout")
    if isinstance(num_faces, bool) or not isinstance(num_faces, int) or num_faces < 0:
        raise ValueError(f"atlas_layout: num_faces must be a non-negative integer, got {num_faces!r}")
    squares = (num_faces + 1) // 2
    S = math.isqrt(squares - 1) + 1 if squares else 0  # ceil(sqrt(squares)) in integers
    Q = P + 3
    W = S * Q
    if W > MAX_SIZE:
        raise ValueError(f"atlas_layout: F = {num_faces} faces at P = {P} texels per triangle leg need a {W} x {W} texture, more than "
                         f"{MAX_SIZE} a side: simplify the mesh further (--target-num-faces) or lower px_per_uv_triangle")
    return W, S, Q


def face_uvs(num_faces: int, px_per_uv_triangle: int = 4, device=None) -> torch.Tensor:
    """[F, 3, 2] fp32: (u, v) of the three corners of every face, u = (x + 0.5) / W, v = 1 - (y + 0.5) / W at the corner's global
    texel index (x, y); computed in float64 and rounded once"""
    W, S, Q = atlas_layout(num_faces, px_per_uv_triangle)
    P = px_per_uv_triangle
    if num_faces == 0:
        return torch.zeros(0, 3, 2, dtype=torch.float32, device=device)
    f = torch.arange(num_faces, dtype=torch.int64, device=device)
    s = f // 2
    lower = torch.tensor([[0, 0], [P, 0], [0, P]], dtype=torch.int64, device=device)
    upper = torch.tensor([[P + 2, P + 2], [2, P + 2], [P + 2, 2]], dtype=torch.int64, device=device)
    corner = torch.where((f % 2 == 1)[:, None, None], upper, lower)              # [F, 3, 2]: (i, j) inside the square
    origin = torch.stack([(s % S) * Q, (s // S) * Q], -1)[:, None, :]            # [F, 1, 2]: (x, y) of the square
    xy = (corner + origin).double()
    return torch.stack([(xy[..., 0] + 0.5) / W, 1.0 - (xy[..., 1] + 0.5) / W], -1).float()


def _squares(num_faces: int, squares, S: int, who: str) -> Tuple[int, int]:
    n_sq = (num_faces + 1) // 2
    if squares is None:
        return 0, n_sq
    s0, s1 = (int(x) for x in squares)
    if not 0 <= s0 <= s1 <= S * S:
        raise ValueError(f"{who}: squares [{s0}, {s1}) outside the atlas of {S} x {S} squares")
    return s0, s1


def _points(v, f, P: int, S: int, Q: int, s0: int, s1: int):
    n = (s1 - s0) * Q * Q
    owner = torch.empty(n, dtype=torch.int32, device=v.device)
    offset = torch.empty(n, dtype=torch.int64, device=v.device)
    points = torch.empty(n, 3, dtype=torch.float32, device=v.device)
    hip.texture_texel_points(v, f, P, S, s0, s1, owner, offset, points)
    return owner, offset, points


def texel_points(mesh: Mesh, px_per_uv_triangle: int = 4, squares: Optional[Tuple[int, int]] = None):
    """(owner int32 [n], offset int64 [n], points fp32 [n, 3]) of the texels of squares [s0, s1) (default: every square that holds a
    face), square after square, row-major inside a square: the face that owns the texel (-1: none), its offset y W + x in the image,
    the point of that face it samples"""
    P = _check_px(px_per_uv_triangle, "texel_points")
    v, f = _check_mesh(mesh, "texel_points")
    W, S, Q = atlas_layout(f.shape[0], P)
    s0, s1 = _squares(f.shape[0], squares, S, "texel_points")
    with torch.cuda.device(v.device):
        return _points(v, f, P, S, Q, s0, s1)


@torch.no_grad()
def bake_texture(mesh: Mesh, field=None, *, shade: Optional[Callable] = None, px_per_uv_triangle: int = 4, normal_map: bool = False,
                 chunk: int = CHUNK) -> TextureAtlas:
    """The atlas of `mesh`: every owned texel carries the sRGB-encoded albedo of `field` at the point it samples (the encoding of the
    mesh's vertex colours), unowned texels are 0.  normal_map: also the unit SDF gradient, as n * 0.5 + 0.5.

    Exactly one of
      field   an SDFAlbedoField on the mesh's device (its prepared weights are refreshed once, then field.field_values per chunk);
      shade   shade(points [n, 3]) -> (linear rgb [n, 3], gradient [n, 3]), fp32 on the points' device: bakes something else.
    chunk: texels per call of field / shade, rounded down to whole squares (at least one); the result does not depend on it."""
    who = "bake_texture"
    P = _check_px(px_per_uv_triangle, who)
    if (field is None) == (shade is None):
        raise ValueError(f"{who}: give exactly one of field and shade")
    if isinstance(chunk, bool) or not isinstance(chunk, int) or chunk < 1:
        raise ValueError(f"{who}: chunk must be a positive integer, got {chunk!r}")
    v, f = _check_mesh(mesh, who)
    if field is not None and _field_device(field) != v.device:
        raise ValueError(f"{who}: the field is on {_field_device(field)}, the mesh on {v.device}")
    F = f.shape[0]
    W, S, Q = atlas_layout(F, P)
    dev = v.device
    with torch.cuda.device(dev):
        image = torch.zeros(W, W, 3, dtype=torch.uint8, device=dev)
        normal_image = torch.zeros(W, W, 3, dtype=torch.uint8, device=dev) if normal_map else None
        uvs = face_uvs(F, P, device=dev)
        if F == 0:
            return TextureAtlas(image, normal_image, uvs, P)
        if field is not None:
            refresh_field(field)
        n_sq = (F + 1) // 2
        step = max(1, chunk // (Q * Q))
        for s0 in range(0, n_sq, step):
            owner, offset, points = _points(v, f, P, S, Q, s0, min(s0 + step, n_sq))
            if field is not None:
                _, grad, rgb = field.field_values(points, want_albedo=True)
            else:
                rgb, grad = shade(points)
            rgb, grad = (_shaded(t, points, name, who) for t, name in ((rgb, "rgb"), (grad, "gradient")))
            hip.texture_texel_store(rgb, grad, owner, offset, image, normal_image)
    return TextureAtlas(image, normal_image, uvs, P)


def _shaded(t, points, name: str, who: str) -> torch.Tensor:
    if not torch.is_tensor(t) or t.device != points.device or t.dtype != torch.float32 or t.numel() != points.numel():
        got = f"{t.dtype} {tuple(t.shape)} on {t.device}" if torch.is_tensor(t) else repr(type(t))
        raise ValueError(f"{who}: {name} must be fp32 {tuple(points.shape)} on {points.device}, got {got}")
    return t.detach().reshape(-1, 3).contiguous()


def _fmt(fmt: str, column) -> np.ndarray:
    return np.char.mod(fmt, column)


def _join(columns, sep: str) -> np.ndarray:
    out = columns[0]
    for c in columns[1:]:
        out = np.char.add(np.char.add(out, sep), c)
    return out


def _lines(head: str, columns) -> str:
    """one line per row, `head` and the row's strings separated by blanks; numpy formats whole columns (no Python loop over rows)"""
    if len(columns[0]) == 0:
        return ""
    return "\n".join(np.char.add(head + " ", _join(columns, " ")).tolist()) + "\n"


def _png(path: str, image: torch.Tensor) -> None:
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(image.detach().cpu().numpy())).save(path, format="PNG")


def write_obj(path, mesh: Mesh, atlas: Optional[TextureAtlas] = None) -> None:
    """<stem>.obj, and with an atlas <stem>.mtl (material_0, map_Kd <stem>.png), <stem>.png and, when the atlas has a normal image,
    <stem>_normal.png.  v lines carry nine significant digits (fp32 round-trips), vn lines when the mesh has normals; with an atlas
    3 F vt lines in face order and faces as a/t/n or a/t (1-based); without one a plain OBJ (a//n or a)."""
    path = os.fspath(path)
    stem = os.path.splitext(path)[0]
    base = os.path.basename(stem)
    v = mesh.vertices.detach().cpu().numpy().astype(np.float32, copy=False).reshape(-1, 3)
    f = mesh.faces.detach().cpu().numpy().astype(np.int64).reshape(-1, 3) + 1
    F = f.shape[0]
    has_n = mesh.normals is not None
    textured = atlas is not None and F > 0 and atlas.image.numel() > 0
    if atlas is not None and tuple(atlas.uvs.shape) != (F, 3, 2):
        raise ValueError(f"write_obj: the atlas holds uvs shaped {tuple(atlas.uvs.shape)}, the mesh has {F} faces")
    chunks = [f"# {v.shape[0]} vertices, {F} faces\n"]
    if textured:
        chunks.append(f"mtllib {base}.mtl\n")
    chunks.append(_lines("v", [_fmt("%.9g", v[:, a]) for a in range(3)]))
    if has_n:
        n = mesh.normals.detach().cpu().numpy().astype(np.float32, copy=False).reshape(-1, 3)
        chunks.append(_lines("vn", [_fmt("%.9g", n[:, a]) for a in range(3)]))
    index = [_fmt("%d", f[:, k]) for k in range(3)]
    if textured:
        uv = atlas.uvs.detach().cpu().numpy().astype(np.float32, copy=False).reshape(-1, 2)
        chunks.append(_lines("vt", [_fmt("%.9g", uv[:, a]) for a in range(2)]))
        chunks.append("usemtl material_0\n")
        t = np.arange(1, 3 * F + 1, dtype=np.int64).reshape(F, 3)
        corners = [_join([index[k], _fmt("%d", t[:, k])] + ([index[k]] if has_n else []), "/") for k in range(3)]
    elif has_n:
        corners = [_join([index[k], index[k]], "//") for k in range(3)]
    else:
        corners = index
    chunks.append(_lines("f", corners))
    with open(path, "w", encoding="ascii", newline="\n") as fh:
        fh.write("".join(chunks))
    if not textured:
        return
    _png(stem + ".png", atlas.image)
    mtl = ["newmtl material_0", "Ka 1.000 1.000 1.000", "Kd 1.000 1.000 1.000", "Ks 0.000 0.000 0.000", "d 1.0", "illum 1",
           f"map_Kd {base}.png"]
    if atlas.normal_image is not None:
        _png(stem + "_normal.png", atlas.normal_image)
        mtl.append(f"# object-space normal map (n * 0.5 + 0.5 of the unit SDF gradient): {base}_normal.png")
    with open(stem + ".mtl", "w", encoding="ascii", newline="\n") as fh:
        fh.write("\n".join(mtl) + "\n")
