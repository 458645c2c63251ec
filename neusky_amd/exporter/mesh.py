"""The field side of the mesh export: a dense SDF grid through the fused value chain, vertex attributes, checkpoint loading."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch
import torch.nn.functional as F

from .. import ops
from ..utils.checkpoints import _put
from ..utils.utils import linear_to_sRGB
from .marching_cubes import marching_cubes

CHUNK = 1 << 20  # grid points per field call: the sdf chain allocates two [rows, 256] fp32 scratch buffers per call


@dataclass
class Mesh:
    vertices: torch.Tensor                  # [V, 3] fp32
    faces: torch.Tensor                     # [F, 3] int32, counter-clockwise seen from the outside (sdf > level)
    normals: Optional[torch.Tensor] = None  # [V, 3] fp32, the normalised sdf gradient
    colours: Optional[torch.Tensor] = None  # [V, 3] uint8, the albedo in sRGB


def _triple(v, name):
    t = (v, v, v) if isinstance(v, (int, float)) else tuple(v)
    if len(t) != 3:
        raise ValueError(f"{name}: expected one value or three, got {v!r}")
    return t


def _field_device(field) -> torch.device:
    return field.encoding.params.device


def refresh_field(field) -> None:
    """drop the prepared (weight-normed / padded / packed) copies of the field's weights, as the checkpoint loader does: a field
    whose parameters changed since its last pass is never evaluated with stale ones"""
    field.invalidate_weight_cache()
    dev = _field_device(field)
    if dev.type == "cuda":
        ops.begin_step(dev)


def grid_axes(resolution, bounding_box_min, bounding_box_max, device) -> List[torch.Tensor]:
    """per-axis coordinates of the grid points: min + i / (N - 1) * (max - min), rounded once from float64"""
    res = _triple(resolution, "resolution")
    lo, hi = _triple(bounding_box_min, "bounding_box_min"), _triple(bounding_box_max, "bounding_box_max")
    if min(res) < 2:
        raise ValueError(f"resolution {res}: every dimension must be >= 2")
    return [torch.linspace(float(lo[a]), float(hi[a]), int(res[a]), dtype=torch.float64).to(torch.float32).to(device) for a in range(3)]


@torch.no_grad()
def sdf_grid(field, resolution: Union[int, Sequence[int]], bounding_box_min=(-1.0, -1.0, -1.0), bounding_box_max=(1.0, 1.0, 1.0),
             chunk: int = CHUNK) -> torch.Tensor:
    """the field's SDF on the dense grid [Nx, Ny, Nz] (z fastest) spanning the box, fp32, on the field's device"""
    dev = _field_device(field)
    if dev.type != "cuda":
        raise ValueError("sdf_grid: the field must be on a CUDA device")
    ax, ay, az = grid_axes(resolution, bounding_box_min, bounding_box_max, dev)
    nx, ny, nz = ax.numel(), ay.numel(), az.numel()
    refresh_field(field)
    out = torch.empty(nx, ny, nz, dtype=torch.float32, device=dev)
    flat = out.view(-1)
    for s in range(0, flat.numel(), chunk):
        idx = torch.arange(s, min(s + chunk, flat.numel()), dtype=torch.int64, device=dev)
        k = idx % nz
        ij = idx // nz
        pts = torch.stack([ax[ij // ny], ay[ij % ny], az[k]], -1)
        flat[s:s + idx.numel()] = field.get_sdf_at_pos(pts)[:, 0]
    return out


@torch.no_grad()
def vertex_attributes(field, vertices: torch.Tensor, chunk: int = CHUNK) -> Tuple[torch.Tensor, torch.Tensor]:
    """(normals [V, 3] fp32, colours [V, 3] uint8): the normalised SDF gradient and the sRGB-encoded albedo at the vertices"""
    normals = torch.empty_like(vertices)
    colours = torch.empty(vertices.shape[0], 3, dtype=torch.uint8, device=vertices.device)
    for s in range(0, vertices.shape[0], chunk):
        x = vertices[s:s + chunk].contiguous()
        _, grad, albedo = field.field_values(x, want_albedo=True)
        normals[s:s + x.shape[0]] = F.normalize(grad.reshape(-1, 3), dim=-1)
        colours[s:s + x.shape[0]] = (linear_to_sRGB(albedo.reshape(-1, 3)) * 255.0).round().clamp(0, 255).to(torch.uint8)
    return normals, colours


def extract_mesh(field, resolution: Union[int, Sequence[int]] = 512, bounding_box_min=(-1.0, -1.0, -1.0),
                 bounding_box_max=(1.0, 1.0, 1.0), isosurface_threshold: float = 0.0, attributes: bool = True,
                 timings: Optional[Dict[str, float]] = None) -> Mesh:
    """marching_cubes(sdf_grid(...)) plus, with `attributes`, per-vertex normals and colours.  `timings` (optional dict) receives
    the seconds of the three parts: sdf_grid, marching_cubes, attributes."""
    import time

    def lap(name, t0):
        if timings is not None:
            torch.cuda.synchronize()
            timings[name] = time.perf_counter() - t0
        return time.perf_counter()

    t = lap("start", time.perf_counter())
    vol = sdf_grid(field, resolution, bounding_box_min, bounding_box_max)
    t = lap("sdf_grid", t)
    vertices, faces = marching_cubes(vol, isosurface_threshold, bounding_box_min, bounding_box_max)
    del vol
    t = lap("marching_cubes", t)
    mesh = Mesh(vertices, faces)
    if attributes:
        mesh.normals, mesh.colours = vertex_attributes(field, vertices)
        lap("attributes", t)
    if timings is not None:
        timings.pop("start", None)
    return mesh


def _field_targets(field) -> Dict[str, torch.Tensor]:
    """checkpoint key (after `_model.field.`) -> parameter, in the names utils/checkpoints.py:load_reference_pipeline_state accepts"""
    t: Dict[str, torch.Tensor] = dict(field.named_parameters())
    t.update(dict(field.named_buffers()))
    t["encoding.params"] = field.encoding.params
    t["deviation_network.variance"] = field.deviation_network.variance
    t["aabb"] = field.aabb
    t["embedding_appearance.embedding.weight"] = field.embedding_appearance.weight  # (nerfstudio's Embedding wrapper)
    for kind in ("glin", "clin"):
        l = 0
        while hasattr(field, f"{kind}{l}"):
            lin = getattr(field, f"{kind}{l}")
            t[f"{kind}{l}.weight_g"] = t[f"{kind}{l}.parametrizations.weight.original0"] = lin.weight_g
            t[f"{kind}{l}.weight_v"] = t[f"{kind}{l}.parametrizations.weight.original1"] = lin.weight_v
            t[f"{kind}{l}.bias"] = lin.bias
            l += 1
    return t


def load_field_state(field, state: Dict[str, torch.Tensor]) -> Tuple[List[str], List[str]]:
    """copy the `_model.field.*` entries of a checkpoint (`{"pipeline": state_dict}`, or the state dict itself) onto a bare
    SDFAlbedoField.  Returns (loaded keys, unmapped `_model.field.*` keys); a shape mismatch raises ValueError."""
    if "pipeline" in state and isinstance(state["pipeline"], dict):
        state = state["pipeline"]
    targets = _field_targets(field)
    loaded, unmapped = [], []
    for k, v in state.items():
        if not k.startswith("_model.field."):
            continue
        name = k[len("_model.field."):]
        if name in targets:
            _put(targets[name], v, k)
            loaded.append(k)
        else:
            unmapped.append(k)
    field.invalidate_weight_cache()
    return loaded, unmapped
