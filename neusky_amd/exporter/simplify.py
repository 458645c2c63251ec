"""Mesh simplification by vertex clustering with quadric-error placement (include/neusky_hip.h, nsky_mesh_*; csrc/simplify.hip).

A uniform grid of cubic cells over the mesh; the vertices of a cell collapse into one, placed where the summed plane quadrics of the
cell's faces are smallest; faces that lose a corner disappear.  One pass, on the device, bitwise repeatable.  The sorts, scans and
the run-length pass between the kernels are torch calls on keys and counters; everything that reads or writes a vertex or a face
is a kernel.  (The box of the vertices and the index range are checked with torch reductions before anything is launched.)

Clustering is not manifold-preserving: where two sheets of the surface pass through one cell they are welded, and the result can
have edges with more than two faces."""
from __future__ import annotations

import math
from typing import Callable, Dict, Optional, Sequence, Tuple

import torch

from .. import hip
from .mesh import Mesh, vertex_attributes

MIN_CELLS, MAX_CELLS = 2, 2048  # the search range of target_num_faces: cells along the longest box axis
KEY_CELLS = 1 << hip.MESH_KEY_BITS


def bisect_cells(count: Callable[[int], int], target: int, n_min: int = MIN_CELLS, n_max: int = MAX_CELLS) -> Tuple[int, int, int]:
    """The largest-resolution grid the bisection can vouch for: (n, count(n), calls) with count(n) <= target < count(n + 1), found
    with the invariant count(n_lo) <= target < count(n_hi) (no monotonicity assumed, none needed for that statement).  n_max when
    count(n_max) <= target; n_min - 1 (reported with count 0: one cell, no face) when count(n_min) > target."""
    c_max = count(n_max)
    if c_max <= target:
        return n_max, c_max, 1
    c_lo = count(n_min)
    if c_lo > target:
        return n_min - 1, 0, 2
    n_lo, n_hi, calls = n_min, n_max, 2
    while n_hi - n_lo > 1:
        mid = (n_lo + n_hi) // 2
        c = count(mid)
        calls += 1
        if c <= target:
            n_lo, c_lo = mid, c
        else:
            n_hi = mid
    return n_lo, c_lo, calls


def _check_mesh(mesh, who: str) -> Tuple[torch.Tensor, torch.Tensor]:
    v, f = mesh.vertices, mesh.faces
    if not torch.is_tensor(v) or not torch.is_tensor(f) or not v.is_cuda or not f.is_cuda:
        raise ValueError(f"{who}: vertices and faces must be CUDA tensors (the kernels run on the device only)")
    if v.dim() != 2 or v.shape[1] != 3 or v.dtype != torch.float32:
        raise ValueError(f"{who}: vertices must be fp32 [V, 3], got {v.dtype} {tuple(v.shape)}")
    if f.dim() != 2 or f.shape[1] != 3 or f.dtype != torch.int32:
        raise ValueError(f"{who}: faces must be int32 [F, 3], got {f.dtype} {tuple(f.shape)}")
    for name, t, dt in (("normals", mesh.normals, torch.float32), ("colours", mesh.colours, torch.uint8)):
        if t is not None and (not t.is_cuda or t.dtype != dt or tuple(t.shape) != tuple(v.shape)):
            raise ValueError(f"{who}: {name} must be a CUDA {dt} tensor shaped {tuple(v.shape)}")
    return v.detach().contiguous(), f.contiguous()


def _box(v: torch.Tensor, f: torch.Tensor, who: str) -> Tuple[Tuple[float, ...], Tuple[float, ...]]:
    """component-wise minimum and maximum of the vertices (float64 values of the fp32 numbers); checks finiteness and the index range"""
    lo, hi = torch.aminmax(v, dim=0)
    parts = [lo.double(), hi.double()]
    if f.numel():
        parts += [t.double().reshape(1) for t in torch.aminmax(f)]
    stats = torch.cat(parts).tolist()
    if not all(math.isfinite(x) for x in stats[:6]):
        raise ValueError(f"{who}: the vertices hold non-finite coordinates")
    if f.numel() and (stats[6] < 0 or stats[7] >= v.shape[0]):
        raise ValueError(f"{who}: face indices span [{int(stats[6])}, {int(stats[7])}], the mesh has {v.shape[0]} vertices")
    return tuple(stats[:3]), tuple(stats[3:6])


def _grid(lo_box, hi_box, cell_size: float, origin, who: str) -> Tuple[Tuple[float, float, float], float]:
    h = float(cell_size)
    if not (math.isfinite(h) and h > 0.0):
        raise ValueError(f"{who}: cell_size must be a positive finite number, got {cell_size!r}")
    lo = tuple(float(x) for x in (lo_box if origin is None else origin))
    if len(lo) != 3 or not all(math.isfinite(x) for x in lo):
        raise ValueError(f"{who}: origin must be three finite numbers, got {origin!r}")
    if max((hi_box[a] - lo[a]) / h for a in range(3)) >= KEY_CELLS:
        raise ValueError(f"{who}: cell_size {h} puts more than 2^{hip.MESH_KEY_BITS} cells along an axis of the mesh")
    return lo, h


def _count(v, f, lo, h) -> int:
    out = torch.zeros(1, dtype=torch.int64, device=v.device)
    hip.mesh_cluster_count(v, f, lo, h, out)
    return int(out.item())


def cluster_face_count(mesh: Mesh, cell_size: float, origin: Optional[Sequence[float]] = None) -> int:
    """the number of faces whose three corners fall into three different cells of the grid (origin, cell_size): what
    simplify_mesh(cell_size=...) keeps before it removes repeated faces.  One kernel, no sort.  origin: the grid's corner (default:
    the component-wise minimum of the vertices)."""
    v, f = _check_mesh(mesh, "cluster_face_count")
    if v.shape[0] == 0 or f.shape[0] == 0:
        return 0
    with torch.cuda.device(v.device):
        lo, h = _grid(*_box(v, f, "cluster_face_count"), cell_size, origin, "cluster_face_count")
        return _count(v, f, lo, h)


def cluster_pass(v, f, normals, colours, lo, h, group: int = 0, want_sums: bool = False):
    """one full pass on checked inputs: (vertices [C, 3], faces [F', 3], normals or None, colours or None[, cell sums [C, 20] fp64])"""
    dev, V, F = v.device, v.shape[0], f.shape[0]
    keys = torch.empty(V, dtype=torch.int64, device=dev)
    hip.mesh_cell_keys(v, lo, h, keys)
    sorted_keys, v_order = torch.sort(keys, stable=True)
    del keys
    cell_keys, rank_sorted, counts = torch.unique_consecutive(sorted_keys, return_inverse=True, return_counts=True)
    del sorted_keys
    C = cell_keys.shape[0]
    cell_start = torch.zeros(C + 1, dtype=torch.int64, device=dev)
    cell_start[1:] = counts.cumsum(0)
    vertex_cell = torch.empty(V, dtype=torch.int32, device=dev)
    hip.mesh_vertex_cells(v_order, rank_sorted, vertex_cell)
    del rank_sorted, counts
    corner_cells = torch.empty(F, 3, dtype=torch.int32, device=dev)
    face_keys = torch.empty(F, dtype=torch.int64, device=dev)
    hip.mesh_remap_faces(f, vertex_cell, corner_cells, face_keys)
    del vertex_cell
    sorted_corners, corner_order = torch.sort(corner_cells.view(-1), stable=True)
    sums = torch.empty(C, hip.MESH_CELL_SUMS, dtype=torch.float64, device=dev)
    hip.mesh_cluster_reduce(v, f, normals, colours, lo, h, v_order, cell_start, sorted_corners, corner_order, sums, group)
    del sorted_corners, corner_order, v_order, cell_start
    out_v = torch.empty(C, 3, dtype=torch.float32, device=dev)
    out_n = torch.empty(C, 3, dtype=torch.float32, device=dev) if normals is not None else None
    out_c = torch.empty(C, 3, dtype=torch.uint8, device=dev) if colours is not None else None
    hip.mesh_cluster_solve(sums, cell_keys, lo, h, out_v, out_n, out_c)
    if F:
        sorted_face_keys, face_order = torch.sort(face_keys, stable=True)
        keep = torch.empty(F, dtype=torch.int32, device=dev)
        hip.mesh_flag_duplicates(corner_cells, sorted_face_keys, face_order, keep)
        del sorted_face_keys, face_order
        ends = keep.cumsum(0, dtype=torch.int64)
        out_f = torch.empty(int(ends[-1].item()), 3, dtype=torch.int32, device=dev)
        hip.mesh_compact_faces(corner_cells, keep, ends, out_f)
    else:
        out_f = torch.empty(0, 3, dtype=torch.int32, device=dev)
    return (out_v, out_f, out_n, out_c, sums) if want_sums else (out_v, out_f, out_n, out_c)


def simplify_mesh(mesh: Mesh, *, cell_size: Optional[float] = None, target_num_faces: Optional[int] = None,
                  origin: Optional[Sequence[float]] = None, field=None, info: Optional[Dict] = None) -> Mesh:
    """The mesh clustered on a grid of cubic cells: one vertex per occupied cell (ascending cell key), placed at the minimum of the
    cell's summed face quadrics (at the mean of its vertices where that is not determined or leaves the cell); faces re-indexed,
    those with two corners in one cell dropped, repeated ones dropped; input order and orientation kept.

    Exactly one of
      cell_size         the cell edge h;
      target_num_faces  a face budget: h = (longest box axis) / n with the n in [2, 2048] found by bisection on cluster_face_count
                        (at most 13 counts, then one full pass); the result has at most that many faces.  A budget at or above the
                        mesh's face count returns `mesh` itself.
    origin: the grid's corner (default: the component-wise minimum of the vertices).  field: when given, normals and colours are
    evaluated from it at the new vertices (vertex_attributes); otherwise a cell takes the normalised sum of its vertices' normals
    and the rounded mean of their colours, where the mesh has them.  info (optional dict) receives cells (n, None with cell_size),
    cell_size, origin, counted_faces (faces before repeated ones are removed) and count_calls."""
    who = "simplify_mesh"
    if (cell_size is None) == (target_num_faces is None):
        raise ValueError(f"{who}: give exactly one of cell_size and target_num_faces")
    if target_num_faces is not None:
        if isinstance(target_num_faces, bool) or not isinstance(target_num_faces, int) or target_num_faces < 0:
            raise ValueError(f"{who}: target_num_faces must be a non-negative integer, got {target_num_faces!r}")
    elif not (isinstance(cell_size, (int, float)) and math.isfinite(cell_size) and cell_size > 0):
        raise ValueError(f"{who}: cell_size must be a positive finite number, got {cell_size!r}")
    if origin is not None and (len(tuple(origin)) != 3 or not all(math.isfinite(float(x)) for x in origin)):
        raise ValueError(f"{who}: origin must be three finite numbers, got {origin!r}")
    v, f = _check_mesh(mesh, who)
    V, F = v.shape[0], f.shape[0]
    if target_num_faces is not None and target_num_faces >= F:
        if info is not None:
            info.update(cells=None, cell_size=None, origin=None, counted_faces=F, count_calls=0)
        return mesh
    if V == 0:
        if info is not None:
            info.update(cells=None, cell_size=cell_size, origin=None, counted_faces=0, count_calls=0)
        return Mesh(v, f, mesh.normals, mesh.colours)
    with torch.cuda.device(v.device):
        lo_box, hi_box = _box(v, f, who)
        cells, counted, calls = None, None, 0
        if target_num_faces is not None:
            lo = lo_box if origin is None else tuple(float(x) for x in origin)
            extent = max(hi_box[a] - lo[a] for a in range(3))  # the longest axis of the box the grid has to cover
            if not extent > 0.0:
                extent = 1.0  # every vertex at one point: any grid holds them in one cell
            cells, counted, calls = bisect_cells(lambda n: _count(v, f, lo, extent / n), target_num_faces)
            cell_size = extent / cells if cells >= MIN_CELLS else 2.0 * extent  # below the range: one cell around the whole mesh
        lo, h = _grid(lo_box, hi_box, cell_size, origin, who)
        use_own = field is None
        out_v, out_f, out_n, out_c = cluster_pass(v, f, mesh.normals.contiguous() if use_own and mesh.normals is not None else None,
                                                  mesh.colours.contiguous() if use_own and mesh.colours is not None else None, lo, h)
        if counted is None and info is not None:
            counted, calls = _count(v, f, lo, h), 1
        if info is not None:
            info.update(cells=cells, cell_size=h, origin=lo, counted_faces=counted, count_calls=calls)
        if field is not None:
            out_n, out_c = vertex_attributes(field, out_v)
    return Mesh(out_v, out_f, out_n, out_c)
