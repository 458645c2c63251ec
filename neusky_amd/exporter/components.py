"""Connected components of a mesh and the removal of floaters (include/neusky_hip.h, nsky_cc_*; csrc/components.hip).

Two faces are connected when they share a vertex index; a component is a class of the transitive closure.  This is VERTEX
connectivity: trimesh and Open3D split by edge adjacency, and on a marching-cubes mesh (one vertex per crossing grid edge, shared by
index) the two differ only at pinch points, where two bodies meet in a single vertex and count as one component here.  A component's
root is its smallest vertex index, its size its face count; components are ranked by size descending, ties by root ascending, so
labels depend on nothing but the mesh: not on the order of the faces, not on scheduling.  A vertex no face references has label -1.

The union-find pass, the flatten pass, the selection and the compaction are kernels; the ranking between them is torch calls on keys
and counters (unique with counts, one sort, a scatter and two gathers), and the two scans are torch cumsums.  Meant to run before
simplify_mesh, on the marching-cubes mesh, where triangles are near-uniform and face count stands for area."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional

import torch

from .. import hip
from .mesh import Mesh
from .simplify import _box, _check_mesh


@dataclass
class MeshComponents:
    labels: torch.Tensor       # [V] int32: the rank of every vertex's component, -1 for a vertex no face references
    face_labels: torch.Tensor  # [F] int32: the rank of every face's component
    roots: torch.Tensor        # [C] int32: the smallest vertex index of each component, by rank
    face_counts: torch.Tensor  # [C] int64: the face count of each component, descending
    num_components: int


def _status_error(status: int, who: str) -> None:
    if status:
        what = [name for bit, name in ((hip.CC_STATUS_INDEX, "a face index outside the vertices"),
                                       (hip.CC_STATUS_LINK, "the link pass reached its iteration cap"),
                                       (hip.CC_STATUS_FLATTEN, "the flatten pass reached its iteration cap")) if status & bit]
        raise RuntimeError(f"{who}: the component kernels reported status {status} ({'; '.join(what)})")


def _label(v: torch.Tensor, f: torch.Tensor):
    """link, flatten and the ranking on checked inputs (V, F > 0): (MeshComponents, status [1] int32, still on the device)"""
    dev, V, F = v.device, v.shape[0], f.shape[0]
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    parent = torch.arange(V, dtype=torch.int32, device=dev)
    hip.cc_link(f, parent, status)
    vertex_root = torch.empty(V, dtype=torch.int32, device=dev)
    face_root = torch.empty(F, dtype=torch.int32, device=dev)
    hip.cc_flatten(parent, f, vertex_root, face_root, status)
    del parent
    roots, counts = torch.unique(face_root, return_counts=True)  # (C reaches the host here: a host read)
    order = torch.argsort((F - counts) * (1 << 31) + roots)  # the keys differ in their roots: any sort gives this order
    roots, counts = roots[order], counts[order]
    C = roots.shape[0]
    rank = torch.full((V,), -1, dtype=torch.int32, device=dev)
    rank[roots.long()] = torch.arange(C, dtype=torch.int32, device=dev)
    labels = rank.index_select(0, vertex_root)
    face_labels = rank.index_select(0, face_root)
    return MeshComponents(labels, face_labels, roots, counts, C), status


def _empty_components(V: int, dev) -> MeshComponents:
    return MeshComponents(torch.full((V,), -1, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int32, device=dev),
                          torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int64, device=dev), 0)


def label_components(mesh: Mesh) -> MeshComponents:
    """The connected components of the mesh (vertex connectivity, see the module's docstring), ranked by face count descending and
    root ascending: labels [V] int32 (-1 for a vertex no face references), face_labels [F] int32, roots [C] int32, face_counts [C]
    int64 and num_components.  Two launches and a handful of torch calls; bitwise repeatable, and the same for any order of the
    faces.  Raises RuntimeError when a kernel reports that it gave up (a defect: no input can cause it)."""
    who = "label_components"
    v, f = _check_mesh(mesh, who)
    if v.shape[0] == 0 or f.shape[0] == 0:
        if f.shape[0]:
            raise ValueError(f"{who}: {f.shape[0]} faces, the mesh has no vertices")
        return _empty_components(v.shape[0], v.device)
    with torch.cuda.device(v.device):
        _box(v, f, who)
        comps, status = _label(v, f)
        _status_error(int(status.item()), who)
    return comps


def _criterion(value, name: str, who: str) -> None:
    if value is not None and (isinstance(value, bool) or not isinstance(value, int) or value < 1):
        raise ValueError(f"{who}: {name} must be a positive integer, got {value!r}")


def remove_floaters(mesh: Mesh, *, keep_largest: Optional[int] = None, min_faces: Optional[int] = None,
                    info: Optional[Dict] = None) -> Mesh:
    """The mesh without its small connected components (label_components' components and ranks).

    At least one of
      keep_largest  K: the K largest components stay (ranks < K);
      min_faces     N: components with at least N faces stay;
    with both, a component has to meet both.  When every face stays the result is `mesh` itself.  Otherwise a new Mesh: the staying
    faces in input order with their orientation, the vertices they reference in input order (so vertices no face references go
    too), positions, normals and colours copied bit for bit.  An empty mesh, or one without faces, gives an empty mesh.
    info (optional dict) receives components, kept_components, faces_before, faces_after and largest (the face count of rank 0).
    Three host reads: the index and box check, the component sizes, and the output counts with the kernels' status word."""
    who = "remove_floaters"
    if keep_largest is None and min_faces is None:
        raise ValueError(f"{who}: give at least one of keep_largest and min_faces")
    _criterion(keep_largest, "keep_largest", who)
    _criterion(min_faces, "min_faces", who)
    v, f = _check_mesh(mesh, who)
    V, F = v.shape[0], f.shape[0]
    dev = v.device
    if V == 0 or F == 0:
        if F:
            raise ValueError(f"{who}: {F} faces, the mesh has no vertices")
        if info is not None:
            info.update(components=0, kept_components=0, faces_before=0, faces_after=0, largest=0)
        return Mesh(v[:0], f, None if mesh.normals is None else mesh.normals[:0], None if mesh.colours is None else mesh.colours[:0])
    with torch.cuda.device(dev):
        _box(v, f, who)
        comps, status = _label(v, f)
        C = comps.num_components
        keep_component = torch.ones(C, dtype=torch.bool, device=dev)
        if keep_largest is not None:
            keep_component &= torch.arange(C, device=dev) < keep_largest
        if min_faces is not None:
            keep_component &= comps.face_counts >= min_faces
        keep_component = keep_component.to(torch.uint8)
        keep = torch.empty(F, dtype=torch.uint8, device=dev)
        vertex_used = torch.zeros(V, dtype=torch.uint8, device=dev)
        hip.cc_select(f, comps.face_labels, keep_component, keep, vertex_used)
        face_ends = keep.cumsum(0, dtype=torch.int64)
        vertex_ends = vertex_used.cumsum(0, dtype=torch.int64)
        F_out, V_out, kept, largest, st = torch.stack([face_ends[-1], vertex_ends[-1], keep_component.sum(dtype=torch.int64),
                                                       comps.face_counts[0], status[0].long()]).tolist()
        _status_error(st, who)
        if info is not None:
            info.update(components=C, kept_components=kept, faces_before=F, faces_after=F_out, largest=largest)
        if F_out == F:
            return mesh
        normals = mesh.normals.contiguous() if mesh.normals is not None else None
        colours = mesh.colours.contiguous() if mesh.colours is not None else None
        out_v = torch.empty(V_out, 3, dtype=torch.float32, device=dev)
        out_n = torch.empty(V_out, 3, dtype=torch.float32, device=dev) if normals is not None else None
        out_c = torch.empty(V_out, 3, dtype=torch.uint8, device=dev) if colours is not None else None
        out_f = torch.empty(F_out, 3, dtype=torch.int32, device=dev)
        hip.cc_compact(v, normals, colours, f, keep, face_ends, vertex_used, vertex_ends, out_v, out_n, out_c, out_f)
    return Mesh(out_v, out_f, out_n, out_c)
