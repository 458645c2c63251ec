"""Host side of the marching-cubes kernels (include/neusky_hip.h, nsky_mc_*): count, scan the tile totals, allocate, write."""
from __future__ import annotations

import math
from typing import Sequence, Tuple

import torch

from .. import hip

INT32_MAX = 2**31 - 1


def marching_cubes(volume: torch.Tensor, level: float = 0.0, bounding_box_min: Sequence[float] = (-1.0, -1.0, -1.0),
                   bounding_box_max: Sequence[float] = (1.0, 1.0, 1.0)) -> Tuple[torch.Tensor, torch.Tensor]:
    """Iso-surface `value == level` of a dense volume [Nx, Ny, Nz] (z fastest, torch.meshgrid(..., indexing="ij") order).

    Grid point (i, j, k) sits at min + (i, j, k) / (N - 1) * (max - min).  A corner is inside when value < level.  Returns
    (vertices [V, 3] fp32, faces [F, 3] int32) on the volume's device: one vertex per crossing grid edge, ordered by the
    owning point's flat index then axis; faces by cell then case-table order, counter-clockwise seen from the outside
    (increasing value) side; a crack-free case table, so the mesh is closed wherever the surface stays inside the box.
    Extra device memory: 5 bytes per grid point (plus 32 bytes per 256 points)."""
    if not torch.is_tensor(volume) or not volume.is_cuda:
        raise ValueError("marching_cubes: the volume must be a CUDA tensor (the kernels run on the device only)")
    if volume.dim() != 3 or min(volume.shape) < 2:
        raise ValueError(f"marching_cubes: volume must be [Nx, Ny, Nz] with every dimension >= 2, got {tuple(volume.shape)}")
    if len(bounding_box_min) != 3 or len(bounding_box_max) != 3:
        raise ValueError("marching_cubes: the bounding box corners must have 3 coordinates each")
    level = float(level)
    if not math.isfinite(level):
        raise ValueError(f"marching_cubes: level {level} is not finite")
    vol = volume.detach()
    if vol.dtype != torch.float32:
        vol = vol.float()
    vol = vol.contiguous()
    dev = vol.device
    with torch.cuda.device(dev):
        n_tiles = (vol.numel() + hip.MC_TILE - 1) // hip.MC_TILE
        counts = torch.empty(4, n_tiles, dtype=torch.int32, device=dev)
        hip.mc_count(vol, level, counts)
        # per-row scans of the tile totals (rows, not columns: a scan along the inner dimension runs in parallel)
        ends = counts[:2].to(torch.int64).cumsum(1)
        V, F, bad = torch.stack([ends[0, -1], ends[1, -1], counts[2].to(torch.int64).sum()]).tolist()
        if bad:
            raise ValueError(f"marching_cubes: the volume holds {bad} non-finite values")
        if V > INT32_MAX or F > INT32_MAX:
            raise ValueError(f"marching_cubes: {V} vertices / {F} faces do not fit int32 indices")
        vertices = torch.empty(V, 3, dtype=torch.float32, device=dev)
        faces = torch.empty(F, 3, dtype=torch.int32, device=dev)
        if V == 0:
            return vertices, faces
        starts = ends - counts[:2]  # exclusive scans of the tile totals
        del ends, counts
        v_off, f_off = starts[0], starts[1]
        base = torch.empty(vol.numel(), dtype=torch.int32, device=dev)
        edge_mask = torch.empty(vol.numel(), dtype=torch.uint8, device=dev)
        hip.mc_vertices(vol, level, bounding_box_min, bounding_box_max, v_off, base, edge_mask, vertices)
        if F:
            hip.mc_faces(vol, level, f_off, base, edge_mask, faces)
        del base, edge_mask
    return vertices, faces
