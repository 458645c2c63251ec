"""Mesh export timing on bench.py's randomised field: at each resolution, the three parts of extract_mesh timed separately with
HIP events after a warm-up -- the SDF grid (fused hash encode + SDF value chain over every grid point), the marching-cubes passes
(count, tile scan, vertices, faces; at the level of the median grid value, so that the surface crosses the box), the vertex
attributes (field_values at the vertices) -- and the peak device memory that marching_cubes allocates beyond its input volume
and its output mesh.  Then the simplification of that mesh (exporter/simplify.py), next to the marching-cubes pass it follows: for a
10x and a 100x face reduction, the grid found by the face-budget search, the median and range of the full clustering pass at that
grid over --simplify-reps repetitions, of one cluster_face_count call, and of the reduce kernel alone with 8 and with 64 lanes
per cell.  Prints one JSON line per resolution; run on the GPU box:
    python tools/bench_mesh.py [--resolutions 256 512 1024] [--iters 3] [--simplify-reps 7]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from neusky_amd import hip  # noqa: E402
from neusky_amd.exporter import Mesh, cluster_face_count, marching_cubes, sdf_grid, simplify_mesh  # noqa: E402
from neusky_amd.exporter.mesh import vertex_attributes  # noqa: E402
from neusky_amd.utils.randomise import randomise  # noqa: E402


def timed(fn, iters):
    fn()  # warm-up
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters, out


def spread(fn, reps):
    """[median, min, max] milliseconds of single calls after one warm-up call"""
    fn()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return [round(ms[len(ms) // 2], 3), round(ms[0], 3), round(ms[-1], 3)]


def reduce_only(mesh, lo, h, group):
    """the inputs of nsky_mesh_cluster_reduce prepared once -> a closure that runs the reduce kernel alone"""
    v, f = mesh.vertices, mesh.faces
    keys = torch.empty(v.shape[0], dtype=torch.int64, device=v.device)
    hip.mesh_cell_keys(v, lo, h, keys)
    sorted_keys, v_order = torch.sort(keys, stable=True)
    cell_keys, rank_sorted, counts = torch.unique_consecutive(sorted_keys, return_inverse=True, return_counts=True)
    cell_start = torch.zeros(cell_keys.shape[0] + 1, dtype=torch.int64, device=v.device)
    cell_start[1:] = counts.cumsum(0)
    vertex_cell = torch.empty(v.shape[0], dtype=torch.int32, device=v.device)
    hip.mesh_vertex_cells(v_order, rank_sorted, vertex_cell)
    corner_cells = torch.empty_like(f)
    hip.mesh_remap_faces(f, vertex_cell, corner_cells, torch.empty(f.shape[0], dtype=torch.int64, device=v.device))
    sorted_corners, corner_order = torch.sort(corner_cells.view(-1), stable=True)
    sums = torch.empty(cell_keys.shape[0], hip.MESH_CELL_SUMS, dtype=torch.float64, device=v.device)
    return lambda: hip.mesh_cluster_reduce(v, f, None, None, lo, h, v_order, cell_start, sorted_corners, corner_order, sums, group)


def simplify_part(mesh, reps):
    out = {}
    F = mesh.faces.shape[0]
    for factor in (10, 100):
        info = {}
        small = simplify_mesh(mesh, target_num_faces=F // factor, info=info)
        lo, h = info["origin"], info["cell_size"]
        row = {"target": F // factor, "cells_along_longest_axis": info["cells"], "count_calls": info["count_calls"],
               "vertices": small.vertices.shape[0], "faces": small.faces.shape[0],
               "search_and_pass_ms": spread(lambda: simplify_mesh(mesh, target_num_faces=F // factor), reps),
               "full_pass_ms": spread(lambda: simplify_mesh(mesh, cell_size=h, origin=lo), reps),
               "count_call_ms": spread(lambda: cluster_face_count(mesh, h, lo), reps)}
        for group in (8, 64):
            row[f"reduce_kernel_group{group}_ms"] = spread(reduce_only(mesh, lo, h, group), reps)
        out[f"x{factor}"] = row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolutions", type=int, nargs="+", default=[256, 512, 1024])
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--simplify-reps", type=int, default=7)
    args = ap.parse_args()
    dev = "cuda:0"
    pipe = bench.build_pipeline(dev, 1, 0)
    randomise(pipe)
    field = pipe.model.field
    lo, hi = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
    for res in args.resolutions:
        ms_sdf, vol = timed(lambda: sdf_grid(field, res, lo, hi), args.iters)
        # the randomised field's zero set need not cross the box: extract the level of its median grid value instead
        level = float(vol.view(-1)[::97].median())
        ms_mc, (v, f) = timed(lambda: marching_cubes(vol, level, lo, hi), args.iters)
        del v, f
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        v, f = marching_cubes(vol, level, lo, hi)
        torch.cuda.synchronize()
        extra = torch.cuda.max_memory_allocated() - base - (v.numel() + f.numel()) * 4
        ms_attr, _ = timed(lambda: vertex_attributes(field, v), args.iters)
        simplify = simplify_part(Mesh(v, f), args.simplify_reps)
        print(json.dumps({"resolution": res, "level": round(level, 5), "points": vol.numel(), "vertices": v.shape[0], "faces": f.shape[0],
                          "sdf_grid_ms": round(ms_sdf, 2), "marching_cubes_ms": round(ms_mc, 3), "attributes_ms": round(ms_attr, 2),
                          "mc_over_sdf": round(ms_mc / ms_sdf, 5), "mc_extra_bytes_per_point": round(extra / vol.numel(), 3),
                          "simplify": simplify, "device": torch.cuda.get_device_name(0)}), flush=True)
        del vol, v, f
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
