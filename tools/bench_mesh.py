"""Mesh export timing on bench.py's randomised field: at each resolution, the three parts of extract_mesh timed separately with
HIP events after a warm-up -- the SDF grid (fused hash encode + SDF value chain over every grid point), the marching-cubes passes
(count, tile scan, vertices, faces; at the level of the median grid value, so that the surface crosses the box), the vertex
attributes (field_values at the vertices) -- and the peak device memory that marching_cubes allocates beyond its input volume
and its output mesh.  Prints one JSON line per resolution; run on the GPU box:
    python tools/bench_mesh.py [--resolutions 256 512 1024] [--iters 3]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from neusky_amd.exporter import marching_cubes, sdf_grid  # noqa: E402
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolutions", type=int, nargs="+", default=[256, 512, 1024])
    ap.add_argument("--iters", type=int, default=3)
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
        print(json.dumps({"resolution": res, "level": round(level, 5), "points": vol.numel(), "vertices": v.shape[0], "faces": f.shape[0],
                          "sdf_grid_ms": round(ms_sdf, 2), "marching_cubes_ms": round(ms_mc, 3), "attributes_ms": round(ms_attr, 2),
                          "mc_over_sdf": round(ms_mc / ms_sdf, 5), "mc_extra_bytes_per_point": round(extra / vol.numel(), 3)}), flush=True)
        del vol, v, f
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
