"""Environment-map relighting timings on a randomised map, with HIP events after a warm-up:
  projection of a map onto D = 512 directions, split into label (HIP) / group (stable sort) / reduce (HIP), at 1024 x 2048,
  4096 x 8192 and 8192 x 16384;
  the sky lookup of 2 073 600 rays (one 1920 x 1080 frame);
  one 1920 x 1080 frame of bench.py's randomised pipeline lit by a 4096 x 8192 map against the same frame lit by a RENI latent,
  alternating on the same box (the chunk graphs of both are captured before the timed frames).
Prints one JSON line per measurement; run on the GPU box:
    python tools/bench_relight.py [--sizes 1024 4096 8192] [--iters 5] [--frames 2] [--no-frame]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from neusky_amd.relight import EnvironmentMap, envmap_lookup, project_envmap  # noqa: E402
from neusky_amd.utils.randomise import randomise  # noqa: E402

DEV = "cuda:0"


def random_map(H, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return EnvironmentMap(torch.rand(H, 2 * H, 3, device=DEV, generator=g) ** 8 * 1e3, "blender")


def unit(n, seed):
    d = torch.randn(n, 3, generator=torch.Generator().manual_seed(seed))
    return (d / d.norm(dim=1, keepdim=True)).to(DEV)


def projection(sizes, iters):
    dirs = unit(512, 1)
    for H in sizes:
        env = random_map(H)
        project_envmap(env, dirs)  # warm-up (sort workspace, code objects)
        parts = {"label": 0.0, "group": 0.0, "reduce": 0.0}
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        for _ in range(iters):
            ev = {}
            project_envmap(env, dirs, timings=ev)
            torch.cuda.synchronize()
            prev = "start"
            for k in parts:
                parts[k] += ev[prev].elapsed_time(ev[k]) / iters
                prev = k
        extra = torch.cuda.max_memory_allocated() - base
        total = sum(parts.values())
        print(json.dumps({"measure": "projection", "map": [H, 2 * H], "texels": 2 * H * H, "directions": 512,
                          **{f"{k}_ms": round(v, 3) for k, v in parts.items()}, "total_ms": round(total, 3),
                          "extra_bytes_per_texel": round(extra / (2 * H * H), 2)}), flush=True)
        del env
        torch.cuda.empty_cache()


def lookup(iters, H=4096):
    env = random_map(H)
    v = unit(2_073_600, 2)
    envmap_lookup(env, v)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        envmap_lookup(env, v)
    e1.record()
    torch.cuda.synchronize()
    print(json.dumps({"measure": "lookup", "map": [H, 2 * H], "rays": v.shape[0], "ms": round(e0.elapsed_time(e1) / iters, 4)}), flush=True)


def frame(frames, chunk=4096):
    pipe = bench.build_pipeline(DEV, 1, 0)
    randomise(pipe)
    pipe.eval()
    rb = bench.frame_1080p_rays(pipe, DEV)[0]
    env = random_map(4096)
    m = pipe.model

    def render(e):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.get_outputs_for_camera_ray_bundle(rb, camera_index=0, chunk=chunk, use_graph=True, envmap=e)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    render(None), render(env)  # the chunk graphs of both (and the sort workspace)
    t = {"reni": [], "envmap": []}
    for _ in range(frames):
        t["reni"].append(render(None))
        t["envmap"].append(render(env))
    reni, envm = min(t["reni"]), min(t["envmap"])
    print(json.dumps({"measure": "frame_1080p", "rays": rb.origins.shape[0] * rb.origins.shape[1], "chunk": chunk,
                      "reni_s": [round(x, 3) for x in t["reni"]], "envmap_s": [round(x, 3) for x in t["envmap"]],
                      "envmap_over_reni": round(envm / reni, 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096, 8192], help="map heights (width = 2 x height)")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--frames", type=int, default=2, help="alternating frame pairs")
    ap.add_argument("--no-frame", action="store_true")
    args = ap.parse_args()
    projection(args.sizes, args.iters)
    lookup(args.iters * 4)
    if not args.no_frame:
        frame(args.frames)


if __name__ == "__main__":
    main()
