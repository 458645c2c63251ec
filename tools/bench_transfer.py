"""Radiance-transfer timings at 1920 x 1080 on bench.py's randomised pipeline (D = its light directions), in one run on one box:
  the bake (fp16 and fp32 storage) against the plain frame of the same pipeline, alternating;
  the relight kernel per light for K = 1 and K = 8 in both storages, with the effective bytes of T per second (HIP events after a warm-up);
  RadianceTransfer.relight() end to end per frame, lit by a latent and by a 4096 x 8192 map, and the latent background decode on its own.
Prints one JSON line per measurement; run on the GPU box:
    python tools/bench_transfer.py [--iters 10] [--frames 2] [--storages fp16 fp32]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from neusky_amd import hip  # noqa: E402
from neusky_amd.relight import EnvironmentMap, bake_transfer, z_rotation  # noqa: E402
from neusky_amd.utils.randomise import randomise  # noqa: E402

DEV = "cuda:0"


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def events(fn, iters):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--frames", type=int, default=2, help="alternating frame / bake rounds")
    ap.add_argument("--storages", nargs="+", default=["fp16", "fp32"], choices=("fp16", "fp32"))
    ap.add_argument("--chunk", type=int, default=4096)
    args = ap.parse_args()
    pipe = bench.build_pipeline(DEV, 1, 0)
    randomise(pipe)
    pipe.eval()
    m = pipe.model
    rb = bench.frame_1080p_rays(pipe, DEV)[0]
    R = rb.origins.shape[0] * rb.origins.shape[1]

    def frame():
        return m.get_outputs_for_camera_ray_bundle(rb, camera_index=0, chunk=args.chunk, use_graph=True)

    wall(frame)  # the frame's chunk graph
    t_frame, t_bake, baked = [], {s: [] for s in args.storages}, {}
    for s in args.storages:  # the bake's code objects (its chunk graph is captured inside every bake, and timed with it)
        wall(lambda: bake_transfer(m, rb, storage=s, chunk=args.chunk, camera_index=0))
    for _ in range(args.frames):
        t_frame.append(wall(frame)[0])
        for s in args.storages:
            t, baked[s] = wall(lambda: bake_transfer(m, rb, storage=s, chunk=args.chunk, camera_index=0))
            t_bake[s].append(t)
    frame_s = min(t_frame)
    D = next(iter(baked.values())).dirs.shape[0]
    for s in args.storages:
        print(json.dumps({"measure": "bake_1080p", "storage": s, "rays": R, "directions": D, "chunk": args.chunk,
                          "frame_s": [round(x, 3) for x in t_frame], "bake_s": [round(x, 3) for x in t_bake[s]],
                          "bake_over_frame": round(min(t_bake[s]) / frame_s, 4), "transfer_bytes": baked[s].nbytes}), flush=True)

    # the relight kernel alone
    g = torch.Generator(device=DEV).manual_seed(0)
    for s in args.storages:
        b = baked[s]
        for K in (1, 8):
            lights = torch.rand(K, D, 3, device=DEV, generator=g)
            bg = torch.rand(K, R, 3, device=DEV, generator=g)
            rgb = torch.empty(K, R, 3, device=DEV)
            ms = events(lambda: hip.transfer_relight(b.T, b.exponents, b.acc, lights, bg, rgb, None), args.iters)
            print(json.dumps({"measure": "relight_kernel", "storage": s, "K": K, "rays": R, "directions": D, "ms_per_pass": round(ms, 4),
                              "ms_per_light": round(ms / K, 4), "transfer_TB_per_s": round(b.nbytes / (ms * 1e-3) / 1e12, 3)}), flush=True)
            del lights, bg, rgb

    # relight() end to end: building L and bg included
    H = 4096
    env = EnvironmentMap(torch.rand(H, 2 * H, 3, device=DEV, generator=g) ** 8 * 1e3, "blender")
    rots = [z_rotation(0.1 * (i + 1)).to(DEV) for i in range(8)]
    latents, scales = m.get_illumination_field()
    for s in args.storages:
        b = baked[s]
        for name, kw in (("latent", {}), ("envmap_4096x8192", {"envmap": env})):
            one = events(lambda: b.relight(m, camera_index=0, rotations=rots[0], **kw), args.iters)
            eight = events(lambda: b.relight(m, camera_index=0, rotations=rots, **kw), max(1, args.iters // 4))
            print(json.dumps({"measure": "relight_end_to_end", "storage": s, "light": name, "ms_per_frame_K1": round(one, 3),
                              "ms_per_frame_K8": round(eight / 8, 3), "frame_s": round(frame_s, 3),
                              "frame_over_relit_frame_K1": round(frame_s * 1e3 / one, 1)}), flush=True)
    b = next(iter(baked.values()))
    ms = events(lambda: b._light(m, None, 0, rots[0]), args.iters)
    print(json.dumps({"measure": "latent_light_decode", "rays": R, "directions": D, "ms": round(ms, 3)}), flush=True)


if __name__ == "__main__":
    main()
