"""Directional-sun timings (relight.SunLight, csrc/sun.hip), with HIP events / wall clock after a warm-up:
  the two sun kernels alone at one render chunk's size (R = 4096 rays, S = 96 samples; K = 1, 8, 32 suns), with the bytes they move
  against the HBM rate;
  one 1920 x 1080 frame of bench.py's randomised pipeline without a sun, with 1 sun and with 32 suns, alternating on the same box (the
  chunk graphs of all three are captured before the timed frames).
Prints one JSON line per measurement; run on the GPU box:
    python tools/bench_sun.py [--iters 20] [--frames 2] [--no-frame] [--hbm-gbs 8000]"""
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
from neusky_amd.relight import SunLight, sun_path  # noqa: E402
from neusky_amd.utils.randomise import randomise  # noqa: E402

DEV = "cuda:0"


def timed(fn, iters):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def kernels(iters, hbm_gbs, R=4096, S=96):
    g = torch.Generator(device=DEV).manual_seed(0)
    albedo, normals = torch.rand(R, S, 3, device=DEV, generator=g), torch.randn(R, S, 3, device=DEV, generator=g)
    weights = torch.rand(R, S, device=DEV, generator=g)
    for K in (1, 8, 32):
        suns = torch.randn(K, 3, device=DEV, generator=g)
        suns = suns / suns.norm(dim=1, keepdim=True)
        t = torch.empty(K, R, 3, device=DEV)
        ms = timed(lambda: hip.sun_transfer(albedo, normals, weights, suns, t), iters)
        passes = (K + 7) // 8
        moved = passes * R * S * 28 + K * R * 12  # a sample is 28 bytes, read once per pass of 8 suns
        print(json.dumps({"measure": "sun_transfer", "R": R, "S": S, "K": K, "ms": round(ms, 4), "bytes": moved,
                          "gb_per_s": round(moved / ms / 1e6, 1), "hbm_fraction": round(moved / ms / 1e6 / hbm_gbs, 4)}), flush=True)
        lin_sky, vis, acc = torch.rand(R, 3, device=DEV, generator=g), torch.rand(K, R, device=DEV, generator=g), torch.rand(R, device=DEV, generator=g)
        thr, colours = torch.zeros(1, device=DEV), torch.rand(K, 3, device=DEV, generator=g)
        rgb, lin, shadow = torch.empty(K, R, 3, device=DEV), torch.empty(K, R, 3, device=DEV), torch.empty(K, R, device=DEV)
        up = suns.abs().contiguous()  # every sun above the horizon: the whole composite runs
        ms = timed(lambda: hip.sun_composite(lin_sky, t, vis, acc, thr, up, colours, rgb, lin, shadow), iters)
        moved = R * 16 + K * R * (12 + 4 + 12 + 12 + 4)  # lin_sky, acc once; t, vis in; rgb, lin, shadow out
        print(json.dumps({"measure": "sun_composite", "R": R, "K": K, "ms": round(ms, 4), "bytes": moved,
                          "gb_per_s": round(moved / ms / 1e6, 1), "hbm_fraction": round(moved / ms / 1e6 / hbm_gbs, 4)}), flush=True)


def frame(frames, chunk=4096):
    pipe = bench.build_pipeline(DEV, 1, 0)
    randomise(pipe)
    pipe.eval()
    rb = bench.frame_1080p_rays(pipe, DEV)[0]
    m = pipe.model
    cases = {"no_sun": None, "sun_1": SunLight(130.0, 35.0), "sun_32": sun_path(90.0, 5.0, 270.0, 60.0, 32)}

    def render(s):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.get_outputs_for_camera_ray_bundle(rb, camera_index=0, chunk=chunk, use_graph=True, sun=s)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for s in cases.values():  # the chunk graphs of all three
        render(s)
    t = {k: [] for k in cases}
    for _ in range(frames):
        for k, s in cases.items():
            t[k].append(render(s))
    base = min(t["no_sun"])
    print(json.dumps({"measure": "frame_1080p", "rays": rb.origins.shape[0] * rb.origins.shape[1], "chunk": chunk,
                      **{f"{k}_s": [round(x, 3) for x in v] for k, v in t.items()},
                      "sun_1_over_no_sun": round(min(t["sun_1"]) / base, 4), "sun_32_over_no_sun": round(min(t["sun_32"]) / base, 4)}),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--frames", type=int, default=2, help="alternating frame triples")
    ap.add_argument("--no-frame", action="store_true")
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="the HBM rate the kernels' bytes are set against (MI355X: 8 TB/s)")
    args = ap.parse_args()
    kernels(args.iters, args.hbm_gbs)
    if not args.no_frame:
        frame(args.frames)


if __name__ == "__main__":
    main()
