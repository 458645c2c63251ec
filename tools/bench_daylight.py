"""Daylight-model timings (relight.DaylightSky, csrc/daylight.hip), medians with HIP events / wall clock after a warm-up:
  nsky_daylight_eval at the rays of a 1920 x 1080 frame (N = 2 073 600) for K = 1, 8, 24 suns, against a torch fill of an equally large
  output in the same process (the store rate this box reaches for those bytes; the two alternate inside every iteration);
  one 1920 x 1080 sweep frame of bench.py's randomised pipeline under the daylight sky against the same sweep of suns over the latent's
  sky, alternating on the same box (the chunk graphs of both are captured before the timed frames).
Prints one JSON line per measurement; run on the GPU box:
    python tools/bench_daylight.py [--iters 20] [--frames 3] [--suns 24] [--no-frame]"""
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
from neusky_amd.relight import DaylightSky, sun_path  # noqa: E402
from neusky_amd.relight.daylight import sun_directions  # noqa: E402
from neusky_amd.utils.randomise import randomise  # noqa: E402

DEV = "cuda:0"
N_1080P = 1920 * 1080


def median(v):
    return sorted(v)[len(v) // 2]


def kernel(iters, N=N_1080P):
    sky = DaylightSky()
    g = torch.Generator(device=DEV).manual_seed(0)
    directions = torch.randn(N, 3, device=DEV, generator=g)
    params = sky.device_parameters(DEV)
    for K in (1, 8, 24):
        suns = sun_directions(sky.sun_path(90.0, 3.0, 270.0, 65.0, K)).to(DEV)
        out, other = torch.empty(K, N, 3, device=DEV), torch.empty(K, N, 3, device=DEV)
        passes = {"eval": lambda: hip.daylight_eval(directions, suns, *params, out), "fill": lambda: other.fill_(1.0)}
        for _ in range(3):
            for fn in passes.values():
                fn()
        times = {k: [] for k in passes}
        for _ in range(iters):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(passes) + 1)]
            ev[0].record()
            for q, fn in enumerate(passes.values()):
                fn()
                ev[q + 1].record()
            torch.cuda.synchronize()
            for q, k in enumerate(passes):
                times[k].append(ev[q].elapsed_time(ev[q + 1]))
        med = {k: median(v) for k, v in times.items()}
        written = K * N * 12
        print(json.dumps({"measure": "daylight_eval", "N": N, "K": K, "iters": iters, "bytes_written": written,
                          **{f"{k}_ms": round(v, 4) for k, v in med.items()}, **{f"{k}_min_ms": round(min(times[k]), 4) for k in times},
                          "eval_over_fill": round(med["eval"] / med["fill"], 3), "eval_gbytes_per_s": round(written / med["eval"] / 1e6, 1),
                          "fill_gbytes_per_s": round(written / med["fill"] / 1e6, 1),
                          "ns_per_direction_and_sun": round(med["eval"] * 1e6 / (K * N), 4)}), flush=True)
        del out, other
        torch.cuda.empty_cache()


def frame(frames, K, chunk=4096):
    pipe = bench.build_pipeline(DEV, 1, 0)
    randomise(pipe)
    pipe.eval()
    rb = bench.frame_1080p_rays(pipe, DEV)[0]
    m = pipe.model
    sky = DaylightSky()
    cases = {"latent_sky": {"sun": sun_path(90.0, 3.0, 270.0, 65.0, K)}, "daylight": {"sun": sky.sun_path(90.0, 3.0, 270.0, 65.0, K), "daylight": sky}}

    def render(kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.get_outputs_for_camera_ray_bundle(rb, camera_index=0, chunk=chunk, use_graph=True, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for kw in cases.values():  # the chunk graphs of both
        render(kw)
    t = {k: [] for k in cases}
    for _ in range(frames):
        for k, kw in cases.items():
            t[k].append(render(kw))
    print(json.dumps({"measure": "sweep_frame_1080p", "rays": rb.origins.shape[0] * rb.origins.shape[1], "chunk": chunk, "suns": K,
                      **{f"{k}_s": [round(x, 3) for x in v] for k, v in t.items()},
                      "daylight_over_latent_sky": round(median(t["daylight"]) / median(t["latent_sky"]), 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--frames", type=int, default=3, help="alternating frame pairs")
    ap.add_argument("--suns", type=int, default=24, help="suns of the sweep frame")
    ap.add_argument("--no-frame", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_daylight: no GPU; timings are taken on the device only")
    kernel(args.iters)
    if not args.no_frame:
        frame(args.frames, args.suns)


if __name__ == "__main__":
    main()
