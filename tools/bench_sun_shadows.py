"""Sphere-traced sun shadow timings (relight.trace_visibility, csrc/sphere_trace.hip), with HIP events / wall clock after a warm-up:
  the three kernels alone at one render chunk's size (R = 4096 rays; K = 1 and 24 suns), each against a `torch` copy that moves the
  same number of bytes, the two alternating in one process, medians of --iters runs.  A run is the replay of a captured graph of
  --inner launches, as a chunk's march is: at these sizes (0.1 to 5 MB) a launch from Python measures the host, not the kernel;
  one 1920 x 1080 frame of bench.py's randomised pipeline with `ddf` and with `sdf` shadows at K = 1 and K = 24 suns, alternating (the
  chunk graphs of every case are captured before the timed frames).
Prints one JSON line per measurement; run on the GPU box:
    python tools/bench_sun_shadows.py [--iters 20] [--inner 50] [--frames 1] [--suns 1 24] [--steps 96] [--no-frame]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from neusky_amd import hip, ops  # noqa: E402
from neusky_amd.relight import shadows, sun_path  # noqa: E402
from neusky_amd.utils.randomise import randomise  # noqa: E402

DEV = "cuda:0"


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def against_a_copy(name, fn, moved, iters, inner, **info):
    """`fn` and a torch copy moving `moved` bytes (half read, half written), each as a captured graph of `inner` launches, replayed
    alternately; medians per launch"""
    src = torch.empty(moved // 2, dtype=torch.uint8, device=DEV)
    dst = torch.empty_like(src)

    def graph_of(f):
        def body(i):
            for _ in range(inner):
                f()
        return ops.CapturedGraph(torch.device(DEV), 1, body)

    gk, gc = graph_of(fn), graph_of(lambda: dst.copy_(src))
    gk.replay(), gc.replay()
    torch.cuda.synchronize()
    k, c = [], []
    for _ in range(iters):
        k.append(event_ms(gk.replay) / inner)
        c.append(event_ms(gc.replay) / inner)
    km, cm = statistics.median(k), statistics.median(c)
    print(json.dumps({"measure": name, **info, "bytes": moved, "kernel_ms": round(km, 4), "copy_ms": round(cm, 4),
                      "kernel_over_copy": round(km / cm, 3), "gb_per_s": round(moved / km / 1e6, 1)}), flush=True)


def kernels(iters, inner, suns, R=4096):
    g = torch.Generator(device=DEV).manual_seed(0)
    o, d = torch.rand(R, 3, device=DEV, generator=g) - 0.5, torch.randn(R, 3, device=DEV, generator=g)
    d = d / d.norm(dim=1, keepdim=True)
    depth, n = torch.rand(R, device=DEV, generator=g) * 0.3, torch.randn(R, 3, device=DEV, generator=g)
    params = shadows.trace_params(shadows.trace_settings(None, shadows.SHADOW_DEFAULTS)).to(DEV)
    for K in suns:
        T = K * R
        s = torch.randn(K, 3, device=DEV, generator=g)
        s = s / s.norm(dim=1, keepdim=True)
        state, points = torch.empty(6, T, device=DEV), torch.empty(T, 3, device=DEV)
        sdf = torch.rand(T, device=DEV, generator=g) * 0.01  # small steps: the rays stay alive, every branch of the step runs
        vis, t, status = torch.empty(T, device=DEV), torch.empty(T, device=DEV), torch.empty(T, dtype=torch.int8, device=DEV)
        begin = lambda: hip.sphere_trace_begin(o, d, depth, n, s, params, state, points)  # noqa: E731
        against_a_copy("sphere_trace_begin", begin, R * 40 + T * 36, iters, inner, R=R, K=K)
        begin()
        step = lambda: hip.sphere_trace_step(state, sdf, s, R, params, 20, 1 << 30, 16, points)  # noqa: E731
        against_a_copy("sphere_trace_step", step, T * (28 + 24), iters, inner, R=R, K=K)
        against_a_copy("sphere_trace_finish", lambda: hip.sphere_trace_finish(state, vis, status, t), T * (12 + 9), iters, inner, R=R, K=K)


def frame(frames, suns, steps, chunk=4096):
    pipe = bench.build_pipeline(DEV, 1, 0)
    randomise(pipe)
    pipe.eval()
    rb = bench.frame_1080p_rays(pipe, DEV)[0]
    m = pipe.model
    cases = {}
    for K in suns:
        path = sun_path(90.0, 5.0, 270.0, 60.0, K) if K > 1 else sun_path(130.0, 35.0, 130.0, 35.0, 1)
        cases[f"ddf_{K}"] = dict(sun=path)
        cases[f"sdf_{K}"] = dict(sun=path, sun_shadows="sdf", shadow_trace={"steps": steps})

    def render(kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = m.get_outputs_for_camera_ray_bundle(rb, camera_index=0, chunk=chunk, use_graph=True, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    exhausted = {}
    for k, kw in cases.items():  # the chunk graphs
        _, out = render(kw)
        if "shadow_status" in out:
            exhausted[k] = round(float((out["shadow_status"] == shadows.EXHAUSTED).float().mean()), 5)
        del out
    t = {k: [] for k in cases}
    for _ in range(frames):
        for k, kw in cases.items():
            t[k].append(render(kw)[0])
    print(json.dumps({"measure": "frame_1080p", "rays": rb.origins.shape[0] * rb.origins.shape[1], "chunk": chunk, "steps": steps,
                      **{f"{k}_s": [round(x, 3) for x in v] for k, v in t.items()},
                      **{f"sdf_over_ddf_{K}": round(min(t[f"sdf_{K}"]) / min(t[f"ddf_{K}"]), 3) for K in suns},
                      "exhausted_share": exhausted}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--inner", type=int, default=50, help="launches per timed graph replay")
    ap.add_argument("--frames", type=int, default=1, help="timed frames of each case, alternating")
    ap.add_argument("--suns", type=int, nargs="+", default=[1, 24])
    ap.add_argument("--steps", type=int, default=96)
    ap.add_argument("--no-frame", action="store_true")
    args = ap.parse_args()
    kernels(args.iters, args.inner, args.suns)
    if not args.no_frame:
        frame(args.frames, args.suns, args.steps)


if __name__ == "__main__":
    main()
