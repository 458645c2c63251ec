"""Atmosphere timings (relight.atmosphere, csrc/atmosphere.hip), with HIP events / wall clock after a warm-up:
  the two kernels alone at one render chunk's size (R = 4096 rays; Kb = 1 and 8 base images; M = 0 and 16 shaft samples), each against
  a `torch` copy that moves the same number of bytes, the two alternating in one process, medians of --iters runs.  A run is the replay
  of a captured graph of --inner launches, as a chunk's work is: at these sizes a launch from Python measures the host, not the kernel;
  one 1920 x 1080 frame of bench.py's randomised pipeline, chunk 4096, one sun with DDF shadows, alternating: clear; with fog; with fog
  and 16 shaft samples (the chunk graphs of every case are captured before the timed frames: the numbers are second frames).
Prints one JSON line per measurement; run on the GPU box:
    python tools/bench_atmosphere.py [--iters 20] [--inner 50] [--frames 1] [--no-frame]"""
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
from neusky_amd.relight import Atmosphere, SunLight  # noqa: E402
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
    alternately; medians per launch -> the kernel's"""
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
    return km


def kernels(iters, inner, R=4096):
    g = torch.Generator(device=DEV).manual_seed(0)
    rand = lambda *s: torch.rand(*s, device=DEV, generator=g)  # noqa: E731
    o, d = rand(R, 3) - 0.5, torch.randn(R, 3, device=DEV, generator=g)
    d = d / d.norm(dim=1, keepdim=True)
    depth, acc = rand(R) * 2.5, rand(R)
    params = Atmosphere((0.5, 1.0, 2.0), scale_height=0.3, anisotropy=0.6).block().to(DEV)
    ro, rd, rt = torch.empty(16 * R, 3, device=DEV), torch.empty(16 * R, 3, device=DEV), torch.empty(16 * R, device=DEV)
    against_a_copy("atmosphere_rows", lambda: hip.atmosphere_rows(o, d, params, 16, ro, rd, rt), R * 24 + 16 * R * 28, iters, inner, R=R, M=16)
    for Kb in (1, 8):
        suns = torch.randn(Kb, 3, device=DEV, generator=g)
        suns[:, 2] = suns[:, 2].abs() + 0.1
        suns = suns / suns.norm(dim=1, keepdim=True)
        colours, abar = rand(Kb, 3) + 0.5, rand(Kb, 3)
        lin_in, bg, light_lin = rand(Kb, R, 3), rand(Kb, R, 3), rand(R, 3)
        lin, rgb, ins = (torch.empty(Kb, R, 3, device=DEV) for _ in range(3))
        T = torch.empty(R, 3, device=DEV)
        for M in (0, 16):
            vis = rand(M, Kb, R) if M else None
            apply = lambda: hip.atmosphere_apply(o, d, depth, acc, lin_in, bg, abar, suns, colours, vis, params, M, lin, rgb, ins, T,  # noqa: E731
                                                 light_lin)
            moved = R * (24 + 8) + Kb * R * (12 + 12 + 36) + R * (12 + 24) + M * Kb * R * 4
            against_a_copy("atmosphere_apply", apply, moved, iters, inner, R=R, Kb=Kb, M=M)


def frame(frames, chunk=4096):
    pipe = bench.build_pipeline(DEV, 1, 0)
    randomise(pipe)
    pipe.eval()
    rb = bench.frame_1080p_rays(pipe, DEV)[0]
    m = pipe.model
    sun = SunLight(130.0, 35.0)
    fog = Atmosphere((0.5, 1.0, 2.0), scale_height=0.3, anisotropy=0.6)
    cases = {"clear": dict(sun=sun), "fog": dict(sun=sun, atmosphere=fog),
             "fog_shafts_16": dict(sun=sun, atmosphere=Atmosphere((0.5, 1.0, 2.0), scale_height=0.3, anisotropy=0.6, shaft_samples=16))}

    def render(kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.get_outputs_for_camera_ray_bundle(rb, camera_index=0, chunk=chunk, use_graph=True, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for kw in cases.values():  # the chunk graphs
        render(kw)
    t = {k: [] for k in cases}
    for _ in range(frames):
        for k, kw in cases.items():
            t[k].append(render(kw))
    print(json.dumps({"measure": "frame_1080p", "rays": rb.origins.shape[0] * rb.origins.shape[1], "chunk": chunk,
                      **{f"{k}_s": [round(x, 3) for x in v] for k, v in t.items()},
                      "fog_over_clear": round(min(t["fog"]) / min(t["clear"]), 4),
                      "fog_shafts_16_over_clear": round(min(t["fog_shafts_16"]) / min(t["clear"]), 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--inner", type=int, default=50, help="launches per timed graph replay")
    ap.add_argument("--frames", type=int, default=1, help="timed frames of each case, alternating")
    ap.add_argument("--no-frame", action="store_true")
    args = ap.parse_args()
    kernels(args.iters, args.inner)
    if not args.no_frame:
        frame(args.frames)


if __name__ == "__main__":
    main()
