"""Point and spot light timings (relight.lights, csrc/lights.hip, the bounded step of csrc/sphere_trace.hip), with HIP events / wall clock
after a warm-up:
  the kernels alone at one render chunk's size (R = 4096 rays, S = 96 samples; L = 1 and 8 lamps), each against a `torch` copy that
  moves the same number of bytes, the two alternating in one process, medians of --iters runs; nsky_light_transfer beside
  nsky_sun_transfer at the same R, S, K, and the bounded step beside nsky_sphere_trace_step at the same T.  A run is the replay of a
  captured graph of --inner launches, as a chunk's work is: at these sizes a launch from Python measures the host, not the kernel;
  one 1920 x 1080 frame of bench.py's randomised pipeline, chunk 4096, alternating: plain; one sun with sun_shadows="sdf"; one lamp;
  four lamps (the chunk graphs of every case are captured before the timed frames).
Prints one JSON line per measurement; run on the GPU box:
    python tools/bench_lights.py [--iters 20] [--inner 50] [--frames 1] [--lights 1 8] [--steps 96] [--no-frame]"""
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
from neusky_amd.relight import PointLight, SunLight, lights_block, shadows  # noqa: E402
from neusky_amd.relight.lights import LIGHT_TRACE_DEFAULTS  # noqa: E402
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


def lamps(L):
    """L lamps about the origin, points and spots by turns"""
    out = []
    for l in range(L):  # noqa: E741
        spot = dict(direction=(0.1 * l - 0.3, 0.2, -1.0), inner_deg=20.0, outer_deg=50.0) if l % 2 else {}
        out.append(PointLight((0.5 - 0.13 * l, 0.1 * l - 0.4, 0.3 + 0.05 * l), (1.0, 0.9, 0.8), radius=0.02, **spot))
    return out


def kernels(iters, inner, counts, R=4096, S=96):
    g = torch.Generator(device=DEV).manual_seed(0)
    x, alb = torch.rand(R, S, 3, device=DEV, generator=g) - 0.5, torch.rand(R, S, 3, device=DEV, generator=g)
    ns, w = torch.randn(R, S, 3, device=DEV, generator=g), torch.rand(R, S, device=DEV, generator=g) / S
    o, d = torch.rand(R, 3, device=DEV, generator=g) - 0.5, torch.randn(R, 3, device=DEV, generator=g)
    d = d / d.norm(dim=1, keepdim=True)
    depth, n = torch.rand(R, device=DEV, generator=g) * 0.3, torch.randn(R, 3, device=DEV, generator=g)
    acc, thr = torch.rand(R, device=DEV, generator=g), torch.zeros(1, device=DEV)
    params = shadows.trace_params(shadows.trace_settings(None, LIGHT_TRACE_DEFAULTS)).to(DEV)
    for L in counts:
        T = L * R
        block = lights_block(lamps(L)).to(DEV)
        suns = torch.randn(L, 3, device=DEV, generator=g)
        suns = suns / suns.norm(dim=1, keepdim=True)
        t = torch.empty(L, R, 3, device=DEV)
        passes = -(-L // 8)
        lt = against_a_copy("light_transfer", lambda: hip.light_transfer(x, alb, ns, w, block, t), passes * R * S * 40 + T * 12, iters, inner,
                            R=R, S=S, L=L)
        st = against_a_copy("sun_transfer", lambda: hip.sun_transfer(alb, ns, w, suns, t), passes * R * S * 28 + T * 12, iters, inner,
                            R=R, S=S, K=L)
        print(json.dumps({"measure": "light_transfer_over_sun_transfer", "R": R, "S": S, "L": L, "ratio": round(lt / st, 3)}), flush=True)
        state, points = torch.empty(6, T, device=DEV), torch.empty(T, 3, device=DEV)
        ray_dirs, bounds = torch.empty(T, 3, device=DEV), torch.empty(2, T, device=DEV)
        sdf = torch.rand(T, device=DEV, generator=g) * 0.01  # small steps: the rays stay alive, every branch of the step runs
        begin = lambda: hip.light_trace_begin(o, d, depth, n, block, params, state, points, ray_dirs, bounds)  # noqa: E731
        against_a_copy("light_trace_begin", begin, R * 40 + T * (36 + 20), iters, inner, R=R, L=L)
        begin()
        bounds[0].fill_(1e30)  # (no ray reaches its lamp during the timed rounds)
        step = lambda: hip.sphere_trace_step(state, sdf, ray_dirs, 1, params, 20, 1 << 30, 16, points, bounds)  # noqa: E731
        sb = against_a_copy("sphere_trace_step_bounded", step, T * (28 + 20 + 24), iters, inner, T=T)
        hip.sphere_trace_begin(o, d, depth, n, suns, params, state, points)
        plain = lambda: hip.sphere_trace_step(state, sdf, suns, R, params, 20, 1 << 30, 16, points)  # noqa: E731
        sp = against_a_copy("sphere_trace_step", plain, T * (28 + 24), iters, inner, T=T)
        print(json.dumps({"measure": "step_bounded_over_step", "T": T, "ratio": round(sb / sp, 3)}), flush=True)
        vis = torch.rand(L, R, device=DEV, generator=g)
        for Kb in (1, 3):
            base = torch.rand(Kb, R, 3, device=DEV, generator=g)
            rgb, lin = torch.empty(Kb, R, 3, device=DEV), torch.empty(Kb, R, 3, device=DEV)
            light_lin, V = torch.empty(R, 3, device=DEV), torch.empty(L, R, device=DEV)
            comp = lambda: hip.lights_composite(base, t, vis, acc, thr, block, rgb, lin, light_lin, V)  # noqa: E731
            against_a_copy("lights_composite", comp, R * 4 + T * (12 + 4 + 4) + Kb * R * 36 + R * 12, iters, inner, R=R, L=L, Kb=Kb)


def frame(frames, steps, chunk=4096):
    pipe = bench.build_pipeline(DEV, 1, 0)
    randomise(pipe)
    pipe.eval()
    rb = bench.frame_1080p_rays(pipe, DEV)[0]
    m = pipe.model
    trace = {"steps": steps}
    cases = {"plain": {}, "sun_sdf_1": dict(sun=SunLight(130.0, 35.0), sun_shadows="sdf", shadow_trace=trace),
             "lamp_1": dict(lights=lamps(1), light_trace=trace), "lamp_4": dict(lights=lamps(4), light_trace=trace)}

    def render(kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = m.get_outputs_for_camera_ray_bundle(rb, camera_index=0, chunk=chunk, use_graph=True, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    exhausted = {}
    for k, kw in cases.items():  # the chunk graphs
        _, out = render(kw)
        for key in ("shadow_status", "light_status"):
            if key in out:
                exhausted[k] = round(float((out[key] == shadows.EXHAUSTED).float().mean()), 5)
        del out
    t = {k: [] for k in cases}
    for _ in range(frames):
        for k, kw in cases.items():
            t[k].append(render(kw)[0])
    print(json.dumps({"measure": "frame_1080p", "rays": rb.origins.shape[0] * rb.origins.shape[1], "chunk": chunk, "steps": steps,
                      **{f"{k}_s": [round(x, 3) for x in v] for k, v in t.items()},
                      "lamp_1_over_sun_sdf_1": round(min(t["lamp_1"]) / min(t["sun_sdf_1"]), 3),
                      "lamp_4_over_lamp_1": round(min(t["lamp_4"]) / min(t["lamp_1"]), 3), "exhausted_share": exhausted}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--inner", type=int, default=50, help="launches per timed graph replay")
    ap.add_argument("--frames", type=int, default=1, help="timed frames of each case, alternating")
    ap.add_argument("--lights", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--steps", type=int, default=96)
    ap.add_argument("--no-frame", action="store_true")
    args = ap.parse_args()
    kernels(args.iters, args.inner, args.lights)
    if not args.no_frame:
        frame(args.frames, args.steps)


if __name__ == "__main__":
    main()
