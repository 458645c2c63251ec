"""Prop timings (relight.props, csrc/props.hip), with HIP events / wall clock after a warm-up:
  the kernels alone at one render chunk's size (R = 4096 rays, S = 96 samples, D = 256 directions; P = 1 and 8 props), each against a
  `torch` copy that moves the same number of bytes, the two alternating in one process, medians of --iters runs: intersect, insert, and
  occlude on the sky's [R, D], the suns' [K, R] (K = 1, 24) and the lamps' [L, R].  A run is the replay of a captured graph of --inner
  launches, as a chunk's work is.  The occlusion's bytes are what it must touch (the points, the normals, the directions and a write of
  every entry), so a ratio far above 1 says the pass is bound by its fp64 interval tests, not by memory;
  one 1920 x 1080 frame of bench.py's randomised pipeline, chunk 4096, alternating in one process: plain and four props (placed in the
  view, half a scene unit along the middle row's rays) under the sky;
  one sun with DDF shadows, without and with the four props (the chunk graphs of every case are captured before the timed frames).
Prints one JSON line per measurement; run on the GPU box:
    python tools/bench_props.py [--iters 20] [--inner 50] [--frames 2] [--props 1 8] [--no-frame]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import bench  # noqa: E402
from bench_lights import DEV, against_a_copy, lamps  # noqa: E402
from neusky_amd import hip  # noqa: E402
from neusky_amd.relight import Prop, SunLight, lights_block, props_block  # noqa: E402
from neusky_amd.utils.randomise import randomise  # noqa: E402


def props(P):
    """P props about the origin, spheres and yawed boxes by turns"""
    out = []
    for p in range(P):
        at = (0.45 - 0.12 * p, 0.1 * p - 0.35, 0.05 * p - 0.1)
        out.append(Prop("box", at, (0.05, 0.08, 0.06), yaw_deg=17.0 * p) if p % 2 else Prop("sphere", at, 0.08))
    return out


def kernels(iters, inner, counts, R=4096, S=96, D=256):
    g = torch.Generator(device=DEV).manual_seed(0)
    rand = lambda *s: torch.rand(*s, device=DEV, generator=g)  # noqa: E731
    unit = lambda n: torch.nn.functional.normalize(torch.randn(n, 3, device=DEV, generator=g), dim=1)  # noqa: E731
    o, d = unit(R) * 1.2, None
    d = torch.nn.functional.normalize(-o + 0.4 * (rand(R, 3) - 0.5), dim=1)
    alb, ns, w = rand(R, S, 3), torch.randn(R, S, 3, device=DEV, generator=g), rand(R, S) / S
    edges = torch.sort(rand(R, S + 1) * 2.0, dim=1).values
    starts, ends = edges[:, :-1].contiguous(), edges[:, 1:].contiguous()
    x, n, bias = (rand(R, 3) - 0.5) * 0.8, torch.randn(R, 3, device=DEV, generator=g), torch.full((1,), 1e-2, device=DEV)
    for P in counts:
        block = props_block(props(P)).to(DEV)
        t_hit, who = torch.empty(R, device=DEV), torch.empty(R, dtype=torch.int32, device=DEV)
        hn, ha = torch.empty(R, 3, device=DEV), torch.empty(R, 3, device=DEV)
        hit = lambda: hip.props_intersect(o, d, block, t_hit, who, hn, ha)  # noqa: E731
        against_a_copy("props_intersect", hit, R * (24 + 32), iters, inner, R=R, P=P)
        hit()
        out = (torch.empty(R, S + 1, device=DEV), torch.empty(R, S + 1, device=DEV), torch.empty(R, S + 1, device=DEV),
               torch.empty(R, S + 1, 3, device=DEV), torch.empty(R, S + 1, 3, device=DEV))
        ins = lambda: hip.props_insert(w, starts, ends, alb, ns, t_hit, who, hn, ha, *out)  # noqa: E731
        against_a_copy("props_insert", ins, R * S * 36 + R * (S + 1) * 36 + R * 32, iters, inner, R=R, S=S, P=P)
        for name, N, lamp in (("sky [R, D]", D, False), ("suns [1, R]", 1, False), ("suns [24, R]", 24, False), ("lamps [1, R]", 1, True),
                              ("lamps [8, R]", 8, True)):
            vis = torch.ones(R, N, device=DEV) if name.startswith("sky") else torch.ones(N, R, device=DEV).t()
            if lamp:
                lights = lights_block(lamps(N)).to(DEV)
                kw = dict(targets=lights[:, 0:3].contiguous(), clearance=lights[:, 9].contiguous())
            else:
                kw = dict(directions=unit(N))
            occ = lambda: hip.props_occlude(x, n, bias, block, vis, **kw)  # noqa: E731
            against_a_copy("props_occlude", occ, R * 24 + N * 12 + R * N * 4, iters, inner, R=R, N=N, P=P, tensor=name)
            print(json.dumps({"measure": "props_occlude_share", "tensor": name, "P": P, "occluded": round(float((vis == 0).float().mean()), 4)}),
                  flush=True)


def frame(frames, chunk=4096):
    pipe = bench.build_pipeline(DEV, 1, 0)
    randomise(pipe)
    pipe.eval()
    rb = bench.frame_1080p_rays(pipe, DEV)[0]
    m = pipe.model
    # four props across the middle of the view, half a scene unit along the rays of the middle row
    Hf, Wf = rb.origins.shape[:2]
    at = [(rb.origins[Hf // 2, x] + 0.5 * rb.directions[Hf // 2, x]).tolist() for x in (Wf // 5, 2 * Wf // 5, 3 * Wf // 5, 4 * Wf // 5)]
    four = [Prop("box", c, (0.05, 0.08, 0.06), yaw_deg=30.0) if i % 2 else Prop("sphere", c, 0.08) for i, c in enumerate(at)]
    sun = SunLight(130.0, 35.0)
    cases = {"plain": {}, "props_4": dict(props=four), "sun_ddf": dict(sun=sun), "sun_ddf_props_4": dict(sun=sun, props=four)}

    def render(kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = m.get_outputs_for_camera_ray_bundle(rb, camera_index=0, chunk=chunk, use_graph=True, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out
    share = {}
    for k, kw in cases.items():  # the chunk graphs
        _, out = render(kw)
        if "prop_weight" in out:
            share[k] = {"weight_above_half": round(float((out["prop_weight"] > 0.5).float().mean()), 5),
                        "entered": round(float((out["prop_id"] >= 0).float().mean()), 5), "mean_weight": round(float(out["prop_weight"].mean()), 5)}
        del out
    t = {k: [] for k in cases}
    for _ in range(frames):
        for k, kw in cases.items():
            t[k].append(render(kw)[0])
    print(json.dumps({"measure": "frame_1080p", "rays": rb.origins.shape[0] * rb.origins.shape[1], "chunk": chunk,
                      **{f"{k}_s": [round(x, 4) for x in v] for k, v in t.items()},
                      "props_4_over_plain": round(min(t["props_4"]) / min(t["plain"]), 4),
                      "sun_ddf_props_4_over_sun_ddf": round(min(t["sun_ddf_props_4"]) / min(t["sun_ddf"]), 4), "prop_pixel_share": share}),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--inner", type=int, default=50, help="launches per timed graph replay")
    ap.add_argument("--frames", type=int, default=2, help="timed frames of each case, alternating")
    ap.add_argument("--props", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--no-frame", action="store_true")
    args = ap.parse_args()
    kernels(args.iters, args.inner, args.props)
    if not args.no_frame:
        frame(args.frames)


if __name__ == "__main__":
    main()
