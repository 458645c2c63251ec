"""Depth-of-field timings (relight.DepthOfField, csrc/dof.hip) at 1920 x 1080, in one process:
  the three kernels: medians of --iters with HIP events after a warm-up, every pass alternating with the others inside each iteration,
  against a torch.clone of a linear image (what this box takes to read and write the image's bytes once): the circle of confusion, the
  mark at reach 16 and at reach 64, and the lens rays at S = 16 with 10 % of the pixels marked;
  and one 1080p frame of bench.py's randomised pipeline (its render-pass configuration: the same camera, chunk 4096) plain and with
  DepthOfField(every_pixel=True, samples=4): wall time of the second frame of each kind (the chunk graph exists); by count the second is
  four frames.  Then, in the same process, the circle of confusion and the mark at reach 16 on that frame's own depth and accumulation,
  against the plain frame: the marking pass is to stay under 1 % of it.  --no-frame skips the frames.
bench.py's frame bundle holds unit directions with directions_norm 1: D = directions * directions_norm is then not affine in the pixel and
the lens refuses it as no pinhole's.  The frames here give the same rays their norms, |((x - W / 2) / f, (y - H / 2) / f, 1)|, as
relight.camera_rays does; the plain frame is timed on that bundle too.
The kernels' depth is synthetic: blocks of 8 x 8 pixels of constant depth and accumulation, a third of them out of focus by up to 24
pixels, so that discs of every radius up to beyond reach 16 are there.
Prints one JSON line for the kernels and one for the frames; run on the GPU box:
    python tools/bench_dof.py [--iters 20] [--no-frame]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402

from neusky_amd import hip  # noqa: E402
from neusky_amd.relight import DepthOfField, lens_table  # noqa: E402

DEV = "cuda:0"
H, W = 1080, 1920
P = H * W


def median(v):
    return sorted(v)[len(v) // 2]


def alternate(passes, iters):
    """{name: (median, min)} in ms of each pass, all alternating inside every iteration, after three warm-up rounds"""
    for _ in range(3):
        for fn in passes.values():
            fn()
    torch.cuda.synchronize()
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
    return {k: (median(v), min(v)) for k, v in times.items()}


def measure(iters):
    g = torch.Generator(device=DEV).manual_seed(1)
    S = 16
    blocks = lambda: torch.rand(H // 8, W // 8, device=DEV, generator=g).repeat_interleave(8, 0).repeat_interleave(8, 1).contiguous()  # noqa: E731
    depth, acc = 0.5 + 2.0 * blocks(), blocks()
    lens = torch.tensor([1, 0, 0, 0, 1, 0, 0, 0, 1, 0.01, 1.0, 0.01 * 1100.0], dtype=torch.float32, device=DEV)  # focus at depth 1, f_px 1100
    coc = torch.empty(H, W, device=DEV)
    mask = torch.empty(H, W, dtype=torch.uint8, device=DEV)
    lin = torch.rand(P, 3, device=DEV, generator=g)
    pixels = torch.randperm(P, device=DEV, generator=g)[:P // 10].sort().values
    E = pixels.shape[0]
    origins, directions = torch.rand(P, 3, device=DEV, generator=g), torch.nn.functional.normalize(torch.rand(P, 3, device=DEV, generator=g) - 0.5, dim=-1)
    norm, area, cams = torch.ones(P, 1, device=DEV), torch.ones(P, 1, device=DEV), torch.zeros(P, 1, dtype=torch.long, device=DEV)
    table = lens_table(S).to(DEV)
    N = E * (S - 1)
    out = [torch.empty(N, 3, device=DEV), torch.empty(N, 3, device=DEV), torch.empty(N, 1, device=DEV), torch.empty(N, 1, device=DEV),
           torch.empty(N, 1, dtype=torch.long, device=DEV)]
    hip.dof_coc(depth, acc, lens, -1, 0.5, coc)
    # two thirds of the blocks in focus, the rest blurred by up to 24 pixels
    coc = torch.where(blocks() < 2.0 / 3.0, torch.zeros_like(coc), coc * (24.0 / coc.max()))
    fresh = torch.empty(H, W, device=DEV)
    passes = {
        "clone": lambda: lin.clone(),
        "coc": lambda: hip.dof_coc(depth, acc, lens, -1, 0.5, fresh),
        "mark_16": lambda: hip.dof_mark(coc, 0.5, 16, mask),
        "mark_64": lambda: hip.dof_mark(coc, 0.5, 64, mask),
        "lens_rays": lambda: hip.dof_lens_rays(origins, directions, norm, area, cams, H, W, pixels, table, lens, True, *out),
    }
    t = alternate(passes, iters)
    hip.dof_mark(coc, 0.5, 16, mask)
    share16 = float(mask.float().mean())
    ray_bytes = N * (3 * 12 + 8 + 2 * 12 + 4 + 4 + 8) + E * 12  # three pixels' directions, the index, the origin, what is written
    line = {"measure": "dof_1080p", "iters": iters, "samples": S, "marked_pixels": E, "mark_16_share": round(share16, 4),
            **{f"{k}_ms": round(v[0], 4) for k, v in t.items()}, **{f"{k}_min_ms": round(v[1], 4) for k, v in t.items()},
            **{f"{k}_over_clone": round(v[0] / t["clone"][0], 3) for k, v in t.items() if k != "clone"},
            "clone_gbytes_per_s": round(P * 24 / t["clone"][0] / 1e6, 1), "coc_gbytes_per_s": round(P * 12 / t["coc"][0] / 1e6, 1),
            "mark_16_gbytes_per_s": round(P * 5 / t["mark_16"][0] / 1e6, 1), "lens_rays_gbytes_per_s": round(ray_bytes / t["lens_rays"][0] / 1e6, 1)}
    print(json.dumps(line), flush=True)


def frames(iters):
    """one 1080p frame of bench.py's randomised pipeline, plain and through a lens at every pixel; the marking pass against the plain frame"""
    import bench
    from util_step import randomise
    pipe = bench.build_pipeline(DEV, 1, 0)
    randomise(pipe)
    pipe.eval()
    rb, _, _, _ = bench.frame_1080p_rays(pipe, DEV)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    rb.metadata["directions_norm"] = torch.stack([(xs - W / 2) / 1100.0, (ys - H / 2) / 1100.0, torch.ones(H, W)], -1).norm(dim=-1, keepdim=True).to(DEV)
    line = {"measure": "dof_frame_1080p", "chunk": 4096}
    lens = DepthOfField(0.02, samples=4, every_pixel=True)
    for name, kw in (("plain", {}), ("dof_4_every_pixel", {"depth_of_field": lens})):
        for _ in range(2):  # the second frame: the chunk graph exists
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = pipe.model.get_outputs_for_camera_ray_bundle(rb, camera_index=0, chunk=4096, use_graph=True, **kw)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        line[f"{name}_ms"] = round(dt * 1e3, 1)
        if "dof_fraction" in out:
            line[f"{name}_marked_share"] = round(out["dof_fraction"], 4)
            izf = float(out["dof_focus"])  # (that pipeline has no surface: the centre pixel is uncovered and the focus lies at infinity)
            line["focus_distance"] = round(1.0 / izf, 4) if izf > 0.0 else "infinity"
        depth, acc = out["depth"].view(H, W).clone(), out["accumulation"].view(H, W).clone()
        del out
    line["dof_4_every_pixel_over_plain"] = round(line["dof_4_every_pixel_ms"] / line["plain_ms"], 3)
    # the marking pass on this frame's own first pass, as the frame render runs it
    from neusky_amd.relight import lens_block, lens_frame
    block = lens_block(lens_frame(rb), 0.02, 0.0)
    coc, mask = torch.empty(H, W, device=DEV), torch.empty(H, W, dtype=torch.uint8, device=DEV)
    focus = (H // 2) * W + W // 2
    t = alternate({"coc": lambda: hip.dof_coc(depth, acc, block, focus, 0.5, coc), "mark_16": lambda: hip.dof_mark(coc, 0.5, 16, mask)}, iters)
    line["frame_coc_ms"], line["frame_mark_16_ms"] = round(t["coc"][0], 4), round(t["mark_16"][0], 4)
    line["frame_mark_16_share"] = round(float(mask.float().mean()), 4)
    line["coc_plus_mark_16_over_plain_frame"] = round((t["coc"][0] + t["mark_16"][0]) / line["plain_ms"], 6)
    line["under_one_percent"] = line["coc_plus_mark_16_over_plain_frame"] < 0.01
    print(json.dumps(line), flush=True)
    return line["under_one_percent"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-frame", action="store_true", help="time the kernels alone")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dof: no GPU; timings are taken on the device only")
    measure(args.iters)
    if not args.no_frame and not frames(args.iters):
        raise SystemExit("bench_dof: the circle of confusion and the mark at reach 16 take 1 % of the plain frame or more")


if __name__ == "__main__":
    main()
