"""Antialiasing timings (relight.Antialias, csrc/antialias.hip) at 1920 x 1080, in one process:
  the three kernels for K = 1 and K = 8 linear images: medians of --iters with HIP events after a warm-up, every pass alternating with the
  others inside each iteration, against a torch.clone of `lin` (what this box takes to read and write the image's bytes once): the edge
  mask, the sub-pixel rays and the resolve of `lin` (with its rgb) at 10 % marked pixels and S = 4;
  and one 1080p frame of bench.py's randomised pipeline (its render-pass configuration: the same bundle, chunk 4096) plain, with
  Antialias(4) and with Antialias(4, every_pixel=True): wall time of the second frame of each kind (the chunk graph exists), with the
  share of marked pixels.  --no-frame skips the frames.
The kernels' G-buffer is synthetic: blocks of 8 x 8 pixels of constant depth, normal and accumulation under exp(uniform) images, so that
the mask's early exits are neither all taken nor all missed.
Prints one JSON line per K and one for the frames; run on the GPU box:
    python tools/bench_antialias.py [--iters 20] [--no-frame]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402

from neusky_amd import hip  # noqa: E402
from neusky_amd.relight import Antialias, r2_offsets  # noqa: E402

DEV = "cuda:0"
H, W = 1080, 1920
P = H * W


def median(v):
    return sorted(v)[len(v) // 2]


def measure(K, iters):
    g = torch.Generator(device=DEV).manual_seed(K)
    aa = Antialias(samples=4)
    S1 = aa.samples - 1
    blocks = lambda c: torch.rand(H // 8, W // 8, c, device=DEV, generator=g).repeat_interleave(8, 0).repeat_interleave(8, 1).contiguous()  # noqa: E731
    depth, acc, normal = 1.0 + blocks(1)[..., 0], blocks(1)[..., 0], blocks(3) - 0.5
    # as a frame of K suns is assembled: ray-major in memory, K leading in the shape alone
    lin = torch.exp(torch.rand(P, K, 3, device=DEV, generator=g) * 0.05).permute(1, 0, 2)
    rgb = torch.empty(P, K, 3, device=DEV).permute(1, 0, 2)
    mask = torch.empty(H, W, dtype=torch.uint8, device=DEV)
    pixels = torch.randperm(P, device=DEV, generator=g)[:P // 10].sort().values
    E = pixels.shape[0]
    origins, directions = torch.rand(P, 3, device=DEV, generator=g), torch.nn.functional.normalize(torch.rand(P, 3, device=DEV, generator=g) - 0.5, dim=-1)
    norm, area, cams = torch.ones(P, 1, device=DEV), torch.ones(P, 1, device=DEV), torch.zeros(P, 1, dtype=torch.long, device=DEV)
    offsets = r2_offsets(aa.samples).to(DEV)
    N = E * S1
    out = [torch.empty(N, 3, device=DEV), torch.empty(N, 3, device=DEV), torch.empty(N, 1, device=DEV), torch.empty(N, 1, device=DEV),
           torch.empty(N, 1, dtype=torch.long, device=DEV)]
    X = torch.rand(E, S1, K, 3, device=DEV, generator=g).permute(2, 0, 1, 3)  # the second pass's chunks: ray-major
    passes = {
        "clone": lambda: lin.clone(),
        "edge_mask": lambda: hip.aa_edge_mask(depth, normal, acc, lin, aa.accumulation, aa.depth, aa.cos2, aa.colour, aa.covered, mask),
        "subpixel_rays": lambda: hip.aa_subpixel_rays(origins, directions, norm, area, cams, H, W, pixels, offsets, *out),
        "resolve": lambda: hip.aa_resolve(lin, X, pixels, rgb),
    }
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
    med = {k: median(v) for k, v in times.items()}
    mask_bytes = P * (4 + 4 + 12 + 12 * K + 1)  # every pixel's own values once (the neighbours' reads hit L2), one byte out
    ray_bytes = N * (3 * 12 + 8 + 2 * 12 + 4 + 4 + 8)  # three pixels' directions, the index, what is written
    resolve_bytes = E * K * 3 * 4 * (S1 + 3) + E * 8  # S1 samples, the frame read and written, rgb written
    line = {"measure": "antialias_1080p", "K": K, "iters": iters, "samples": aa.samples, "marked_pixels": E, "marked_share_of_the_mask": round(float(mask.float().mean()), 4),
            **{f"{k}_ms": round(v, 4) for k, v in med.items()}, **{f"{k}_min_ms": round(min(times[k]), 4) for k in times},
            **{f"{k}_over_clone": round(med[k] / med["clone"], 3) for k in med if k != "clone"},
            "clone_gbytes_per_s": round(P * K * 24 / med["clone"] / 1e6, 1), "edge_mask_gbytes_per_s": round(mask_bytes / med["edge_mask"] / 1e6, 1),
            "subpixel_rays_gbytes_per_s": round(ray_bytes / med["subpixel_rays"] / 1e6, 1), "resolve_gbytes_per_s": round(resolve_bytes / med["resolve"] / 1e6, 1)}
    print(json.dumps(line), flush=True)


def frames():
    """one 1080p frame of bench.py's randomised pipeline, three ways"""
    import bench
    from util_step import randomise
    pipe = bench.build_pipeline(DEV, 1, 0)
    randomise(pipe)
    pipe.eval()
    rb, _, _, _ = bench.frame_1080p_rays(pipe, DEV)
    line = {"measure": "antialias_frame_1080p", "chunk": 4096}
    for name, kw in (("plain", {}), ("antialias_4", {"antialias": Antialias(samples=4)}),
                     ("antialias_4_every_pixel", {"antialias": Antialias(samples=4, every_pixel=True)})):
        for _ in range(2):  # the second frame: the chunk graph exists
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = pipe.model.get_outputs_for_camera_ray_bundle(rb, camera_index=0, chunk=4096, use_graph=True, **kw)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        line[f"{name}_ms"] = round(dt * 1e3, 1)
        if "aa_fraction" in out:
            line[f"{name}_marked_share"] = round(out["aa_fraction"], 4)
        del out
    line["antialias_4_over_plain"] = round(line["antialias_4_ms"] / line["plain_ms"], 3)
    line["antialias_4_every_pixel_over_plain"] = round(line["antialias_4_every_pixel_ms"] / line["plain_ms"], 3)
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-frame", action="store_true", help="time the kernels alone")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_antialias: no GPU; timings are taken on the device only")
    for K in (1, 8):
        measure(K, args.iters)
    if not args.no_frame:
        frames()


if __name__ == "__main__":
    main()
