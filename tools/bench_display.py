"""Display-transform timings (relight.DisplayTransform, csrc/display.hip) at 1920 x 1080 for K = 1 and K = 8 images: medians of --iters
with HIP events after a warm-up, every pass alternating with the others inside each iteration, in one process:
  each kernel (histogram, exposure, map with and without the float image, the bloom's blur) and the whole transform (metered per frame,
  with and without a bloom), against a torch.clone of `lin` (what this box takes to read and write the image's bytes once);
  and, for K = 1, the whole transform against one dense fp16 K = 1 nsky_transfer_relight pass over a synthetic T of the frame's size
  (--directions, default 512; halved until it fits), the pass that makes the image the transform shows.
The image is synthetic: exp(uniform(-8, 8)) per channel, 23 octaves of luminance spread over some 1500 bins.
Prints one JSON line per K; run on the GPU box:
    python tools/bench_display.py [--iters 20] [--directions 512] [--sigma 4]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from neusky_amd import hip  # noqa: E402
from neusky_amd.relight import DisplayTransform  # noqa: E402
from neusky_amd.relight.display import bloom_weights  # noqa: E402

DEV = "cuda:0"
H, W = 1080, 1920


def median(v):
    return sorted(v)[len(v) // 2]


def synthetic_transfer(D):
    """fp16 T [R, D, 3] with its exponents, acc, one light and a background, or None where it does not fit"""
    R = H * W
    while D >= 8:
        try:
            T = torch.empty(R, D, 3, dtype=torch.float16, device=DEV).uniform_(0.0, 1.0)
            g = torch.Generator(device=DEV).manual_seed(1)
            return (T, torch.zeros(R, dtype=torch.int32, device=DEV), torch.rand(R, device=DEV, generator=g),
                    torch.rand(1, D, 3, device=DEV, generator=g), torch.rand(1, R, 3, device=DEV, generator=g))
        except torch.OutOfMemoryError:
            D //= 2
    return None


def measure(K, iters, sigma, transfer):
    g = torch.Generator(device=DEV).manual_seed(K)
    lin = torch.exp(torch.rand(K, H, W, 3, device=DEV, generator=g) * 16.0 - 8.0)
    metered = DisplayTransform(curve="aces", exposure="frame")
    bloomed = DisplayTransform(curve="aces", exposure="frame", bloom_sigma=sigma)
    params, weights = metered.params(DEV), bloom_weights(sigma).to(DEV)
    hist = torch.zeros(K, hip.DISPLAY_BINS, dtype=torch.int64, device=DEV)
    E = torch.empty(K, dtype=torch.float32, device=DEV)
    rgb8, rgb = torch.empty(lin.shape, dtype=torch.uint8, device=DEV), torch.empty_like(lin)
    scratch, B = torch.empty_like(lin), torch.empty_like(lin)
    passes = {
        "clone": lambda: lin.clone(),
        "histogram": lambda: hip.display_histogram(lin, None, params, hist),
        "exposure": lambda: hip.display_exposure(hist, params, E),
        "map": lambda: hip.display_map(lin, None, E, params, "aces", rgb8, rgb),
        "map_8bit_only": lambda: hip.display_map(lin, None, E, params, "aces", rgb8, None),
        "map_with_bloom": lambda: hip.display_map(lin, B, E, params, "aces", rgb8, rgb),
        "blur": lambda: hip.display_blur(lin, E, params, weights, scratch, B),
        "transform": lambda: metered.apply(lin),
        "transform_with_bloom": lambda: bloomed.apply(lin),
    }
    if transfer is not None and K == 1:
        T, exps, acc, lights, bg = transfer
        out_rgb, out_lin = torch.empty(1, H * W, 3, device=DEV), torch.empty(1, H * W, 3, device=DEV)
        passes["relight_fp16"] = lambda: hip.transfer_relight(T, exps, acc, lights, bg, out_rgb, out_lin)
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
    pixels = K * H * W
    line = {"measure": "display_1080p", "K": K, "iters": iters, "bloom_sigma": sigma, "bloom_radius": weights.numel() // 2,
            **{f"{k}_ms": round(v, 4) for k, v in med.items()}, **{f"{k}_min_ms": round(min(times[k]), 4) for k in times},
            **{f"{k}_over_clone": round(med[k] / med["clone"], 3) for k in med if k not in ("clone", "relight_fp16")},
            "clone_gbytes_per_s": round(pixels * 24 / med["clone"] / 1e6, 1), "histogram_gbytes_per_s": round(pixels * 12 / med["histogram"] / 1e6, 1),
            "map_gbytes_per_s": round(pixels * 27 / med["map"] / 1e6, 1), "exposures": [round(float(e), 6) for e in E.tolist()[:2]]}
    if "relight_fp16" in med:
        line.update({"relight_directions": transfer[0].shape[1], "relight_gbytes_per_s": round(transfer[0].numel() * 2 / med["relight_fp16"] / 1e6, 1),
                     "transform_over_relight": round(med["transform"] / med["relight_fp16"], 4),
                     "transform_within_a_tenth_of_the_relight": bool(med["transform"] <= 0.1 * med["relight_fp16"])})
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--directions", type=int, default=512, help="D of the synthetic transfer (a multiple of 8)")
    ap.add_argument("--sigma", type=float, default=4.0, help="of the bloom's blur")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_display: no GPU; timings are taken on the device only")
    transfer = synthetic_transfer(args.directions)
    for K in (1, 8):
        measure(K, args.iters, args.sigma, transfer)


if __name__ == "__main__":
    main()
