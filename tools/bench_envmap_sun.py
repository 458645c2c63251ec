"""Sun-extraction timings (csrc/envmap_sun.hip) with HIP events after a warm-up, on a random sky with a small bright disc, at the map
size tools/bench_relight.py renders its frame under (4096 x 8192): the three entry points peak / ring / split, and a torch.clone of the
same map in the same process -- one read and one write of the map, the yardstick of the split's streamed copy.  The passes alternate
inside every iteration.  Prints one JSON line per map size; run on the GPU box:
    python tools/bench_envmap_sun.py [--sizes 4096] [--iters 20] [--radius-deg 2.5]"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from neusky_amd import hip  # noqa: E402
from neusky_amd.relight import EnvironmentMap, extract_sun  # noqa: E402

DEV = "cuda:0"


def sunny_map(H, seed=0):
    """a uniform random sky and a 9 x 9 texel patch of radiance 5e4 at 40 degrees of elevation"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    data = torch.rand(H, 2 * H, 3, device=DEV, generator=g)
    i, j = int(H * 50.0 / 180.0), int(2 * H * 0.3)
    data[i - 4:i + 5, j - 4:j + 5] = 5.0e4
    return EnvironmentMap(data, "blender")


def measure(H, iters, radius_deg, ratio=10.0):
    env = sunny_map(H)
    data, conv, rho = env.data, env.convention_id, math.radians(radius_deg)
    scratch = torch.empty(hip.ENVMAP_SUN_SCRATCH_BYTES // 8, dtype=torch.float64, device=DEV)
    peak = torch.empty(2, dtype=torch.int64, device=DEV)
    ring, stats = torch.empty(2, dtype=torch.float64, device=DEV), torch.empty(12, dtype=torch.float64, device=DEV)
    residual = torch.empty_like(data)
    passes = {"peak": lambda: hip.envmap_peak(data, conv, scratch, peak),
              "ring": lambda: hip.envmap_sun_ring(data, conv, peak, rho, scratch, ring),
              "split": lambda: hip.envmap_sun_split(data, conv, peak, ring, rho, ratio, scratch, residual, stats),
              "clone": lambda: data.clone()}
    for _ in range(3):
        for fn in passes.values():
            fn()
    torch.cuda.synchronize()
    assert stats[9].item() == 1.0, "the benchmark's sun was not found"
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
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    nbytes = data.numel() * 4
    ext = extract_sun(env, radius_deg=radius_deg, min_peak_ratio=ratio)
    print(json.dumps({"measure": "envmap_sun", "map": [H, 2 * H], "map_bytes": nbytes, "radius_deg": radius_deg, "iters": iters,
                      **{f"{k}_ms": round(v, 4) for k, v in med.items()}, **{f"{k}_min_ms": round(min(times[k]), 4) for k in times},
                      "three_passes_ms": round(med["peak"] + med["ring"] + med["split"], 4),
                      "split_over_clone": round(med["split"] / med["clone"], 3),
                      "three_passes_over_clone": round((med["peak"] + med["ring"] + med["split"]) / med["clone"], 3),
                      "clone_gbytes_per_s": round(2 * nbytes / med["clone"] / 1e6, 1), "split_gbytes_per_s": round(2 * nbytes / med["split"] / 1e6, 1),
                      "peak_gbytes_per_s": round(nbytes / 2 / med["peak"] / 1e6, 1),
                      "found": ext.found, "flux_fraction": round(ext.flux_fraction, 4), "sun_diameter_deg": round(ext.angular_diameter_deg, 3)}),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096], help="map heights (width = 2 x height)")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--radius-deg", type=float, default=2.5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_envmap_sun: no GPU; timings are taken on the device only")
    for H in args.sizes:
        measure(H, args.iters, args.radius_deg)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
