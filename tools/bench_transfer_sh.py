"""Timings of the transfer in a spherical-harmonic basis at 1920 x 1080 and D = 512 light directions, for orders 2, 5 and 8 with T and C
in fp32 and in scaled fp16 (random contents: the kernels' time does not depend on them), in one run on one box:
  the projection of one 4096-row chunk (what bake_transfer_sh adds to each chunk of a bake);
  the projection of a full dense frame, against a torch copy of T's bytes;
  the relight of coefficient rows (nsky_transfer_relight_short) for K = 1 and K = 8, against nsky_transfer_relight on the same C with
  D := J, against a torch copy of C's bytes, and against the dense relight of the same frame from T;
  the bytes of C against the bytes of T.
Every timing is the median of --runs (20) runs between HIP events, the alternatives of a comparison taking turns in one process.
Prints one JSON line per measurement; run on the GPU box:
    python tools/bench_transfer_sh.py [--runs 20] [--orders 2 5 8] [--storages fp32 fp16]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from neusky_amd import hip  # noqa: E402
from neusky_amd.model_components.illumination import antipodal_sphere  # noqa: E402
from neusky_amd.relight import light_basis  # noqa: E402

DEV = "cuda:0"
R, D, CHUNK = 1920 * 1080, 512, 4096


def alternate(fns, runs):
    """{name: median ms} of `runs` rounds in which every fn runs once, in turn, each between two HIP events"""
    for fn in fns.values():
        fn()
    pairs = {name: [] for name in fns}
    for _ in range(runs):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            pairs[name].append((e0, e1))
    torch.cuda.synchronize()
    return {name: statistics.median(a.elapsed_time(b) for a, b in ev) for name, ev in pairs.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--orders", type=int, nargs="+", default=[2, 5, 8])
    ap.add_argument("--storages", nargs="+", default=["fp32", "fp16"], choices=("fp32", "fp16"))
    args = ap.parse_args()
    g = torch.Generator(device=DEV).manual_seed(0)
    dirs = antipodal_sphere(D).to(DEV)
    acc = torch.rand(R, device=DEV, generator=g)
    for storage in args.storages:
        half = storage == "fp16"
        dtype = torch.float16 if half else torch.float32
        T = torch.rand(R, D, 3, device=DEV, generator=g, dtype=dtype)
        exps = torch.randint(0, 12, (R,), dtype=torch.int32, device=DEV) if half else None
        T_copy = torch.empty_like(T)
        for K in (1, 8):  # the dense relight of the frame
            lights = torch.rand(K, D, 3, device=DEV, generator=g)
            bg = torch.rand(K, R, 3, device=DEV, generator=g)
            rgb = torch.empty(K, R, 3, device=DEV)
            ms = alternate({"dense": lambda: hip.transfer_relight(T, exps, acc, lights, bg, rgb, None)}, args.runs)["dense"]
            print(json.dumps({"measure": "dense_relight", "storage": storage, "K": K, "ms": round(ms, 4),
                              "transfer_TB_per_s": round(T.numel() * T.element_size() / (ms * 1e-3) / 1e12, 3)}), flush=True)
            del lights, bg, rgb
        for order in args.orders:
            Q = light_basis(dirs, order)
            J = Q.shape[1]
            C = torch.empty(R, J, 3, device=DEV, dtype=dtype)
            cexps = torch.empty(R, dtype=torch.int32, device=DEV) if half else None
            t_bytes, c_bytes = T.numel() * T.element_size(), C.numel() * C.element_size()
            Tc, ec = T[:CHUNK], None if exps is None else exps[:CHUNK]
            ms = alternate({"chunk": lambda: hip.transfer_project(Tc, ec, Q, C, 0, cexps),
                            "frame": lambda: hip.transfer_project(T, exps, Q, C, 0, cexps),
                            "copy": lambda: T_copy.copy_(T)}, args.runs)
            print(json.dumps({"measure": "project", "storage": storage, "order": order, "J": J, "chunk_rows": CHUNK,
                              "chunk_ms": round(ms["chunk"], 4), "frame_ms": round(ms["frame"], 3), "torch_copy_of_T_ms": round(ms["copy"], 3),
                              "frame_over_copy": round(ms["frame"] / ms["copy"], 3), "T_bytes": t_bytes, "C_bytes": c_bytes,
                              "T_over_C": round(t_bytes / c_bytes, 2)}), flush=True)
            C_copy = torch.empty_like(C)
            for K in (1, 8):
                l = torch.rand(K, J, 3, device=DEV, generator=g)  # noqa: E741
                bg = torch.rand(K, R, 3, device=DEV, generator=g)
                rgb = torch.empty(K, R, 3, device=DEV)
                ms = alternate({"short": lambda: hip.transfer_relight_short(C, cexps, acc, l, bg, rgb, None),
                                "existing": lambda: hip.transfer_relight(C, cexps, acc, l, bg, rgb, None),
                                "copy": lambda: C_copy.copy_(C)}, args.runs)
                print(json.dumps({"measure": "relight_short", "storage": storage, "order": order, "J": J, "K": K,
                                  "short_ms": round(ms["short"], 4), "existing_kernel_ms": round(ms["existing"], 4),
                                  "torch_copy_of_C_ms": round(ms["copy"], 4), "existing_over_short": round(ms["existing"] / ms["short"], 3),
                                  "C_TB_per_s": round(c_bytes / (ms["short"] * 1e-3) / 1e12, 3)}), flush=True)
                del l, bg, rgb
            del C, C_copy, cexps
        del T, T_copy, exps


if __name__ == "__main__":
    main()
