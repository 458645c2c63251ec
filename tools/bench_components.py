"""Mesh-component timing (exporter/components.py) next to two yardsticks: marching_cubes of the volume the mesh came from, and a
torch.clone of its face array (the cheapest pass over the faces there is).  Two volumes per resolution: an analytic one with one
large body and many small ones (a big sphere among a lattice of small spheres), and a random one (thousands of crumbs around one
sponge).  In one process the calls alternate -- marching_cubes, clone, label_components, remove_floaters, again -- and each is timed
on its own with HIP events; medians of --reps rounds after a warm-up round.  Then, alternating in the same way, the parts of
label_components: the index and box check before the launches (simplify._box: two aminmax reductions and a host read), the link
kernel, the flatten kernel, and the torch ranking (unique with counts, sort, scatter, two gathers).
Prints one JSON line per volume; run on the GPU box:
    python tools/bench_components.py [--resolutions 512] [--reps 20]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from neusky_amd import hip  # noqa: E402
from neusky_amd.exporter import Mesh, label_components, marching_cubes, remove_floaters  # noqa: E402
from neusky_amd.exporter.simplify import _box  # noqa: E402

DEV = "cuda:0"


def bodies_volume(n, lattice=12):
    """one sphere of radius 0.45 at the centre and lattice^3 small spheres on a grid, those inside or near the large one left out"""
    x = torch.linspace(-1.0, 1.0, n, device=DEV)
    c = (torch.arange(lattice, device=DEV, dtype=torch.float32) + 0.5) / lattice * 2.0 - 1.0
    r = 0.3 / lattice
    near = lambda t: (t[:, None] - c[None, :]).abs().min(dim=1).values  # noqa: E731  (per axis: distance to the nearest lattice centre)
    out = torch.empty(n, n, n, device=DEV)
    nx, ny, nz = near(x), near(x), near(x)
    for i in range(n):  # a slab at a time: no [n, n, n, 3] temporaries
        small = torch.sqrt(nx[i] ** 2 + ny[:, None] ** 2 + nz[None, :] ** 2) - r
        big = torch.sqrt(x[i] ** 2 + x[:, None] ** 2 + x[None, :] ** 2) - 0.45
        small = torch.where(big < 3.0 * r, torch.full_like(small, 1.0), small)
        out[i] = torch.minimum(big, small)
    return out


def random_volume(n):
    return torch.randn(n, n, n, generator=torch.Generator().manual_seed(0)).to(DEV)


def alternating(fns, reps):
    """{name: [median, min, max] ms}: the calls in turn, `reps` rounds after one warm-up round, each call between its own events"""
    ms = {k: [] for k in fns}
    for rnd in range(reps + 1):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if rnd:
                ms[name].append(e0.elapsed_time(e1))
    return {k: [round(sorted(v)[len(v) // 2], 3), round(min(v), 3), round(max(v), 3)] for k, v in ms.items()}


def parts(mesh):
    """closures for the link kernel, the flatten kernel and the torch ranking of label_components, on prepared inputs"""
    v, f = mesh.vertices, mesh.faces
    V, F = v.shape[0], f.shape[0]
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    linked = torch.arange(V, dtype=torch.int32, device=DEV)
    hip.cc_link(f, linked, status)
    vertex_root = torch.empty(V, dtype=torch.int32, device=DEV)
    face_root = torch.empty(F, dtype=torch.int32, device=DEV)
    hip.cc_flatten(linked, f, vertex_root, face_root, status)
    fresh = torch.empty_like(linked)

    def link():
        torch.arange(V, dtype=torch.int32, device=DEV, out=fresh)
        hip.cc_link(f, fresh, status)

    def rank():
        roots, counts = torch.unique(face_root, return_counts=True)
        order = torch.argsort((F - counts) * (1 << 31) + roots)
        table = torch.full((V,), -1, dtype=torch.int32, device=DEV)
        table[roots[order].long()] = torch.arange(roots.shape[0], dtype=torch.int32, device=DEV)
        return table.index_select(0, vertex_root), table.index_select(0, face_root)

    return {"index_and_box_check": lambda: _box(v, f, "bench_components"), "link_kernel_with_arange": link,
            "flatten_kernel": lambda: hip.cc_flatten(linked, f, vertex_root, face_root, status), "torch_ranking": rank}, status


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolutions", type=int, nargs="+", default=[512])
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    lo, hi = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
    for res in args.resolutions:
        for name, make in (("bodies", bodies_volume), ("random", random_volume)):
            vol = make(res)
            v, f = marching_cubes(vol, 0.0, lo, hi)
            mesh = Mesh(v, f)
            comps, info = label_components(mesh), {}
            remove_floaters(mesh, keep_largest=1, info=info)
            calls = alternating({"marching_cubes": lambda: marching_cubes(vol, 0.0, lo, hi), "clone_faces": lambda: f.clone(),
                                 "label_components": lambda: label_components(mesh),
                                 "remove_floaters": lambda: remove_floaters(mesh, keep_largest=1)}, args.reps)
            part_fns, status = parts(mesh)
            inner = alternating(part_fns, args.reps)
            assert int(status.item()) == 0
            print(json.dumps({"volume": name, "resolution": res, "vertices": v.shape[0], "faces": f.shape[0],
                              "components": comps.num_components, "largest": info["largest"], "faces_after": info["faces_after"],
                              "ms_median_min_max": calls, "label_components_parts_ms": inner,
                              "label_over_marching_cubes": round(calls["label_components"][0] / calls["marching_cubes"][0], 3),
                              "remove_over_marching_cubes": round(calls["remove_floaters"][0] / calls["marching_cubes"][0], 3),
                              "label_over_clone": round(calls["label_components"][0] / calls["clone_faces"][0], 1),
                              "remove_over_clone": round(calls["remove_floaters"][0] / calls["clone_faces"][0], 1),
                              "reps": args.reps, "device": torch.cuda.get_device_name(0)}), flush=True)
            del vol, v, f, mesh, comps
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
