"""Texture-bake timing on a checkpoint's field or on bench.py's randomised one: a mesh is extracted (at the level of the median grid
value for the randomised field, so that the surface crosses the box), simplified to the face budget, and its atlas baked at P texels
per triangle leg.  The three parts of the bake are timed separately with HIP events, summed over the chunks of one bake, median of
--reps bakes after a warm-up: the texel-points kernel, the field evaluation (field.field_values, the fused chain) and the
texel-store kernel; then bake_texture as a whole, and the host side on the wall clock: the PNG alone and write_obj (OBJ + MTL +
PNG).  Prints one JSON line per face budget; run on the GPU box:
    python tools/bench_texture.py [--checkpoint CKPT] [--faces 100000 400000] [--px-per-uv-triangle 4] [--resolution 256]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from neusky_amd import hip  # noqa: E402
from neusky_amd.exporter import atlas_layout, bake_texture, extract_mesh, load_field_state, sdf_grid, simplify_mesh, write_obj  # noqa: E402
from neusky_amd.exporter import texture  # noqa: E402
from neusky_amd.exporter.mesh import refresh_field  # noqa: E402


def load_field(args, dev):
    if args.checkpoint:
        from neusky_amd.exporter.__main__ import build_field
        ckpt = torch.load(args.checkpoint, map_location="cpu", weights_only=False)
        state = ckpt["pipeline"] if "pipeline" in ckpt else ckpt
        field = build_field(state, dev)
        load_field_state(field, state)
        return field, args.isosurface_threshold
    import bench
    from neusky_amd.utils.randomise import randomise
    pipe = bench.build_pipeline(dev, 1, 0)
    randomise(pipe)
    field = pipe.model.field
    return field, float(sdf_grid(field, 65).median())


def bake_parts(mesh, field, P, normal_map, chunk):
    """one bake, its three parts under HIP events: milliseconds of (texel points, field evaluation, texel store) over all chunks"""
    v, f = mesh.vertices, mesh.faces
    F = f.shape[0]
    W, S, Q = atlas_layout(F, P)
    image = torch.zeros(W, W, 3, dtype=torch.uint8, device=v.device)
    normal_image = torch.zeros_like(image) if normal_map else None
    refresh_field(field)
    n_sq, step = (F + 1) // 2, max(1, chunk // (Q * Q))
    marks = []
    for s0 in range(0, n_sq, step):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record()
        owner, offset, points = texture._points(v, f, P, S, Q, s0, min(s0 + step, n_sq))
        e[1].record()
        _, grad, rgb = field.field_values(points, want_albedo=True)
        e[2].record()
        hip.texture_texel_store(rgb.reshape(-1, 3), grad.reshape(-1, 3), owner, offset, image, normal_image)
        e[3].record()
        marks.append(e)
    torch.cuda.synchronize()
    return [sum(e[k].elapsed_time(e[k + 1]) for e in marks) for k in range(3)]


def wall(fn, reps):
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3)
    return round(statistics.median(ms), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--checkpoint", default=None, help="a checkpoint of the neusky method (default: bench.py's randomised field)")
    ap.add_argument("--isosurface-threshold", type=float, default=0.0, help="with --checkpoint (the randomised field uses its median)")
    ap.add_argument("--faces", type=int, nargs="+", default=[100000], help="face budgets (simplify_mesh target_num_faces)")
    ap.add_argument("--px-per-uv-triangle", type=int, default=4)
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--normal-map", action="store_true")
    ap.add_argument("--chunk", type=int, default=texture.CHUNK)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    dev = "cuda:0"
    field, level = load_field(args, dev)
    full = extract_mesh(field, args.resolution, isosurface_threshold=level, attributes=False)
    P = args.px_per_uv_triangle
    for budget in args.faces:
        mesh = simplify_mesh(full, target_num_faces=budget, field=field)
        F = mesh.faces.shape[0]
        W, S, Q = atlas_layout(F, P)
        bake_parts(mesh, field, P, args.normal_map, args.chunk)  # warm-up
        parts = [bake_parts(mesh, field, P, args.normal_map, args.chunk) for _ in range(args.reps)]
        points_ms, field_ms, store_ms = (statistics.median(p[k] for p in parts) for k in range(3))
        bake_ms = wall(lambda: bake_texture(mesh, field, px_per_uv_triangle=P, normal_map=args.normal_map, chunk=args.chunk), args.reps)
        atlas = bake_texture(mesh, field, px_per_uv_triangle=P, normal_map=args.normal_map, chunk=args.chunk)
        with tempfile.TemporaryDirectory() as tmp:
            png_ms = wall(lambda: texture._png(os.path.join(tmp, "only.png"), atlas.image), 3)
            obj_ms = wall(lambda: write_obj(os.path.join(tmp, "mesh.obj"), mesh, atlas), 3)
        kernels = points_ms + store_ms
        print(json.dumps({"faces_before": full.faces.shape[0], "budget": budget, "faces": F, "vertices": mesh.vertices.shape[0],
                          "px_per_uv_triangle": P, "texture": W, "texels": (F + 1) // 2 * Q * Q, "normal_map": args.normal_map,
                          "texel_points_ms": round(points_ms, 3), "field_values_ms": round(field_ms, 3), "texel_store_ms": round(store_ms, 3),
                          "new_kernels_share_of_bake": round(kernels / (kernels + field_ms), 4), "bake_texture_ms": bake_ms,
                          "png_ms": png_ms, "write_obj_ms": obj_ms, "device": torch.cuda.get_device_name(0)}), flush=True)


if __name__ == "__main__":
    main()
