"""python -m neusky_amd.exporter --checkpoint CKPT --output mesh.ply: the SDF field of a checkpoint as a PLY mesh.

An --output ending in .obj writes a textured Wavefront OBJ instead (mesh.obj, mesh.mtl, mesh.png): the albedo baked into a
per-triangle-pair atlas on the mesh that is written, that is after --target-num-faces / --simplify-cell-size.
--keep-largest-components K / --min-component-faces N drop floaters (small connected components) from the marching-cubes mesh, before
any simplification.  The other flags carry the names of nerfstudio's `ns-export marching-cubes`.  The field is built from the `neusky` method's config; no
dataset is needed (the scene box and the number of training images come from the checkpoint)."""
from __future__ import annotations

import argparse
import sys
import time


def build_field(state, device):
    from ..configs.neusky_config import NeuSky
    cfg = NeuSky.config.pipeline.model.sdf_field
    aabb = state["_model.field.aabb"].float()
    emb = state.get("_model.field.embedding_appearance.weight", state.get("_model.field.embedding_appearance.embedding.weight"))
    num_images = int(emb.shape[0]) if emb is not None else 1
    return cfg.setup(aabb=aabb, num_images=num_images, spatial_distortion=None).to(device)


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m neusky_amd.exporter", description=__doc__.splitlines()[0])
    ap.add_argument("--checkpoint", required=True, help="a nerfstudio-layout checkpoint (step-*.ckpt) of the neusky method")
    ap.add_argument("--output", required=True, help="the .ply file to write, or a .obj file for a textured mesh (.obj, .mtl, .png)")
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--bounding-box-min", type=float, nargs=3, default=(-1.0, -1.0, -1.0))
    ap.add_argument("--bounding-box-max", type=float, nargs=3, default=(1.0, 1.0, 1.0))
    ap.add_argument("--isosurface-threshold", type=float, default=0.0)
    ap.add_argument("--no-attributes", action="store_true", help="write positions and faces only (no normals, no colours)")
    ap.add_argument("--device", default="cuda:0")
    simplify = ap.add_mutually_exclusive_group()
    simplify.add_argument("--target-num-faces", type=int, default=None, metavar="N",
                          help="simplify the mesh by vertex clustering to at most N faces (nerfstudio's --target-num-faces; off by default)")
    simplify.add_argument("--simplify-cell-size", type=float, default=None, metavar="H",
                          help="simplify the mesh by vertex clustering on cubic cells of edge H (scene units; off by default)")
    ap.add_argument("--keep-largest-components", type=int, default=None, metavar="K",
                    help="drop floaters: keep the K connected components with the most faces (before simplification; off by default)")
    ap.add_argument("--min-component-faces", type=int, default=None, metavar="N",
                    help="drop floaters: keep the connected components with at least N faces (with --keep-largest-components: both hold)")
    ap.add_argument("--px-per-uv-triangle", type=int, default=None, metavar="P",
                    help=".obj output: texels along a leg of each face's texture triangle (nerfstudio's --px-per-uv-triangle; default 4)")
    ap.add_argument("--texture-normal-map", action="store_true",
                    help=".obj output: also write <stem>_normal.png, the unit SDF gradient as an object-space normal map")
    return ap


def main(argv=None) -> int:
    ap = build_parser()
    args = ap.parse_args(argv)
    textured = args.output.lower().endswith(".obj")
    if not textured and (args.px_per_uv_triangle is not None or args.texture_normal_map):
        ap.error("--px-per-uv-triangle and --texture-normal-map need an --output ending in .obj")
    if args.px_per_uv_triangle is not None and args.px_per_uv_triangle < 1:
        ap.error("--px-per-uv-triangle must be >= 1")
    if args.keep_largest_components is not None and args.keep_largest_components < 1:
        ap.error("--keep-largest-components must be >= 1")
    if args.min_component_faces is not None and args.min_component_faces < 1:
        ap.error("--min-component-faces must be >= 1")

    import torch
    from . import bake_texture, extract_mesh, load_field_state, remove_floaters, simplify_mesh, write_obj, write_ply

    t0 = time.perf_counter()
    ckpt = torch.load(args.checkpoint, map_location="cpu", weights_only=False)
    state = ckpt["pipeline"] if "pipeline" in ckpt else ckpt
    field = build_field(state, args.device)
    loaded, unmapped = load_field_state(field, state)
    if not loaded:
        raise SystemExit(f"{args.checkpoint}: no _model.field.* entries")
    if unmapped:
        print(f"warning: {len(unmapped)} field entries not mapped: {unmapped[:4]}", file=sys.stderr)
    t_load = time.perf_counter() - t0
    timings = {}
    simplifying = args.target_num_faces is not None or args.simplify_cell_size is not None
    filtering = args.keep_largest_components is not None or args.min_component_faces is not None
    # with floater removal or simplification the attributes are evaluated once, on the vertices that are written
    mesh = extract_mesh(field, args.resolution, args.bounding_box_min, args.bounding_box_max, args.isosurface_threshold,
                        attributes=not args.no_attributes and not simplifying and not filtering, timings=timings)
    before = ""
    if filtering or simplifying:
        before = f"V {mesh.vertices.shape[0]} F {mesh.faces.shape[0]}"
    if filtering:
        t1 = time.perf_counter()
        found = {}
        mesh = remove_floaters(mesh, keep_largest=args.keep_largest_components, min_faces=args.min_component_faces, info=found)
        torch.cuda.synchronize()
        timings["components"] = time.perf_counter() - t1
        before += f", components {found['components']} -> {found['kept_components']}"
    if simplifying:
        t1 = time.perf_counter()
        mesh = simplify_mesh(mesh, cell_size=args.simplify_cell_size, target_num_faces=args.target_num_faces)
        torch.cuda.synchronize()
        timings["simplify"] = time.perf_counter() - t1
    if filtering or simplifying:
        before += " -> "
        if not args.no_attributes:
            from .mesh import vertex_attributes
            t1 = time.perf_counter()
            mesh.normals, mesh.colours = vertex_attributes(field, mesh.vertices)
            torch.cuda.synchronize()
            timings["attributes"] = time.perf_counter() - t1
    atlas, size = None, ""
    if textured and not args.no_attributes:
        t1 = time.perf_counter()
        atlas = bake_texture(mesh, field, px_per_uv_triangle=args.px_per_uv_triangle or 4, normal_map=args.texture_normal_map)
        torch.cuda.synchronize()
        timings["texture"] = time.perf_counter() - t1
        size = f" texture {atlas.image.shape[1]} x {atlas.image.shape[0]}"
    t1 = time.perf_counter()
    if textured:
        write_obj(args.output, mesh, atlas)
    else:
        write_ply(args.output, mesh)
    t_write = time.perf_counter() - t1
    parts = " ".join(f"{k} {v:.3f}s" for k, v in timings.items())
    print(f"{args.output}: {before}V {mesh.vertices.shape[0]} F {mesh.faces.shape[0]}{size} | load {t_load:.3f}s {parts} write {t_write:.3f}s")
    return 0


if __name__ == "__main__":
    sys.exit(main())
