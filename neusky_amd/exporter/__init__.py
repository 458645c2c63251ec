"""Mesh export of the learned surface: a dense SDF grid from the field's fused value chain, marching cubes on the GPU
(csrc/mesh.hip), per-vertex normals and albedo from the field, simplification by quadric vertex clustering (csrc/simplify.hip), and a binary PLY
writer.

  python -m neusky_amd.exporter --checkpoint CKPT --output mesh.ply   (flags named as nerfstudio's `ns-export marching-cubes`)
"""
from .marching_cubes import marching_cubes
from .mesh import Mesh, extract_mesh, load_field_state, sdf_grid
from .ply import write_ply
from .simplify import cluster_face_count, simplify_mesh

__all__ = ["Mesh", "cluster_face_count", "extract_mesh", "load_field_state", "marching_cubes", "sdf_grid", "simplify_mesh", "write_ply"]
