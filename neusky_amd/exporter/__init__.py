"""Mesh export of the learned surface: a dense SDF grid from the field's fused value chain, marching cubes on the GPU
(csrc/mesh.hip), per-vertex normals and albedo from the field, connected components and the removal of floaters
(csrc/components.hip), simplification by quadric vertex clustering (csrc/simplify.hip), a binary PLY writer, and -- the stage after simplification -- the albedo baked into a per-triangle-pair texture atlas (csrc/texture.hip) with an
OBJ + MTL + PNG writer.

  python -m neusky_amd.exporter --checkpoint CKPT --output mesh.ply   (flags named as nerfstudio's `ns-export marching-cubes`)
  python -m neusky_amd.exporter --checkpoint CKPT --output mesh.obj --target-num-faces 100000   (textured: mesh.obj, mesh.mtl, mesh.png)
"""
from .components import MeshComponents, label_components, remove_floaters
from .marching_cubes import marching_cubes
from .mesh import Mesh, extract_mesh, load_field_state, sdf_grid
from .ply import write_ply
from .simplify import cluster_face_count, simplify_mesh
from .texture import TextureAtlas, atlas_layout, bake_texture, face_uvs, texel_points, write_obj

__all__ = ["Mesh", "MeshComponents", "TextureAtlas", "atlas_layout", "bake_texture", "cluster_face_count", "extract_mesh", "face_uvs",
           "label_components", "load_field_state", "marching_cubes", "remove_floaters", "sdf_grid", "simplify_mesh", "texel_points",
           "write_obj", "write_ply"]
