"""Relighting under a user-supplied HDR environment map: readers of equirectangular maps, the projection of a map onto the renderer's
light directions and the bilinear sky lookup on the GPU (csrc/envmap.hip), and the frame render with `envmap=`.

  python -m neusky_amd.relight --checkpoint CKPT --camera-path camera_path.json --output-dir frames/ --envmap sky.hdr
"""
from .cameras import CameraPath, camera_rays, load_camera_path
from .envmap import EnvironmentMap, envmap_labels, envmap_lookup, project_envmap, z_rotation
from .io import read_envmap, srgb_to_linear

__all__ = ["CameraPath", "EnvironmentMap", "camera_rays", "envmap_labels", "envmap_lookup", "load_camera_path", "project_envmap",
           "read_envmap", "srgb_to_linear", "z_rotation"]
