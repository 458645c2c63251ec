"""nerfstudio camera-path files (`camera_path.json` of the viewer / `ns-render camera-path`) and the pinhole rays of their poses."""
from __future__ import annotations

import json
import math
from dataclasses import dataclass
from typing import List

import torch

from ..cameras.rays import RayBundle


@dataclass
class CameraPath:
    width: int
    height: int
    camera_to_world: torch.Tensor  # [N, 3, 4] fp32 (OpenGL convention: the camera looks down its -z axis, +y up)
    fov: torch.Tensor              # [N] vertical field of view in degrees

    def __len__(self) -> int:
        return int(self.camera_to_world.shape[0])

    def focal(self, i: int) -> float:
        """fx = fy = 0.5 H / tan(fov / 2), the viewer's perspective camera"""
        return 0.5 * self.height / math.tan(math.radians(float(self.fov[i])) / 2.0)


def load_camera_path(path) -> CameraPath:
    """render_width, render_height, camera_type "perspective", camera_path[*].camera_to_world (16 floats, row-major) and .fov"""
    with open(path) as f:
        d = json.load(f)
    kind = d.get("camera_type", "perspective")
    if kind != "perspective":
        raise ValueError(f"{path}: camera_type {kind!r} is not supported (only 'perspective')")
    cams = d.get("camera_path")
    if not cams:
        raise ValueError(f"{path}: no camera_path entries")
    c2w: List[torch.Tensor] = []
    fov: List[float] = []
    for i, c in enumerate(cams):
        m = torch.tensor(c["camera_to_world"], dtype=torch.float64).reshape(-1)
        if m.numel() != 16:
            raise ValueError(f"{path}: camera_path[{i}].camera_to_world has {m.numel()} values, not 16")
        c2w.append(m.reshape(4, 4)[:3])
        fov.append(float(c.get("fov", d.get("default_fov", 50.0))))
    return CameraPath(int(d["render_width"]), int(d["render_height"]), torch.stack(c2w).float(), torch.tensor(fov, dtype=torch.float32))


def camera_rays(path: CameraPath, i: int, device="cuda:0", camera_index: int = 0) -> RayBundle:
    """the [H, W] ray bundle of pose i: DeviceImageDataManager.generate_rays' pinhole with the principal point at the centre
    (cx = W / 2, cy = H / 2): d = R ((x + 0.5 - cx) / fx, -(y + 0.5 - cy) / fy, -1), normalised, directions_norm = |d|"""
    H, W = path.height, path.width
    f = path.focal(i)
    c2w = path.camera_to_world[i].to(device)
    y, x = torch.meshgrid(torch.arange(H, device=device, dtype=torch.float32), torch.arange(W, device=device, dtype=torch.float32),
                          indexing="ij")
    d_cam = torch.stack([(x + 0.5 - 0.5 * W) / f, -(y + 0.5 - 0.5 * H) / f, -torch.ones_like(x)], -1)
    d = d_cam @ c2w[:, :3].T
    norm = d.norm(dim=-1, keepdim=True)
    return RayBundle(origins=c2w[:, 3].expand(H, W, 3).contiguous(), directions=(d / norm).contiguous(),
                     pixel_area=torch.full((H, W, 1), 1.0 / (f * f), device=device),
                     camera_indices=torch.full((H, W, 1), int(camera_index), dtype=torch.long, device=device),
                     metadata={"directions_norm": norm})
