"""Equirectangular environment maps on the device, their projection onto the renderer's light directions and the sky lookup
(csrc/envmap.hip; the definitions are in include/neusky_hip.h).

The renderer treats its D light directions as point samples of radiance.  A map is therefore projected first: each texel belongs to
the cell of the direction nearest to it, and each direction takes the solid-angle-weighted mean of its cell.  Point samples of an
HDRI would miss a small sun almost always and, when one landed on it, make it thousands of times too bright."""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple, Union

import numpy as np
import torch

from .. import hip
from .io import read_envmap

CONVENTIONS = {"neusky": hip.ENVMAP_NEUSKY, "blender": hip.ENVMAP_BLENDER}


class EnvironmentMap:
    """An equirectangular map of linear radiance on the device: `data` fp32 [H, W, 3], row 0 at the top (polar angle from +z).

    convention: how a column maps to the azimuth phi (from +x toward +y), u = (j + 0.5) / W:
      "blender" (default): phi = pi - 2 pi u, Blender's world-texture mapping;
      "neusky":            phi = 2 pi u.
    Which one the reference's HDRIs were authored in is not pinned (the generator is not available); "blender" is the default.
    exposure: a scalar multiplying every colour the map gives.  It lives in device memory, so changing it needs no graph recapture."""

    def __init__(self, data: Union[torch.Tensor, np.ndarray], convention: str = "blender", exposure: float = 1.0,
                 device: Union[str, torch.device] = "cuda"):
        if convention not in CONVENTIONS:
            raise ValueError(f"EnvironmentMap: convention must be one of {sorted(CONVENTIONS)}, got {convention!r}")
        t = torch.as_tensor(data)
        if t.dim() != 3 or t.shape[2] not in (3, 4) or t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError(f"EnvironmentMap: expected [H, W, 3] or [H, W, 4], got {tuple(t.shape)}")
        self.data = t[..., :3].to(device=device, dtype=torch.float32).contiguous()
        if not self.data.is_cuda:
            raise ValueError("EnvironmentMap: the map must live on a GPU (the kernels run on the device only)")
        self.convention = convention
        self._exposure = torch.empty(1, dtype=torch.float32, device=self.data.device)
        self.exposure = exposure

    @classmethod
    def from_file(cls, path, convention: str = "blender", exposure: float = 1.0, device: Union[str, torch.device] = "cuda") -> "EnvironmentMap":
        """.hdr / .pic (RGBE), .pfm, .npy ([H, W, 3|4]), .png / .jpg (8-bit sRGB, linearised), .exr (needs pyexr)"""
        return cls(read_envmap(path), convention, exposure, device)

    @property
    def exposure(self) -> float:
        return self._exposure_value

    @exposure.setter
    def exposure(self, value: float) -> None:
        value = float(value)
        if not math.isfinite(value):
            raise ValueError(f"EnvironmentMap: exposure {value} is not finite")
        self._exposure_value = value
        self._exposure.fill_(value)

    @property
    def exposure_tensor(self) -> torch.Tensor:
        """fp32 [1] in device memory: what the kernels read"""
        return self._exposure

    @property
    def convention_id(self) -> int:
        return CONVENTIONS[self.convention]

    @property
    def shape(self) -> Tuple[int, int]:
        return int(self.data.shape[0]), int(self.data.shape[1])

    @property
    def device(self) -> torch.device:
        return self.data.device

    def __repr__(self) -> str:
        H, W = self.shape
        return f"EnvironmentMap({H}x{W}, convention={self.convention!r}, exposure={self.exposure:g}, device={self.device})"


def z_rotation(angle_rad: float) -> torch.Tensor:
    """fp32 [3, 3] rotation about +z by angle_rad, the matrix the `rotation=` arguments take (direction d is lit by the map at R d).

    With an environment map and angle = 2 pi m / W, rendering with this rotation equals rendering the column-rolled map without one:
      convention "neusky":  np.roll(map, -m, axis=1)   (the map turns toward +phi: column j shows the old column j + m)
      convention "blender": np.roll(map, +m, axis=1)   (Blender's azimuth runs against the column index)"""
    c, s = math.cos(angle_rad), math.sin(angle_rad)
    return torch.tensor([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float32)


def _directions(directions: torch.Tensor, dev, name: str) -> torch.Tensor:
    d = torch.as_tensor(directions)
    if d.dim() != 2 or d.shape[1] != 3:
        raise ValueError(f"{name}: directions must be [N, 3], got {tuple(d.shape)}")
    return d.detach().to(device=dev, dtype=torch.float32).contiguous()


def _rotation(rotation, dev) -> Optional[torch.Tensor]:
    if rotation is None:
        return None
    r = torch.as_tensor(rotation)
    if r.shape != (3, 3):
        raise ValueError(f"rotation must be [3, 3], got {tuple(r.shape)}")
    return r.detach().to(device=dev, dtype=torch.float32).contiguous()


def _check_d(D: int, name: str) -> None:
    if not 1 <= D <= hip.ENVMAP_MAX_DIRECTIONS:
        raise ValueError(f"{name}: {D} directions; the projection takes 1..{hip.ENVMAP_MAX_DIRECTIONS}")


def envmap_labels(envmap: EnvironmentMap, directions: torch.Tensor, rotation=None) -> torch.Tensor:
    """int16 [H, W]: the cell of every texel, argmax_k <t, R d_k> with ties to the lower k (fp32, one fixed expression order)"""
    dirs = _directions(directions, envmap.device, "envmap_labels")
    _check_d(dirs.shape[0], "envmap_labels")
    H, W = envmap.shape
    labels = torch.empty(H, W, dtype=torch.int16, device=envmap.device)
    with torch.cuda.device(envmap.device):
        hip.envmap_label(dirs, _rotation(rotation, envmap.device), H, W, envmap.convention_id, labels)
    return labels


def project_envmap(envmap: EnvironmentMap, directions: torch.Tensor, rotation=None,
                   timings: Optional[Dict[str, torch.cuda.Event]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The map's cell averages at the D light directions: (colours fp32 [D, 3], cell_weight fp32 [D]).

    colours_k = exposure * sum_{label(t)=k} omega_t L_t / sum_{label(t)=k} omega_t (a cell without a texel centre -- a map too coarse
    for D -- takes the bilinear lookup at R d_k); cell_weight_k = sum_{label(t)=k} omega_t, the cell's solid angle (0 when empty).
    Three steps: label every texel (HIP), group texels by label with a stable sort, reduce each cell in a fixed order (HIP); the
    result is bitwise repeatable.  Extra device memory: about 30 bytes per texel while it runs.  No host synchronisation.
    timings: when given, CUDA events "start", "label", "group", "reduce" are recorded into it."""
    dev = envmap.device
    dirs = _directions(directions, dev, "project_envmap")
    D = dirs.shape[0]
    _check_d(D, "project_envmap")
    rot = _rotation(rotation, dev)
    H, W = envmap.shape

    def mark(name):
        if timings is not None:
            timings[name] = torch.cuda.Event(enable_timing=True)
            timings[name].record()

    with torch.cuda.device(dev):
        mark("start")
        labels = torch.empty(H * W, dtype=torch.int16, device=dev)
        hip.envmap_label(dirs, rot, H, W, envmap.convention_id, labels)
        mark("label")
        sorted_labels, order = torch.sort(labels, stable=True)
        del labels
        mark("group")
        colours = torch.empty(D, 3, dtype=torch.float32, device=dev)
        cell_weight = torch.empty(D, dtype=torch.float32, device=dev)
        hip.envmap_reduce(envmap.data, envmap.convention_id, dirs, rot, envmap.exposure_tensor, sorted_labels, order, colours, cell_weight)
        mark("reduce")
    return colours, cell_weight


def envmap_lookup(envmap: EnvironmentMap, directions: torch.Tensor, rotation=None) -> torch.Tensor:
    """fp32 [N, 3]: the map at R d for each direction d (any length), bilinear (columns wrap, rows clamp), times the exposure --
    the sky behind a camera ray"""
    dev = envmap.device
    dirs = _directions(directions, dev, "envmap_lookup")
    out = torch.empty(dirs.shape[0], 3, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        hip.envmap_lookup(envmap.data, envmap.convention_id, dirs, _rotation(rotation, dev), envmap.exposure_tensor, out)
    return out
