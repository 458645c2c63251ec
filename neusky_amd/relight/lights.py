"""Point and spot lights inside the scene: `PointLight`, the device block of L of them, and their shadow march, `trace_visibility_to`,
the primitive beside `trace_visibility`.  Definitions and rules: include/neusky_hip.h; kernels: csrc/lights.hip and the bounded step of
csrc/sphere_trace.hip.

Every other light of the frame render is at infinity.  A lamp has a direction and a distance of its own at every sample (inverse-square
falloff with a floor, an optional smoothstep cone), and its shadow ray ends at the lamp: geometry behind the lamp does not shadow it.
A spherical source of radius `radius` gives a penumbra by the closest-approach estimate of relight.shadows with the tangent
radius / distance of each ray's own.  The L lamps of a frame add into one image; each one is a whole march, so a frame takes at most
MAX_LIGHTS.  The defaults of `clearance` and `min_distance`, like the march's, are design choices, not measurements."""
from __future__ import annotations

import json
import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple, Union

import torch

from .. import hip
from .shadows import SHADOW_DEFAULTS, SphereTrace, _march, _start, trace_params, trace_settings

MAX_LIGHTS = 64
# the march towards a lamp: the sun's, but the penumbra's width is the lamp's radius over each ray's length, not an angular diameter
LIGHT_TRACE_DEFAULTS = {k: v for k, v in SHADOW_DEFAULTS.items() if k != "angular_diameter_deg"}
_KEYS = ("position", "intensity", "radius", "direction", "inner_deg", "outer_deg", "clearance", "min_distance")


def _vec3(name: str, v) -> Tuple[float, float, float]:
    try:
        out = tuple(float(x) for x in v)
    except TypeError:
        raise ValueError(f"a light's {name} has 3 numbers, got {v!r}") from None
    if len(out) != 3 or not all(math.isfinite(x) for x in out):
        raise ValueError(f"a light's {name} has 3 finite numbers, got {v!r}")
    return out


@dataclass(frozen=True)
class PointLight:
    """position: [3], scene units.  intensity: I [3], the colour a SunLight would need to light a facing surface as this lamp does from
    distance 1 (irradiance units times scene units squared).  radius: of the spherical source; 0 gives a hard shadow.  direction with
    0 <= inner_deg <= outer_deg <= 180 (half-angles of the cone about it: full light inside inner, none outside outer, a smoothstep of
    the cosine between) makes it a spot.  clearance: the shadow ray ends this far in front of the lamp (default max(radius, 0.02)).
    min_distance: the floor of the inverse-square law (default max(radius, 0.01))."""
    position: Tuple[float, float, float]
    intensity: Tuple[float, float, float]
    radius: float = 0.0
    direction: Optional[Tuple[float, float, float]] = None
    inner_deg: Optional[float] = None
    outer_deg: Optional[float] = None
    clearance: Optional[float] = None
    min_distance: Optional[float] = None

    def __post_init__(self):
        set_ = lambda k, v: object.__setattr__(self, k, v)  # noqa: E731
        set_("position", _vec3("position", self.position))
        set_("intensity", _vec3("intensity", self.intensity))
        radius = float(self.radius)
        if not (math.isfinite(radius) and radius >= 0.0):
            raise ValueError(f"a light's radius is finite and >= 0, got {self.radius!r}")
        set_("radius", radius)
        if self.direction is None:
            if self.inner_deg is not None or self.outer_deg is not None:
                raise ValueError("inner_deg and outer_deg shape a spot's cone: they need a direction")
        else:
            d = _vec3("direction", self.direction)
            n = math.sqrt(sum(x * x for x in d))
            if not n > 0.0:
                raise ValueError(f"a spot's direction has a length above zero, got {self.direction!r}")
            set_("direction", tuple(x / n for x in d))
            outer = 180.0 if self.outer_deg is None else float(self.outer_deg)
            inner = outer if self.inner_deg is None else float(self.inner_deg)
            if not 0.0 <= inner <= outer <= 180.0:
                raise ValueError(f"a spot's cone has 0 <= inner_deg <= outer_deg <= 180, got {self.inner_deg!r} and {self.outer_deg!r}")
            set_("inner_deg", inner)
            set_("outer_deg", outer)
        clearance = max(radius, 0.02) if self.clearance is None else float(self.clearance)
        min_distance = max(radius, 0.01) if self.min_distance is None else float(self.min_distance)
        if not (math.isfinite(clearance) and clearance >= 0.0):
            raise ValueError(f"a light's clearance is finite and >= 0, got {self.clearance!r}")
        if not (math.isfinite(min_distance) and min_distance > 0.0):
            raise ValueError(f"a light's min_distance is finite and > 0, got {self.min_distance!r}")
        set_("clearance", clearance)
        set_("min_distance", min_distance)

    @property
    def row(self) -> List[float]:
        """the light's 16 columns of the device block, as Python floats (float64)"""
        if self.direction is None:
            a, ci, co = (0.0, 0.0, -1.0), -1.0, -1.0
        else:
            a, ci, co = self.direction, math.cos(math.radians(self.inner_deg)), math.cos(math.radians(self.outer_deg))
        return [*self.position, *a, ci, co, self.radius, self.clearance, self.min_distance, 0.0, *self.intensity, 0.0]


def as_lights(lights: Union[PointLight, Sequence[PointLight], None]) -> Tuple[PointLight, ...]:
    """one PointLight or a sequence of them as a tuple; None and an empty sequence are no lights"""
    if lights is None:
        return ()
    if isinstance(lights, PointLight):
        return (lights,)
    out = tuple(lights)
    if not all(isinstance(x, PointLight) for x in out):
        raise TypeError("lights: a PointLight or a sequence of them")
    if len(out) > MAX_LIGHTS:
        raise ValueError(f"{len(out)} lights: each one is a whole shadow march, a frame takes at most {MAX_LIGHTS}")
    return out


def lights_block(lights) -> torch.Tensor:
    """the device form of the lights as a host tensor [L, 16] float32, built in float64 (the cone's cosines rounded once)"""
    lights = as_lights(lights)
    if not lights:
        raise ValueError("lights_block: at least one light")
    return torch.tensor([x.row for x in lights], dtype=torch.float64).to(torch.float32)


def load_lights(path) -> Tuple[PointLight, ...]:
    """a JSON file: a list of objects with PointLight's keywords (position and intensity required)"""
    with open(path) as f:
        data = json.load(f)
    if not isinstance(data, list):
        raise ValueError(f"{path}: a list of lights, got {type(data).__name__}")
    out = []
    for i, entry in enumerate(data):
        if not isinstance(entry, dict) or set(entry) - set(_KEYS) or not {"position", "intensity"} <= set(entry):
            raise ValueError(f"{path}: light {i}: an object with position, intensity and any of {_KEYS[2:]}, got {entry!r}")
        out.append(PointLight(**entry))
    return as_lights(out)


def save_lights(path, lights) -> None:
    """the inverse of load_lights: every field of every light, the defaults written out"""
    with open(path, "w") as f:
        json.dump([{k: getattr(x, k) for k in _KEYS if getattr(x, k) is not None} for x in as_lights(lights)], f, indent=1)


def trace_visibility_to(sdf, origins: torch.Tensor, lights, *, steps: int = 96, eps: float = 1e-3, relax: float = 1.0,
                        min_step: float = 1e-3, grace: int = 16, radius: float = 1.0) -> SphereTrace:
    """March shadow rays from the start points `origins` [M, 3] to each of L lights (PointLight, a sequence of them, or a device block
    [L, 16]); the results are [L, M].  sdf, and the parameters: relight.trace_visibility.  A ray ends `clearance` in front of its
    light and is then ESCAPED, as one that leaves the scene bound is; its penumbra has the tangent radius / distance."""
    p = trace_settings({"steps": steps, "eps": eps, "relax": relax, "min_step": min_step, "grace": grace, "radius": radius},
                       {**LIGHT_TRACE_DEFAULTS, "radius": 1.0})
    block = lights.to(torch.float32).contiguous() if torch.is_tensor(lights) else lights_block(lights)
    if block.dim() != 2 or block.shape[1] != hip.LIGHT_FLOATS or not 1 <= block.shape[0] <= MAX_LIGHTS:
        raise ValueError(f"lights: 1 to {MAX_LIGHTS} of them, a block [L, {hip.LIGHT_FLOATS}], got {tuple(block.shape)}")
    L = block.shape[0]
    origins, state, points = _start(sdf, origins, lambda M: L * M, f"origins [M, 3], got {tuple(origins.shape)}")
    dev = origins.device
    params = trace_params({**p, "bias": 0.0}).to(dev)
    ray_dirs, bounds = torch.empty_like(points), torch.empty(2, points.shape[0], device=dev)
    hip.light_trace_begin_points(origins, block.to(dev), params, state, points, ray_dirs, bounds)
    return _march(sdf, state, points, ray_dirs, 1, params, p["steps"], p["grace"], (L, origins.shape[0]), bounds)


def trace_light_shadows(sdf, origins: torch.Tensor, directions: torch.Tensor, depth: torch.Tensor, normals: torch.Tensor,
                        lights: torch.Tensor, params: torch.Tensor, steps: int, grace: int) -> SphereTrace:
    """the frame render's march: camera rays `origins`, `directions` [R, 3] (unit), their rendered `depth` [R] along the ray and
    `normals` [R, 3] (any length; a zero one is replaced by the direction to the lamp), `lights`: the device block [L, 16]; `params`:
    the device block of trace_params, whose bias lifts the start point o + depth d along the normal.  Results [L, R].  Nothing is read
    on the host and every shape is static: a captured chunk replays with new lights and a new parameter block."""
    R, L, dev = origins.shape[0], lights.shape[0], origins.device
    T = L * R
    state, points, ray_dirs, bounds = (torch.empty(6, T, device=dev), torch.empty(T, 3, device=dev), torch.empty(T, 3, device=dev),
                                       torch.empty(2, T, device=dev))
    hip.light_trace_begin(origins.detach().contiguous(), directions.detach().contiguous(), depth.detach().reshape(-1).contiguous(),
                          normals.detach().contiguous(), lights, params, state, points, ray_dirs, bounds)
    return _march(sdf, state, points, ray_dirs, 1, params, steps, grace, (L, R), bounds)
