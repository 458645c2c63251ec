"""A directional sun for the frame render (get_outputs_for_camera_ray_bundle(..., sun=)): its direction from azimuth and elevation,
its colour in the renderer's irradiance units, and a sweep between two positions.  Definitions: include/neusky_hip.h; kernels:
csrc/sun.hip.

The frame render sees light as its D = 512 directions, one cell of which covers 4 pi / 512 = 0.025 sr; the sun covers 6.8e-5 sr.  A
`SunLight` is one more direction with one DDF shadow query per ray (the reference's render_shadow_map, neusky_model.py:637-670), so its
shadow is an edge instead of the average of a cell."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Sequence, Tuple, Union

SUN_ANGULAR_DIAMETER_DEG = 0.533


def sun_direction(azimuth_deg: float, elevation_deg: float) -> Tuple[float, float, float]:
    """the unit vector towards the sun, z up (neusky_model.py:641-645)"""
    az, el = math.radians(azimuth_deg), math.radians(elevation_deg)
    return (math.cos(az) * math.cos(el), math.sin(az) * math.cos(el), math.sin(el))


def sun_solid_angle(angular_diameter_deg: float = SUN_ANGULAR_DIAMETER_DEG) -> float:
    """of a disc of this angular diameter, in steradians: 2 pi (1 - cos(diameter / 2)), written without the cancellation"""
    return 4.0 * math.pi * math.sin(math.radians(angular_diameter_deg) / 4.0) ** 2


@dataclass(frozen=True)
class SunLight:
    """colour: C [3] in the renderer's irradiance units: the hemisphere term of the render is the mean of clamp(<n,d>) L_d over the
    normal's hemisphere, an estimate of (1 / 2 pi) int L cos, so a source of radiance L and solid angle Omega has C = L Omega / (2 pi)."""
    azimuth_deg: float
    elevation_deg: float
    colour: Tuple[float, float, float] = (1.0, 1.0, 1.0)

    def __post_init__(self):
        c = tuple(float(x) for x in self.colour)
        if len(c) != 3:
            raise ValueError(f"a sun's colour has 3 channels, got {self.colour!r}")
        object.__setattr__(self, "colour", c)
        object.__setattr__(self, "azimuth_deg", float(self.azimuth_deg))
        object.__setattr__(self, "elevation_deg", float(self.elevation_deg))

    @property
    def direction(self) -> Tuple[float, float, float]:
        return sun_direction(self.azimuth_deg, self.elevation_deg)

    @classmethod
    def from_radiance(cls, azimuth_deg: float, elevation_deg: float, radiance: Sequence[float],
                      angular_diameter_deg: float = SUN_ANGULAR_DIAMETER_DEG) -> "SunLight":
        k = sun_solid_angle(angular_diameter_deg) / (2.0 * math.pi)
        return cls(azimuth_deg, elevation_deg, tuple(float(x) * k for x in radiance))

    @classmethod
    def from_direction(cls, direction: Sequence[float], colour: Sequence[float] = (1.0, 1.0, 1.0)) -> "SunLight":
        """the sun towards `direction` (any length > 0), the inverse of sun_direction: az = atan2(y, x), el = asin(z / |d|), in degrees"""
        x, y, z = (float(v) for v in direction)
        n = math.sqrt(x * x + y * y + z * z)
        if not (n > 0.0 and math.isfinite(n)):
            raise ValueError(f"a sun's direction has a finite length above zero, got {direction!r}")
        return cls(math.degrees(math.atan2(y, x)), math.degrees(math.asin(max(-1.0, min(1.0, z / n)))), colour)


def sun_path(az0: float, el0: float, az1: float, el1: float, steps: int, colour=(1.0, 1.0, 1.0)) -> List[SunLight]:
    """`steps` suns from (az0, el0) to (az1, el1), linear in both angles, endpoints included"""
    if steps < 1:
        raise ValueError("a sun path has at least one step")
    if steps == 1:
        return [SunLight(az0, el0, colour)]
    return [SunLight(az0 + (az1 - az0) * i / (steps - 1), el0 + (el1 - el0) * i / (steps - 1), colour) for i in range(steps)]


def as_suns(sun: Union[SunLight, Sequence[SunLight]]) -> Tuple[List[SunLight], bool]:
    """(the suns as a list, whether a single SunLight was given)"""
    if isinstance(sun, SunLight):
        return [sun], True
    suns = list(sun)
    if not suns or not all(isinstance(s, SunLight) for s in suns):
        raise TypeError("sun: a SunLight or a non-empty sequence of them")
    return suns, False
