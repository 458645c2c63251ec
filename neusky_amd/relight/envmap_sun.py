"""The sun of an HDR environment map, lifted out of it into a shadow-casting `SunLight` (csrc/envmap_sun.hip; the definitions are in
include/neusky_hip.h).

`project_envmap` turns a map into the cell averages of the frame's D light directions: the sun ends up smeared over a cell hundreds of
times its size and its shadow is the average of a cell's visibilities, not an edge.  `extract_sun` finds the sun in the map, clamps the
texels of a small cap about it to the luminance of the sky around the cap, and returns the energy taken out as the colour of a
directional sun, which the frame render lights with one DDF shadow query per ray.  Energy is conserved: the residual map plus the sun
carry the flux of the original map, so the sun is not counted twice."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from .. import hip
from .envmap import EnvironmentMap
from .sun import SunLight

LUMINANCE = (0.2126, 0.7152, 0.0722)


@dataclass(frozen=True)
class SunExtraction:
    """What `extract_sun` found.  Directions are in the MAP frame; `colour` is without the map's exposure.

    envmap: the residual map (same convention, exposure and device as the input, which is not modified); the input's values when
      nothing was found.
    found: whether the peak stood out from the sky around it.
    direction: unit vector towards the sun (the flux-weighted mean direction of the excess); the peak texel's when not found.
    colour: C [3] in `SunLight`'s irradiance units, (1 / 2 pi) sum omega (L - L'); zero when not found.
    peak_luminance, sky_luminance: Y of the peak texel, and the solid-angle-weighted mean Y of the ring about the cap.
    solid_angle: of the texels that lost energy, in steradians.
    flux_fraction: the share of the map's luminous flux that went to the sun, 2 pi Y(C) / sum omega Y."""
    envmap: EnvironmentMap
    found: bool
    direction: Tuple[float, float, float]
    colour: Tuple[float, float, float]
    peak_luminance: float
    sky_luminance: float
    solid_angle: float
    flux_fraction: float

    def sun(self, rotation=None) -> Optional[SunLight]:
        """The sun in the scene frame for a frame rendered with `rotation` (fp32 [3, 3] or None): the renderer lights direction d with
        the map at R d, so the sun stands at R^T m.  Its colour is C times the residual map's current exposure.  None when not found."""
        if not self.found:
            return None
        m = np.asarray(self.direction, np.float64)
        if rotation is not None:
            R = rotation.detach().cpu().numpy() if isinstance(rotation, torch.Tensor) else np.asarray(rotation)
            if R.shape != (3, 3):
                raise ValueError(f"rotation must be [3, 3], got {R.shape}")
            m = R.astype(np.float64).T @ m
        ex = float(self.envmap.exposure)
        return SunLight.from_direction(tuple(m), tuple(c * ex for c in self.colour))

    @property
    def angular_diameter_deg(self) -> float:
        """of a disc of `solid_angle`"""
        return math.degrees(4.0 * math.asin(min(1.0, math.sqrt(self.solid_angle / (4.0 * math.pi)))))


def check_radius(radius_deg: float, H: int) -> None:
    if not radius_deg >= 180.0 / H:
        raise ValueError(f"extract_sun: radius_deg {radius_deg} is less than a texel row ({180.0 / H:g} degrees at H = {H}): the ring "
                         "about the cap could be empty")
    if radius_deg >= 45.0:
        raise ValueError(f"extract_sun: radius_deg {radius_deg} must be below 45")


def extract_sun(envmap: EnvironmentMap, radius_deg: float = 2.5, min_peak_ratio: float = 10.0) -> SunExtraction:
    """Find the sun of `envmap`, take its excess over the sky out of the map and return both (see SunExtraction).

    The peak is the brightest finite texel of the map's upper hemisphere.  The cap is everything within radius_deg of it, the ring
    everything between radius_deg and twice that; the sky level tau is the ring's mean luminance.  The sun is found when the peak is
    positive and at least min_peak_ratio tau.  A cap texel brighter than tau is scaled to luminance tau (chromaticity kept); what it
    lost goes to the sun.  Three HIP passes on the current stream (peak, ring, split), then ONE read of 13 numbers to the host; the
    result is bitwise repeatable.

    The two defaults are design choices, not measurements.  2.5 degrees covers a lens-blurred disc, and its 5-degree ring stays inside
    one light cell (about 5.1 degrees in radius at D = 512).  A ratio of 10 separates any real sun (1e3 to 1e5 times the sky) from a
    bright cloud.

    Raises ValueError for radius_deg < 180 / H (the ring could be empty) or radius_deg >= 45."""
    H, W = envmap.shape
    check_radius(radius_deg, H)
    if not min_peak_ratio >= 0.0:
        raise ValueError(f"extract_sun: min_peak_ratio {min_peak_ratio} must be >= 0")
    rho = math.radians(radius_deg)
    dev, data, conv = envmap.device, envmap.data, envmap.convention_id
    with torch.cuda.device(dev):
        scratch = torch.empty(hip.ENVMAP_SUN_SCRATCH_BYTES // 8, dtype=torch.float64, device=dev)
        peak = torch.empty(2, dtype=torch.int64, device=dev)
        ring = torch.empty(2, dtype=torch.float64, device=dev)
        stats = torch.empty(12, dtype=torch.float64, device=dev)
        residual = torch.empty_like(data)
        hip.envmap_peak(data, conv, scratch, peak)
        hip.envmap_sun_ring(data, conv, peak, rho, scratch, ring)
        hip.envmap_sun_split(data, conv, peak, ring, rho, min_peak_ratio, scratch, residual, stats)
        # the map's luminous flux, for flux_fraction alone (a reported figure): row sums in fp64, non-finite texels left out
        finite = torch.isfinite(data).all(dim=2, keepdim=True)
        rows = torch.where(finite, data, torch.zeros((), dtype=data.dtype, device=dev)).sum(dim=1, dtype=torch.float64)
        theta = (torch.arange(H, dtype=torch.float64, device=dev) + 0.5) * (math.pi / H)
        omega = torch.sin(theta) * ((2.0 * math.pi / W) * 2.0 * math.sin(math.pi / (2.0 * H)))
        flux = (rows @ torch.tensor(LUMINANCE, dtype=torch.float64, device=dev) * omega).sum()
        s = torch.cat([stats, flux[None]]).cpu().tolist()  # the one host read
    colour = (s[3], s[4], s[5])
    flux_sun = 2.0 * math.pi * sum(w * c for w, c in zip(LUMINANCE, colour))
    out = EnvironmentMap(residual, envmap.convention, envmap.exposure, dev)
    return SunExtraction(envmap=out, found=s[9] != 0.0, direction=(s[0], s[1], s[2]), colour=colour, peak_luminance=s[6], sky_luminance=s[7],
                         solid_angle=s[8], flux_fraction=flux_sun / s[12] if s[12] > 0.0 else 0.0)
