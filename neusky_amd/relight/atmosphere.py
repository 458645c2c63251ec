"""Height fog and haze with shadowed sun shafts: `Atmosphere`, a participating medium between the camera and what a frame shows.  The rule
(optical depth, source, in-scatter, the pixel): include/neusky_hip.h ("Height fog"); kernels: csrc/atmosphere.hip.

The medium has an extinction coefficient that falls off exponentially with height (or none: a homogeneous haze), a single-scattering
albedo and a Henyey-Greenstein phase function.  A ray is attenuated to its rendered depth and gains the light the medium scatters into
it on the way: the frame's sky, averaged over its light directions and not shadowed, and each sun, optionally shadowed at
`shaft_samples` points along the ray by the frame's own shadow mode (DDF queries or marches through the SDF).  What lies behind the
scene (the background, and the see-through share of a ray) sits at the distance `far`.

The rule uses a ray's rendered depth, as the suns' and the lamps' shadows do, not a per-sample transmittance inside the alpha composite,
and adds no glow around lamps.  Every default below is a design choice, not a measurement."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Tuple, Union

import torch

from .. import hip

MAX_SHAFT_SAMPLES = hip.ATMOSPHERE_MAX_SHAFTS  # 64
MAX_FAR_OVER_SCALE_HEIGHT = 60.0  # exp(60) times exp(80) stays finite in float64, and exp(60) in float32
MAX_ANISOTROPY = 0.99


def _triple(name: str, v, lo: float, hi: Optional[float]) -> Tuple[float, float, float]:
    try:
        t = tuple(float(x) for x in v) if hasattr(v, "__len__") or hasattr(v, "__iter__") else (float(v),) * 3
    except (TypeError, ValueError):
        raise ValueError(f"{name} is a number or an RGB triple, got {v!r}") from None
    if len(t) != 3:
        raise ValueError(f"{name} is a number or an RGB triple, got {v!r}")
    if not all(math.isfinite(x) and x >= lo and (hi is None or x <= hi) for x in t):
        bound = f">= {lo:g}" if hi is None else f"in [{lo:g}, {hi:g}]"
        raise ValueError(f"{name}: every component is finite and {bound}, got {v!r}")
    return t


def _number(name: str, v) -> float:
    try:
        if isinstance(v, bool):
            raise TypeError
        x = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"{name} is a number, got {v!r}") from None
    if not math.isfinite(x):
        raise ValueError(f"{name} must be finite, got {v!r}")
    return x


@dataclass(frozen=True)
class Atmosphere:
    """density: the extinction coefficient per scene unit at height `base_height`, one number or an RGB triple (wavelength-dependent
    haze), each >= 0.
    scale_height H: None is a homogeneous medium; otherwise > 0, and sigma_c(z) = density_c exp(-(z - base_height) / H), z up.
    albedo: the single-scattering albedo, one number or a triple in [0, 1].
    anisotropy g: of the Henyey-Greenstein phase function, |g| <= 0.99 (0: isotropic; > 0: forward, a glow around the sun).
    far: > 0, the path length, in scene units from the ray origin, of what lies behind the scene: the background, and the see-through
    share of a ray.  With a finite H, far / H <= 60.
    shaft_samples M: 0..64; the suns' in-scatter is shadowed at M points along every ray, by the frame's own shadow mode; 0: unshadowed.
    background: whether the sky behind the scene is fogged too (a daylight sky already contains its own atmosphere)."""
    density: Union[float, Tuple[float, float, float]]
    scale_height: Optional[float] = None
    base_height: float = 0.0
    albedo: Union[float, Tuple[float, float, float]] = 1.0
    anisotropy: float = 0.0
    far: float = 2.0
    shaft_samples: int = 0
    background: bool = True

    def __post_init__(self):
        set_ = lambda k, v: object.__setattr__(self, k, v)  # noqa: E731
        set_("density", _triple("density", self.density, 0.0, None))
        set_("albedo", _triple("albedo", self.albedo, 0.0, 1.0))
        set_("base_height", _number("base_height", self.base_height))
        set_("anisotropy", _number("anisotropy", self.anisotropy))
        if abs(self.anisotropy) > MAX_ANISOTROPY:
            raise ValueError(f"anisotropy: |g| <= {MAX_ANISOTROPY}, got {self.anisotropy!r}")
        set_("far", _number("far", self.far))
        if not self.far > 0.0:
            raise ValueError(f"far must be > 0, got {self.far!r}")
        if self.scale_height is not None:
            set_("scale_height", _number("scale_height", self.scale_height))
            if not self.scale_height > 0.0:
                raise ValueError(f"scale_height is None (a homogeneous medium) or > 0, got {self.scale_height!r}")
            if self.far / self.scale_height > MAX_FAR_OVER_SCALE_HEIGHT:
                raise ValueError(f"far / scale_height <= {MAX_FAR_OVER_SCALE_HEIGHT:g} (no exponential may overflow), got "
                                 f"{self.far!r} / {self.scale_height!r}")
        M = self.shaft_samples
        if isinstance(M, bool) or not isinstance(M, int) or not 0 <= M <= MAX_SHAFT_SAMPLES:
            raise ValueError(f"shaft_samples is an integer in 0..{MAX_SHAFT_SAMPLES}, got {M!r}")
        if not isinstance(self.background, bool):
            raise ValueError(f"background is a bool, got {self.background!r}")

    def block(self) -> torch.Tensor:
        """the kernels' parameter block as a host tensor [hip.ATMOSPHERE_FLOATS]: density (0..2), albedo (3..5), H (0: homogeneous),
        base_height, g, far, the background flag (1 or 0), pad"""
        H = 0.0 if self.scale_height is None else self.scale_height
        block = torch.tensor([*self.density, *self.albedo, H, self.base_height, self.anisotropy, self.far, 1.0 if self.background else 0.0, 0.0],
                             dtype=torch.float64).to(torch.float32)
        assert block.shape == (hip.ATMOSPHERE_FLOATS,)
        return block

    def extra_shadow_rows(self, suns: int) -> int:
        """what the shafts cost per ray, as a count: M K further DDF rows (beside the sky pass's D), or M K further marched shadow rays"""
        return self.shaft_samples * max(int(suns), 0)
