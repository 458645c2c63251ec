"""A clear-sky daylight model whose sky follows the sun: Preetham, Shirley, Smits, "A Practical Analytic Model for Daylight", 1999.
Definitions: include/neusky_hip.h; kernel: csrc/daylight.hip.

`DaylightSky` is a sky that is a function of the sun: its radiance distribution (`radiance`, on the GPU), and the colour of the direct
sun behind the same atmosphere (`sun_colour`, a few numbers on the host).  The frame render with `daylight=` lights a frame with both,
so that a sweep of K suns gets K skies, K sun colours and K backgrounds from one field pass per chunk.

The sky's radiance comes out of the model in kcd / m^2; `exposure` brings it to the renderer's range.  The direct sun is
C = exposure (133.1 / 2 pi) tau in the unit of SunLight.colour, C = L Omega / 2 pi: 133.1 klx of extraterrestrial solar illuminance, through
the Rayleigh and aerosol transmittance tau of the paper's appendix at three wavelengths standing for R, G, B.  The 133.1 klx, the three
wavelengths and the default exposure are design choices, not measurements."""
from __future__ import annotations

import math
from typing import List, Sequence, Tuple, Union

from .sun import SunLight, sun_direction, sun_path

TURBIDITY_RANGE = (2.0, 10.0)
SOLAR_ILLUMINANCE_KLX = 133.1
WAVELENGTHS_UM = (0.610, 0.550, 0.465)


class DaylightSky:
    """turbidity: 2 (very clear) .. 10 (hazy).  exposure: multiplies sky and sun alike.  ground: what a direction below the horizon
    shows, as a factor on the sky at its horizon point."""

    def __init__(self, turbidity: float = 3.0, exposure: float = 0.1, ground: Sequence[float] = (0.25, 0.25, 0.25)):
        T = float(turbidity)
        if not TURBIDITY_RANGE[0] <= T <= TURBIDITY_RANGE[1]:
            raise ValueError(f"the daylight model holds for a turbidity in [2, 10], got {turbidity!r}")
        e = float(exposure)
        if not (math.isfinite(e) and e >= 0.0):
            raise ValueError(f"exposure must be finite and >= 0, got {exposure!r}")
        g = tuple(float(x) for x in ground)
        if len(g) != 3 or not all(math.isfinite(x) and x >= 0.0 for x in g):
            raise ValueError(f"ground has 3 finite channels >= 0, got {ground!r}")
        self.turbidity, self.exposure, self.ground = T, e, g

    def __repr__(self) -> str:
        return f"DaylightSky(turbidity={self.turbidity}, exposure={self.exposure}, ground={self.ground})"

    # ------------------------------------------------------------------ the sun
    def transmittance(self, elevation_deg: float) -> Tuple[float, float, float]:
        """of the direct sun at the three wavelengths: exp(-0.008735 lam^-4.08 m) exp(-beta lam^-1.3 m), beta = 0.04608 T - 0.04586,
        along the relative air mass m = 1 / (cos ts + 0.15 (93.885 - ts_deg)^-1.253)"""
        ts_deg = 90.0 - float(elevation_deg)
        m = 1.0 / (math.cos(math.radians(ts_deg)) + 0.15 * (93.885 - ts_deg) ** -1.253)
        beta = 0.04608 * self.turbidity - 0.04586
        return tuple(math.exp(-0.008735 * lam ** -4.08 * m) * math.exp(-beta * lam ** -1.3 * m) for lam in WAVELENGTHS_UM)

    def sun_colour(self, azimuth_deg: float, elevation_deg: float) -> Tuple[float, float, float]:
        """C [3] in the renderer's irradiance units (SunLight.colour); a sun that has set (direction z <= 0) has C = 0"""
        if not sun_direction(azimuth_deg, elevation_deg)[2] > 0.0:
            return (0.0, 0.0, 0.0)
        k = self.exposure * SOLAR_ILLUMINANCE_KLX / (2.0 * math.pi)
        return tuple(k * t for t in self.transmittance(elevation_deg))

    def sun(self, azimuth_deg: float, elevation_deg: float) -> SunLight:
        return SunLight(azimuth_deg, elevation_deg, self.sun_colour(azimuth_deg, elevation_deg))

    def sun_path(self, az0: float, el0: float, az1: float, el1: float, steps: int) -> List[SunLight]:
        """relight.sun_path, each sun with its own colour"""
        return [self.sun(s.azimuth_deg, s.elevation_deg) for s in sun_path(az0, el0, az1, el1, steps)]

    # ------------------------------------------------------------------ the sky
    def device_parameters(self, device):
        """(turbidity [1], exposure [1], ground [3]) on `device`, what nsky_daylight_eval reads: views of one fp32 buffer [5]"""
        import torch
        packed = torch.tensor([self.turbidity, self.exposure, *self.ground], dtype=torch.float32).to(device)
        return packed[0:1], packed[1:2], packed[2:5]

    def radiance(self, directions, suns):
        """directions: [N, 3] on the GPU (any length, normalised by the kernel; a zero or non-finite one gives 0); suns: a [K, 3]
        tensor of unit vectors towards the sun, a SunLight or a sequence of them -> linear sRGB [K, N, 3].  Point samples of the
        model, one kernel launch, nothing read back."""
        import torch

        from .. import hip
        directions = torch.as_tensor(directions)
        dev = directions.device
        directions = directions.to(torch.float32).reshape(-1, 3).contiguous()
        if not torch.is_tensor(suns):
            suns = sun_directions(suns)
        suns = suns.to(device=dev, dtype=torch.float32).reshape(-1, 3).contiguous()
        out = torch.empty(suns.shape[0], directions.shape[0], 3, dtype=torch.float32, device=dev)
        hip.daylight_eval(directions, suns, *self.device_parameters(dev), out)
        return out


def sun_directions(suns: Union[SunLight, Sequence[SunLight]]):
    """[K, 3] fp32 (host): the directions of SunLights, rounded once from float64 as the frame render does"""
    import torch
    suns = [suns] if isinstance(suns, SunLight) else list(suns)
    return torch.tensor([s.direction for s in suns], dtype=torch.float64).to(torch.float32)
