"""The display transform: from a linear, high-dynamic-range image to a picture, on the device.  Definitions: include/neusky_hip.h
("A display transform"); kernels: csrc/display.hip.

A relit frame holds radiance far above 1 (a sun's disc is 1e3 to 1e5 times its sky).  `DisplayTransform` meters the image (a histogram of
luminance with 64 bins per octave, read off the floats' bit patterns; the mean of the bins between two percentiles, a piecewise-linear log2,
sets the exposure E = key 2^(ev - mean)), optionally
adds a bloom (a Gaussian of what exceeds a threshold), applies a tone curve and the sRGB transfer function and rounds to 8 bits:

    x = max(E lin + strength B, 0);   rgb = clamp(linear_to_sRGB(curve(x)), 0, 1);   rgb8 = rint(255 rgb)

With the defaults (curve "clamp", exposure 1, no bloom) `rgb` has the bits of the renderer's own clipped `rgb`.  key = 0.18, the
percentiles (0.05, 0.95), ev = 0, the white point 4 and the bloom's threshold and strength are design choices, not measurements.

The frame render, `RadianceTransfer.relight` and `SHRadianceTransfer.relight` take a transform as `display=` and add `display_rgb8`,
`display_rgb` and `display_exposure` to their outputs (`frame_display`).  Nothing here is read on the host."""
from __future__ import annotations

import math
from dataclasses import dataclass
from functools import lru_cache
from typing import Dict, Optional, Tuple, Union

import torch

CURVES = ("clamp", "reinhard", "aces", "hable")
AUTO_EXPOSURES = ("frame", "sequence")
BINS = 3072
MAX_BLOOM_SIGMA = 32.0


def bloom_weights(sigma: float) -> torch.Tensor:
    """the 2 r + 1 weights of the bloom's Gaussian, r = ceil(3 sigma): normalised in float64, rounded to float32"""
    r = int(math.ceil(3.0 * sigma))
    t = torch.arange(-r, r + 1, dtype=torch.float64)
    w = torch.exp(-(t * t) / (2.0 * float(sigma) ** 2))
    return (w / w.sum()).to(torch.float32)


# what a transform keeps on a device, made once per value: a later call with the same values copies nothing from the host
@lru_cache(maxsize=64)
def _device_values(values: tuple, device: str) -> torch.Tensor:
    return torch.tensor(values, dtype=torch.float32).to(device)


@lru_cache(maxsize=16)
def _device_weights(sigma: float, device: str) -> torch.Tensor:
    return bloom_weights(sigma).to(device)


def _images(lin: torch.Tensor) -> torch.Tensor:
    """a linear image as [K, H, W, 3]: [H, W, 3] is one image, [N, 3] one row of N pixels"""
    if not torch.is_tensor(lin) or lin.dim() not in (2, 3, 4) or lin.shape[-1] != 3:
        raise ValueError(f"a linear image is [K, H, W, 3], [H, W, 3] or [N, 3], got {tuple(getattr(lin, 'shape', ()))}")
    lin = lin.detach().to(torch.float32)
    lin = lin[None, None] if lin.dim() == 2 else lin[None] if lin.dim() == 3 else lin
    return lin.contiguous()


@dataclass(frozen=True)
class DisplayTransform:
    """curve: "clamp", "reinhard" (white point `white`), "aces" (Narkowicz's fit) or "hable" (the Uncharted-2 operator).
    exposure: a factor, or "frame" (every image is metered and takes its own E) or "sequence" (the images of a call, or of several
    `luminance_histogram` calls into one histogram, share one E: what a time-of-day sweep needs).
    key, ev, percentiles: E = key 2^(ev - m), m the mean (piecewise-linear) log2 luminance of the metered pixels between the two percentiles.
    bloom_sigma: pixels, 0 = off, at most 32; bloom_threshold, bloom_strength: B = G_sigma * max(E lin - threshold, 0) is added `strength`
    times.
    meter_mask_threshold: with a mask (a frame's accumulation), meter the pixels whose mask exceeds it; None: the mask is not read."""
    curve: str = "clamp"
    exposure: Union[float, str] = 1.0
    key: float = 0.18
    ev: float = 0.0
    percentiles: Tuple[float, float] = (0.05, 0.95)
    white: float = 4.0
    bloom_sigma: float = 0.0
    bloom_threshold: float = 1.0
    bloom_strength: float = 0.1
    meter_mask_threshold: Optional[float] = None

    def __post_init__(self):
        def number(name, lo=None, positive=False):
            try:
                v = float(getattr(self, name))
            except (TypeError, ValueError):
                raise ValueError(f"{name} is a number, got {getattr(self, name)!r}") from None
            if not math.isfinite(v) or (positive and not v > 0.0) or (lo is not None and v < lo):
                bound = " and > 0" if positive else f" and >= {lo:g}" if lo is not None else ""
                raise ValueError(f"{name} must be finite{bound}, got {getattr(self, name)!r}")
            object.__setattr__(self, name, v)

        if self.curve not in CURVES:
            raise ValueError(f"curve: one of {CURVES}, got {self.curve!r}")
        if isinstance(self.exposure, str):
            if self.exposure not in AUTO_EXPOSURES:
                raise ValueError(f"exposure: a factor, or one of {AUTO_EXPOSURES}, got {self.exposure!r}")
        else:
            number("exposure", lo=0.0)
        number("key", positive=True)
        number("ev")
        number("white", positive=True)
        number("bloom_sigma", lo=0.0)
        number("bloom_threshold", lo=0.0)
        number("bloom_strength", lo=0.0)
        if self.bloom_sigma > MAX_BLOOM_SIGMA:
            raise ValueError(f"bloom_sigma is at most {MAX_BLOOM_SIGMA:g} pixels, got {self.bloom_sigma!r}")
        if self.meter_mask_threshold is not None:
            number("meter_mask_threshold")
        try:
            lo, hi = (float(p) for p in self.percentiles)
        except (TypeError, ValueError):
            raise ValueError(f"percentiles: two numbers 0 <= lo < hi <= 1, got {self.percentiles!r}") from None
        if not 0.0 <= lo < hi <= 1.0:
            raise ValueError(f"percentiles: two numbers 0 <= lo < hi <= 1, got {self.percentiles!r}")
        object.__setattr__(self, "percentiles", (lo, hi))

    # ------------------------------------------------------------------ device state
    @property
    def metered(self) -> bool:
        return isinstance(self.exposure, str)

    def params(self, device) -> torch.Tensor:
        """the kernels' parameter block [8]: key, ev, p_lo, p_hi, white, bloom threshold, bloom strength, meter_mask_threshold"""
        thr = 0.0 if self.meter_mask_threshold is None else self.meter_mask_threshold
        return _device_values((self.key, self.ev, *self.percentiles, self.white, self.bloom_threshold, self.bloom_strength, thr), str(device))

    def _mask(self, mask: Optional[torch.Tensor], lin: torch.Tensor) -> Optional[torch.Tensor]:
        """the mask the meter reads: [K, H, W] like `lin`, one mask of [H, W] (or [H, W, 1]) serving all K images"""
        if mask is None or self.meter_mask_threshold is None:
            return None
        K, H, W, _ = lin.shape
        m = mask.detach().to(torch.float32)
        if m.numel() == H * W:
            m = m.reshape(1, H, W).expand(K, H, W)
        elif m.numel() == K * H * W:
            m = m.reshape(K, H, W)
        else:
            raise ValueError(f"a mask of {tuple(mask.shape)} for images {tuple(lin.shape)}")
        return m.contiguous()

    # ------------------------------------------------------------------ the meter
    def luminance_histogram(self, lin: torch.Tensor, mask: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """int64 [K, 3072] of lin [K, H, W, 3] ([H, W, 3]: K = 1), or `out` with the counts added: [K, 3072], or [1, 3072] for all the
        images of this and of other calls together, which is how "sequence" meters many calls into one E"""
        from .. import hip
        lin = _images(lin)
        if out is None:
            out = torch.zeros(lin.shape[0], BINS, dtype=torch.int64, device=lin.device)
        hip.display_histogram(lin, self._mask(mask, lin), self.params(lin.device), out)
        return out

    def exposure_from_histogram(self, hist: torch.Tensor) -> torch.Tensor:
        """E fp32 [K] of int64 histograms [K, 3072]"""
        from .. import hip
        E = torch.empty(hist.shape[0], dtype=torch.float32, device=hist.device)
        hip.display_exposure(hist, self.params(hist.device), E)
        return E

    # ------------------------------------------------------------------ the transform
    def apply(self, lin: torch.Tensor, mask: Optional[torch.Tensor] = None,
              exposure: Union[None, float, torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """lin [K, H, W, 3] (or [H, W, 3], or [N, 3]: without a bloom the layout of the pixels does not matter) -> {"rgb8": uint8 and
        "rgb": float32, shaped like lin, "exposure": float32 [K], or [1] when the images share one}.  exposure: the E to use in place
        of this transform's own rule: a factor, or a device tensor [K] or [1] (of exposure_from_histogram)."""
        from .. import hip
        shape = lin.shape
        lin = _images(lin)
        K, dev = lin.shape[0], lin.device
        params = self.params(dev)
        if exposure is None and self.metered:
            hist = torch.zeros(1 if self.exposure == "sequence" else K, BINS, dtype=torch.int64, device=dev)
            hip.display_histogram(lin, self._mask(mask, lin), params, hist)
            E = torch.empty(hist.shape[0], dtype=torch.float32, device=dev)
            hip.display_exposure(hist, params, E)
        elif torch.is_tensor(exposure):
            E = exposure.detach().to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
            if E.shape[0] not in (1, K):
                raise ValueError(f"{E.shape[0]} exposures for {K} images")
        else:
            E = _device_values((float(self.exposure if exposure is None else exposure),), str(dev)).clone()  # (the caller owns what it gets back)
        B = None
        if self.bloom_sigma > 0.0 and self.bloom_strength > 0.0:
            B = torch.empty_like(lin)
            hip.display_blur(lin, E, params, _device_weights(self.bloom_sigma, str(dev)), torch.empty_like(lin), B)
        rgb8 = torch.empty(lin.shape, dtype=torch.uint8, device=dev)
        rgb = torch.empty_like(lin)
        hip.display_map(lin, B, E, params, self.curve, rgb8, rgb)
        return {"rgb8": rgb8.view(shape), "rgb": rgb.view(shape), "exposure": E}


def frame_display(display: Optional[DisplayTransform], lin: torch.Tensor, shape, mask: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """what `display=` adds to a frame's outputs: display_rgb8, display_rgb (shaped like `lin`: [*shape, 3] or [K, *shape, 3]) and
    display_exposure; nothing without a transform.  shape: the frame's, (H, W) for a bloom."""
    if display is None:
        return {}
    if not isinstance(display, DisplayTransform):
        raise ValueError(f"display: a relight.DisplayTransform, got {display!r}")
    shape = tuple(int(v) for v in shape)
    if len(shape) != 2:
        if display.bloom_sigma > 0.0:
            raise ValueError(f"a bloom needs a frame of (H, W) pixels, not {shape}")
        n = 1
        for v in shape:
            n *= v
        shape = (1, n)
    res = display.apply(lin.reshape(-1, *shape, 3), mask)
    return {"display_rgb8": res["rgb8"].view(lin.shape), "display_rgb": res["rgb"].view(lin.shape), "display_exposure": res["exposure"]}
