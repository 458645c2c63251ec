"""Adaptive antialiasing of a frame: a second pass of sub-pixel rays through the pixels an edge detector marks, resolved in linear light.
Definitions: include/neusky_hip.h ("Adaptive antialiasing of a frame"); kernels: csrc/antialias.hip.

The frame render takes one ray through every pixel centre.  With `antialias=Antialias(S)` it then reads the frame's own G-buffer (depth,
normal, accumulation) and its linear image, marks the pixels that differ from one of their 4 neighbours (`edge_mask`), traces S - 1 further
rays through each marked pixel (`subpixel_rays`: made from the ray bundle itself, no camera is needed) and averages the S samples of
`lin`, `albedo`, `accumulation` and `shadow_map` (`resolve`; with lamps `light_lin` and `light_visibility` too); `rgb` is the sRGB of the
resolved `lin`.  `depth`, `p2p_dist`, `normal`, `shadow_difference`, `shadow_status` and `light_status` stay the centre ray's.  `aa_mask` (uint8 [H, W, 1]) and `aa_fraction` (the share of marked pixels,
a Python float) join the outputs.

S = 4, the thresholds (colour 0.1, depth 0.02, normal 15 degrees, accumulation 0.1, covered 0.5) and the slices of 2^18 marked pixels are
design choices, not measurements.  The list of marked pixels is torch.nonzero of the mask: one host synchronisation per frame, for the
count that sizes the second pass.  `second_pass` is that pass without its mask: the slices, the chunks and the resolve, for any function
from a slice of marked pixels to their rays; the lens of depth_of_field.py runs through it too."""
from __future__ import annotations

import math
from dataclasses import dataclass
from functools import lru_cache
from typing import Dict, Optional

import torch

from ..cameras.rays import RayBundle

MAX_SAMPLES = 64
R2_G = 1.32471795724474602596  # the plastic number: the real root of g^3 = g + 1
# what the second pass's samples are averaged into (`rgb` follows `lin`); `light_*` are a frame's with `lights`, `prop_weight` one's with
# `props` (its `prop_id` stays the centre ray's)
RESOLVED_KEYS = ("lin", "albedo", "accumulation", "shadow_map", "light_lin", "light_visibility", "prop_weight")


def r2_offsets(samples: int) -> torch.Tensor:
    """float32 [samples - 1, 2]: o_s = frac(0.5 + s (1 / g, 1 / g^2)) - 0.5 for s = 1 .. samples - 1, the R2 low-discrepancy sequence about
    the pixel centre, in float64.  s = 0 would be the centre itself: the ray the first pass has traced."""
    s = torch.arange(1, int(samples), dtype=torch.float64)[:, None]
    a = torch.tensor([1.0 / R2_G, 1.0 / (R2_G * R2_G)], dtype=torch.float64)
    return (torch.frac(0.5 + s * a) - 0.5).to(torch.float32)


@lru_cache(maxsize=32)
def _device_r2(samples: int, device: str) -> torch.Tensor:
    return r2_offsets(samples).to(device)


@dataclass(frozen=True, eq=False)
class Antialias:
    """samples: per marked pixel, the centre ray included (2..64).
    colour, depth, normal_deg, accumulation, covered: the edge rule's thresholds (`edge_mask`): a relative difference of luminance, a
    relative difference of depth and an angle between normals (both among pixels whose accumulation exceeds `covered`), a difference of
    accumulation.
    every_pixel: mark every pixel: plain supersampling.
    offsets: the S - 1 sub-pixel offsets (dx, dy) in pixels, each component in [-0.5, 0.5], in place of the R2 sequence's.
    batch_pixels: the second pass runs over slices of at most this many marked pixels (whatever the slices, the same bits).
    (It may hold a tensor: like FrameLighting it has no `==` of its own.)"""
    samples: int = 4
    colour: float = 0.1
    depth: float = 0.02
    normal_deg: float = 15.0
    accumulation: float = 0.1
    covered: float = 0.5
    every_pixel: bool = False
    offsets: Optional[torch.Tensor] = None
    batch_pixels: int = 1 << 18

    def __post_init__(self):
        def integer(name, lo, hi=None):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int) or v < lo or (hi is not None and v > hi):
                bound = f"in {lo}..{hi}" if hi is not None else f">= {lo}"
                raise ValueError(f"{name} is an integer {bound}, got {v!r}")

        integer("samples", 2, MAX_SAMPLES)
        integer("batch_pixels", 1)
        for name in ("colour", "depth", "normal_deg", "accumulation", "covered"):
            try:
                v = float(getattr(self, name))
            except (TypeError, ValueError):
                raise ValueError(f"{name} is a number, got {getattr(self, name)!r}") from None
            if not math.isfinite(v) or v < 0.0:
                raise ValueError(f"{name} must be finite and >= 0, got {getattr(self, name)!r}")
            object.__setattr__(self, name, v)
        if not self.normal_deg < 90.0:
            raise ValueError(f"normal_deg must be < 90 degrees, got {self.normal_deg!r}")
        object.__setattr__(self, "every_pixel", bool(self.every_pixel))
        if self.offsets is not None:
            o = torch.as_tensor(self.offsets).detach().to(device="cpu", dtype=torch.float32)
            if tuple(o.shape) != (self.samples - 1, 2):
                raise ValueError(f"offsets: [samples - 1, 2] = [{self.samples - 1}, 2] sub-pixel offsets (dx, dy), got {tuple(o.shape)}")
            if not bool(torch.isfinite(o).all()) or bool((o.abs() > 0.5).any()):
                raise ValueError("offsets: every component lies in [-0.5, 0.5] (pixels about the centre)")
            object.__setattr__(self, "offsets", o.contiguous())

    @property
    def cos2(self) -> float:
        """cos^2(normal_deg), in float64: what the normal test compares with"""
        return math.cos(math.radians(self.normal_deg)) ** 2

    def sample_offsets(self, device="cpu") -> torch.Tensor:
        """float32 [samples - 1, 2] on `device`: the caller's offsets, or the R2 sequence's"""
        if self.offsets is None:
            return _device_r2(self.samples, str(device))
        return self.offsets.to(device)

    def edge_mask(self, depth: torch.Tensor, normal: torch.Tensor, accumulation: torch.Tensor, lin: Optional[torch.Tensor]) -> torch.Tensor:
        """uint8 [H, W] of a frame's depth [H, W, 1], normal [H, W, 3], accumulation [H, W, 1] and linear images [K, H, W, 3] ([H, W, 3]: one;
        None: no colour test): 1 where the rule of include/neusky_hip.h marks the pixel; all ones under every_pixel"""
        from .. import hip
        H, W = normal.shape[0], normal.shape[1]
        mask = torch.empty(H, W, dtype=torch.uint8, device=normal.device)
        if self.every_pixel:
            return mask.fill_(1)
        f = lambda t: t.detach().to(torch.float32).contiguous()  # noqa: E731
        # (the images through their strides: a frame of K suns is ray-major in memory, K leads in its shape alone)
        hip.aa_edge_mask(f(depth).view(H, W), f(normal), f(accumulation).view(H, W),
                         None if lin is None else lin.detach().to(torch.float32).view(-1, H * W, 3), self.accumulation, self.depth, self.cos2,
                         self.colour, self.covered, mask)
        return mask


def _subpixel_flat(flat: RayBundle, H: int, W: int, pixels: torch.Tensor, offsets: torch.Tensor) -> RayBundle:
    """subpixel_rays on a flat bundle of H W rays, `pixels` trusted (the frame render's own list)"""
    from .. import hip
    dev = flat.origins.device
    N = pixels.shape[0] * offsets.shape[0]
    norm = flat.metadata.get("directions_norm")
    out = RayBundle(origins=torch.empty(N, 3, device=dev), directions=torch.empty(N, 3, device=dev),
                    pixel_area=None if flat.pixel_area is None else torch.empty(N, 1, device=dev),
                    camera_indices=None if flat.camera_indices is None else torch.empty(N, 1, dtype=torch.long, device=dev),
                    metadata={"directions_norm": torch.empty(N, 1, device=dev)})
    hip.aa_subpixel_rays(flat.origins, flat.directions, norm, flat.pixel_area, flat.camera_indices, H, W, pixels, offsets, out.origins,
                         out.directions, out.metadata["directions_norm"], out.pixel_area, out.camera_indices)
    if offsets.shape[0] > 0:
        for name in ("nears", "fars"):  # not read by the frame render; carried for a caller that set them
            t = getattr(flat, name)
            if t is not None:
                setattr(out, name, t[pixels].repeat_interleave(offsets.shape[0], 0))
    return out


def subpixel_rays(ray_bundle: RayBundle, pixels: torch.Tensor, offsets: torch.Tensor) -> RayBundle:
    """the flat bundle [E (S - 1)] of the rays through pixels [E] (flat indices y W + x into the [H, W] bundle) at the sub-pixel offsets
    [S - 1, 2] = (dx, dy), pixel-major: row e (S - 1) + s.  With D = directions * directions_norm, D' = D + dx g_x + dy g_y from the
    bundle's own differences between neighbouring pixels: for a pinhole bundle the ray through (x + 0.5 + dx, y + 0.5 + dy)."""
    shape = tuple(ray_bundle.origins.shape[:-1])
    if len(shape) != 2:
        raise ValueError(f"sub-pixel rays are made from the bundle of a frame, [H, W]: got {shape}")
    H, W = shape
    dev = ray_bundle.origins.device
    pixels = torch.as_tensor(pixels, device=dev).to(torch.long).reshape(-1).contiguous()
    offsets = torch.as_tensor(offsets).to(device=dev, dtype=torch.float32)
    if offsets.dim() != 2 or offsets.shape[1] != 2:
        raise ValueError(f"offsets: [S - 1, 2], got {tuple(offsets.shape)}")
    if pixels.numel() and (int(pixels.min()) < 0 or int(pixels.max()) >= H * W):
        raise ValueError(f"pixels: flat indices into {H} x {W} pixels, got {int(pixels.min())}..{int(pixels.max())}")
    return _subpixel_flat(_flat_float(ray_bundle), H, W, pixels, offsets.contiguous())


def _flat_float(ray_bundle: RayBundle) -> RayBundle:
    """the bundle as contiguous rows: what the ray kernel indexes"""
    flat = ray_bundle.slice(0, 1 << 62)
    c = lambda t: None if t is None else t.contiguous()  # noqa: E731
    return RayBundle(c(flat.origins), c(flat.directions), c(flat.pixel_area), c(flat.camera_indices), c(flat.nears), c(flat.fars),
                     {k: c(v) for k, v in flat.metadata.items()})


def resolve(frame: torch.Tensor, samples: torch.Tensor, pixels: torch.Tensor, rgb: Optional[torch.Tensor] = None) -> None:
    """frame [K, P, C] (in place, through its strides: a frame of K suns is ray-major in memory) <- (frame + the sum of its S - 1 samples) / S
    at `pixels` [E]; samples [E, S - 1, K, C], as the second pass's chunks arrive (ray-major), any strides with a contiguous C; rgb
    [K, P, C]: also <- sRGB of what was written"""
    from .. import hip
    hip.aa_resolve(frame, samples.permute(2, 0, 1, 3), pixels, rgb)


def second_pass(runner, res: Dict[str, torch.Tensor], P: int, suns: int, pixels: torch.Tensor, rays, samples: int, batch_pixels: int) -> None:
    """a frame's further rays, between FrameRenderer.render's chunk loop and its `end`: res, the assembled first pass on the device (sun
    keys with K leading), is resolved in place at `pixels` [E] (ascending, pairwise distinct, not empty).  rays: a function from a slice of
    `pixels` to the flat bundle of its samples - 1 rays per pixel, pixel-major; samples: S, the first pass included.  suns: K, 0 for a
    frame under the sky alone.
    The rays form one pixel-major stream that is cut into the runner's chunks at multiples of its chunk size, wherever a slice of
    `batch_pixels` ends: a chunk that straddles two slices is run for each, so every ray sees the same chunk whatever the slices, and
    the same bits."""
    K, E = max(int(suns), 1), int(pixels.shape[0])
    S1, chunk = samples - 1, runner.chunk
    total = E * S1
    # key -> (the frame [K', P, C], its rgb or None, K' of the chunk's rows [n, K', C] or [n, C])
    frames = {}
    for k in RESOLVED_KEYS:
        if k in res:
            lead = K if (suns and k in ("lin", "shadow_map")) else 1
            frames[k] = (res[k].view(lead, P, -1), res["rgb"].view(lead, P, -1) if k == "lin" else None, lead)
    for a in range(0, E, batch_pixels):
        b = min(a + batch_pixels, E)
        r0, r1 = a * S1, b * S1  # this slice's rays in the stream
        c0, c1 = r0 // chunk, -(-r1 // chunk)  # the chunks that hold them
        g1 = min(c1 * chunk, total)
        pa, pb = c0 * chunk // S1, -(-g1 // S1)  # the pixels those chunks touch
        sub = rays(pixels[pa:pb])
        base = pa * S1
        X = {k: torch.empty(r1 - r0, lead, f.shape[-1], device=f.device) for k, (f, _, lead) in frames.items()}
        for c in range(c0, c1):
            lo, hi = c * chunk, min((c + 1) * chunk, total)
            out = runner.forward_rows(sub, lo - base, hi - base)
            u, v = max(lo, r0), min(hi, r1)
            for k, x in X.items():
                x[u - r0:v - r0].copy_(out[k][u - lo:v - lo].reshape(v - u, *x.shape[1:]))
        for k, (f, rgb, lead) in frames.items():
            resolve(f, X[k].view(b - a, S1, lead, -1), pixels[a:b], rgb)


def antialias_frame(antialias: Antialias, runner, flat: RayBundle, shape, res: Dict[str, torch.Tensor], suns: int,
                    mask: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """the antialiasing pass of FrameRenderer.render (`second_pass`): res is resolved in place; -> aa_mask, aa_fraction.  mask: uint8
    [H, W] in place of the edge mask of `res`: what a frame with a depth of field, which takes the edge mask on its first pass and
    leaves the pixels its lens marks to the lens, hands over."""
    H, W = (int(v) for v in shape)
    P = H * W
    given = mask is not None
    if not given:
        mask = antialias.edge_mask(res["depth"], res["normal"], res["accumulation"], res["lin"])
    if antialias.every_pixel and not given:
        pixels = torch.arange(P, device=mask.device)
    else:
        pixels = torch.nonzero(mask.view(-1)).view(-1)  # ascending; the one host synchronisation: the count sizes the second pass
    E = int(pixels.shape[0])
    added = {"aa_mask": mask.view(H, W, 1), "aa_fraction": E / max(P, 1)}
    if E == 0:
        return added
    flat = _flat_float(flat)
    offsets = antialias.sample_offsets(mask.device)
    second_pass(runner, res, P, suns, pixels, lambda px: _subpixel_flat(flat, H, W, px, offsets), antialias.samples, antialias.batch_pixels)
    return added
