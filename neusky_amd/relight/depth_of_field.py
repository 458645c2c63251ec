"""Thin-lens depth of field of a frame: a second pass of lens rays through the pixels a blurred pixel's disc reaches, resolved in linear light.
Definitions: include/neusky_hip.h ("Depth of field of a frame"); kernels: csrc/dof.hip.

The frame render's camera is a pinhole: its ray goes through the lens centre and the pixel centre, and every depth is sharp.  With
`depth_of_field=DepthOfField(aperture, ...)` that ray is sample 0.  The frame then reads its own `depth` and `accumulation`, computes a
circle of confusion per pixel (`circle_of_confusion`: the blur radius in pixels of a point at that depth, for a lens of radius `aperture`
focused at `focus_distance`, or on what the first pass saw at `focus_pixel`), marks every pixel that the disc of some blurred pixel reaches
(`mark_pixels`), traces S - 1 rays from points of the lens through each marked pixel (`lens_rays`: made from the ray bundle itself, no
camera is needed) and averages the S samples with the antialiasing pass's resolve, over the same keys.  `depth`, `p2p_dist`, `normal`, the
status maps and the atmosphere's two outputs stay the centre ray's.  `dof_coc` (float32 [H, W, 1]), `dof_mask` (uint8 [H, W, 1]),
`dof_fraction` (the share of marked pixels, a Python float) and `dof_focus` ([1]: 1 / z_f as used) join the outputs.

Two approximations.  `reach` caps how far a disc marks: a pixel blurred over more than `reach` pixels leaves sharp pixels further away
unmarked (the lens rays themselves are exact at any blur).  And the circle of confusion is the pinhole pass's: a surface that pass never
saw, hidden behind a foreground edge, can appear only inside marked regions.

S = 16, threshold 0.5 pixel, reach 16, covered 0.5 and the slices of 2^18 marked pixels are design choices, not measurements.  The list of
marked pixels is torch.nonzero of the mask: one host synchronisation per frame, for the count that sizes the second pass; the check that
the bundle is a pinhole's is read behind it."""
from __future__ import annotations

import math
from dataclasses import dataclass
from functools import lru_cache
from typing import Dict, NamedTuple, Optional, Tuple

import torch

from ..cameras.rays import RayBundle
from .antialias import MAX_SAMPLES, _flat_float, second_pass

MAX_REACH = 64
R4_G = 1.16730397826141868426  # the real root of g^5 = g + 1: the R2 sequence's constant in four dimensions
PINHOLE_TOLERANCE = 1e-3  # of |g|: how far a corner pixel's g_x, g_y may lie from the centre pixel's


def lens_table(samples: int) -> torch.Tensor:
    """float32 [samples - 1, 4] = (dx, dy, u, v) for s = 1 .. samples - 1, in float64: t = frac(0.5 + s (1 / g, 1 / g^2, 1 / g^3, 1 / g^4));
    (dx, dy) = (t_0, t_1) - 0.5 about the pixel centre; (u, v) the concentric map of (t_2, t_3) onto the unit disc: a point of the lens.
    s = 0 would be the first pass: the pixel centre through the lens centre."""
    s = torch.arange(1, int(samples), dtype=torch.float64)[:, None]
    t = torch.frac(0.5 + s * torch.tensor([R4_G ** -k for k in (1, 2, 3, 4)], dtype=torch.float64))
    a, b = 2.0 * t[:, 2] - 1.0, 2.0 * t[:, 3] - 1.0
    wide = a.abs() > b.abs()
    one = torch.ones_like(a)
    r = torch.where(wide, a, b)
    phi = torch.where(wide, (math.pi / 4.0) * (b / torch.where(wide, a, one)),
                      math.pi / 2.0 - (math.pi / 4.0) * (a / torch.where(b == 0.0, one, b)))
    u, v = r * torch.cos(phi), r * torch.sin(phi)
    return torch.stack([t[:, 0] - 0.5, t[:, 1] - 0.5, u, v], 1).to(torch.float32)


@lru_cache(maxsize=32)
def _device_table(samples: int, device: str) -> torch.Tensor:
    return lens_table(samples).to(device)


@dataclass(frozen=True, eq=False)
class DepthOfField:
    """aperture: the lens radius a in scene units (0: nothing is marked).
    focus_distance: z_f > 0, the depth of the plane in focus along the optical axis, in the units of the frame's `depth` output
    (p2p_dist / directions_norm: for a pinhole, the z-depth).  focus_pixel: (x, y) inside the frame: the plane goes through what the first
    pass saw there (read on the device; an uncovered pixel focuses at infinity).  They exclude each other; with neither, the centre
    pixel (W // 2, H // 2).
    samples: per marked pixel, the first pass's ray included (2..64).
    threshold, reach: a pixel blurred over at least `threshold` pixels marks the pixels of its disc, `reach` (1..64) pixels away at the most.
    covered: a pixel whose accumulation does not exceed it lies at infinity.
    every_pixel: mark every pixel.
    rotate: turn the lens pattern by an angle hashed from the pixel (without it every pixel repeats one pattern: S ghost images).
    table: the S - 1 rows (dx, dy, u, v), |dx|, |dy| <= 0.5 and u^2 + v^2 <= 1, in place of `lens_table`'s.
    batch_pixels: the second pass runs over slices of at most this many marked pixels (whatever the slices, the same bits).
    (It may hold a tensor: like Antialias it has no `==` of its own.)"""
    aperture: float
    focus_distance: Optional[float] = None
    focus_pixel: Optional[Tuple[int, int]] = None
    samples: int = 16
    threshold: float = 0.5
    reach: int = 16
    covered: float = 0.5
    every_pixel: bool = False
    rotate: bool = True
    table: Optional[torch.Tensor] = None
    batch_pixels: int = 1 << 18

    def __post_init__(self):
        def integer(name, lo, hi=None):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int) or v < lo or (hi is not None and v > hi):
                bound = f"in {lo}..{hi}" if hi is not None else f">= {lo}"
                raise ValueError(f"{name} is an integer {bound}, got {v!r}")

        def number(name):
            try:
                v = float(getattr(self, name))
            except (TypeError, ValueError):
                raise ValueError(f"{name} is a number, got {getattr(self, name)!r}") from None
            if isinstance(getattr(self, name), bool) or not math.isfinite(v) or v < 0.0:
                raise ValueError(f"{name} must be finite and >= 0, got {getattr(self, name)!r}")
            object.__setattr__(self, name, v)
            return v

        integer("samples", 2, MAX_SAMPLES)
        integer("reach", 1, MAX_REACH)
        integer("batch_pixels", 1)
        for name in ("aperture", "threshold", "covered"):
            number(name)
        if self.focus_distance is not None and self.focus_pixel is not None:
            raise ValueError("focus_distance and focus_pixel exclude each other: the plane in focus is given once")
        if self.focus_distance is not None and not number("focus_distance") > 0.0:
            raise ValueError(f"focus_distance must be > 0, got {self.focus_distance!r}")
        if self.focus_pixel is not None:
            try:
                x, y = self.focus_pixel
            except (TypeError, ValueError):
                raise ValueError(f"focus_pixel is a pixel (x, y), got {self.focus_pixel!r}") from None
            if any(isinstance(v, bool) or not isinstance(v, int) or v < 0 for v in (x, y)):
                raise ValueError(f"focus_pixel is a pixel (x, y) of integers >= 0, got {self.focus_pixel!r}")
            object.__setattr__(self, "focus_pixel", (x, y))
        object.__setattr__(self, "every_pixel", bool(self.every_pixel))
        object.__setattr__(self, "rotate", bool(self.rotate))
        if self.table is not None:
            t = torch.as_tensor(self.table).detach().to(device="cpu", dtype=torch.float32)
            if tuple(t.shape) != (self.samples - 1, 4):
                raise ValueError(f"table: [samples - 1, 4] = [{self.samples - 1}, 4] rows (dx, dy, u, v), got {tuple(t.shape)}")
            d = t.double()
            if not bool(torch.isfinite(t).all()) or bool((d[:, :2].abs() > 0.5).any()):
                raise ValueError("table: dx and dy lie in [-0.5, 0.5] (pixels about the centre)")
            if bool((d[:, 2] ** 2 + d[:, 3] ** 2 > 1.0 + 1e-6).any()):  # (1e-6: the rounding of a point on the rim to float32)
                raise ValueError("table: (u, v) is a point of the unit disc, u^2 + v^2 <= 1")
            object.__setattr__(self, "table", t.contiguous())

    def sample_table(self, device="cpu") -> torch.Tensor:
        """float32 [samples - 1, 4] on `device`: the caller's table, or `lens_table`'s"""
        if self.table is None:
            return _device_table(self.samples, str(device))
        return self.table.to(device)

    def focus_index(self, H: int, W: int) -> int:
        """the flat index of the pixel the focus is read at; -1 under a focus_distance"""
        if self.focus_distance is not None:
            return -1
        x, y = (W // 2, H // 2) if self.focus_pixel is None else self.focus_pixel
        if not (x < W and y < H):
            raise ValueError(f"focus_pixel {(x, y)} lies outside the frame of {W} x {H} pixels")
        return y * W + x


class LensFrame(NamedTuple):
    """the lens of a frame's bundle, float64 on the bundle's device: the image plane's axes r^, s^ [3], the optical axis w^ [3], the focal
    length in pixels f_px [], and `bent` (bool []): whether a corner pixel's g_x or g_y differs from the centre's: not a pinhole's bundle"""
    r: torch.Tensor
    s: torch.Tensor
    w: torch.Tensor
    f_px: torch.Tensor
    bent: torch.Tensor


def _frame_shape(ray_bundle: RayBundle) -> Tuple[int, int]:
    shape = tuple(ray_bundle.origins.shape[:-1])
    if len(shape) != 2 or shape[0] < 2 or shape[1] < 2:
        raise ValueError(f"a lens is made from the bundle of a frame, [H, W] with H, W >= 2: got {shape}")
    return shape


def _lens_frame(flat: RayBundle, H: int, W: int) -> LensFrame:
    """lens_frame on a flat bundle of H W rays; nothing is read on the host: `bent` is the caller's to read"""
    D = flat.directions.detach().double()
    norm = flat.metadata.get("directions_norm")
    if norm is not None:
        D = D * norm.detach().double()
    D = D.view(H, W, 3)

    def g(y, x):
        a, b = (x if x + 1 < W else x - 1), (y if y + 1 < H else y - 1)  # forward differences; backward in the last column and row
        return D[y, a + 1] - D[y, a], D[b + 1, x] - D[b, x]

    cy, cx = H // 2, W // 2
    gx, gy = g(cy, cx)
    lx, ly = gx.norm(), gy.norm()
    bent = ~(torch.isfinite(lx) & torch.isfinite(ly) & (lx > 0) & (ly > 0))
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        hx, hy = g(y, x)
        bent = bent | ~((hx - gx).norm() <= PINHOLE_TOLERANCE * lx) | ~((hy - gy).norm() <= PINHOLE_TOLERANCE * ly)
    r, s = gx / lx, gy / ly
    w = torch.linalg.cross(r, s)
    w = torch.where((D[cy, cx] * w).sum() > 0, w, -w)
    return LensFrame(r, s, w, 1.0 / lx, bent)


NOT_A_PINHOLE = ("the bundle is not a pinhole's: g_x or g_y at a corner pixel differs from the centre pixel's by more than 1e-3 of its "
                 "length (perspective cameras only: a depth of field needs one lens)")


def lens_frame(ray_bundle: RayBundle) -> LensFrame:
    """the lens of the bundle [H, W] of a frame, from the bundle alone (include/neusky_hip.h, "lens"); a ValueError for a bundle that is
    not a pinhole's"""
    H, W = _frame_shape(ray_bundle)
    frame = _lens_frame(_flat_float(ray_bundle), H, W)
    if bool(frame.bent):
        raise ValueError(NOT_A_PINHOLE)
    return frame


def lens_block(frame: LensFrame, aperture: float, focus=0.0) -> torch.Tensor:
    """float32 [12] on the frame's device: r^, s^, w^, a, 1 / z_f, a f_px, rounded once from float64.  focus: 1 / z_f, a number or a
    device tensor [1] (`dof_focus`); the frame render leaves 0 there for `circle_of_confusion` to fill from the focus pixel"""
    dev = frame.r.device
    a = torch.tensor([float(aperture)], dtype=torch.float64, device=dev)
    izf = focus.detach().to(device=dev, dtype=torch.float64).reshape(1) if torch.is_tensor(focus) else torch.tensor(
        [float(focus)], dtype=torch.float64, device=dev)
    return torch.cat([frame.r, frame.s, frame.w, a, izf, a * frame.f_px.reshape(1)]).to(torch.float32)


def circle_of_confusion(depth: torch.Tensor, accumulation: torch.Tensor, lens: torch.Tensor, focus_pixel: int = -1,
                        covered: float = 0.5) -> torch.Tensor:
    """float32 [H, W] of a frame's depth and accumulation [H, W, 1] (or [H, W]) and its lens block [12]: c = (a f_px) |1 / depth - 1 / z_f|,
    an uncovered pixel at infinity.  focus_pixel >= 0 (a flat index): 1 / z_f is read from that pixel and written into lens[10]"""
    from .. import hip
    H, W = depth.shape[0], depth.shape[1]
    f = lambda t: t.detach().to(torch.float32).contiguous().view(H, W)  # noqa: E731
    coc = torch.empty(H, W, dtype=torch.float32, device=depth.device)
    hip.dof_coc(f(depth), f(accumulation), lens, focus_pixel, covered, coc)
    return coc


def mark_pixels(coc: torch.Tensor, threshold: float = 0.5, reach: int = 16) -> torch.Tensor:
    """uint8 [H, W] of the circles of confusion [H, W]: 1 where some pixel q within `reach` has c_q >= threshold and c_q + 0.5 >= the
    Chebyshev distance to it"""
    from .. import hip
    mask = torch.empty(coc.shape, dtype=torch.uint8, device=coc.device)
    hip.dof_mark(coc, float(threshold), reach, mask)
    return mask


def _lens_flat(flat: RayBundle, H: int, W: int, pixels: torch.Tensor, table: torch.Tensor, lens: torch.Tensor, rotate: bool) -> RayBundle:
    """lens_rays on a flat bundle of H W rays, `pixels` trusted (the frame render's own list)"""
    from .. import hip
    dev = flat.origins.device
    N = pixels.shape[0] * table.shape[0]
    out = RayBundle(origins=torch.empty(N, 3, device=dev), directions=torch.empty(N, 3, device=dev),
                    pixel_area=None if flat.pixel_area is None else torch.empty(N, 1, device=dev),
                    camera_indices=None if flat.camera_indices is None else torch.empty(N, 1, dtype=torch.long, device=dev),
                    metadata={"directions_norm": torch.empty(N, 1, device=dev)})
    hip.dof_lens_rays(flat.origins, flat.directions, flat.metadata.get("directions_norm"), flat.pixel_area, flat.camera_indices, H, W, pixels,
                      table, lens, rotate, out.origins, out.directions, out.metadata["directions_norm"], out.pixel_area, out.camera_indices)
    if table.shape[0] > 0:
        for name in ("nears", "fars"):  # not read by the frame render; carried for a caller that set them
            t = getattr(flat, name)
            if t is not None:
                setattr(out, name, t[pixels].repeat_interleave(table.shape[0], 0))
    return out


def lens_rays(ray_bundle: RayBundle, pixels: torch.Tensor, dof: DepthOfField, focus=None) -> RayBundle:
    """the flat bundle [E (S - 1)] of the thin-lens rays through pixels [E] (flat indices y W + x into the [H, W] bundle), pixel-major: row
    e (S - 1) + s is row s of the lens table.  focus: 1 / z_f, a number or a tensor [1] (a frame's `dof_focus`); by default
    1 / dof.focus_distance (a focus pixel needs the first pass it is read from: give that frame's `dof_focus`).  Every ray of a pixel
    passes through the pixel's point on the plane in focus; `depth` along it stays the z-depth."""
    H, W = _frame_shape(ray_bundle)
    if not isinstance(dof, DepthOfField):
        raise ValueError(f"dof: a relight.DepthOfField, got {dof!r}")
    if focus is None:
        if dof.focus_distance is None:
            raise ValueError("a focus pixel is read from a frame's first pass: give focus=, that frame's dof_focus (1 / z_f)")
        focus = 1.0 / dof.focus_distance
    dev = ray_bundle.origins.device
    pixels = torch.as_tensor(pixels, device=dev).to(torch.long).reshape(-1).contiguous()
    if pixels.numel() and (int(pixels.min()) < 0 or int(pixels.max()) >= H * W):
        raise ValueError(f"pixels: flat indices into {H} x {W} pixels, got {int(pixels.min())}..{int(pixels.max())}")
    flat = _flat_float(ray_bundle)
    frame = _lens_frame(flat, H, W)
    if bool(frame.bent):
        raise ValueError(NOT_A_PINHOLE)
    return _lens_flat(flat, H, W, pixels, dof.sample_table(dev).contiguous(), lens_block(frame, dof.aperture, focus), dof.rotate)


def depth_of_field_frame(dof: DepthOfField, runner, flat: RayBundle, shape, res: Dict[str, torch.Tensor], suns: int) -> Dict[str, torch.Tensor]:
    """the lens pass of FrameRenderer.render, between its chunk loop and `end` (antialias.second_pass): res, the assembled first pass on the
    device, is resolved in place; -> dof_coc, dof_mask, dof_fraction, dof_focus.  suns: K, 0 for a frame under the sky alone."""
    H, W = (int(v) for v in shape)
    P = H * W
    flat = _flat_float(flat)
    frame = _lens_frame(flat, H, W)
    lens = lens_block(frame, dof.aperture, 0.0 if dof.focus_distance is None else 1.0 / dof.focus_distance)
    coc = circle_of_confusion(res["depth"], res["accumulation"], lens, dof.focus_index(H, W), dof.covered)
    dev = coc.device
    if dof.every_pixel:
        mask = torch.ones(H, W, dtype=torch.uint8, device=dev)
        pixels = torch.arange(P, device=dev)
    else:
        # (a lens of radius 0 blurs nothing: c = 0 everywhere, which a threshold of 0 would mark)
        mask = torch.zeros(H, W, dtype=torch.uint8, device=dev) if dof.aperture == 0.0 else mark_pixels(coc, dof.threshold, dof.reach)
        pixels = torch.nonzero(mask.view(-1)).view(-1)  # ascending; the one host synchronisation: the count sizes the second pass
    if bool(frame.bent):  # (read behind the list: the device has drained)
        raise ValueError(NOT_A_PINHOLE)
    E = int(pixels.shape[0])
    added = {"dof_coc": coc.view(H, W, 1), "dof_mask": mask.view(H, W, 1), "dof_fraction": E / max(P, 1), "dof_focus": lens[10:11].clone()}
    if E == 0:
        return added
    table = dof.sample_table(dev).contiguous()
    second_pass(runner, res, P, suns, pixels, lambda px: _lens_flat(flat, H, W, px, table, lens, dof.rotate), dof.samples, dof.batch_pixels)
    return added
