"""The run of python -m neusky_amd.relight, in five pieces.  `frame_plan`: which renders serve a camera's frames (a `Shot` is one call of a
renderer).  `RenderSource` and `BakedSource`: a shot's frames, as `Frame` records, from model.frames.render and from a baked transfer's
relight.  `FrameWriter`: every output file of a frame, and the frames that wait for their camera's exposure.  `Tally`: what the closing
lines count.  Exposures, the shares of marked pixels and the SH residual stay device tensors until `Tally.report`."""
from __future__ import annotations

import dataclasses
import math
import os
import time
from typing import Any, List, NamedTuple, Optional

import numpy as np
import torch
from PIL import Image

from .depth_of_field import DepthOfField
from .display import DisplayTransform
from .envmap import z_rotation
from .io import srgb_to_linear
from .props import PROP_BIAS
from .shadows import EXHAUSTED
from .transfer import LIGHTS_PER_PASS, bake_transfer
from .transfer_sh import bake_transfer_sh


class Shot(NamedTuple):
    """one call of a renderer: the frames it yields and what differs from the run's base lighting"""
    frames: range
    angles: tuple  # the illumination's turn about +z, radians, one per rotation the call takes; None: exactly none
    lamp: Optional[tuple] = None  # where the first lamp stands, if it moves
    sweep: bool = False  # one render under all the suns of a path: a frame per sun
    prop: Optional[tuple] = None  # where the first prop stands, if it moves


def frame_plan(turntable: int, rotation_deg: float, suns: Optional[list], sun_path: bool, light_path: Optional[list],
               transfer: str, prop_path: Optional[list] = None) -> List[Shot]:
    """The shots of one camera, in order; their frames are 0..F-1, each once.  A moving prop: a render per position, all at the first
    rotation, first sun and first lamp position.  A moving lamp: a render per position, all at the first
    rotation (a sun path of one step under it is one sun, suns[0]).  A sun path: one render that yields a frame per sun.  A baked
    transfer: one relight pass per LIGHTS_PER_PASS rotations of the turntable.  Else a render per rotation of the turntable."""
    def angle(f):
        a = math.radians(rotation_deg) + 2.0 * math.pi * f / turntable
        return None if a == 0.0 else a

    if prop_path is not None:
        lamp = None if light_path is None else tuple(light_path[0])
        return [Shot(range(f, f + 1), (angle(0),), lamp=lamp, prop=tuple(p)) for f, p in enumerate(prop_path)]
    if light_path is not None:
        return [Shot(range(f, f + 1), (angle(0),), lamp=tuple(p)) for f, p in enumerate(light_path)]
    if sun_path:
        return [Shot(range(len(suns)), (angle(0),), sweep=True)]
    step = 1 if transfer == "off" else LIGHTS_PER_PASS
    spans = [range(f, min(f + step, turntable)) for f in range(0, turntable, step)]
    return [Shot(span, tuple(angle(f) for f in span)) for span in spans]


def turn(angle: Optional[float], device) -> Optional[torch.Tensor]:
    """the rotation of one of a shot's angles, on the device"""
    return None if angle is None else z_rotation(angle).to(device)


@dataclasses.dataclass
class Frame:
    """what a writer needs of one frame; what the run does not have is None"""
    camera: int
    index: int
    rgb: Optional[np.ndarray] = None  # the clamped float image on the host, where the host reads it at all
    lin: Optional[torch.Tensor] = None  # with a display transform: the linear image, its 8-bit picture and the meter's mask, on the device
    rgb8: Optional[torch.Tensor] = None
    mask: Optional[torch.Tensor] = None
    shadow: Optional[torch.Tensor] = None  # the sun's shadow map
    light_lin: Optional[torch.Tensor] = None  # the lamps' share of `lin`
    aa_mask: Optional[torch.Tensor] = None  # (a sweep's frames come from one render: they share its mask)
    exposure: Optional[torch.Tensor] = None  # with a display transform and lamps: what the render showed the frame at, for the lamps' picture
    transmittance: Optional[torch.Tensor] = None  # under an atmosphere: T to each ray's depth (a sweep's frames share it)
    inscatter: Optional[torch.Tensor] = None  # under an atmosphere: what the medium added to the frame's `lin`
    coc: Optional[torch.Tensor] = None  # with a depth of field: the circle of confusion in pixels (a sweep's frames share it)
    prop_weight: Optional[torch.Tensor] = None  # with props: the share of each pixel that is a prop (a sweep's frames share it)


class Tally:
    """what the closing lines report; sources and writer add to it, main times the run"""

    def __init__(self, t_load: float = 0.0):
        self.t_load, self.t_render, self.t_bake, self.t_relight = t_load, 0.0, 0.0, 0.0
        self.frames = 0
        self.exposures, self.marked = [], []  # device tensors, read once, in report; marked: of --antialias, every render's share of marked pixels
        self.shadow_rays = self.exhausted = 0  # of --sun-shadows sdf
        self.light_rays = self.light_exhausted = 0  # of the lamps' shadow march
        self.sh_residual = self.sh_store = None  # of --sh-order: the largest light_residual so far, and a camera's (coefficients, bytes)
        self.transmittances = []  # of --fog-density: every render's mean transmittance, device tensors
        self.focuses, self.lens_marked = [], []  # of --dof-aperture: every render's 1 / z_f (device tensors) and share of marked pixels
        self.prop_shares = []  # of the props: every render's share of pixels with prop_weight > 0.5, device tensors

    def report(self, args, size, display, antialias, shadow_trace, lights, light_trace, atmosphere=None, suns: int = 0,
               ddf_shadows: bool = True, depth_of_field=None, props=None) -> None:
        """size: the frames' (width, height); shadow_trace: of --sun-shadows sdf, else None; suns: per render; ddf_shadows: whether the
        model has a visibility network (without one the DDF mode shadows nothing); the rest as the parse_* functions return them"""
        transfer = "" if args.transfer == "off" else f" | transfer {args.transfer}: bake {self.t_bake:.3f}s relight {self.t_relight:.3f}s"
        if self.sh_residual is not None:
            transfer += (f" | sh order {args.sh_order} ({self.sh_store[0]} coefficients, {self.sh_store[1] / 1e6:.1f} MB per camera): "
                         f"largest light_residual {float(self.sh_residual):.3e}")
        print(f"{args.output_dir}: {self.frames} frames {size[0]}x{size[1]} | load {self.t_load:.3f}s render {self.t_render:.3f}s "
              f"({self.t_render / max(self.frames, 1):.3f}s/frame){transfer}")
        if display is not None and self.exposures:
            E = torch.cat([e.reshape(-1) for e in self.exposures])
            how = "set" if not display.metered else "metered per frame" if display.exposure == "frame" else "metered per camera"
            print(f"display: tonemap {display.curve} | exposure {how}: smallest {float(E.min()):.4g} largest {float(E.max()):.4g}")
        if antialias is not None and self.marked:
            how = "every pixel" if antialias.every_pixel else "the pixels its edge rule marks"
            print(f"antialias: {antialias.samples} samples through {how} | share of marked pixels: smallest {min(self.marked):.4g} "
                  f"largest {max(self.marked):.4g}")
        if depth_of_field is not None and self.lens_marked:
            how = "every pixel" if depth_of_field.every_pixel else "the pixels a blurred pixel's disc reaches"
            z = [1.0 / v if v > 0.0 else math.inf for v in torch.cat([f.reshape(-1) for f in self.focuses]).tolist()]
            print(f"depth of field: {depth_of_field.samples} samples through {how} | focus distance: smallest {min(z):.4g} largest {max(z):.4g} "
                  f"| share of marked pixels: smallest {min(self.lens_marked):.4g} largest {max(self.lens_marked):.4g}")
        still = "{} of {} shadow rays ({:.3f}%) were still marching after {} steps (raise {} if that is too many)"
        if shadow_trace is not None:
            share = 100.0 * self.exhausted / max(self.shadow_rays, 1)
            print("sdf shadows: " + still.format(self.exhausted, self.shadow_rays, share, shadow_trace["steps"], "--shadow-steps"))
        if lights is not None:
            share = 100.0 * self.light_exhausted / max(self.light_rays, 1)
            marched = "no shadows" if light_trace is None else still.format(self.light_exhausted, self.light_rays, share, light_trace["steps"],
                                                                            "--light-shadow-steps")
            print(f"lights: {len(lights)} lamp{'s' if len(lights) > 1 else ''} | {marched}")
        if atmosphere is not None and self.transmittances:
            T = torch.stack(self.transmittances)
            rows = atmosphere.extra_shadow_rows(suns)
            if rows == 0:
                what = "no shafts"
            elif shadow_trace is None and not ddf_shadows:
                what = f"{atmosphere.shaft_samples} shaft samples, unshadowed (the model has no visibility network): no extra rows"
            else:
                what = (f"{atmosphere.shaft_samples} shaft samples x {suns} sun{'s' if suns > 1 else ''}: {rows} extra "
                        f"{'DDF rows' if shadow_trace is None else 'marched shadow rays'} per ray")
            print(f"fog: mean transmittance smallest {float(T.min()):.4g} largest {float(T.max()):.4g} | {what}")
        if props is not None and self.prop_shares:
            share = torch.stack(self.prop_shares)
            print(f"props: {len(props)} prop{'s' if len(props) > 1 else ''} | share of pixels with prop_weight > 0.5: smallest "
                  f"{float(share.min()):.4g} largest {float(share.max()):.4g}")


class RenderSource:
    """a shot's frames from model.frames.render: direct renders, sweeps, moving lamps, and extracted suns, which turn with their map.
    base: the run's FrameLighting; a shot replaces its rotation and, with them, the extracted sun and the first lamp.  props: the
    run's relight.Prop, which travel beside the lighting; a shot replaces the first one's position."""

    def __init__(self, model, base, tally: Tally, *, chunk: int, display, antialias, extraction, floats: bool, deferred: bool,
                 depth_of_field=None, props=None, prop_bias: float = PROP_BIAS):
        self.props, self.prop_bias = props, prop_bias
        self.model, self.base, self.tally, self.chunk, self.extraction = model, base, tally, chunk, extraction
        self.display, self.floats, self.deferred = display, floats, deferred
        self.camera = self.rays = None  # of `open`
        self.shown = {k: v for k, v in (("display", display), ("antialias", antialias), ("depth_of_field", depth_of_field)) if v is not None}

    def open(self, camera: int, rays) -> None:
        self.camera, self.rays = camera, rays

    def frames(self, shot: Shot):
        base, tally, display = self.base, self.tally, self.display
        rot = turn(shot.angles[0], self.rays.origins.device)
        turned = {} if self.extraction is None else {"suns": (self.extraction.sun(rot),)}
        if shot.lamp is not None:
            turned["lights"] = (dataclasses.replace(base.lights[0], position=shot.lamp),) + tuple(base.lights[1:])
        placed = {}
        if self.props is not None:
            first = self.props[0] if shot.prop is None else self.props[0].moved_to(shot.prop)
            placed = {"props": (first,) + tuple(self.props[1:]), "prop_bias": self.prop_bias}
        out = self.model.frames.render(self.rays, dataclasses.replace(base, rotation=rot, **turned), camera_index=0, chunk=self.chunk,
                                       **self.shown, **placed)
        if placed:
            tally.prop_shares.append((out["prop_weight"] > 0.5).to(torch.float32).mean())
        if base.light_trace is not None:
            tally.light_rays += out["light_status"].numel()
            tally.light_exhausted += int((out["light_status"] == EXHAUSTED).sum())
        if base.suns is not None and base.sun_shadows == "sdf":  # (a sweep's status holds all its frames)
            tally.shadow_rays += out["shadow_status"].numel()
            tally.exhausted += int((out["shadow_status"] == EXHAUSTED).sum())
        if display is not None and not self.deferred:
            tally.exposures.append(out["display_exposure"])
        if "antialias" in self.shown:
            tally.marked.append(out["aa_fraction"])
        lens = "depth_of_field" in self.shown
        if lens:
            tally.focuses.append(out["dof_focus"])
            tally.lens_marked.append(out["dof_fraction"])
        fogged = base.atmosphere is not None
        if fogged:
            tally.transmittances.append(out["atmosphere_transmittance"].mean())
        for i, f in enumerate(shot.frames):
            own = (lambda k: out[k][i]) if shot.sweep else out.__getitem__  # (a sweep's images lead with its frames)
            frame = Frame(self.camera, f, shadow=own("shadow_map") if base.suns is not None else None,
                          light_lin=out["light_lin"] if base.lights else None, aa_mask=out["aa_mask"] if "antialias" in self.shown else None,
                          transmittance=out["atmosphere_transmittance"] if fogged else None,
                          inscatter=own("atmosphere_inscatter") if fogged else None, coc=out["dof_coc"] if lens else None,
                          prop_weight=out["prop_weight"] if placed else None)
            if self.floats:
                frame.rgb = own("rgb").clamp(0.0, 1.0).cpu().numpy()
            if display is not None:
                frame.lin, frame.rgb8, frame.mask = own("lin"), own("display_rgb8"), out["accumulation"]
                if base.lights:
                    frame.exposure = out["display_exposure"].reshape(-1)[i:i + 1] if shot.sweep else out["display_exposure"]
            yield frame


class BakedSource:
    """a shot's frames from a camera's radiance transfer, baked when the camera opens: one relight pass per shot"""

    def __init__(self, model, envmap, tally: Tally, *, storage: str, sh_order: Optional[int], chunk: int, display, floats: bool, deferred: bool):
        self.model, self.envmap, self.tally, self.storage, self.sh_order = model, envmap, tally, storage, sh_order
        self.chunk, self.display, self.floats, self.deferred = chunk, display, floats, deferred
        self.camera = self.baked = None  # of `open`

    def open(self, camera: int, rays) -> None:
        tb = time.perf_counter()
        if self.sh_order is None:
            self.baked = bake_transfer(self.model, rays, storage=self.storage, chunk=self.chunk, camera_index=0)
        else:
            self.baked = bake_transfer_sh(self.model, rays, order=self.sh_order, storage=self.storage, chunk=self.chunk, camera_index=0)
            self.tally.sh_store = (self.baked.C.shape[1], self.baked.nbytes)
        torch.cuda.synchronize()
        self.tally.t_bake += time.perf_counter() - tb
        self.camera = camera

    def frames(self, shot: Shot):
        tally, display = self.tally, self.display
        tr = time.perf_counter()
        shown = {} if display is None else {"display": display, "return_linear": True}
        rotations = [turn(a, self.baked.device) for a in shot.angles]
        relit = self.baked.relight(self.model, envmap=self.envmap, camera_index=0, rotations=rotations, **shown)
        if display is not None and not self.deferred:
            tally.exposures.append(relit["display_exposure"])
        if self.sh_order is not None:
            worst = relit["light_residual"].max()
            tally.sh_residual = worst if tally.sh_residual is None else torch.maximum(tally.sh_residual, worst)
        batch = relit["rgb"].clamp(0.0, 1.0).cpu().numpy() if self.floats else None
        tally.t_relight += time.perf_counter() - tr
        for i, f in enumerate(shot.frames):
            frame = Frame(self.camera, f, rgb=None if batch is None else batch[i])
            if display is not None:  # (no lamps under a transfer: nothing takes a frame's exposure)
                frame.lin, frame.rgb8, frame.mask = relit["linear"][i], relit["display_rgb8"][i], self.baked.acc
            yield frame


class FrameWriter:
    """Every output file of a run.  Without a display transform a frame's PNG is the renderer's clipped image, rounded on the host; with
    one it is the transform's 8-bit output.  deferred (--auto-exposure sequence over frames that are not rendered together): a camera's
    frames are metered into one histogram as they come and wait, as linear images on the device, for end_camera and its one exposure.
    The lamps' share of a frame goes through the frame's own path to a picture."""

    def __init__(self, args, display, tally: Tally):
        """args: output_dir, sun_path and the flags save_hdr, save_linear, shadow_map, aa_mask, light_map, fog_map, dof_map (and dof_reach, its scale).  What the sources ask the
        writer: floats, whether anything reads a frame's float image on the host, and deferred: under "sequence" the frames of a sun
        path are metered by the one render that yields them; any others are not rendered together, and wait"""
        self.args, self.display, self.tally = args, display, tally
        self.floats = display is None or args.save_hdr
        self.deferred = display is not None and display.exposure == "sequence" and args.sun_path is None
        self.pending: List[Frame] = []
        self.hist: Any = None

    def _path(self, kind: str, frame: Frame, suffix: str) -> str:
        return os.path.join(self.args.output_dir, f"{kind}_{frame.camera:04d}_{frame.index:03d}{suffix}")

    def write(self, frame: Frame) -> None:
        args = self.args
        if self.display is None:
            Image.fromarray(np.round(frame.rgb * 255.0).astype(np.uint8)).save(self._path("frame", frame, ".png"))
            self._lamps(frame, DisplayTransform(), None)  # (the default transform is the sRGB curve and 8 bits)
        elif self.deferred:
            self.hist = self.display.luminance_histogram(frame.lin, frame.mask, out=self.hist)  # (the first call makes the [1, 3072] the rest add to)
            self.pending.append(Frame(frame.camera, frame.index, lin=frame.lin, light_lin=frame.light_lin))  # (what end_camera reads)
        else:
            self._shown(frame, frame.rgb8, frame.exposure)
        if args.save_hdr:
            np.save(self._path("frame", frame, ".npy"), srgb_to_linear(frame.rgb).astype(np.float32))
        if args.shadow_map and frame.shadow is not None:  # (--extract-sun that found nothing has no shadow to write)
            grey = np.round(frame.shadow[..., 0].clamp(0.0, 1.0).cpu().numpy() * 255.0).astype(np.uint8)
            Image.fromarray(grey, mode="L").save(self._path("shadow", frame, ".png"))
        if args.aa_mask and frame.aa_mask is not None:
            Image.fromarray(frame.aa_mask[..., 0].cpu().numpy() * np.uint8(255), mode="L").save(self._path("aa", frame, ".png"))
        if frame.coc is not None and getattr(args, "dof_map", False):
            reach = self.args.dof_reach if getattr(self.args, "dof_reach", None) is not None else DepthOfField.reach
            c8 = torch.round((frame.coc[..., 0] / reach).clamp(0.0, 1.0).nan_to_num(0.0) * 255.0).to(torch.uint8)
            Image.fromarray(c8.cpu().numpy(), mode="L").save(self._path("coc", frame, ".png"))
        if frame.prop_weight is not None and getattr(args, "prop_mask", False):
            w8 = torch.round(frame.prop_weight[..., 0].clamp(0.0, 1.0).nan_to_num(0.0) * 255.0).to(torch.uint8)
            Image.fromarray(w8.cpu().numpy(), mode="L").save(self._path("prop", frame, ".png"))
        if frame.transmittance is not None:
            if args.fog_map:
                T8 = np.round(frame.transmittance.clamp(0.0, 1.0).cpu().numpy() * 255.0).astype(np.uint8)
                Image.fromarray(T8).save(self._path("fog", frame, ".png"))
            if args.save_linear:
                np.save(self._path("frame", frame, ".inscatter.npy"), frame.inscatter.cpu().numpy())
        self.tally.frames += 1

    def _shown(self, frame: Frame, rgb8: torch.Tensor, exposure: Optional[torch.Tensor]) -> None:
        """a frame's picture from its display transform, and its lamps' at the same exposure"""
        Image.fromarray(rgb8.cpu().numpy()).save(self._path("frame", frame, ".png"))
        if self.args.save_linear:
            np.save(self._path("frame", frame, ".lin.npy"), frame.lin.cpu().numpy())
        self._lamps(frame, self.display, exposure)

    def _lamps(self, frame: Frame, transform: DisplayTransform, exposure: Optional[torch.Tensor]) -> None:
        if frame.light_lin is None:
            return
        if self.args.light_map:
            rgb8 = transform.apply(frame.light_lin, exposure=exposure)["rgb8"]
            Image.fromarray(rgb8.cpu().numpy()).save(self._path("lights", frame, ".png"))
        if self.args.save_linear:
            np.save(self._path("frame", frame, ".lights.npy"), frame.light_lin.cpu().numpy())

    def end_camera(self) -> None:
        if self.pending:
            E = self.display.exposure_from_histogram(self.hist)
            self.tally.exposures.append(E)
            for frame in self.pending:
                self._shown(frame, self.display.apply(frame.lin, exposure=E)["rgb8"], E)
            self.pending, self.hist = [], None
