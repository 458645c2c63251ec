"""The lighting of one rendered frame as one value: `FrameLighting`, what a caller may say about a frame's light, normalised and checked
once (`FrameLighting.of`), and the light's two constructions the frame render and a transfer's relight share (`light_colours`,
`ray_background`).  `models/frame.py` turns a `FrameLighting` into the device state of a frame (`FrameRenderer.begin`)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Optional, Tuple

import torch

from .. import hip
from .atmosphere import Atmosphere
from .envmap import project_envmap
from .lights import LIGHT_TRACE_DEFAULTS, PointLight, as_lights
from .shadows import SHADOW_DEFAULTS, trace_settings
from .sun import SunLight, as_suns

COLLIDER_RADIUS = 1.0  # of NeuSkyModel.collider: the scene bound of a shadow march


@dataclass(frozen=True, eq=False)
class FrameLighting:
    """Build one with `FrameLighting.of`, which takes the keywords of get_outputs_for_camera_ray_bundle and holds the rules between
    them; vary one with dataclasses.replace (a new rotation, new suns), which checks nothing.  It holds tensors and a dictionary: it
    has no hash and no `==` of its own, and is compared field by field."""
    __hash__ = None

    rotation: Optional[torch.Tensor] = None
    """[3, 3]: turns the camera's illumination latent, or the `envmap` (direction d is then lit by the map at R d)"""
    envmap: Any = None
    """a relight.EnvironmentMap to light the frame with instead of the camera's illumination latent: the light colours are the map's
    cell averages at the frame's directions (relight.project_envmap), the rays' background its bilinear lookup"""
    daylight: Any = None
    """a relight.DaylightSky: a clear sky that follows the sun, in place of the latent's or a map's (needs `suns`, excludes `envmap`,
    `rotation` and `bake`; the camera's latent is not decoded).  Each of the K suns then has its own sky at the frame's light
    directions (point samples of the model), its own background behind the rays and, from DaylightSky.sun / sun_path, its own colour;
    the outputs are those of a sun frame, and a set sun's frame is black.  The field, the sampler and the visibility pass of a chunk
    still run once for all K."""
    bake: Optional[str] = None
    """the storage of a radiance-transfer bake (relight.bake_transfer), which takes the place of the shading"""
    suns: Optional[Tuple[SunLight, ...]] = None
    """K relight.SunLight on top of either sky (include/neusky_hip.h: a directional sun).  `rgb` is then the frame lit by sky and sun,
    and `lin` (its linear image), `shadow_map` and `shadow_difference` [*shape, 1] join the outputs.  The field, the sampler and the
    sky pass of a chunk run once for all K suns.  A sun with elevation <= 0 has set: it adds no light and no shadow."""
    single_sun: bool = True
    """whether one SunLight rather than a sequence was given: a sequence puts a leading K on the suns' four outputs"""
    shadow_threshold: Optional[float] = None
    """of the DDF shadow; None: the model's trained visibility threshold"""
    shadow_sigmoid_scale: Optional[float] = None
    """of the DDF shadow; None: the model's sigmoid scale"""
    accumulation_mask_threshold: float = 0.0
    """the shadow is masked by accumulation > accumulation_mask_threshold"""
    sun_shadows: str = "ddf"
    """"ddf" (the default: one DDF query per ray and sun) or "sdf": the suns' shadow rays are sphere-traced through the SDF field
    (relight.shadows, include/neusky_hip.h), from each ray's rendered depth and normal; this needs no visibility network
    (use_visibility = False renders too).  The shadow then follows the surface the mesh export writes and has a penumbra of the sun's
    angular diameter.  `shadow_difference`, a DDF quantity, is all zeros in this mode, and `shadow_status` [*shape, 1] (int8:
    relight.shadows.HIT / ESCAPED / EXHAUSTED, the march's verdict before the set-sun and accumulation rules) joins the outputs.
    shadow_threshold and shadow_sigmoid_scale are errors with it."""
    shadow_trace: Optional[dict] = None
    """with "sdf", every parameter of the march (relight.shadows.SHADOW_DEFAULTS, checked by trace_settings): steps, eps, relax,
    min_step, grace, radius (default: the sphere collider's), angular_diameter_deg (0 gives a hard edge) and bias (the lift of the
    start point off the rendered surface along its normal, scene units); None under "ddf".  Only steps and grace are held by a
    captured chunk: the others replay it."""
    # a frame with lamps is a LitFrameLighting, which adds these three as fields; a frame without them is this value, field for field
    lights = None
    light_shadows = True
    light_trace = None
    # a frame seen through a medium is a FoggedFrameLighting (or a FoggedLitFrameLighting), which adds this one as a field
    atmosphere = None

    @classmethod
    def of(cls, rotation: Optional[torch.Tensor] = None, envmap=None, sun=None, shadow_threshold: Optional[float] = None,
           shadow_sigmoid_scale: Optional[float] = None, accumulation_mask_threshold: float = 0.0, bake: Optional[str] = None,
           daylight=None, sun_shadows: str = "ddf", shadow_trace: Optional[dict] = None, lights=None, light_shadows: bool = True,
           light_trace: Optional[dict] = None, atmosphere: Optional[Atmosphere] = None) -> "FrameLighting":
        """sun: one SunLight or a sequence of K; shadow_trace: any of SHADOW_DEFAULTS' keys, the rest take their defaults; lights: one
        PointLight or a sequence of L (None or empty: none); light_trace: any of LIGHT_TRACE_DEFAULTS' keys; atmosphere: a
        relight.Atmosphere or None"""
        if sun_shadows not in ("ddf", "sdf"):
            raise ValueError(f"sun_shadows: 'ddf' or 'sdf', got {sun_shadows!r}")
        if sun_shadows == "sdf":
            if sun is None or bake is not None:
                raise ValueError("sun_shadows='sdf' marches the shadow rays of a sun: give `sun` (and no bake)")
            if shadow_threshold is not None or shadow_sigmoid_scale is not None:
                raise ValueError("shadow_threshold and shadow_sigmoid_scale shape the DDF shadow: they exclude sun_shadows='sdf'")
        elif shadow_trace is not None:
            raise ValueError("shadow_trace holds the parameters of the march: it needs sun_shadows='sdf'")
        if daylight is not None:
            if sun is None:
                raise ValueError("daylight: the sky follows a sun: give `sun`, one SunLight or K (DaylightSky.sun, DaylightSky.sun_path)")
            if envmap is not None or rotation is not None or bake is not None:
                raise ValueError("daylight takes the place of the latent's or the map's sky: it excludes envmap, rotation and a bake")
        suns, single = (None, True) if sun is None else as_suns(sun)
        if sun_shadows == "sdf":
            shadow_trace = trace_settings(shadow_trace, {**SHADOW_DEFAULTS, "radius": COLLIDER_RADIUS})
        lights = as_lights(lights) or None
        if lights is None or not light_shadows:
            if light_trace is not None:
                raise ValueError("light_trace holds the parameters of the lamps' shadow march: it needs `lights` with light_shadows=True")
        else:
            light_trace = trace_settings(light_trace, {**LIGHT_TRACE_DEFAULTS, "radius": COLLIDER_RADIUS})
        if lights is not None and bake is not None:
            raise ValueError("a bake holds the transfer of lights at infinity: it excludes `lights`")
        if atmosphere is not None:
            if not isinstance(atmosphere, Atmosphere):
                raise ValueError(f"atmosphere: a relight.Atmosphere, got {atmosphere!r}")
            if bake is not None:
                raise ValueError("a bake takes the place of the shading: it has no image for an atmosphere to fog")
            if atmosphere.shaft_samples > 0 and suns is None:
                raise ValueError("shaft_samples shadows the suns' in-scatter: it needs `sun`")
        base = (rotation, envmap, daylight, bake, None if suns is None else tuple(suns), single, shadow_threshold, shadow_sigmoid_scale,
                accumulation_mask_threshold, sun_shadows, shadow_trace)
        if lights is None:
            return cls(*base) if atmosphere is None else FoggedFrameLighting(*base, atmosphere)
        lit = (*base, lights, bool(light_shadows), light_trace)
        return LitFrameLighting(*lit) if atmosphere is None else FoggedLitFrameLighting(*lit, atmosphere)


@dataclass(frozen=True, eq=False)
class LitFrameLighting(FrameLighting):
    """what FrameLighting.of builds when lamps are given: a FrameLighting with their three fields"""
    __hash__ = None

    lights: Optional[Tuple[PointLight, ...]] = None
    """L relight.PointLight inside the scene (include/neusky_hip.h: point and spot lights), added to the frame of any sky and of each of
    K suns: `rgb` and `lin` are then lit by them too, and `light_lin` [*shape, 3] (their share of `lin`) and `light_visibility`
    [*shape, L] join the outputs.  They go with the sky alone, `envmap`, `rotation`, suns, `daylight` and both `sun_shadows` modes, and
    exclude `bake`.  None: the frame without the feature."""
    light_shadows: bool = True
    """the lamps' shadow rays are sphere-traced through the SDF field, each to its lamp (relight.lights); `light_status` [*shape, L]
    (int8, the march's verdicts) then joins the outputs.  False: `light_visibility` is the accumulation mask alone."""
    light_trace: Optional[dict] = None
    """with lights and light_shadows, every parameter of that march (relight.lights.LIGHT_TRACE_DEFAULTS, checked by trace_settings):
    steps, eps, relax, min_step, grace, radius and bias; None otherwise.  Only steps and grace are held by a captured chunk."""


@dataclass(frozen=True, eq=False)
class FoggedFrameLighting(FrameLighting):
    """what FrameLighting.of builds when an atmosphere is given and no lamps: a FrameLighting with its field"""
    __hash__ = None

    atmosphere: Optional[Atmosphere] = None
    """a relight.Atmosphere (include/neusky_hip.h: height fog): fog or haze between the camera and the frame, applied last, to the image
    of any sky, of each of K suns and of the lamps: `rgb` and `lin` are then seen through it, and `atmosphere_transmittance`
    [*shape, 3] and `atmosphere_inscatter` (shaped as `lin`) join the outputs.  It goes with everything but `bake`; shaft_samples > 0
    needs `suns`, whose shadow mode then shadows their in-scatter too.  None: the frame without the feature."""


@dataclass(frozen=True, eq=False)
class FoggedLitFrameLighting(LitFrameLighting):
    """what FrameLighting.of builds when lamps and an atmosphere are given: a LitFrameLighting with FoggedFrameLighting's field"""
    __hash__ = None

    atmosphere: Optional[Atmosphere] = None


def light_colours(model, dirs: torch.Tensor, cam: int, rotation: Optional[torch.Tensor] = None, envmap=None) -> torch.Tensor:
    """[D, 3]: the light at the frame's directions, of camera `cam`'s latent (turned by `rotation`) or of a relight.EnvironmentMap: the
    map's cell averages (relight.project_envmap)"""
    if envmap is not None:
        return project_envmap(envmap, dirs, rotation)[0]
    latents, scales = model.get_illumination_field()
    if rotation is None:
        return model.illumination_field.forward_grid(dirs, latents[cam][None], scales[cam][None])[0]
    return model.illumination_field.forward_camera(dirs, latents[cam], scales[cam], rotation)


def ray_background(model, ray_directions: torch.Tensor, cam: int, rotation: Optional[torch.Tensor] = None, envmap=None,
                   daylight=None) -> torch.Tensor:
    """[R, 3]: the sky behind the rays, of camera `cam`'s latent (turned by `rotation`) or of the frame's environment map (a
    models/frame.py FrameEnvmap: its bilinear lookup, read through the static buffers); under a daylight sky (a FrameDaylight)
    [K, R, 3]: the sky of each of the frame's suns"""
    if daylight is not None:
        bg = torch.empty(daylight.suns.shape[0], ray_directions.shape[0], 3, dtype=torch.float32, device=ray_directions.device)
        hip.daylight_eval(ray_directions.contiguous(), daylight.suns, daylight.turbidity, daylight.exposure, daylight.ground, bg)
        return bg
    if envmap is not None:
        bg = torch.empty(ray_directions.shape[0], 3, dtype=torch.float32, device=ray_directions.device)
        hip.envmap_lookup(envmap.data, envmap.convention, ray_directions.contiguous(), envmap.rotation, envmap.exposure, bg)
        return bg
    latents, scales = model.get_illumination_field()
    return model.illumination_field.forward_camera(ray_directions, latents[cam], scales[cam], rotation)
