"""The chunked full-frame render: the state of a frame and its one owner.

A frame is rendered in static-shape chunks whose forward is captured once in a HIP graph and replayed (`_ChunkRunner`).  What is decided
once per frame is a `FrameLight`; the model's `FrameRenderer` (`model.frames`) builds it in `begin`, holds it as `active` until `end`, and
owns what outlives a frame: the static device buffers, the rotations pinned per value and the cache of chunk runners.

A captured chunk reads a tensor through the pointer it was captured with.  So a value that may change between two frames served by one
graph lives in a static buffer allocated here once and overwritten by `begin`; a value the capture holds as a Python number or through a
pointer of its own is part of `FrameLight.key`, under which the runner is cached."""
from __future__ import annotations

from collections import namedtuple
from dataclasses import InitVar, dataclass, field
from typing import Any, Callable, Dict, Optional

import torch

from .. import hip, ops
from ..cameras.rays import RayBundle
from ..field_components.neusky_fieldheadnames import FieldHeadNames, NeuSkyFieldHeadNames
from ..relight.lighting import FrameLighting, light_colours
from ..relight.lights import lights_block, trace_light_shadows
from ..relight.props import PROP_BIAS, as_props, occlude_by_props, props_block
from ..relight.shadows import trace_params, trace_sun_shadows
from ..relight.transfer import bake_rows

# how what lights a chunk travels inside `shade`, the light's index leading: images [Kb, R, 3], one per sun (Kb = 1 for a frame without
# suns); the suns' maps [K, R]; the lamps' maps [L, R].  Every other output is per ray: [R, ...]
IMAGES = ("rgb", "lin", "atmosphere_inscatter")
SUN_MAPS = ("shadow_map", "shadow_difference", "shadow_status")
LIGHT_MAPS = ("light_visibility", "light_status")


# the static buffers of a frame, as FrameRenderer.static keeps them; a member that is none of the entry's own (`data`, `convention`, `scale`,
# `suns`, `steps`, `grace`: held by a captured chunk by value or by another's pointer) is None there and set per frame with _replace.
# the sky: dirs [D, 3], the frame camera's colours at them [1, D, 3], sel
FrameSky = namedtuple("FrameSky", "dirs cols sel")
# a relight.EnvironmentMap: its data and convention id, and the frame's rotation [3, 3] and the map's exposure [1]
FrameEnvmap = namedtuple("FrameEnvmap", "data convention rotation exposure")
# K suns: dirs, colours [K, 3], the thresholds [1], sel = int32 arange(K) (every sun direction is queried).  `scale` is a float, a
# by-value argument of nsky_visibility_finish_fwd
FrameSuns = namedtuple("FrameSuns", "dirs colours threshold acc_threshold sel scale")
# a relight.DaylightSky under the frame's K suns: lights [K, D, 3], the sky of each sun at the frame's D directions (nsky_daylight_eval
# there: point samples of the model, not cell averages); turbidity, exposure [1], ground [3]; suns = FrameSuns.dirs.  `packed` [5] is
# the allocation the three are views of: begin fills them with one copy into it, and nothing else reads it
FrameDaylight = namedtuple("FrameDaylight", "lights turbidity exposure ground suns packed")
# sun_shadows="sdf": the suns' shadows are marched through the SDF (relight/shadows.py).  params: the kernels' parameter block [6] (eps,
# relax, min_step, tan_half, radius, bias); steps and grace are Python numbers, by-value arguments of the step kernel
FrameTrace = namedtuple("FrameTrace", "params steps grace")
# L relight.PointLight inside the scene: block [L, 16] (include/neusky_hip.h), the accumulation threshold [1] and the parameter block
# [6] of their shadow march; steps and grace as FrameTrace's; shadows: whether the march runs at all (a Python bool)
FrameLights = namedtuple("FrameLights", "block acc_threshold params steps grace shadows")
# a relight.Atmosphere: params: the kernels' parameter block [12] (include/neusky_hip.h: every number of the medium); abar [Kb, 3]: the
# mean light colour of each base image's sky; samples: shaft_samples M, a Python number, a by-value argument of both kernels
FrameAtmosphere = namedtuple("FrameAtmosphere", "params abar samples")
# P relight.Prop placed in the frame: block [P, 16] (include/neusky_hip.h) and the parameter block [1]: prop_bias, the lift of a shadow
# ray's start point off the rendered surface.  Geometry, not light: it travels beside the FrameLighting, not in it
FrameProps = namedtuple("FrameProps", "block params")


@dataclass
class FrameLight:
    """the light of the active frame: directions [D, 3], the frame camera's colours at them [1, D, 3] and the upper-hemisphere subset, in
    static buffers; the camera and the (pinned) rotation of its latent; optionally an environment map, suns, a transfer-bake storage, a
    daylight sky (which takes the place of the latent's: `cols` is then not decoded and not read), a shadow march in place of the suns'
    DDF queries, lamps inside the scene on top of whichever of these lights it; `linear`: a frame under the sky alone also keeps its
    linear image `lin` (a sun frame and a frame with lamps or an atmosphere always do), for a display transform; a medium the frame is
    seen through, applied last; props placed in the scene, which are no light at all but travel with it into every chunk"""
    dirs: torch.Tensor
    cols: torch.Tensor
    sel: torch.Tensor
    cam: int
    rotation: Optional[torch.Tensor]
    rotation_values: InitVar[Optional[tuple]] = None  # of a latent's rotation, for the key (an envmap's is read from its static buffer)
    envmap: Optional[FrameEnvmap] = None
    sun: Optional[FrameSuns] = None
    bake: Optional[str] = None
    daylight: Optional[FrameDaylight] = None
    trace: Optional[FrameTrace] = None
    linear: bool = False
    lights: Optional[FrameLights] = None
    atmosphere: Optional[FrameAtmosphere] = None
    props: Optional[FrameProps] = None
    key: tuple = field(init=False)

    def __post_init__(self, rotation_values):
        """what a captured chunk holds by value or by a pointer that is not a static buffer's.  An envmap frame is keyed on the map's
        storage, shape and convention only, so a new rotation or exposure replays the chunk; a sun frame adds K and the sigmoid scale,
        so a new position, colour or threshold does; a daylight frame adds K once more and drops the camera, so a new turbidity,
        exposure, ground or camera does; a frame with marched shadows adds the march's length and leaving phase, so a new eps, bias or
        angular diameter does; a sky frame that keeps its linear image says so (its chunk has one more output); a frame with lamps adds
        their number, whether their shadows are marched and that march's length and leaving phase, so a new position, intensity, cone,
        radius, eps or bias replays the chunk; a frame seen through an atmosphere adds its shaft samples and nothing else, so a new
        density, height, albedo, anisotropy, far or background flag replays the chunk; a frame with props adds their number and nothing
        else, so a prop that moves, turns, changes size, colour or flags, or a new prop_bias, replays the chunk."""
        env = self.envmap
        key = (self.cam, rotation_values) if env is None else ("envmap", env.data.data_ptr(), tuple(env.data.shape), env.convention)
        if self.daylight is not None:  # no latent is read: one chunk graph serves every camera
            key = "daylight sky"
        if self.sun is not None:
            key = (key, "sun", self.sun.dirs.shape[0], self.sun.scale)
        if self.bake is not None:
            key = (key, "bake", self.bake)
        if self.daylight is not None:
            key = (key, "daylight", self.daylight.lights.shape[0])
        if self.trace is not None:
            key = (key, "sdf shadows", self.trace.steps, self.trace.grace)
        if self.linear and self.shading == "sky":
            key = (key, "linear")
        if self.lights is not None:
            key = (key, ("lights", self.lights.block.shape[0], self.lights.shadows, self.lights.steps, self.lights.grace))
        if self.atmosphere is not None:
            key = (key, ("atmosphere", self.atmosphere.samples))
        if self.props is not None:
            key = (key, ("props", self.props.block.shape[0]))
        self.key = key

    @property
    def shading(self) -> str:
        return "bake" if self.bake is not None else "daylight" if self.daylight is not None else "sun" if self.sun is not None else "sky"


def shade(model, light: FrameLight, so: Dict[str, Any], ray_bundle: RayBundle) -> Dict[str, torch.Tensor]:
    """what the active frame's shading mode adds to a chunk's outputs: `rgb` under the sky alone; `rgb`, `lin`, `shadow_map` and
    `shadow_difference` with suns, under the frame's sky or a daylight sky of each sun's own; the transfer keys and no `rgb` for a bake
    (no light enters).  A sky frame asked for its linear image adds `lin`: what the renderer's kernel computes beside `rgb` and drops.
    An atmosphere is applied last, to whatever lit the chunk, and never to a bake.  Between the functions below the outputs travel with
    the light's index leading; the chunk's own form is made here, once: ray-major views of that storage, [0] for a frame without suns."""
    if light.shading == "bake":
        fo = so["field_outputs"]
        visibility = sky_visibility(model, so)
        return bake_rows(fo[NeuSkyFieldHeadNames.ALBEDO], fo[FieldHeadNames.NORMALS], so["weights"][..., 0], so["illumination_directions"],
                         visibility, light.bake)
    if light.sun is not None:
        out = _sun_outputs(model, light.sun, so, ray_bundle, light.daylight, light.trace, light)
    elif light.linear or light.lights is not None or light.atmosphere is not None:  # (lamps and fog add to the linear image)
        out = _sky_outputs(model, so)
    else:
        out = {"rgb": model.render_lambertian(so)[None]}
    if light.lights is not None:
        out = _add_lights(model, light.lights, so, ray_bundle, out, light)
    if light.atmosphere is not None:
        out = _apply_atmosphere(model, light, so, ray_bundle, out)
    image = (lambda t: t.permute(1, 0, 2)) if light.sun is not None else (lambda t: t[0])
    return {k: image(v) if k in IMAGES else v.t() if k in SUN_MAPS + LIGHT_MAPS else v for k, v in out.items()}


def sky_visibility(model, so: Dict[str, Any]) -> Optional[torch.Tensor]:
    """the sky's visibility [R, D] of a chunk, or None: the DDF's, or, in a frame with props, the one their occlusion was applied to
    (sample_and_forward_field: ones times the occlusion on a model without a visibility field)"""
    if "prop_sky_visibility" in so:
        return so["prop_sky_visibility"]
    return so["visibility_dict"]["visibility"].contiguous() if model.config.use_visibility else None


def ray_points(origins: torch.Tensor, directions: torch.Tensor, depth: torch.Tensor) -> torch.Tensor:
    """the points [R, 3] a prop's shadow is looked up from: o + d depth in fp32, the product and the sum rounded once each"""
    return (origins.detach() + directions.detach() * depth.detach().reshape(-1, 1)).contiguous()


def _occluded(light: FrameLight, so: Dict[str, Any], vis: Optional[torch.Tensor], n: int, **towards) -> Optional[torch.Tensor]:
    """vis [n, R], a chunk's visibility of n lights from its rendered surface points (None: ones), times the props' occlusion towards
    them; untouched in a frame without props"""
    if light.props is None:
        return vis
    x = so["prop_points"]
    if vis is None:
        vis = torch.ones(n, x.shape[0], device=x.device)
    occlude_by_props(vis.t(), x, so["normal"].detach().contiguous(), light.props.params, light.props.block, **towards)
    return vis


def chunk_keys(lighting: FrameLighting, linear: bool = False):
    """(keys, sun_keys): the keys `shade` adds to a chunk of a frame lit by `lighting` (linear: FrameRenderer.begin's), and those of them
    that carry the K suns: ray-major [n, K, ...] in a chunk, K leading in the frame"""
    if lighting.bake is not None:
        return ("transfer", "transfer_acc") + (("transfer_exponents",) if lighting.bake == "fp16" else ()), ()
    suns, fogged = lighting.suns is not None, lighting.atmosphere is not None
    keys = ["rgb", "lin"] if suns or linear or lighting.lights or fogged else ["rgb"]  # (lamps and fog add to the linear image)
    if suns:
        keys += ["shadow_map", "shadow_difference"] + (["shadow_status"] if lighting.sun_shadows == "sdf" else [])
    if fogged:
        keys += ["atmosphere_transmittance", "atmosphere_inscatter"]  # (the inscatter is shaped as `lin`)
    if lighting.lights:
        keys += ["light_lin", "light_visibility"] + (["light_status"] if lighting.light_trace is not None else [])
    return tuple(keys), tuple(k for k in keys if suns and k in IMAGES + SUN_MAPS)


def _sky_outputs(model, so: Dict[str, Any]) -> Dict[str, torch.Tensor]:
    """render_lambertian's kernel on the same inputs, keeping both of its outputs: rgb (the same bits) and lin [1, R, 3]"""
    fo = so["field_outputs"]
    a, n = fo[NeuSkyFieldHeadNames.ALBEDO].contiguous(), fo[FieldHeadNames.NORMALS].contiguous()
    R, dev = a.shape[0], a.device
    rgb, lin = torch.empty(R, 3, device=dev), torch.empty(R, 3, device=dev)
    hip.hemi_composite_fwd(a, n, so["weights"][..., 0].contiguous(), so["illumination_directions"].contiguous(),
                           so["hdr_illumination_colours"].contiguous(), so["cam_of_ray"],
                           sky_visibility(model, so), so["hdr_background_colours"].contiguous(), rgb, lin)
    return {"rgb": rgb[None], "lin": lin[None]}


def _sun_outputs(model, sun: FrameSuns, so: Dict[str, Any], ray_bundle: RayBundle, daylight: Optional[FrameDaylight] = None,
                 trace: Optional[FrameTrace] = None, light: Optional[FrameLight] = None) -> Dict[str, torch.Tensor]:
    """a chunk lit by its sky and the frame's K suns (include/neusky_hip.h): the hemisphere kernel's linear image, one DDF query per
    (ray, sun), the sun transfer and the composite: rgb, lin [K, R, 3], shadow_map, shadow_difference [K, R].
    Under a daylight sky the linear image is one per sun [K, R, 3]: the chunk's radiance transfer (fp32, in a scratch) relit by the K
    skies at the frame's directions, over the K backgrounds sample_illumination_compact evaluated at the rays.
    With `trace` the K visibilities come from a march through the SDF instead of the DDF (whether or not the model has one), from the
    chunk's rendered depth along the ray and its rendered normal; `shadow_difference`, a DDF quantity, is then zero, and `shadow_status`
    [K, R] (int8) is the march's own verdict on each shadow ray (relight.shadows: HIT, ESCAPED, EXHAUSTED), before the set-sun and
    accumulation rules.  In a frame with props (`light`) the K visibilities, ones when there are none, are multiplied by the props'
    occlusion along the K sun directions before the composite: `shadow_map` shows the props' shadows too."""
    fo = so["field_outputs"]
    a, n = fo[NeuSkyFieldHeadNames.ALBEDO].contiguous(), fo[FieldHeadNames.NORMALS].contiguous()
    w = so["weights"][..., 0].contiguous()
    R, K, dev = a.shape[0], sun.dirs.shape[0], a.device
    use_visibility = model.config.use_visibility
    vis_sky = sky_visibility(model, so)
    if daylight is None:
        lin_sky = torch.empty(R, 3, device=dev)
        hip.hemi_composite_fwd(a, n, w, so["illumination_directions"].contiguous(), so["hdr_illumination_colours"].contiguous(),
                               so["cam_of_ray"], vis_sky, so["hdr_background_colours"].contiguous(), torch.empty(R, 3, device=dev), lin_sky)
    else:
        dirs = so["illumination_directions"].contiguous()
        T, t_acc = torch.empty(R, dirs.shape[0], 3, device=dev), torch.empty(R, device=dev)
        hip.transfer_bake(a, n, w, dirs, vis_sky, T, 0, None, t_acc)
        lin_sky = torch.empty(K, R, 3, device=dev)
        hip.transfer_relight(T, None, t_acc, daylight.lights, so["hdr_background_colours"], torch.empty(K, R, 3, device=dev), lin_sky)
    acc = so["accumulation"].reshape(-1).contiguous()
    vis = diff = status = None
    if trace is not None:
        march = trace_sun_shadows(model.field, ray_bundle.origins, ray_bundle.directions, so["p2p_dist"], so["normal"], sun.dirs, trace.params,
                                  trace.steps, trace.grace)
        vis, status = march.visibility, march.status
    elif use_visibility:
        vd = model.compute_visibility_compact(ray_bundle.origins, ray_bundle.directions, so["p2p_dist"].detach(), sun.dirs, sun.threshold,
                                              sun.scale, compute_shadow_map=True, sel=sun.sel)
        vis = vd["visibility"].t().contiguous()  # [K, R]
        diff = vd["difference"].view(R, K)
    if light is not None:
        vis = _occluded(light, so, vis, K, directions=sun.dirs)
    t = torch.empty(K, R, 3, device=dev)
    hip.sun_transfer(a, n, w, sun.dirs, t)
    rgb, lin, shadow = torch.empty(K, R, 3, device=dev), torch.empty(K, R, 3, device=dev), torch.empty(K, R, device=dev)
    hip.sun_composite(lin_sky, t, vis, acc, sun.acc_threshold, sun.dirs, sun.colours, rgb, lin, shadow)  # (one sky [R, 3], or a daylight sky each)
    on = (acc > sun.acc_threshold)[:, None] & (sun.dirs[:, 2] > 0)[None]
    diff = torch.where(on, diff, torch.zeros((), device=dev)) if diff is not None else torch.zeros(R, K, device=dev)
    out = {"rgb": rgb, "lin": lin, "shadow_map": shadow, "shadow_difference": diff.t()}
    if status is not None:
        out["shadow_status"] = status
    return out


def _add_lights(model, lights: FrameLights, so: Dict[str, Any], ray_bundle: RayBundle, out: Dict[str, torch.Tensor],
                light: Optional[FrameLight] = None) -> Dict[str, torch.Tensor]:
    """the frame's L lamps on top of a chunk lit by its sky or by sky and K suns (out: rgb, lin [Kb, R, 3]): the lamps' transfer at the
    samples' positions, a march from each ray's rendered surface point to each lamp (or none), and the composite, which adds the one
    lamp image to every base image (include/neusky_hip.h).  `rgb` and `lin` are replaced by the lit ones; light_lin [R, 3],
    light_visibility [L, R] and, with shadows, light_status [L, R] (int8) join them."""
    fo = so["field_outputs"]
    a, n = fo[NeuSkyFieldHeadNames.ALBEDO].contiguous(), fo[FieldHeadNames.NORMALS].contiguous()
    w = so["weights"][..., 0].contiguous()
    x = so["ray_samples"].frustums.get_positions().to(torch.float32).contiguous()
    R, L, dev = a.shape[0], lights.block.shape[0], a.device
    t = torch.empty(L, R, 3, device=dev)
    hip.light_transfer(x, a, n, w, lights.block, t)
    vis = status = None
    if lights.shadows:
        march = trace_light_shadows(model.field, ray_bundle.origins, ray_bundle.directions, so["p2p_dist"], so["normal"], lights.block,
                                    lights.params, lights.steps, lights.grace)
        vis, status = march.visibility, march.status
    if light is not None:  # (a prop between the point and the lamp; one behind the lamp shadows nothing)
        vis = _occluded(light, so, vis, L, lights=lights.block)
    base = out["lin"]
    rgb, lin, light_lin, V = torch.empty_like(base), torch.empty_like(base), torch.empty(R, 3, device=dev), torch.empty(L, R, device=dev)
    hip.lights_composite(base, t, vis, so["accumulation"].reshape(-1).contiguous(), lights.acc_threshold, lights.block, rgb, lin, light_lin, V)
    out = {**out, "rgb": rgb, "lin": lin, "light_lin": light_lin, "light_visibility": V}
    if status is not None:
        out["light_status"] = status
    return out


def _apply_atmosphere(model, light: FrameLight, so: Dict[str, Any], ray_bundle: RayBundle, out: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """the frame's medium in front of a lit chunk (include/neusky_hip.h: height fog): out holds rgb, lin [Kb, R, 3].  With shaft samples
    M the K suns are queried once more at M points along every ray, by the frame's own shadow mode: M R rows through the DDF (with no
    visibility network: no shadow, as for the surface) or through the march, which lifts a start point with no normal along the sun's
    direction.  `rgb` and `lin` are replaced by the fogged ones, `light_lin` is scaled in place; atmosphere_transmittance [R, 3] and
    atmosphere_inscatter (shaped as lin) join them."""
    atm, sun = light.atmosphere, light.sun
    suns, lin_in = sun is not None, out["lin"]
    Kb, R, dev = lin_in.shape[0], lin_in.shape[1], lin_in.device
    o, d = ray_bundle.origins.detach().contiguous(), ray_bundle.directions.detach().contiguous()
    M, vis = atm.samples, None
    props = light.props if suns else None  # (shafts are the suns': a sky frame has none to occlude)
    if M > 0 and (light.trace is not None or model.config.use_visibility or props is not None):
        rows_o, rows_d, rows_t = torch.empty(M * R, 3, device=dev), torch.empty(M * R, 3, device=dev), torch.empty(M * R, device=dev)
        hip.atmosphere_rows(o, d, atm.params, M, rows_o, rows_d, rows_t)
        if light.trace is not None:
            march = trace_sun_shadows(model.field, rows_o, rows_d, rows_t, torch.zeros(M * R, 3, device=dev), sun.dirs, light.trace.params,
                                      light.trace.steps, light.trace.grace)
            vis = march.visibility.view(Kb, M, R).permute(1, 0, 2)
        elif model.config.use_visibility:
            vd = model.compute_visibility_compact(rows_o, rows_d, rows_t[:, None], sun.dirs, sun.threshold, sun.scale, sel=sun.sel)
            vis = vd["visibility"].view(M, R, Kb).permute(0, 2, 1)
        else:
            vis = torch.ones(M, R, Kb, device=dev).permute(0, 2, 1)
        if props is not None:  # every (row, sun) entry, from the rows' own points; no normal, so no lift.  (a view, or an error)
            occlude_by_props(vis.permute(0, 2, 1).view(M * R, Kb), ray_points(rows_o, rows_d, rows_t), None, props.params, props.block,
                    directions=sun.dirs)
    rgb, lin, inscatter = torch.empty(Kb, R, 3, device=dev), torch.empty(Kb, R, 3, device=dev), torch.empty(Kb, R, 3, device=dev)
    transmittance = torch.empty(R, 3, device=dev)
    hip.atmosphere_apply(o, d, so["p2p_dist"].detach().reshape(-1).contiguous(), so["accumulation"].reshape(-1).contiguous(), lin_in,
                         so["hdr_background_colours"].contiguous(), atm.abar, sun.dirs if suns else None, sun.colours if suns else None, vis,
                         atm.params, M, lin, rgb, inscatter, transmittance, out.get("light_lin"))
    return {**out, "rgb": rgb, "lin": lin, "atmosphere_transmittance": transmittance, "atmosphere_inscatter": inscatter}


class FrameRenderer:
    """one per model (`model.frames`); plain Python, nothing of it is in the model's state_dict"""

    def __init__(self, model):
        self.model = model
        self.active: Optional[FrameLight] = None
        # the static buffers, one named tuple per key, kept for the model's lifetime (a captured chunk holds their pointers): "sky" ->
        # FrameSky; ("envmap", device) -> FrameEnvmap; ("suns", K, device) -> FrameSuns; ("daylight", K, D, device) -> FrameDaylight;
        # ("trace", device) -> FrameTrace; ("lights", L, device) -> FrameLights; ("atmosphere", Kb, device) -> FrameAtmosphere;
        # ("props", P, device) -> FrameProps.  Only "sky" is ever allocated again, on a new D or device, and takes the runners with it
        self.static: Dict[Any, tuple] = {}
        # a chunk graph cached under a rotation's values reads the rotation through the pointer it was captured with: the first tensor
        # seen with these values is kept, and serves every later frame that asks for them (one entry per value ever seen)
        self.rotations: Dict[tuple, torch.Tensor] = {}
        self.runners: Dict[tuple, "_ChunkRunner"] = {}  # (chunk, use_graph, key if use_graph else None) -> runner

    # ------------------------------------------------------------------ the frame's light
    def _static(self, key, allocate: Callable[[], tuple]) -> tuple:
        st = self.static.get(key)
        if st is None:
            st = self.static[key] = allocate()
        return st

    def begin(self, camera_index: int, lighting: FrameLighting, *, linear: bool = False, props=None, prop_bias: float = PROP_BIAS) -> None:
        """the device state of a frame lit by `lighting`, active until `end`: the rotation pinned, the static buffers filled.  linear: a
        frame under the sky alone keeps its linear image `lin` too (it joins the chunk runner's key only when set).  props: a
        relight.Prop or a sequence of them, placed in the scene; prop_bias: the lift of their shadow rays off the rendered surface"""
        model = self.model
        props = self._props(props, prop_bias, lighting)  # (refused before anything is written)
        rotation, envmap = lighting.rotation, lighting.envmap
        fixed = model.config.fix_test_illumination_directions
        dirs, sel = model.illumination_sampler.on_device(model.device, apply_random_rotation=False if fixed else None)
        cam = int(camera_index)
        values = None if (rotation is None or envmap is not None) else tuple(rotation.reshape(-1).tolist())
        if values is not None:
            rotation = self.rotations.setdefault(values, rotation)
        # (a daylight frame reads no `cols`: the camera's latent is not decoded, the buffer keeps what it held)
        cols = light_colours(model, dirs, cam, rotation, envmap)[None] if lighting.daylight is None else None
        # static per-model buffers: a chunk graph captured for one frame stays valid for the next (animation frames
        # only change the camera / rotation, render_animation.py:196-207)
        sky = self.static.get("sky")
        if sky is None or sky.dirs.shape != dirs.shape or sky.dirs.device != dirs.device:
            sky = self.static["sky"] = FrameSky(torch.empty_like(dirs), torch.zeros(1, *dirs.shape, dtype=dirs.dtype, device=dirs.device),
                                                torch.empty_like(sel))
            self.runners = {}  # (the dropped runners' graphs retire themselves: ops.CapturedGraph)
        sky.dirs.copy_(dirs); sky.sel.copy_(sel)
        if cols is not None:
            sky.cols.copy_(cols)
        suns = self._suns(lighting)
        daylight = self._daylight(lighting.daylight, sky.dirs, suns)
        self.active = FrameLight(sky.dirs, sky.cols, sky.sel, cam, rotation, values, self._envmap(envmap, rotation), suns, lighting.bake,
                                 daylight, self._trace(lighting.shadow_trace), bool(linear), self._lights(lighting),
                                 self._atmosphere(lighting.atmosphere, sky, suns, daylight), props)

    def _envmap(self, envmap, rotation) -> Optional[FrameEnvmap]:
        if envmap is None:
            return None
        dev = envmap.device
        st = self._static(("envmap", str(dev)), lambda: FrameEnvmap(None, None, torch.empty(3, 3, dtype=torch.float32, device=dev),
                                                                    torch.empty(1, dtype=torch.float32, device=dev)))
        if rotation is None:
            st.rotation.copy_(torch.eye(3, dtype=torch.float32))
        else:
            st.rotation.copy_(torch.as_tensor(rotation).reshape(3, 3))
        st.exposure.copy_(envmap.exposure_tensor)
        return st._replace(data=envmap.data, convention=envmap.convention_id)

    def _suns(self, lighting: FrameLighting) -> Optional[FrameSuns]:
        suns = lighting.suns
        if suns is None:
            return None
        model = self.model
        K, dev = len(suns), model.device
        st = self._static(("suns", K, str(dev)), lambda: FrameSuns(
            torch.empty(K, 3, device=dev), torch.empty(K, 3, device=dev), torch.empty(1, device=dev), torch.empty(1, device=dev),
            torch.arange(K, device=dev, dtype=torch.int32), None))
        st.dirs.copy_(torch.tensor([s.direction for s in suns], dtype=torch.float64).to(torch.float32))
        st.colours.copy_(torch.tensor([s.colour for s in suns], dtype=torch.float32))
        if lighting.shadow_threshold is None:
            st.threshold.copy_(model.visibility_threshold.detach() if model.config.use_visibility else torch.zeros(1))
        else:
            st.threshold.copy_(torch.tensor([float(lighting.shadow_threshold)]))
        st.acc_threshold.copy_(torch.tensor([float(lighting.accumulation_mask_threshold)]))
        scale = 0.0  # (a model without a visibility field has no sigmoid_scale: read it under use_visibility only)
        if model.config.use_visibility:
            scale = float(model.sigmoid_scale if lighting.shadow_sigmoid_scale is None else lighting.shadow_sigmoid_scale)
        return st._replace(scale=scale)

    def _daylight(self, daylight, dirs: torch.Tensor, suns: Optional[FrameSuns]) -> Optional[FrameDaylight]:
        if daylight is None:
            return None
        K, D, dev = suns.dirs.shape[0], dirs.shape[0], dirs.device

        def allocate():
            packed = torch.empty(5, device=dev)
            return FrameDaylight(torch.empty(K, D, 3, device=dev), packed[0:1], packed[1:2], packed[2:5], None, packed)
        st = self._static(("daylight", K, D, str(dev)), allocate)._replace(suns=suns.dirs)
        st.packed.copy_(torch.tensor([daylight.turbidity, daylight.exposure, *daylight.ground], dtype=torch.float32))
        hip.daylight_eval(dirs, st.suns, st.turbidity, st.exposure, st.ground, st.lights)
        return st

    def _trace(self, shadow_trace: Optional[dict]) -> Optional[FrameTrace]:
        """shadow_trace: FrameLighting's, every parameter of the march or None"""
        if shadow_trace is None:
            return None
        dev = self.model.device
        st = self._static(("trace", str(dev)), lambda: FrameTrace(torch.empty(hip.TRACE_PARAMS, device=dev), None, None))
        st.params.copy_(trace_params(shadow_trace))
        return st._replace(steps=shadow_trace["steps"], grace=shadow_trace["grace"])

    def _lights(self, lighting: FrameLighting) -> Optional[FrameLights]:
        lights = lighting.lights
        if not lights:
            return None
        L, dev = len(lights), self.model.device
        st = self._static(("lights", L, str(dev)), lambda: FrameLights(
            torch.empty(L, hip.LIGHT_FLOATS, device=dev), torch.empty(1, device=dev), torch.empty(hip.TRACE_PARAMS, device=dev), None, None,
            None))
        st.block.copy_(lights_block(lights))
        st.acc_threshold.copy_(torch.tensor([float(lighting.accumulation_mask_threshold)]))
        trace = lighting.light_trace
        if trace is None:
            return st._replace(steps=0, grace=0, shadows=False)
        st.params.copy_(trace_params(trace))
        return st._replace(steps=trace["steps"], grace=trace["grace"], shadows=True)

    def _atmosphere(self, atmosphere, sky: FrameSky, suns: Optional[FrameSuns], daylight: Optional[FrameDaylight]) -> Optional[FrameAtmosphere]:
        """the medium's parameter block, and the mean light colour of each base image's sky: of the frame's one sky under every sun, or
        of each sun's own daylight sky"""
        if atmosphere is None:
            return None
        Kb, dev = 1 if suns is None else suns.dirs.shape[0], sky.dirs.device
        st = self._static(("atmosphere", Kb, str(dev)), lambda: FrameAtmosphere(
            torch.empty(hip.ATMOSPHERE_FLOATS, device=dev), torch.empty(Kb, 3, device=dev), None))
        st.params.copy_(atmosphere.block())
        st.abar.copy_(sky.cols[0].mean(0, keepdim=True).expand(Kb, 3) if daylight is None else daylight.lights.mean(1))
        return st._replace(samples=atmosphere.shaft_samples)

    def _props(self, props, prop_bias: float, lighting: FrameLighting) -> Optional[FrameProps]:
        props = as_props(props)
        if not props:
            return None
        if lighting.bake is not None:
            raise ValueError("a bake keeps the scene's own transfer: props are placed in a rendered frame, not in a bake")
        bias = float(prop_bias)
        if not (bias >= 0.0 and bias < float("inf")):
            raise ValueError(f"prop_bias is finite and >= 0, got {prop_bias!r}")
        P, dev = len(props), self.model.device
        st = self._static(("props", P, str(dev)), lambda: FrameProps(torch.empty(P, hip.PROP_FLOATS, device=dev), torch.empty(1, device=dev)))
        st.block.copy_(props_block(props))
        st.params.copy_(torch.tensor([bias], dtype=torch.float32))
        return st

    def end(self) -> None:
        self.active = None

    # ------------------------------------------------------------------ chunks
    def runner(self, chunk: int, flat: RayBundle, use_graph: bool, cached: bool = True) -> "_ChunkRunner":
        """the chunk runner of the active frame.  The background term depends on (camera, rotation) through python values baked into a
        capture, so graphs are cached per (chunk, frame key); eager runners are free to share.  cached=False: a runner of the caller's
        own, which the caller retires."""
        if not cached:
            return _ChunkRunner(self.model, chunk, flat, use_graph)
        key = (chunk, use_graph, self.active.key if use_graph else None)
        runner = self.runners.get(key)
        if runner is None:
            runner = _ChunkRunner(self.model, chunk, flat, use_graph)
            if len(self.runners) >= 4:
                self.runners.clear()
            self.runners[key] = runner
        return runner

    @torch.no_grad()
    def render(self, camera_ray_bundle: RayBundle, lighting: FrameLighting, *, to_cpu: bool = False, camera_index: Optional[int] = None,
               chunk: Optional[int] = None, use_graph: bool = True, display=None, antialias=None,
               depth_of_field=None, props=None, prop_bias: float = PROP_BIAS) -> Dict[str, torch.Tensor]:
        """model.get_outputs_for_camera_ray_bundle, which documents the chunking and the outputs.  display: a relight.DisplayTransform of
        the frame's linear image, metered where the accumulation exceeds its meter_mask_threshold: adds display_rgb8, display_rgb and
        display_exposure (and, to a frame under the sky alone, its `lin`); it runs on the assembled frame, after the chunks, so its
        parameters touch no chunk graph.  antialias: a relight.Antialias: a second pass of sub-pixel rays through the pixels its edge rule
        marks, through the same runner and inside the same begin / end, resolved into `lin` (and `rgb` from it), `albedo`, `accumulation`
        and `shadow_map`; adds aa_mask and aa_fraction (and `lin` as `display` does); `display` then sees the resolved frame.  Under an
        atmosphere both see the fogged frame: every sub-pixel sample is fogged at its own depth; atmosphere_transmittance and
        atmosphere_inscatter stay the centre ray's, as `depth` does.  depth_of_field: a relight.DepthOfField: a second pass of thin-lens
        rays through the pixels a blurred pixel's disc reaches, through the same runner, resolved into the same keys; adds dof_coc,
        dof_mask, dof_fraction and dof_focus.  With antialias as well the edge mask is taken on the first pass, the lens pass runs, and
        the antialiasing pass takes the edge-marked pixels the lens did not mark (their lens samples are jittered inside the pixel
        already): aa_mask reports exactly those.  props, prop_bias: relight.Prop placed in the scene (`begin`): every output is then that of
        the scene with the props in it; adds prop_id (int32: the nearest visible prop the pixel's ray enters, -1 for none, whatever
        stands in front of it) and prop_weight (the share of the pixel that is the prop), which both second passes resolve as they
        do `accumulation`, keeping the centre ray's prop_id."""
        model = self.model
        assert not model.training, "call model.eval() first"
        chunk = chunk or max(model.config.eval_num_rays_per_chunk, 4096)
        shape = camera_ray_bundle.origins.shape[:-1]
        flat = camera_ray_bundle.slice(0, 1 << 62)
        num_rays = flat.origins.shape[0]
        if camera_index is None:
            camera_index = int(flat.camera_indices.reshape(-1)[0]) if flat.camera_indices is not None else 0
        if display is not None and lighting.bake is not None:
            raise ValueError("a bake takes the place of the shading: it has no image to display")
        if antialias is not None:
            from ..relight.antialias import Antialias, antialias_frame
            if not isinstance(antialias, Antialias):
                raise ValueError(f"antialias: a relight.Antialias, got {antialias!r}")
            if lighting.bake is not None:
                raise ValueError("a bake takes the place of the shading: antialias has no image to resolve")
            if len(shape) != 2:
                raise ValueError(f"antialias reads a pixel's neighbours: it needs the ray bundle of a frame, [H, W], not {tuple(shape)}")
        if depth_of_field is not None:
            from ..relight.depth_of_field import DepthOfField, depth_of_field_frame
            if not isinstance(depth_of_field, DepthOfField):
                raise ValueError(f"depth_of_field: a relight.DepthOfField, got {depth_of_field!r}")
            if lighting.bake is not None:
                raise ValueError("a bake takes the place of the shading: depth_of_field has no image to resolve")
            if len(shape) != 2 or shape[0] < 2 or shape[1] < 2:
                raise ValueError(f"a lens is made from the ray bundle of a frame, [H, W] with H, W >= 2, not {tuple(shape)}")
            depth_of_field.focus_index(int(shape[0]), int(shape[1]))  # (a focus pixel outside the frame: refused before anything runs)
        passes = antialias is not None or depth_of_field is not None
        linear = display is not None or passes
        self.begin(camera_index, lighting, linear=linear, props=props, prop_bias=prop_bias)
        suns = lighting.suns
        lit, sun_keys = chunk_keys(lighting, linear)
        keys = ["rgb", "albedo", "accumulation", "depth", "p2p_dist", "normal"] + [k for k in lit if k != "rgb"]
        if self.active.props is not None:
            keys += ["prop_id", "prop_weight"]
        out = {k: [] for k in keys}
        early = to_cpu and not passes  # (a second pass resolves on the device: its frame goes to the host afterwards)
        try:
            runner = self.runner(chunk, flat, use_graph)
            for i in range(0, num_rays, chunk):
                res = runner.run(flat, i, min(i + chunk, num_rays))
                for k in keys:
                    out[k].append(res[k].cpu() if early else res[k])
            if suns is not None:  # chunks are ray-major [n, K, ...]: K leads, and a single SunLight drops it
                K = len(suns)
                lead = () if lighting.single_sun else (K,)
                for k in sun_keys:
                    full = torch.cat(out.pop(k))
                    out[k] = [full.reshape(num_rays, K, -1).transpose(0, 1).reshape(*lead, *shape, -1)]
            res = {k: torch.cat(v).view(*shape, -1) if k not in sun_keys else v[0] for k, v in out.items()}
            K = 0 if suns is None else len(suns)
            edges = None
            if depth_of_field is not None:
                if antialias is not None:  # the edges of the first pass, before the lens resolves into it
                    edges = antialias.edge_mask(res["depth"], res["normal"], res["accumulation"], res["lin"])
                res.update(depth_of_field_frame(depth_of_field, runner, flat, shape, res, K))
                if edges is not None:
                    edges = edges * (1 - res["dof_mask"].view_as(edges))
            if antialias is not None:
                res.update(antialias_frame(antialias, runner, flat, shape, res, K, mask=edges))
            if passes and to_cpu:
                res = {k: v.cpu() if torch.is_tensor(v) else v for k, v in res.items()}
        finally:
            self.end()
        if display is not None:
            from ..relight.display import frame_display
            res.update(frame_display(display, res["lin"].to(self.model.device), shape, res["accumulation"].to(self.model.device)))
        return res


class _ChunkRunner:
    """static-shape forward of one render chunk, optionally captured in a HIP graph and replayed"""

    def __init__(self, model, chunk: int, flat: RayBundle, use_graph: bool):
        self.model, self.chunk, self.graph = model, chunk, None
        dev = flat.origins.device
        self.rb = RayBundle(origins=torch.zeros(chunk, 3, device=dev), directions=torch.zeros(chunk, 3, device=dev),
                            pixel_area=torch.ones(chunk, 1, device=dev), camera_indices=torch.zeros(chunk, 1, dtype=torch.long, device=dev),
                            metadata={"directions_norm": torch.ones(chunk, 1, device=dev)})
        self.rb.directions[:, 2] = 1.0
        if use_graph:
            self._load(flat, 0, min(chunk, flat.origins.shape[0]))
            self.graph = ops.CapturedGraph(dev, 2, lambda i: model.forward(self.rb))  # (retires itself when this runner is dropped)

    def _load(self, flat: RayBundle, a: int, b: int) -> None:
        n = b - a
        self.rb.origins[:n].copy_(flat.origins[a:b])
        self.rb.directions[:n].copy_(flat.directions[a:b])
        if "directions_norm" in flat.metadata:
            self.rb.metadata["directions_norm"][:n].copy_(flat.metadata["directions_norm"][a:b])
        if n < self.chunk:  # pad the last chunk with copies of its first ray (results discarded)
            self.rb.origins[n:].copy_(self.rb.origins[:1].expand(self.chunk - n, 3))
            self.rb.directions[n:].copy_(self.rb.directions[:1].expand(self.chunk - n, 3))

    def forward_rows(self, flat: RayBundle, a: int, b: int) -> Dict:
        """rows a:b of `flat` through the model: the chunk's whole output dictionary, NOT cloned (under a graph: its static outputs,
        overwritten by the next call), rows past b - a being padding"""
        self._load(flat, a, b)
        if self.graph is None:
            return self.model.forward(self.rb)
        self.graph.replay()
        return self.graph.outputs

    def retire(self) -> None:
        """for an owner that is done with the runner at a known point (bake_transfer), rather than when its last reference goes"""
        if self.graph is not None:
            self.graph.retire()

    def run(self, flat: RayBundle, a: int, b: int) -> Dict[str, torch.Tensor]:
        out = self.forward_rows(flat, a, b)
        return {k: v[:b - a].clone() for k, v in out.items() if torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == self.chunk}
