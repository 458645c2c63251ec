"""python -m neusky_amd.relight: render a checkpoint's scene along a nerfstudio camera path, lit by an HDR environment map (or by one of
its training illumination latents, or by a clear-sky daylight model that follows the sun), as 8-bit sRGB PNG frames.

The pipeline is built from the `neusky` method's config with no dataset: the scene box comes from the checkpoint's `_model.field.aabb`,
the numbers of train / eval latent rows and the latent dimension from its latent tables."""
from __future__ import annotations

import argparse
import dataclasses
import math
import os
import sys
import time

from .sun import SUN_ANGULAR_DIAMETER_DEG


def build_pipeline(state, device):
    """the `neusky` method's pipeline sized from a checkpoint's state dict, on a stand-in datamanager (no dataset)"""
    import copy

    import torch

    from ..configs.neusky_config import NeuSky
    from ..data.synthetic_datamanager import SyntheticDataManagerConfig

    train = state.get("_model.train_illumination_latents")
    if train is None:
        raise SystemExit("checkpoint has no _model.train_illumination_latents")
    evals = state.get("_model.eval_illumination_latents", train[:1])
    aabb = state["_model.field.aabb"].float() if "_model.field.aabb" in state else torch.tensor([[-1.0] * 3, [1.0] * 3])

    class _BoxedConfig(SyntheticDataManagerConfig):
        def setup(self, **kwargs):
            dm = super().setup(**kwargs)
            box = {"aabb": aabb.clone()}
            dm.train_dataset.scene_box = box
            dm.eval_dataset.scene_box = box
            return dm

    cfg = copy.deepcopy(NeuSky.config.pipeline)
    cfg.datamanager = _BoxedConfig(num_train_images=int(train.shape[0]), num_eval_images=int(evals.shape[0]))
    cfg.model.illumination_field.latent_dim = int(train.shape[1])
    return cfg.setup(device=device)


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m neusky_amd.relight", description=__doc__.splitlines()[0])
    ap.add_argument("--checkpoint", required=True, help="a nerfstudio-layout checkpoint (step-*.ckpt) of the neusky method")
    ap.add_argument("--camera-path", required=True, help="nerfstudio camera_path.json (perspective cameras)")
    ap.add_argument("--output-dir", required=True)
    light = ap.add_mutually_exclusive_group(required=True)
    light.add_argument("--envmap", help="equirectangular map: .hdr/.pic, .pfm, .npy, .png/.jpg (sRGB), .exr (with pyexr)")
    light.add_argument("--latent-index", type=int, help="light with this training illumination latent instead")
    light.add_argument("--daylight", action="store_true",
                       help="light with a clear-sky daylight model instead: sky, sun colour and background follow the sun (relight.DaylightSky)")
    ap.add_argument("--convention", default="blender", choices=("blender", "neusky"), help="the map's azimuth convention")
    ap.add_argument("--exposure", type=float, default=1.0)
    ap.add_argument("--rotation-deg", type=float, default=0.0, help="turn the illumination about +z")
    ap.add_argument("--turntable", type=int, default=1, help="frames per camera, the illumination turned through 360 degrees")
    ap.add_argument("--save-hdr", action="store_true", help="also write the linear-light image of each frame as .npy")
    ap.add_argument("--chunk", type=int, default=4096)
    ap.add_argument("--transfer", default="off", choices=("off", "fp32", "fp16"),
                    help="bake each camera's radiance transfer once (stored as fp32 or scaled fp16) and relight its frames from it")
    ap.add_argument("--sh-order", type=int, metavar="N",
                    help="with --transfer: keep each camera's transfer as (N + 1)^2 spherical-harmonic coefficients per ray (N in 0..8) and "
                         "relight from them; the last line reports the largest light_residual, the share of a frame's light the order left out")
    day = ap.add_argument_group("daylight", "with --daylight (Preetham, Shirley, Smits 1999)")
    day.add_argument("--turbidity", type=float, help="2 (very clear) .. 10 (hazy), default 3")
    day.add_argument("--sky-exposure", type=float, help="multiplies the model's sky (kcd / m^2) and its sun, default 0.1")
    day.add_argument("--ground", type=float, nargs=3, metavar=("R", "G", "B"),
                     help="factor on the horizon's sky for what lies below it (default 0.25 0.25 0.25)")
    sun = ap.add_argument_group("sun", "a directional sun on top of the sky, with its DDF or sphere-traced shadow (relight.SunLight)")
    sun.add_argument("--sun-azimuth", type=float, help="degrees, counter-clockwise from +x about +z")
    sun.add_argument("--sun-elevation", type=float, help="degrees above the horizon; a sun at or below it has set")
    sun.add_argument("--sun-colour", type=float, nargs=3, metavar=("R", "G", "B"), help="in the renderer's irradiance units (default 1 1 1)")
    sun.add_argument("--sun-radiance", type=float, nargs=3, metavar=("R", "G", "B"), help="the disc's radiance instead: colour = L Omega / 2 pi")
    sun.add_argument("--sun-angular-diameter", type=float, default=SUN_ANGULAR_DIAMETER_DEG, help="degrees, with --sun-radiance")
    sun.add_argument("--sun-path", type=float, nargs=4, metavar=("AZ0", "EL0", "AZ1", "EL1"),
                     help="sweep the sun between two positions: --sun-steps frames per camera from one field pass per chunk")
    sun.add_argument("--sun-steps", type=int, help="frames of --sun-path")
    sun.add_argument("--shadow-map", action="store_true", help="also write the sun's shadow map of each frame as shadow_CCCC_FFF.png")
    sun.add_argument("--shadow-threshold", type=float, help="default: the model's trained visibility threshold")
    sun.add_argument("--shadow-sigmoid-scale", type=float, help="default: the model's sigmoid scale")
    sun.add_argument("--sun-shadows", default="ddf", choices=("ddf", "sdf"),
                     help="the sun's shadow from one DDF query per ray (default), or sphere-traced through the SDF with a penumbra "
                          "(relight.trace_visibility): it follows the exported surface and needs no visibility network")
    sun.add_argument("--shadow-steps", type=int, metavar="N", help="with --sun-shadows sdf: rounds of the march (default 96)")
    sun.add_argument("--shadow-bias", type=float, metavar="B",
                     help="with --sun-shadows sdf: lift of the start point off the rendered surface along its normal, scene units (default 1e-2)")
    sun.add_argument("--shadow-angular-diameter", type=float, metavar="DEG",
                     help=f"with --sun-shadows sdf: the disc the penumbra is as wide as (default {SUN_ANGULAR_DIAMETER_DEG}, the sun; 0: a hard edge)")
    sun.add_argument("--extract-sun", action="store_true",
                     help="find the sun in --envmap, take its excess over the sky out of the map and light with it as the sun (relight.extract_sun)")
    sun.add_argument("--sun-search-radius", type=float, metavar="DEG", help="with --extract-sun: the cap about the peak (default 2.5)")
    sun.add_argument("--sun-min-peak-ratio", type=float, metavar="X",
                     help="with --extract-sun: the peak must be X times the sky around the cap (default 10)")
    show = ap.add_argument_group("display", "from the linear image to the PNG on the device (relight.DisplayTransform): with any of these "
                                 "the PNG is written from the transform's 8-bit output instead of the renderer's clipped one")
    show.add_argument("--tonemap", choices=("clamp", "reinhard", "aces", "hable"), help="the tone curve; the flags below but the last need it")
    show.add_argument("--auto-exposure", choices=("off", "frame", "sequence"),
                      help="meter the exposure: per frame, or once for all frames of a camera's turntable or sun sweep (default off)")
    show.add_argument("--exposure-key", type=float, metavar="KEY", help="with a metered exposure: what the mean luminance maps to (default 0.18)")
    show.add_argument("--exposure-ev", type=float, metavar="EV", help="with a metered exposure: stops on top of it (default 0)")
    show.add_argument("--meter-percentiles", type=float, nargs=2, metavar=("LO", "HI"),
                      help="with a metered exposure: the share of the metered pixels, by luminance, whose mean counts (default 0.05 0.95)")
    show.add_argument("--white-point", type=float, metavar="W", help="with --tonemap reinhard: the value that maps to 1 (default 4)")
    show.add_argument("--bloom-sigma", type=float, metavar="PIXELS", help="add a Gaussian bloom of this width, at most 32 (default: none)")
    show.add_argument("--bloom-threshold", type=float, metavar="T", help="with --bloom-sigma: what exceeds T after exposure blooms (default 1)")
    show.add_argument("--bloom-strength", type=float, metavar="S", help="with --bloom-sigma: the bloom's factor (default 0.1)")
    show.add_argument("--save-linear", action="store_true",
                      help="also write frame_*.lin.npy: the unclipped linear image of each frame, before exposure")
    aa = ap.add_argument_group("antialiasing", "adaptive supersampling (relight.Antialias): the pixels an edge rule marks in the frame's own "
                               "depth, normals, accumulation and linear image take further sub-pixel rays, averaged in linear light")
    aa.add_argument("--antialias", type=int, default=1, metavar="S",
                    help="samples per marked pixel, the centre ray included (2..64); 1 (default): off.  The flags below need it above 1")
    aa.add_argument("--aa-colour", type=float, metavar="T", help="mark a relative difference of luminance above T (default 0.1)")
    aa.add_argument("--aa-depth", type=float, metavar="T", help="mark a relative difference of depth above T (default 0.02)")
    aa.add_argument("--aa-normal-deg", type=float, metavar="DEG", help="mark an angle between normals above DEG (default 15)")
    aa.add_argument("--aa-accumulation", type=float, metavar="T", help="mark a difference of accumulation above T (default 0.1)")
    aa.add_argument("--aa-all", action="store_true", help="mark every pixel: plain supersampling")
    aa.add_argument("--aa-mask", action="store_true", help="also write the marked pixels of each frame as aa_CCCC_FFF.png (0 or 255)")
    lens = ap.add_argument_group("depth of field", "a thin lens in place of the pinhole (relight.DepthOfField): the pixels a blurred pixel's "
                                 "disc reaches take further rays from points of the lens, averaged in linear light")
    lens.add_argument("--dof-aperture", type=float, metavar="A", help="the lens radius in scene units; turns the feature on, the flags below need it")
    lens.add_argument("--dof-focus-distance", type=float, metavar="Z",
                      help="the depth of the plane in focus along the optical axis, in the units of the frame's depth")
    lens.add_argument("--dof-focus-pixel", type=int, nargs=2, metavar=("X", "Y"),
                      help="focus on what the frame shows at this pixel (default: the centre pixel); excludes --dof-focus-distance")
    lens.add_argument("--dof-samples", type=int, metavar="S", help="samples per marked pixel, the pinhole's ray included (2..64, default 16)")
    lens.add_argument("--dof-threshold", type=float, metavar="PIXELS", help="a pixel blurred over at least this radius marks its disc (default 0.5)")
    lens.add_argument("--dof-reach", type=int, metavar="PIXELS", help="how far a disc marks at the most (1..64, default 16)")
    lens.add_argument("--dof-all", action="store_true", help="mark every pixel")
    lens.add_argument("--dof-map", action="store_true",
                      help="also write the circle of confusion of each frame as coc_CCCC_FFF.png (8 bits: min(c / reach, 1))")
    lamps = ap.add_argument_group("lights", "point and spot lights inside the scene (relight.PointLight), on top of the sky and any sun, with "
                                  "shadow rays sphere-traced through the SDF to each lamp")
    lamps.add_argument("--light", type=float, nargs=6, action="append", metavar=("X", "Y", "Z", "R", "G", "B"),
                       help="an omnidirectional lamp at X Y Z (scene units) of intensity R G B (the colour of a sun that lights a facing "
                            "surface as the lamp does from distance 1); repeatable")
    lamps.add_argument("--light-radius", type=float, metavar="RHO", help="the radius of the lamps given by --light (default 0: hard shadows)")
    lamps.add_argument("--lights", metavar="FILE.json", help="a list of lamps with every field of relight.PointLight; adds to --light")
    lamps.add_argument("--no-light-shadows", action="store_true", help="the lamps cast no shadows: no march")
    lamps.add_argument("--light-shadow-steps", type=int, metavar="N", help="rounds of the lamps' shadow march (default 96)")
    lamps.add_argument("--light-shadow-bias", type=float, metavar="B", help="the lift of that march's start points off the surface (default 1e-2)")
    lamps.add_argument("--light-map", action="store_true", help="also write the lamps' share of each frame as lights_CCCC_FFF.png")
    lamps.add_argument("--light-path", type=float, nargs=6, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"),
                       help="the first lamp moves along this segment: --light-steps frames per camera, from one set of chunk graphs")
    lamps.add_argument("--light-steps", type=int, metavar="N", help="frames of --light-path")
    fog = ap.add_argument_group("atmosphere", "height fog or haze between the camera and the frame (relight.Atmosphere): the frame is "
                                "attenuated to each ray's depth and gains the sky's and the suns' light scattered into the ray")
    fog.add_argument("--fog-density", type=float, nargs="+", metavar="D",
                     help="the extinction coefficient per scene unit at --fog-base-height, one number or R G B; turns the feature on, "
                          "the flags below need it")
    fog.add_argument("--fog-scale-height", type=float, metavar="H", help="the density falls off as exp(-(z - base) / H) (default: homogeneous)")
    fog.add_argument("--fog-base-height", type=float, metavar="Z", help="the height --fog-density holds at (default 0)")
    fog.add_argument("--fog-albedo", type=float, nargs="+", metavar="A", help="the single-scattering albedo, one number or R G B (default 1)")
    fog.add_argument("--fog-anisotropy", type=float, metavar="G", help="the Henyey-Greenstein parameter, |G| <= 0.99 (default 0: isotropic)")
    fog.add_argument("--fog-far", type=float, metavar="T", help="the path length given to what lies behind the scene (default 2)")
    fog.add_argument("--fog-shafts", type=int, metavar="M",
                     help="shadow the suns' in-scatter at M points along every ray (0..64, default 0), by --sun-shadows' mode: M further "
                          "shadow queries per ray and sun")
    fog.add_argument("--fog-clear-background", action="store_true", help="leave the sky behind the scene as it is (a daylight sky has its own atmosphere)")
    fog.add_argument("--fog-map", action="store_true", help="also write the transmittance of each frame as fog_CCCC_FFF.png")
    props = ap.add_argument_group("props", "solid spheres and boxes placed in the scene (relight.Prop): lit by the frame's light, shadowed by the "
                                  "scene and shadowing it under every sky, sun, lamp and fog")
    props.add_argument("--prop-sphere", type=float, nargs=7, action="append", metavar=("X", "Y", "Z", "RADIUS", "R", "G", "B"),
                       help="a sphere at X Y Z (scene units) of linear albedo R G B; repeatable")
    props.add_argument("--prop-box", type=float, nargs=10, action="append", metavar=("X", "Y", "Z", "HX", "HY", "HZ", "YAW", "R", "G", "B"),
                       help="a box at X Y Z with half-extents HX HY HZ, turned YAW degrees about +z, of linear albedo R G B; repeatable")
    props.add_argument("--props", metavar="FILE.json", help="a list of props with every field of relight.Prop; adds to the two above")
    props.add_argument("--prop-bias", type=float, metavar="B", help="the lift of a prop's shadow rays off the rendered surface (default relight.PROP_BIAS, 1e-2)")
    props.add_argument("--prop-mask", action="store_true", help="also write the props' share of each pixel as prop_CCCC_FFF.png (8 bits)")
    props.add_argument("--prop-path", type=float, nargs=6, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"),
                       help="the first prop moves along this segment: --prop-steps frames per camera, from one set of chunk graphs")
    props.add_argument("--prop-steps", type=int, metavar="N", help="frames of --prop-path")
    ap.add_argument("--device", default="cuda:0")
    return ap


def refuse_given(ap: argparse.ArgumentParser, flags, message: str) -> None:
    """ap.error for the first of `flags`, pairs (flag, value), whose value is not None: `message` with the flag in place of {}"""
    for flag, given in flags:
        if given is not None:
            ap.error(message.format(flag))


def parse_lights(ap: argparse.ArgumentParser, args):
    """(lights, light_shadows, light_trace, path) of the frame render from the light flags: (None, True, None, None) with none of them;
    path: the --light-steps positions of the first lamp along --light-path, or None"""
    flags = (("--light-radius", args.light_radius), ("--no-light-shadows", args.no_light_shadows or None),
             ("--light-shadow-steps", args.light_shadow_steps), ("--light-shadow-bias", args.light_shadow_bias),
             ("--light-map", args.light_map or None), ("--light-path", args.light_path), ("--light-steps", args.light_steps))
    if args.light is None and args.lights is None:
        refuse_given(ap, flags, "{} needs a light: --light or --lights")
        return None, True, None, None
    if args.transfer != "off":
        ap.error("a baked transfer holds lights at infinity: --light and --lights exclude --transfer")
    if args.light_radius is not None and args.light is None:
        ap.error("--light-radius is the radius of the lamps given by --light")
    from .lights import LIGHT_TRACE_DEFAULTS, PointLight, as_lights, load_lights
    from .shadows import trace_settings
    try:
        lights = [PointLight(v[:3], v[3:], radius=args.light_radius or 0.0) for v in args.light or ()]
        if args.lights is not None:
            lights += list(load_lights(args.lights))
        lights = as_lights(lights)
    except (OSError, TypeError, ValueError) as e:
        ap.error(str(e))
    if not lights:
        ap.error(f"{args.lights}: no lights")
    trace = None
    if args.no_light_shadows:
        refuse_given(ap, flags[2:4], "{} shapes the lamps' shadow march: it excludes --no-light-shadows")
    else:
        trace = {k: LIGHT_TRACE_DEFAULTS[k] if v is None else v for k, v in (("steps", args.light_shadow_steps), ("bias", args.light_shadow_bias))}
        try:
            trace_settings(trace, LIGHT_TRACE_DEFAULTS)
        except ValueError as e:
            ap.error(str(e))
    path = None
    if (args.light_path is None) != (args.light_steps is None):
        ap.error("--light-path and --light-steps go together")
    if args.light_path is not None:
        if args.light_steps < 1:
            ap.error("--light-steps must be >= 1")
        if args.turntable > 1 or (args.sun_steps or 1) > 1:
            ap.error("--light-path moves a lamp from frame to frame: it excludes --turntable and --sun-steps above 1")
        a, b, n = args.light_path[:3], args.light_path[3:], args.light_steps
        path = [tuple(a[i] + (b[i] - a[i]) * (f / (n - 1) if n > 1 else 0.0) for i in range(3)) for f in range(n)]
    return lights, not args.no_light_shadows, trace, path


def parse_props(ap: argparse.ArgumentParser, args):
    """(props, prop_bias, path) of the frame render from the prop flags: (None, None, None) with none of them; path: the --prop-steps
    positions of the first prop along --prop-path, or None"""
    dependent = (("--prop-bias", args.prop_bias), ("--prop-mask", args.prop_mask or None), ("--prop-path", args.prop_path),
                 ("--prop-steps", args.prop_steps))
    if args.prop_sphere is None and args.prop_box is None and args.props is None:
        refuse_given(ap, dependent, "{} needs a prop: --prop-sphere, --prop-box or --props")
        return None, None, None
    if args.transfer != "off":
        ap.error("a baked transfer keeps the scene's own samples: --prop-sphere, --prop-box and --props exclude --transfer " + args.transfer)
    from .props import PROP_BIAS, Prop, as_props, load_props
    try:
        props = [Prop("sphere", v[:3], v[3], v[4:]) for v in args.prop_sphere or ()]
        props += [Prop("box", v[:3], v[3:6], v[7:], yaw_deg=v[6]) for v in args.prop_box or ()]
        if args.props is not None:
            props += list(load_props(args.props))
        props = as_props(props)
    except (OSError, TypeError, ValueError) as e:
        ap.error(str(e))
    if not props:
        ap.error(f"{args.props}: no props")
    if args.prop_bias is not None and not (0.0 <= args.prop_bias < math.inf):
        ap.error("--prop-bias must be finite and >= 0")
    path = None
    if (args.prop_path is None) != (args.prop_steps is None):
        ap.error("--prop-path and --prop-steps go together")
    if args.prop_path is not None:
        if args.prop_steps < 1:
            ap.error("--prop-steps must be >= 1")
        if args.turntable > 1 or (args.sun_steps or 1) > 1 or (args.light_steps or 1) > 1:
            ap.error("--prop-path moves a prop from frame to frame: it excludes --turntable, --sun-steps and --light-steps above 1")
        a, b, n = args.prop_path[:3], args.prop_path[3:], args.prop_steps
        path = [tuple(a[i] + (b[i] - a[i]) * (f / (n - 1) if n > 1 else 0.0) for i in range(3)) for f in range(n)]
    return props, PROP_BIAS if args.prop_bias is None else args.prop_bias, path


def parse_atmosphere(ap: argparse.ArgumentParser, args):
    """the relight.Atmosphere of --fog-density and its flags; None without it"""
    flags = (("--fog-density", args.fog_density), ("--fog-scale-height", args.fog_scale_height), ("--fog-base-height", args.fog_base_height),
             ("--fog-albedo", args.fog_albedo), ("--fog-anisotropy", args.fog_anisotropy), ("--fog-far", args.fog_far),
             ("--fog-shafts", args.fog_shafts), ("--fog-clear-background", args.fog_clear_background or None), ("--fog-map", args.fog_map or None))
    if args.transfer != "off":
        refuse_given(ap, flags, "a baked transfer has no depth to fog: {} goes with --transfer off, not --transfer " + args.transfer)
    if args.fog_density is None:
        refuse_given(ap, flags[1:], "{} needs --fog-density")
        return None
    from .atmosphere import Atmosphere

    for flag, v in (("--fog-density", args.fog_density), ("--fog-albedo", args.fog_albedo)):
        if v is not None and len(v) not in (1, 3):
            ap.error(f"{flag} takes one number or R G B")
    if args.fog_shafts and args.sun_azimuth is None and args.sun_path is None and not args.extract_sun:
        ap.error("--fog-shafts shadows the suns' in-scatter: it needs a sun: --sun-azimuth and --sun-elevation, --sun-path, or --extract-sun")
    one = lambda v: v[0] if len(v) == 1 else tuple(v)  # noqa: E731
    given = {"scale_height": args.fog_scale_height, "base_height": args.fog_base_height, "anisotropy": args.fog_anisotropy, "far": args.fog_far,
             "albedo": None if args.fog_albedo is None else one(args.fog_albedo), "shaft_samples": args.fog_shafts}
    try:
        return Atmosphere(one(args.fog_density), background=not args.fog_clear_background, **{k: v for k, v in given.items() if v is not None})
    except ValueError as e:
        ap.error(str(e))


def parse_antialias(ap: argparse.ArgumentParser, args):
    """the relight.Antialias of --antialias S and its flags; None for S = 1"""
    from .antialias import Antialias

    given = {"colour": args.aa_colour, "depth": args.aa_depth, "normal_deg": args.aa_normal_deg, "accumulation": args.aa_accumulation}
    if args.antialias == 1:
        flags = [("--aa-" + k.replace("_", "-"), v) for k, v in given.items()] + [("--aa-all", args.aa_all or None), ("--aa-mask", args.aa_mask or None)]
        refuse_given(ap, flags, "{} needs --antialias S with S > 1")
        return None
    if args.transfer != "off":
        ap.error(f"--antialias {args.antialias} traces further rays through the marked pixels: it goes with --transfer off, not --transfer {args.transfer}")
    try:
        return Antialias(samples=args.antialias, every_pixel=args.aa_all, **{k: v for k, v in given.items() if v is not None})
    except ValueError as e:
        ap.error(str(e))


def parse_depth_of_field(ap: argparse.ArgumentParser, args):
    """the relight.DepthOfField of --dof-aperture and its flags; None without it"""
    given = {"focus_distance": args.dof_focus_distance, "focus_pixel": None if args.dof_focus_pixel is None else tuple(args.dof_focus_pixel),
             "samples": args.dof_samples, "threshold": args.dof_threshold, "reach": args.dof_reach}
    flags = [("--dof-aperture", args.dof_aperture)] + [("--dof-" + k.replace("_", "-"), v) for k, v in given.items()]
    flags += [("--dof-all", args.dof_all or None), ("--dof-map", args.dof_map or None)]
    if args.transfer != "off":
        refuse_given(ap, flags, "a lens traces further rays through the marked pixels: {} goes with --transfer off, not --transfer " + args.transfer)
    if args.dof_aperture is None:
        refuse_given(ap, flags[1:], "{} needs --dof-aperture")
        return None
    if args.dof_focus_distance is not None and args.dof_focus_pixel is not None:
        ap.error("--dof-focus-distance and --dof-focus-pixel exclude each other")
    from .depth_of_field import DepthOfField
    try:
        return DepthOfField(args.dof_aperture, every_pixel=args.dof_all, **{k: v for k, v in given.items() if v is not None})
    except ValueError as e:
        ap.error(str(e))


def parse_display(ap: argparse.ArgumentParser, args):
    """the relight.DisplayTransform of --tonemap and its flags; the default transform (which reproduces the clipped image) for
    --save-linear alone; None with none of them"""
    from .display import DisplayTransform

    metered = args.auto_exposure in ("frame", "sequence")
    dependent = (("--auto-exposure", args.auto_exposure), ("--exposure-key", args.exposure_key), ("--exposure-ev", args.exposure_ev),
                 ("--meter-percentiles", args.meter_percentiles), ("--white-point", args.white_point), ("--bloom-sigma", args.bloom_sigma),
                 ("--bloom-threshold", args.bloom_threshold), ("--bloom-strength", args.bloom_strength))
    if args.tonemap is None:
        refuse_given(ap, dependent, "{} needs --tonemap")
        return DisplayTransform() if args.save_linear else None
    if not metered:
        refuse_given(ap, dependent[1:4], "{} shapes the metered exposure: it needs --auto-exposure frame or --auto-exposure sequence")
    if args.white_point is not None and args.tonemap != "reinhard":
        ap.error("--white-point is the white point of --tonemap reinhard")
    if args.bloom_sigma is None:
        refuse_given(ap, dependent[6:], "{} needs --bloom-sigma")
    given = {"key": args.exposure_key, "ev": args.exposure_ev, "percentiles": args.meter_percentiles, "white": args.white_point,
             "bloom_sigma": args.bloom_sigma, "bloom_threshold": args.bloom_threshold, "bloom_strength": args.bloom_strength}
    try:
        return DisplayTransform(curve=args.tonemap, exposure=args.auto_exposure if metered else 1.0,
                                **{k: (tuple(v) if k == "percentiles" else v) for k, v in given.items() if v is not None})
    except ValueError as e:
        ap.error(str(e))


def parse_daylight(ap: argparse.ArgumentParser, args):
    """the relight.DaylightSky of --daylight, or None; what the flag excludes is an error here"""
    from .daylight import DaylightSky

    if not args.daylight:
        refuse_given(ap, (("--turbidity", args.turbidity), ("--sky-exposure", args.sky_exposure), ("--ground", args.ground)), "{} needs --daylight")
        return None
    if args.extract_sun:
        ap.error("--extract-sun finds the sun in a map: it excludes --daylight")
    if args.transfer != "off":
        ap.error("--daylight needs the per-sample normals the baked transfer does not keep: it goes with --transfer off")
    if args.rotation_deg != 0.0:
        ap.error("--daylight: the sky follows the sun: move the sun instead of --rotation-deg")
    if args.turntable > 1:
        ap.error("--daylight: the sky follows the sun: sweep the sun with --sun-path instead of --turntable > 1")
    if args.exposure != 1.0:
        ap.error("--exposure scales a map or a latent: the daylight model's exposure is --sky-exposure")
    if args.sun_path is None and (args.sun_azimuth is None or args.sun_elevation is None):
        ap.error("--daylight needs a sun: --sun-azimuth with --sun-elevation, or --sun-path with --sun-steps")
    try:
        given = {"turbidity": args.turbidity, "exposure": args.sky_exposure, "ground": args.ground}
        return DaylightSky(**{k: v for k, v in given.items() if v is not None})
    except ValueError as e:
        ap.error(str(e))


def parse_suns(ap: argparse.ArgumentParser, args, daylight=None):
    """the frame's suns from the command line: None, or a list of relight.SunLight (one per frame of a --sun-path).  With --extract-sun
    the sun comes out of the map at run time: None, after the checks.  Under a daylight sky a sun takes the model's colour unless
    --sun-colour or --sun-radiance names one."""
    from .sun import SunLight, sun_path, sun_solid_angle

    fixed = args.sun_azimuth is not None or args.sun_elevation is not None
    any_sun = fixed or args.sun_path is not None
    if not args.extract_sun:
        refuse_given(ap, (("--sun-search-radius", args.sun_search_radius), ("--sun-min-peak-ratio", args.sun_min_peak_ratio)),
                     "{} needs --extract-sun")
    if args.extract_sun:
        if args.envmap is None:
            ap.error("--extract-sun finds the sun in a map: it needs --envmap")
        if args.transfer != "off":
            ap.error("a sun needs the per-sample normals the baked transfer does not keep: --extract-sun goes with --transfer off")
        diameter = None if args.sun_angular_diameter == SUN_ANGULAR_DIAMETER_DEG else args.sun_angular_diameter
        refuse_given(ap, (("--sun-azimuth", args.sun_azimuth), ("--sun-elevation", args.sun_elevation), ("--sun-path", args.sun_path),
                          ("--sun-steps", args.sun_steps), ("--sun-colour", args.sun_colour), ("--sun-radiance", args.sun_radiance),
                          ("--sun-angular-diameter", diameter)), "--extract-sun takes the sun's position and colour from the map: it excludes {}")
        if args.sun_search_radius is not None and not 0.0 < args.sun_search_radius < 45.0:
            ap.error("--sun-search-radius must lie in (0, 45) degrees")
        if args.sun_min_peak_ratio is not None and not args.sun_min_peak_ratio >= 0.0:
            ap.error("--sun-min-peak-ratio must be >= 0")
        return None
    if not any_sun:
        refuse_given(ap, (("--sun-colour", args.sun_colour), ("--sun-radiance", args.sun_radiance), ("--sun-steps", args.sun_steps),
                          ("--shadow-map", args.shadow_map or None), ("--shadow-threshold", args.shadow_threshold),
                          ("--shadow-sigmoid-scale", args.shadow_sigmoid_scale)),
                     "{} needs a sun: --sun-azimuth and --sun-elevation, --sun-path, or --extract-sun")
        return None
    if args.transfer != "off":
        ap.error("a sun needs the per-sample normals the baked transfer does not keep: sun flags go with --transfer off")
    if fixed and args.sun_path is not None:
        ap.error("--sun-path replaces --sun-azimuth / --sun-elevation")
    if fixed and (args.sun_azimuth is None or args.sun_elevation is None):
        ap.error("--sun-azimuth and --sun-elevation go together")
    if args.sun_colour is not None and args.sun_radiance is not None:
        ap.error("--sun-colour or --sun-radiance, not both")
    if args.sun_steps is not None and args.sun_path is None:
        ap.error("--sun-steps needs --sun-path")
    if args.sun_path is not None:
        if args.sun_steps is None or args.sun_steps < 1:
            ap.error("--sun-path needs --sun-steps N >= 1")
        if args.turntable > 1:
            ap.error("--sun-path sweeps the sun: it excludes --turntable > 1")
    colour = tuple(args.sun_colour) if args.sun_colour is not None else (1.0, 1.0, 1.0)
    if args.sun_radiance is not None:
        k = sun_solid_angle(args.sun_angular_diameter) / (2.0 * math.pi)
        colour = tuple(x * k for x in args.sun_radiance)
    if daylight is not None and args.sun_colour is None and args.sun_radiance is None:
        if args.sun_path is not None:
            return daylight.sun_path(*args.sun_path, args.sun_steps)
        return [daylight.sun(args.sun_azimuth, args.sun_elevation)]
    if args.sun_path is not None:
        return sun_path(*args.sun_path, args.sun_steps, colour)
    return [SunLight(args.sun_azimuth, args.sun_elevation, colour)]


def parse_shadows(ap: argparse.ArgumentParser, args):
    """(sun_shadows, shadow_trace) of the frame render from --sun-shadows and its flags: ("ddf", None), or "sdf" and the march's
    parameters the command line names, defaults filled in"""
    from .shadows import SHADOW_DEFAULTS, trace_settings

    marched = (("--shadow-steps", args.shadow_steps), ("--shadow-bias", args.shadow_bias),
               ("--shadow-angular-diameter", args.shadow_angular_diameter))
    if args.sun_shadows == "ddf":
        refuse_given(ap, marched, "{} needs --sun-shadows sdf")
        return "ddf", None
    refuse_given(ap, (("--shadow-threshold", args.shadow_threshold), ("--shadow-sigmoid-scale", args.shadow_sigmoid_scale)),
                 "{} shapes the DDF shadow: it excludes --sun-shadows sdf")
    if args.sun_azimuth is None and args.sun_path is None and not args.extract_sun:
        ap.error("--sun-shadows sdf needs a sun: --sun-azimuth and --sun-elevation, --sun-path, or --extract-sun")
    trace = {"steps": args.shadow_steps, "bias": args.shadow_bias, "angular_diameter_deg": args.shadow_angular_diameter}
    trace = {k: SHADOW_DEFAULTS[k] if v is None else v for k, v in trace.items()}
    try:
        trace_settings(trace, SHADOW_DEFAULTS)
    except ValueError as e:
        ap.error(str(e))
    return "sdf", trace


def load_scene(args, daylight, suns):
    """(model, envmap, extraction): the checkpoint's model in eval mode and the run's light: --envmap's map (with --extract-sun the
    SunExtraction found in it, and the map it left), else None; --latent-index is copied into eval row 0, which the frame render reads"""
    import torch

    from ..utils.checkpoints import load_reference_pipeline_state
    from . import EnvironmentMap

    ckpt = torch.load(args.checkpoint, map_location="cpu", weights_only=False)
    state = ckpt["pipeline"] if "pipeline" in ckpt else ckpt
    pipe = build_pipeline(state, args.device)
    loaded, unmapped = load_reference_pipeline_state(pipe, state)
    if not loaded:
        raise SystemExit(f"{args.checkpoint}: no pipeline entries")
    if unmapped:
        print(f"warning: {len(unmapped)} checkpoint entries not mapped: {unmapped[:4]}", file=sys.stderr)
    pipe.eval()
    model = pipe.model
    envmap = extraction = None
    if args.envmap is not None:
        envmap = EnvironmentMap.from_file(args.envmap, convention=args.convention, exposure=args.exposure, device=args.device)
        if args.extract_sun:
            from . import extract_sun
            from .sun import SunLight
            given = {k: v for k, v in (("radius_deg", args.sun_search_radius), ("min_peak_ratio", args.sun_min_peak_ratio)) if v is not None}
            try:
                found = extract_sun(envmap, **given)
            except ValueError as e:
                raise SystemExit(str(e))
            if found.found:
                at = SunLight.from_direction(found.direction)
                print(f"sun found: azimuth {at.azimuth_deg:.2f} elevation {at.elevation_deg:.2f} degrees (map frame) | colour "
                      f"{found.colour[0]:.4g} {found.colour[1]:.4g} {found.colour[2]:.4g} | {100.0 * found.flux_fraction:.1f}% of the map's flux | "
                      f"apparent diameter {found.angular_diameter_deg:.2f} degrees")
                extraction, envmap = found, found.envmap
            else:
                print(f"warning: --extract-sun: no sun stands out in {args.envmap} (peak luminance {found.peak_luminance:.4g}, sky around it "
                      f"{found.sky_luminance:.4g}): rendering with the map as it is", file=sys.stderr)
    elif daylight is not None:
        first, last = suns[0], suns[-1]
        print(f"daylight: turbidity {daylight.turbidity:g} sky exposure {daylight.exposure:g} | {len(suns)} sun{'s' if len(suns) > 1 else ''}: "
              f"elevation {first.elevation_deg:.2f} colour {first.colour[0]:.4g} {first.colour[1]:.4g} {first.colour[2]:.4g} -> "
              f"elevation {last.elevation_deg:.2f} colour {last.colour[0]:.4g} {last.colour[1]:.4g} {last.colour[2]:.4g}")
    else:
        n = model.train_illumination_latents.shape[0]
        if not 0 <= args.latent_index < n:
            raise SystemExit(f"--latent-index {args.latent_index}: the checkpoint has {n} training latents")
        with torch.no_grad():  # the frame render reads eval row 0: it takes the training latent (in memory only)
            model.eval_illumination_latents[0].copy_(model.train_illumination_latents[args.latent_index])
            model.eval_scale[0].copy_(model.train_scale[args.latent_index])
            if args.exposure != 1.0:
                model.eval_scale[0].mul_(args.exposure)
    return model, envmap, extraction


def main(argv=None) -> int:
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.turntable < 1:
        ap.error("--turntable must be >= 1")
    if args.sh_order is not None:
        if args.transfer == "off":
            ap.error("--sh-order keeps a baked transfer in spherical harmonics: it needs --transfer fp32 or --transfer fp16")
        if not 0 <= args.sh_order <= 8:
            ap.error("--sh-order must lie in 0..8")
    daylight = parse_daylight(ap, args)
    suns = parse_suns(ap, args, daylight)
    sun_shadows, shadow_trace = parse_shadows(ap, args)
    display = parse_display(ap, args)
    antialias = parse_antialias(ap, args)
    depth_of_field = parse_depth_of_field(ap, args)
    lights, light_shadows, light_trace, light_path = parse_lights(ap, args)
    atmosphere = parse_atmosphere(ap, args)
    props, prop_bias, prop_path = parse_props(ap, args)

    import torch

    from . import FrameLighting, camera_rays, load_camera_path
    from .sequence import BakedSource, FrameWriter, RenderSource, Tally, frame_plan

    t0 = time.perf_counter()
    cams = load_camera_path(args.camera_path)
    if depth_of_field is not None:
        try:
            depth_of_field.focus_index(cams.height, cams.width)
        except ValueError as e:
            ap.error(str(e))
    model, envmap, extraction = load_scene(args, daylight, suns)
    tally = Tally(t_load=time.perf_counter() - t0)
    os.makedirs(args.output_dir, exist_ok=True)
    shots = frame_plan(args.turntable, args.rotation_deg, suns, args.sun_path is not None, light_path, args.transfer, prop_path=prop_path)
    # what every frame shares; a shot then differs by its rotation, its first lamp and, under an extracted sun, its sun: that sun turns
    # with its sky, so the one given here only stands for "one sun" and every shot replaces it
    sun = None
    if extraction is not None:
        sun = extraction.sun(None)
    elif suns is not None:
        sun = suns if shots[0].sweep else suns[0]
    marched = {} if sun is None else {"sun_shadows": sun_shadows, "shadow_trace": shadow_trace}  # (--extract-sun may have found none)
    lamps = {} if lights is None else {"lights": lights, "light_shadows": light_shadows, "light_trace": light_trace}
    if atmosphere is not None and sun is None and atmosphere.shaft_samples > 0:  # (--extract-sun found none: nothing to shadow)
        atmosphere = dataclasses.replace(atmosphere, shaft_samples=0)
    fog = {} if atmosphere is None else {"atmosphere": atmosphere}
    base = FrameLighting.of(None, envmap, sun, args.shadow_threshold, args.shadow_sigmoid_scale, daylight=daylight, **marched, **lamps, **fog)
    writer = FrameWriter(args, display, tally)
    shared = {"chunk": args.chunk, "display": display, "floats": writer.floats, "deferred": writer.deferred}
    if args.transfer == "off":
        placed = {} if props is None else {"props": props, "prop_bias": prop_bias}
        source = RenderSource(model, base, tally, antialias=antialias, extraction=extraction, depth_of_field=depth_of_field, **placed, **shared)
    else:
        source = BakedSource(model, envmap, tally, storage=args.transfer, sh_order=args.sh_order, **shared)
    t1 = time.perf_counter()
    for c in range(len(cams)):
        source.open(c, camera_rays(cams, c, args.device))
        for shot in shots:
            for frame in source.frames(shot):
                writer.write(frame)
        writer.end_camera()
    torch.cuda.synchronize()
    tally.t_render = time.perf_counter() - t1
    suns_per_render = 0 if sun is None else len(suns) if shots[0].sweep else 1
    tally.report(args, (cams.width, cams.height), display, antialias, shadow_trace, lights, light_trace, atmosphere, suns_per_render,
                 bool(model.config.use_visibility), depth_of_field=depth_of_field, props=props)
    return 0


if __name__ == "__main__":
    sys.exit(main())
