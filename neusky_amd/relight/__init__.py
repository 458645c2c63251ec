"""Relighting under a user-supplied HDR environment map: readers of equirectangular maps, the projection of a map onto the renderer's
light directions and the bilinear sky lookup on the GPU (csrc/envmap.hip), and the frame render with `envmap=`.

  python -m neusky_amd.relight --checkpoint CKPT --camera-path camera_path.json --output-dir frames/ --envmap sky.hdr

`bake_transfer` / `RadianceTransfer` (transfer.py, csrc/transfer.hip): a camera's frame baked once into its radiance transfer, then relit
under any number of lights at one streaming pass over the transfer each (`--transfer fp32|fp16` on the command line).

`bake_transfer_sh` / `compress_transfer` / `SHRadianceTransfer` (transfer_sh.py, csrc/transfer_sh.hip): the same transfer kept as
(order + 1)^2 spherical-harmonic coefficients per ray in place of D directions; every relight reports the `light_residual` of its light
(`--sh-order N` with `--transfer`).

`SunLight` / `sun_path` (sun.py, csrc/sun.hip): a directional sun on top of either sky, with one DDF shadow query per ray; the frame
render with `sun=` returns the lit frame, its `shadow_map` and `shadow_difference` (`--sun-azimuth/--sun-elevation`, `--sun-path`).

`extract_sun` / `SunExtraction` (envmap_sun.py, csrc/envmap_sun.hip): the sun of an HDR map found, taken out of the map and handed to the
`SunLight` path with its energy conserved, so that a sunny HDRI casts shadows (`--extract-sun`).

`DaylightSky` (daylight.py, csrc/daylight.hip): a clear-sky daylight model whose sky, sun colour and background follow the sun; the
frame render with `daylight=` gives each of K suns its own sky from one field pass per chunk (`--daylight`, `--turbidity`).

`trace_visibility` / `SphereTrace` (shadows.py, csrc/sphere_trace.hip): shadow rays sphere-traced through the SDF, with penumbrae; the
frame render with `sun_shadows="sdf"` takes every sun's shadow from it instead of the DDF (`--sun-shadows sdf`).

`PointLight` / `trace_visibility_to` (lights.py, csrc/lights.hip): point and spot lights inside the scene, with inverse-square falloff
and shadow rays that end at the lamp; the frame render with `lights=` adds them to any sky and sun (`--light`, `--lights`).

`DisplayTransform` (display.py, csrc/display.hip): from a linear image to a picture on the device: metered exposure, bloom, a tone curve,
sRGB and 8 bits; the frame render and both transfers' `relight` take one as `display=` (`--tonemap`, `--auto-exposure`).

`Antialias` (antialias.py, csrc/antialias.hip): adaptive supersampling of a frame: an edge mask from the frame's own G-buffer and linear
image, `subpixel_rays` through the marked pixels, a resolve in linear light; the frame render takes one as `antialias=` (`--antialias`).

`DepthOfField` (depth_of_field.py, csrc/dof.hip): a thin lens in place of the pinhole: a circle of confusion per pixel from the frame's own
depth, a mark on every pixel a blurred pixel's disc reaches, `lens_rays` through the marked pixels, the same resolve; the frame render
takes one as `depth_of_field=` (`--dof-aperture`).

`Atmosphere` (atmosphere.py, csrc/atmosphere.hip): height fog and haze between the camera and the frame, with the suns' in-scatter
shadowed along the ray by the frame's own shadow mode; the frame render takes one as `atmosphere=` (`--fog-density`, `--fog-shafts`).

`FrameLighting` (lighting.py): all of the above as the one value a frame's light is said in, with the rules between its options.

`Prop` (props.py, csrc/props.hip): solid spheres and boxes placed in a frame as one more sample per ray and an analytic factor on every
visibility the frame forms: lit by the frame's light, shadowed by the scene and shadowing it.  Geometry, not light: the frame render
takes them beside its lighting, as `props=` (`--prop-sphere`, `--prop-box`, `--props`).

sequence.py: the run of the command line: the plan of a camera's renders, the two sources of its frames, the writer of its files, the
tally of its closing lines.
"""
from .antialias import Antialias, r2_offsets, subpixel_rays
from .atmosphere import Atmosphere
from .cameras import CameraPath, camera_rays, load_camera_path
from .daylight import DaylightSky
from .depth_of_field import (DepthOfField, circle_of_confusion, depth_of_field_frame, lens_block, lens_frame, lens_rays, lens_table,
                             mark_pixels)
from .display import DisplayTransform, bloom_weights, frame_display
from .envmap import EnvironmentMap, envmap_labels, envmap_lookup, project_envmap, z_rotation
from .envmap_sun import SunExtraction, extract_sun
from .io import read_envmap, srgb_to_linear
from .lighting import FrameLighting
from .lights import (LIGHT_TRACE_DEFAULTS, MAX_LIGHTS, PointLight, as_lights, lights_block, load_lights, save_lights, trace_light_shadows,
                     trace_visibility_to)
from .props import MAX_PROPS, PROP_BIAS, Prop, as_props, load_props, props_block, save_props
from .shadows import ALIVE, ESCAPED, EXHAUSTED, HIT, SHADOW_DEFAULTS, TRACE_DEFAULTS, SphereTrace, trace_sun_shadows, trace_visibility
from .sun import SunLight, sun_direction, sun_path, sun_solid_angle
from .transfer import RadianceTransfer, bake_transfer, pack_fp16, unpack_fp16
from .transfer_sh import SHRadianceTransfer, bake_transfer_sh, compress_transfer, light_basis, project_lights, sh_basis

__all__ = ["ALIVE", "Antialias", "Atmosphere", "CameraPath", "DaylightSky", "DisplayTransform", "ESCAPED", "EXHAUSTED", "EnvironmentMap", "FrameLighting", "HIT", "LIGHT_TRACE_DEFAULTS", "MAX_LIGHTS", "PointLight", "RadianceTransfer",
           "SHADOW_DEFAULTS", "SHRadianceTransfer", "SphereTrace", "SunExtraction", "SunLight", "TRACE_DEFAULTS", "bake_transfer",
           "bake_transfer_sh", "bloom_weights", "camera_rays", "compress_transfer", "envmap_labels", "envmap_lookup", "extract_sun", "frame_display", "light_basis",
           "load_camera_path", "pack_fp16", "project_envmap", "project_lights", "r2_offsets", "read_envmap", "sh_basis", "srgb_to_linear", "sun_direction",
           "subpixel_rays", "sun_path", "sun_solid_angle", "trace_sun_shadows", "trace_visibility", "unpack_fp16", "z_rotation", "as_lights", "lights_block", "load_lights", "save_lights",
           "trace_light_shadows", "trace_visibility_to", "DepthOfField", "circle_of_confusion", "depth_of_field_frame", "lens_block", "lens_frame",
           "lens_rays", "lens_table", "mark_pixels", "MAX_PROPS", "PROP_BIAS", "Prop", "as_props", "load_props",
           "props_block", "save_props"]
