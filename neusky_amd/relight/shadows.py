"""Sphere-traced shadow rays through the SDF, with penumbrae: `trace_visibility`, the visibility primitive behind the frame render's
`sun_shadows="sdf"`.  The march rule and its parameters: include/neusky_hip.h; kernels: csrc/sphere_trace.hip.

The DDF shadow of a `SunLight` is one query of a second, learned approximation of the geometry; this one marches the ray through the
SDF itself, so the shadow follows the surface the mesh export writes, is sharp at the contact point and widens with the distance from
the occluder (by the closest-approach estimate m = min f / (t tan(diameter / 2)): an approximation of a disc light, not an integral
over it), and needs no visibility network.  A round of the march is the field's sdf at every ray's point (`get_sdf_at_pos`: the
non-tangent hash encode and the sdf value chain) and one `nsky_sphere_trace_step`; all rays run all `steps` rounds, dead ones idle, so
the shape is static and a chunk's march captures in its graph.  (Compacting the dead rays away is the follow-up; it gives up that.)
Every default below is a design choice, not a measurement."""
from __future__ import annotations

import math
from collections import namedtuple
from typing import Callable, Union

import torch

from .. import hip
from .sun import SUN_ANGULAR_DIAMETER_DEG

ALIVE, HIT, ESCAPED, EXHAUSTED = hip.TRACE_ALIVE, hip.TRACE_HIT, hip.TRACE_ESCAPED, hip.TRACE_EXHAUSTED
# visibility: fp32, 0 on HIT rays, the penumbra estimate m in [0, 1] otherwise (1 for a hard shadow); status: int8, one of HIT, ESCAPED,
# EXHAUSTED (still marching after `steps` rounds: it keeps its m); t: fp32, the ray parameter the march ended at
SphereTrace = namedtuple("SphereTrace", "visibility status t")
TRACE_DEFAULTS = {"steps": 96, "eps": 1e-3, "relax": 1.0, "min_step": 1e-3, "grace": 16, "radius": 1.0, "angular_diameter_deg": 0.0}
# the frame render's `shadow_trace`: the sun's disc, and a start point lifted 1e-2 scene units off the rendered surface along its normal
SHADOW_DEFAULTS = {**TRACE_DEFAULTS, "angular_diameter_deg": SUN_ANGULAR_DIAMETER_DEG, "bias": 1e-2}


def trace_settings(given, defaults) -> dict:
    """`defaults` overridden by the dictionary `given` (or None), every value checked"""
    unknown = set(given or {}) - set(defaults)
    if unknown:
        raise ValueError(f"unknown shadow-trace parameters {sorted(unknown)}: known are {sorted(defaults)}")
    p = {**defaults, **(given or {})}
    steps, grace = p["steps"], p["grace"]
    if int(steps) != steps or steps < 1 or int(grace) != grace or grace < 0:
        raise ValueError(f"steps must be a whole number >= 1 and grace one >= 0, got {steps!r} and {grace!r}")
    p["steps"], p["grace"] = int(steps), int(grace)
    for k in set(p) - {"steps", "grace"}:
        p[k] = float(p[k])
        if not math.isfinite(p[k]):
            raise ValueError(f"{k} must be finite, got {p[k]!r}")
    if not (p["eps"] > 0.0 and p["relax"] > 0.0 and p["min_step"] > 0.0 and p["radius"] > 0.0):
        raise ValueError("eps, relax, min_step and radius must be positive")
    if not 0.0 <= p.get("angular_diameter_deg", 0.0) < 180.0:  # (a march towards a lamp has none: relight.lights)
        raise ValueError(f"angular_diameter_deg must lie in [0, 180), got {p['angular_diameter_deg']!r}")
    return p


def trace_params(p: dict) -> torch.Tensor:
    """the device parameter block of the kernels as a host tensor [6]: eps, relax, min_step, tan_half, radius, bias"""
    tan_half = math.tan(math.radians(p.get("angular_diameter_deg", 0.0)) / 2.0)
    return torch.tensor([p["eps"], p["relax"], p["min_step"], tan_half, p["radius"], p.get("bias", 0.0)], dtype=torch.float64).to(torch.float32)


def _sdf_function(sdf) -> Callable[[torch.Tensor], torch.Tensor]:
    if hasattr(sdf, "get_sdf_at_pos"):
        return lambda points: sdf.get_sdf_at_pos(points).reshape(-1)

    def call(points):
        f = sdf(points)
        if not torch.is_tensor(f) or f.numel() != points.shape[0] or f.device != points.device:
            raise ValueError(f"sdf: a function of points [M, 3] returning [M] on their device, got {getattr(f, 'shape', type(f))}")
        return f.reshape(-1).to(torch.float32).contiguous()
    return call


def _march(sdf, state, points, directions, dir_div: int, params, steps: int, grace: int, shape, bounds=None) -> SphereTrace:
    """`steps` rounds from a begun state, and the finish.  `points` is one buffer, rewritten by every round: an `sdf` that keeps it must
    copy it.  bounds: of rays that end at a light (relight.lights)."""
    f = _sdf_function(sdf)
    with torch.no_grad():
        for i in range(steps):
            hip.sphere_trace_step(state, f(points), directions, dir_div, params, i, steps, grace, points, bounds)
    T, dev = points.shape[0], points.device
    vis, t, status = torch.empty(T, device=dev), torch.empty(T, device=dev), torch.empty(T, dtype=torch.int8, device=dev)
    hip.sphere_trace_finish(state, vis, status, t)
    return SphereTrace(vis.view(shape), status.view(shape), t.view(shape))


def _start(sdf, origins: torch.Tensor, rays: Callable[[int], int], error: str, ok: bool = True):
    """the start points [M, 3] of a march, checked, as contiguous fp32, and the state and points of its rays(M) rays"""
    if not ok or origins.dim() != 2 or origins.shape[1] != 3 or origins.shape[0] < 1:
        raise ValueError(error)
    if hasattr(sdf, "invalidate_weight_cache"):
        sdf.invalidate_weight_cache()  # its prepared weights are built once for all rounds, from the parameters as they are now
    T, dev = rays(origins.shape[0]), origins.device
    return origins.detach().to(torch.float32).contiguous(), torch.empty(6, T, device=dev), torch.empty(T, 3, device=dev)


def trace_visibility(sdf: Union[Callable[[torch.Tensor], torch.Tensor], object], origins: torch.Tensor, directions: torch.Tensor, *,
                     steps: int = 96, eps: float = 1e-3, relax: float = 1.0, min_step: float = 1e-3, grace: int = 16, radius: float = 1.0,
                     angular_diameter_deg: float = 0.0) -> SphereTrace:
    """March shadow rays from the start points `origins` [M, 3] towards the light.
    sdf: an SDFAlbedoField (its get_sdf_at_pos is evaluated) or any function of device points [M', 3] returning their signed distances
    [M'] (an analytic scene, another field).
    directions: unit vectors, [M, 3] (one per ray; the results are [M]) or [K, 3] with K != M (every start point under each of K
    lights; the results are [K, M]).
    angular_diameter_deg: of the light's disc; 0 gives a hard shadow (visibility 0 or 1).  radius: the scene bound about the origin
    (the model's sphere collider has 1); a ray leaves the march there, and one that starts beyond it escapes at once."""
    p = trace_settings({"steps": steps, "eps": eps, "relax": relax, "min_step": min_step, "grace": grace, "radius": radius,
                        "angular_diameter_deg": angular_diameter_deg}, TRACE_DEFAULTS)
    ok = directions.dim() == 2 and directions.shape[1] == 3
    K = directions.shape[0] if ok else 0
    origins, state, points = _start(sdf, origins, lambda M: M if K == M else K * M, "origins [M, 3] and directions [M, 3] or [K, 3], got "
                                    f"{tuple(origins.shape)} and {tuple(directions.shape)}", ok)
    M, directions = origins.shape[0], directions.detach().to(torch.float32).contiguous()
    params = trace_params(p).to(origins.device)
    hip.sphere_trace_begin_points(origins, directions, params, state, points)
    return _march(sdf, state, points, directions, hip.trace_dir_div(directions, M, points.shape[0]), params, p["steps"], p["grace"],
                  (M,) if K == M else (K, M))


def trace_sun_shadows(sdf, origins: torch.Tensor, directions: torch.Tensor, depth: torch.Tensor, normals: torch.Tensor, suns: torch.Tensor,
                      params: torch.Tensor, steps: int, grace: int) -> SphereTrace:
    """the frame render's march: camera rays `origins`, `directions` [R, 3] (unit), their rendered `depth` [R] along the ray and
    `normals` [R, 3] (any length; a zero one is replaced by the sun's direction), `suns` [K, 3]; `params`: the device block of
    trace_params, whose bias lifts the start point o + depth d along the normal.  Results [K, R].  Nothing is read on the host and
    every shape is static: a captured chunk replays with new suns and a new parameter block."""
    R, K, dev = origins.shape[0], suns.shape[0], origins.device
    state, points = torch.empty(6, K * R, device=dev), torch.empty(K * R, 3, device=dev)
    hip.sphere_trace_begin(origins.detach().contiguous(), directions.detach().contiguous(), depth.detach().reshape(-1).contiguous(),
                           normals.detach().contiguous(), suns, params, state, points)
    return _march(sdf, state, points, suns, max(R, 1), params, steps, grace, (K, R))
