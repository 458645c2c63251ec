"""Solid props placed in a frame: `Prop`, the device block of P of them, and the two seams through which they enter a chunk.
Definitions and rules: include/neusky_hip.h; kernels: csrc/props.hip.

Every shading kernel of the frame render is a sum over a ray's samples of weights, albedo and normals (and positions for lamps), and
every shadow is a factor on a visibility tensor.  So a prop needs none of them changed.  Seen: the prop's hit becomes one more sample of
the ray, and the scene's samples behind it lose their weight (`insert_props`).  Shadowing: every visibility tensor the frame forms is
multiplied by an analytic occlusion test (`occlude_by_props`).  The frame's light then shades the prop, the scene's own shadow queries start from
the prop's surface where it is seen, and the prop shadows the scene, under every sky, sun, lamp, fog, lens and display.

Props are geometry, not light: they travel beside a frame's `FrameLighting`, not inside it.  A sample that straddles the hit is kept or
dropped whole, and shadow edges are hard: both are approximations.  `prop_bias` = 1e-2, the midpoint rule and MAX_PROPS are design
choices, not measurements."""
from __future__ import annotations

import json
import math
from dataclasses import dataclass
from typing import NamedTuple, Optional, Sequence, Tuple, Union

import torch

from .. import hip

MAX_PROPS = hip.MAX_PROPS
PROP_BIAS = 1e-2  # the default lift of a prop's shadow rays off the rendered surface, scene units: a design choice
SHAPES = ("sphere", "box")
_KEYS = ("shape", "position", "size", "albedo", "yaw_deg", "visible", "casts_shadows")


def _vec3(name: str, v) -> Tuple[float, float, float]:
    try:
        out = tuple(float(x) for x in v)
    except TypeError:
        raise ValueError(f"a prop's {name} has 3 numbers, got {v!r}") from None
    if len(out) != 3 or not all(math.isfinite(x) for x in out):
        raise ValueError(f"a prop's {name} has 3 finite numbers, got {v!r}")
    return out


@dataclass(frozen=True)
class Prop:
    """shape: "sphere" or "box".  position: the centre [3], scene units.  size: a sphere's radius > 0; a box's three half-extents > 0 in
    its own frame, which is turned by yaw_deg about +z.  albedo: linear, in [0, 1].  visible=False with casts_shadows=True is a shadow
    caster the camera does not see: a detailed object rendered elsewhere is composited over the frame's shadow this way.  Both False
    is an error: such a prop does nothing."""
    shape: str
    position: Tuple[float, float, float]
    size: Union[float, Tuple[float, float, float]]
    albedo: Tuple[float, float, float] = (0.5, 0.5, 0.5)
    yaw_deg: float = 0.0
    visible: bool = True
    casts_shadows: bool = True

    def __post_init__(self):
        set_ = lambda k, v: object.__setattr__(self, k, v)  # noqa: E731
        if self.shape not in SHAPES:
            raise ValueError(f"a prop's shape is one of {SHAPES}, got {self.shape!r}")
        set_("position", _vec3("position", self.position))
        if self.shape == "sphere":
            try:
                size = float(self.size)
            except (TypeError, ValueError):
                raise ValueError(f"a sphere's size is its radius, one number, got {self.size!r}") from None
            if not (math.isfinite(size) and size > 0.0):
                raise ValueError(f"a sphere's radius is finite and > 0, got {self.size!r}")
        else:
            size = _vec3("size", self.size)
            if not all(x > 0.0 for x in size):
                raise ValueError(f"a box's half-extents are > 0, got {self.size!r}")
        set_("size", size)
        albedo = _vec3("albedo", self.albedo)
        if not all(0.0 <= x <= 1.0 for x in albedo):
            raise ValueError(f"a prop's albedo is linear, in [0, 1], got {self.albedo!r}")
        set_("albedo", albedo)
        yaw = float(self.yaw_deg)
        if not math.isfinite(yaw):
            raise ValueError(f"a prop's yaw_deg is finite, got {self.yaw_deg!r}")
        set_("yaw_deg", yaw)
        if not isinstance(self.visible, (bool, int)) or not isinstance(self.casts_shadows, (bool, int)):
            raise ValueError(f"a prop's visible and casts_shadows are booleans, got {self.visible!r} and {self.casts_shadows!r}")
        set_("visible", bool(self.visible))
        set_("casts_shadows", bool(self.casts_shadows))
        if not (self.visible or self.casts_shadows):
            raise ValueError("a prop that is neither visible nor casts shadows does nothing")

    @property
    def row(self):
        """the prop's 16 columns of the device block, as Python floats (float64)"""
        sphere = self.shape == "sphere"
        h = (self.size,) * 3 if sphere else self.size
        yaw = 0.0 if sphere else math.radians(self.yaw_deg)
        return [0.0 if sphere else 1.0, *self.position, *h, math.cos(yaw), math.sin(yaw), *self.albedo, float(self.visible),
                float(self.casts_shadows), 0.0, 0.0]

    def moved_to(self, position) -> "Prop":
        return Prop(self.shape, position, self.size, self.albedo, self.yaw_deg, self.visible, self.casts_shadows)


def as_props(props: Union[Prop, Sequence[Prop], None]) -> Tuple[Prop, ...]:
    """one Prop or a sequence of them as a tuple; None and an empty sequence are no props"""
    if props is None:
        return ()
    if isinstance(props, Prop):
        return (props,)
    out = tuple(props)
    if not all(isinstance(x, Prop) for x in out):
        raise TypeError("props: a Prop or a sequence of them")
    if len(out) > MAX_PROPS:
        raise ValueError(f"{len(out)} props: every ray and every shadow entry tests each one, a frame takes at most {MAX_PROPS}")
    return out


def props_block(props) -> torch.Tensor:
    """the device form of the props as a host tensor [P, 16] float32, built in float64 (the yaw's cosine and sine rounded once)"""
    props = as_props(props)
    if not props:
        raise ValueError("props_block: at least one prop")
    return torch.tensor([x.row for x in props], dtype=torch.float64).to(torch.float32)


def load_props(path) -> Tuple[Prop, ...]:
    """a JSON file: a list of objects with Prop's keywords (shape, position and size required)"""
    with open(path) as f:
        data = json.load(f)
    if not isinstance(data, list):
        raise ValueError(f"{path}: a list of props, got {type(data).__name__}")
    out = []
    for i, entry in enumerate(data):
        if not isinstance(entry, dict) or set(entry) - set(_KEYS) or not set(_KEYS[:3]) <= set(entry):
            raise ValueError(f"{path}: prop {i}: an object with shape, position, size and any of {_KEYS[3:]}, got {entry!r}")
        out.append(Prop(**entry))
    return as_props(out)


def save_props(path, props) -> None:
    """the inverse of load_props: every field of every prop, the defaults written out"""
    with open(path, "w") as f:
        json.dump([{k: getattr(x, k) for k in _KEYS} for x in as_props(props)], f, indent=1)


class PropSamples(NamedTuple):
    """a chunk's samples with the props in them: weights, starts, ends [R, S + 1]; albedo, normals [R, S + 1, 3]; prop_id int32 [R]"""
    weights: torch.Tensor
    starts: torch.Tensor
    ends: torch.Tensor
    albedo: torch.Tensor
    normals: torch.Tensor
    prop_id: torch.Tensor


def intersect_props(origins: torch.Tensor, directions: torch.Tensor, block: torch.Tensor):
    """(t_hit [R], prop_id int32 [R], normal [R, 3], albedo [R, 3]) of the rays origins, directions [R, 3] among the visible props of the
    device block [P, 16]: nsky_props_intersect"""
    R, dev = origins.shape[0], origins.device
    t_hit, prop_id = torch.empty(R, device=dev), torch.empty(R, dtype=torch.int32, device=dev)
    normal, albedo = torch.empty(R, 3, device=dev), torch.empty(R, 3, device=dev)
    hip.props_intersect(origins.detach().contiguous(), directions.detach().contiguous(), block, t_hit, prop_id, normal, albedo)
    return t_hit, prop_id, normal, albedo


def insert_props(origins: torch.Tensor, directions: torch.Tensor, weights: torch.Tensor, starts: torch.Tensor, ends: torch.Tensor,
                 albedo: torch.Tensor, normals: torch.Tensor, block: torch.Tensor) -> PropSamples:
    """the seam of the seen prop: rays origins, directions [R, 3]; their samples weights, starts, ends [R, S], albedo, normals [R, S, 3];
    the device block [P, 16] -> the samples with the nearest entered prop as sample S.  Every shape is static and nothing is read on the
    host: a captured chunk replays under a new block."""
    R, S = weights.shape
    dev = weights.device
    hit = intersect_props(origins, directions, block)
    out = PropSamples(torch.empty(R, S + 1, device=dev), torch.empty(R, S + 1, device=dev), torch.empty(R, S + 1, device=dev),
                      torch.empty(R, S + 1, 3, device=dev), torch.empty(R, S + 1, 3, device=dev), hit[1])
    hip.props_insert(weights.detach().contiguous(), starts.detach().contiguous(), ends.detach().contiguous(), albedo.detach().contiguous(),
                     normals.detach().contiguous(), *hit, out.weights, out.starts, out.ends, out.albedo, out.normals)
    return out


def occlude_by_props(vis: torch.Tensor, x: torch.Tensor, normals: Optional[torch.Tensor], bias: torch.Tensor, block: torch.Tensor, *,
            directions: Optional[torch.Tensor] = None, lights: Optional[torch.Tensor] = None) -> torch.Tensor:
    """the seam of the shadowing prop: vis [M, N] (any strides: the transposed view of [N, M] serves), in place and returned: entry (m, n)
    is multiplied by 0 when a shadow-casting prop of the block stands between the point x[m], lifted `bias` [1] along normals[m] (None: no
    lift), and light n: directions [N, 3] towards lights at infinity, or `lights`, the lamps' device block [L, 16], whose rays end
    `clearance` in front of each lamp"""
    if lights is not None:
        hip.props_occlude(x, normals, bias, block, vis, targets=lights[:, 0:3].contiguous(), clearance=lights[:, 9].contiguous())
    else:
        hip.props_occlude(x, normals, bias, block, vis, directions=directions.contiguous())
    return vis
