"""relight.FrameLighting, the one value a frame's light is said in: every rule between its options is an error with the text the frame
render has always given, one sun and a sequence normalise to the same suns, and the march's parameters come out complete.  No device."""
import dataclasses
import math
import re

import pytest
import torch

from neusky_amd.relight import SHADOW_DEFAULTS, DaylightSky, FrameLighting, SunLight

SUN = SunLight(130.0, 35.0, (2.0, 1.7, 1.2))
SKY = DaylightSky()
MAP = object()  # the rules ask only whether a map is given
KNOWN = sorted(SHADOW_DEFAULTS)

RULES = [
    (dict(sun_shadows="soft"), "sun_shadows: 'ddf' or 'sdf', got 'soft'"),
    (dict(sun_shadows="sdf"), "sun_shadows='sdf' marches the shadow rays of a sun: give `sun` (and no bake)"),
    (dict(sun_shadows="sdf", sun=SUN, bake="fp32"), "sun_shadows='sdf' marches the shadow rays of a sun: give `sun` (and no bake)"),
    (dict(sun_shadows="sdf", sun=SUN, shadow_threshold=0.3),
     "shadow_threshold and shadow_sigmoid_scale shape the DDF shadow: they exclude sun_shadows='sdf'"),
    (dict(sun_shadows="sdf", sun=SUN, shadow_sigmoid_scale=2.0),
     "shadow_threshold and shadow_sigmoid_scale shape the DDF shadow: they exclude sun_shadows='sdf'"),
    (dict(sun=SUN, shadow_trace={"steps": 16}), "shadow_trace holds the parameters of the march: it needs sun_shadows='sdf'"),
    (dict(shadow_trace={}), "shadow_trace holds the parameters of the march: it needs sun_shadows='sdf'"),
    (dict(daylight=SKY), "daylight: the sky follows a sun: give `sun`, one SunLight or K (DaylightSky.sun, DaylightSky.sun_path)"),
    (dict(daylight=SKY, sun=SUN, envmap=MAP),
     "daylight takes the place of the latent's or the map's sky: it excludes envmap, rotation and a bake"),
    (dict(daylight=SKY, sun=SUN, rotation=torch.eye(3)),
     "daylight takes the place of the latent's or the map's sky: it excludes envmap, rotation and a bake"),
    (dict(daylight=SKY, sun=SUN, bake="fp16"),
     "daylight takes the place of the latent's or the map's sky: it excludes envmap, rotation and a bake"),
]
TRACE_RULES = [
    ({"step": 16, "tilt": 1.0}, f"unknown shadow-trace parameters ['step', 'tilt']: known are {KNOWN}"),
    ({"steps": 0}, "steps must be a whole number >= 1 and grace one >= 0, got 0 and 16"),
    ({"steps": 7.5}, "steps must be a whole number >= 1 and grace one >= 0, got 7.5 and 16"),
    ({"grace": -1}, "steps must be a whole number >= 1 and grace one >= 0, got 96 and -1"),
    ({"bias": math.inf}, "bias must be finite, got inf"),
    ({"eps": math.nan}, "eps must be finite, got nan"),
    ({"eps": 0.0}, "eps, relax, min_step and radius must be positive"),
    ({"relax": -1.0}, "eps, relax, min_step and radius must be positive"),
    ({"min_step": 0.0}, "eps, relax, min_step and radius must be positive"),
    ({"radius": 0.0}, "eps, relax, min_step and radius must be positive"),
    ({"angular_diameter_deg": -0.5}, "angular_diameter_deg must lie in [0, 180), got -0.5"),
    ({"angular_diameter_deg": 180.0}, "angular_diameter_deg must lie in [0, 180), got 180.0"),
]


def _ids(rules):
    return ["-".join(given) or "none" for given, _ in rules]


@pytest.mark.parametrize("keywords, text", RULES, ids=_ids(RULES))
def test_every_exclusion_rule_is_a_value_error_with_its_text(keywords, text):
    with pytest.raises(ValueError, match="^" + re.escape(text) + "$"):
        FrameLighting.of(**keywords)


@pytest.mark.parametrize("trace, text", TRACE_RULES, ids=_ids(TRACE_RULES))
def test_the_marchs_parameters_are_checked(trace, text):
    with pytest.raises(ValueError, match="^" + re.escape(text) + "$"):
        FrameLighting.of(sun=SUN, sun_shadows="sdf", shadow_trace=trace)


def test_one_sun_and_a_list_of_one_are_the_same_suns():
    one, listed = FrameLighting.of(sun=SUN), FrameLighting.of(sun=[SUN])
    assert one.suns == listed.suns == (SUN,)
    assert one.single_sun is True and listed.single_sun is False
    other = SunLight(250.0, 15.0, (3.0, 2.0, 0.5))
    assert FrameLighting.of(sun=(s for s in (SUN, other))).suns == (SUN, other)
    assert FrameLighting.of().suns is None
    for wrong in ([], [SUN, "noon"]):
        with pytest.raises(TypeError, match="sun: a SunLight or a non-empty sequence of them"):
            FrameLighting.of(sun=wrong)


def test_the_march_takes_its_defaults_and_only_under_sdf():
    assert FrameLighting.of(sun=SUN, sun_shadows="sdf").shadow_trace == {**SHADOW_DEFAULTS, "radius": 1.0}
    given = FrameLighting.of(sun=SUN, sun_shadows="sdf", shadow_trace={"steps": 16.0, "bias": 0, "radius": 2}).shadow_trace
    assert given == {**SHADOW_DEFAULTS, "steps": 16, "bias": 0.0, "radius": 2.0}
    assert type(given["steps"]) is int and type(given["grace"]) is int and type(given["bias"]) is float
    assert FrameLighting.of(sun=SUN).shadow_trace is None and FrameLighting.of(sun=SUN, sun_shadows="ddf").shadow_trace is None
    assert FrameLighting.of().sun_shadows == "ddf"


def test_it_is_a_frozen_value_compared_field_by_field():
    R = torch.eye(3)
    keywords = dict(rotation=R, envmap=MAP, sun=[SUN], shadow_threshold=0.3, shadow_sigmoid_scale=4.0, accumulation_mask_threshold=0.5)
    a, b = FrameLighting.of(**keywords), FrameLighting.of(**keywords)
    names = [f.name for f in dataclasses.fields(FrameLighting)]
    assert names == ["rotation", "envmap", "daylight", "bake", "suns", "single_sun", "shadow_threshold", "shadow_sigmoid_scale",
                     "accumulation_mask_threshold", "sun_shadows", "shadow_trace"]
    for name in names:
        x, y = getattr(a, name), getattr(b, name)
        assert x is y or x == y, name
    assert a.rotation is R and a.envmap is MAP and a.daylight is None and a.bake is None
    assert (a.shadow_threshold, a.shadow_sigmoid_scale, a.accumulation_mask_threshold) == (0.3, 4.0, 0.5)
    assert FrameLighting.of(bake="fp16").bake == "fp16" and FrameLighting.of(daylight=SKY, sun=SUN).daylight is SKY
    with pytest.raises(TypeError):
        hash(a)
    with pytest.raises(dataclasses.FrozenInstanceError):
        a.bake = "fp32"
    turned = dataclasses.replace(a, rotation=None, suns=(SUN, SUN))
    assert turned.rotation is None and turned.suns == (SUN, SUN) and turned.envmap is MAP and a.suns == (SUN,)
