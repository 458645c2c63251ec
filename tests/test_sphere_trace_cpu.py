"""The march rule of the sphere-traced shadows (include/neusky_hip.h), restated in float64 numpy (sphere_trace_cpu.py), on the analytic
scene the GPU tests use: a plane and a sphere above it, 64 x 64 start points under a sun at azimuth 30, elevation 40 degrees, the start
points on, above and a few eps below the plane.  What the restatement gives here is what the kernels are then held to.  And the command
line's --sun-shadows flags, argument parsing only."""
import numpy as np
import pytest

import sphere_trace_cpu as ST
from neusky_amd.relight.__main__ import build_parser, parse_daylight, parse_shadows, parse_suns

OFFSETS = (1e-2, 0.0, -5e-3)
S = ST.sun_direction()
_CACHE = {}


def _march(z, deg, **kw):
    """marched once per (offset, angular diameter, settings); the results are read, never written"""
    key = (z, deg, tuple(sorted(kw.items())))
    if key not in _CACHE:
        x = ST.scene_starts(64, z)
        _CACHE[key] = (x, *ST.analytic_shadow(x, S), *ST.march(ST.scene_sdf, x, S, tan_half=ST.tan_half(deg), **kw))
    return _CACHE[key]


@pytest.mark.parametrize("z", OFFSETS)
def test_hard_shadow_is_the_analytic_one_off_the_band(z):
    x, shadowed, dist, m, status, t = _march(z, 0.0)
    off = dist >= ST.BAND
    band = 1.0 - off.mean()
    print(f"offset {z:+.0e}: band {100 * band:.2f}% of the rays, {int((status == ST.HIT).sum())} hits, {int((status == ST.EXHAUSTED).sum())} exhausted")
    assert band <= 0.05
    assert not (status == ST.EXHAUSTED).any() and not (status == ST.ALIVE).any()
    assert np.array_equal((status == ST.HIT)[off], shadowed[off])
    assert np.array_equal(m, np.where(status == ST.HIT, 0.0, 1.0))  # a hard shadow is 0 or 1
    assert shadowed.sum() > 500 and (~shadowed).sum() > 2000  # both sides are there


@pytest.mark.parametrize("z", OFFSETS)
def test_float32_reaches_the_same_statuses(z):
    x, _, _, _, status, _ = _march(z, 0.0)
    assert np.array_equal(ST.march(ST.scene_sdf, x, S, dtype=np.float32)[1], status)


@pytest.mark.parametrize("deg", (0.533, 4.0))
@pytest.mark.parametrize("z", OFFSETS)
def test_soft_shadow(z, deg):
    x, shadowed, dist, m, status, t = _march(z, deg)
    assert m.min() >= 0.0 and m.max() <= 1.0
    assert (m[status == ST.HIT] == 0.0).all()
    assert (m[~shadowed & (dist > 0.05)] == 1.0).all()
    assert np.array_equal(status, _march(z, 0.0)[4])  # the penumbra does not steer the march
    part = (m > 0.0) & (m < 1.0)
    assert part.any() and (dist[part] <= 0.05).all()  # there is a penumbra, and it hugs the silhouette
    m32 = ST.march(ST.scene_sdf, x, S, tan_half=ST.tan_half(deg), dtype=np.float32)[0]
    print(f"offset {z:+.0e}, {deg} degrees: {int(part.sum())} penumbra rays, float32 differs by {np.abs(m32 - m).max():.2e}")
    assert np.abs(m32 - m).max() < 1e-4


def test_a_wider_disc_has_a_wider_penumbra():
    narrow, wide = _march(1e-2, 0.533)[3], _march(1e-2, 4.0)[3]
    assert (wide <= narrow).all() and (wide < narrow).sum() > 50


def test_too_few_steps_exhaust():
    status = _march(0.0, 0.0, steps=64)[4]
    n = int((status == ST.EXHAUSTED).sum())
    assert 1 <= n <= 20, n  # (9 of 4096: grazing rays crawling along the sphere)


def test_a_start_inside_the_surface_climbs_out_or_is_caught():
    x = np.array([[0.5, 0.5, -5e-3], [-0.3, -0.3, -0.5]])  # a few eps under the plane; and deep under it
    m, status, t = ST.march(ST.scene_sdf, x, S, relax=0.5)
    assert status[0] == ST.ESCAPED and m[0] == 1.0
    # half steps close 32 % of the gap each: after the 16 rounds of the leaving phase the ray is still inside, and the hit is forced
    assert status[1] == ST.HIT and m[1] == 0.0 and t[1] < 0.5 / S[2]


def test_a_start_beyond_the_radius_escapes_at_once():
    m, status, t = ST.march(ST.scene_sdf, np.array([[0.9, 0.9, 0.1]]), S)
    assert status[0] == ST.ESCAPED and t[0] == 0.0 and m[0] == 1.0


# ---------------------------------------------------------------------------------------------- the command line
BASE = ["--checkpoint", "c.ckpt", "--camera-path", "p.json", "--output-dir", "o"]
SUN = ["--sun-azimuth", "10", "--sun-elevation", "20"]


def _parse(*extra):
    ap = build_parser()
    args = ap.parse_args(BASE + list(extra))
    daylight = parse_daylight(ap, args)
    return parse_suns(ap, args, daylight), parse_shadows(ap, args), args


ERRORS = {
    "threshold": (["--latent-index", "0", "--sun-shadows", "sdf", "--shadow-threshold", "0.1"] + SUN, "--shadow-threshold"),
    "sigmoid scale": (["--latent-index", "0", "--sun-shadows", "sdf", "--shadow-sigmoid-scale", "9"] + SUN, "--shadow-sigmoid-scale"),
    "steps without sdf": (["--latent-index", "0", "--shadow-steps", "32"] + SUN, "--sun-shadows sdf"),
    "bias without sdf": (["--latent-index", "0", "--shadow-bias", "0.02"] + SUN, "--sun-shadows sdf"),
    "diameter without sdf": (["--latent-index", "0", "--sun-shadows", "ddf", "--shadow-angular-diameter", "2"] + SUN, "--sun-shadows sdf"),
    "no sun": (["--latent-index", "0", "--sun-shadows", "sdf"], "needs a sun"),
    "no steps": (["--latent-index", "0", "--sun-shadows", "sdf", "--shadow-steps", "0"] + SUN, "steps"),
    "a diameter of 180": (["--latent-index", "0", "--sun-shadows", "sdf", "--shadow-angular-diameter", "180"] + SUN, "angular_diameter_deg"),
    "another mode": (["--latent-index", "0", "--sun-shadows", "mesh"] + SUN, "--sun-shadows"),
}


@pytest.mark.parametrize("extra, names", list(ERRORS.values()), ids=list(ERRORS))
def test_cli_argument_errors(extra, names, capsys):
    with pytest.raises(SystemExit) as e:
        _parse(*extra)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "error:" in err and names in err


def test_cli_defaults():
    _, (mode, trace), args = _parse("--latent-index", "0", *SUN)
    assert (mode, trace) == ("ddf", None) and args.sun_shadows == "ddf"
    _, (mode, trace), _ = _parse("--latent-index", "0", "--sun-shadows", "sdf", *SUN)
    assert mode == "sdf" and trace == {"steps": 96, "bias": 1e-2, "angular_diameter_deg": 0.533}
    _, (mode, trace), _ = _parse("--latent-index", "0", "--sun-shadows", "sdf", "--shadow-steps", "48", "--shadow-bias", "0.02",
                                 "--shadow-angular-diameter", "0", *SUN)
    assert mode == "sdf" and trace == {"steps": 48, "bias": 0.02, "angular_diameter_deg": 0.0}


@pytest.mark.parametrize("sun", (["--latent-index", "0", "--sun-path", "90", "5", "180", "50", "--sun-steps", "4", "--shadow-map"],
                                 ["--envmap", "a.hdr", "--extract-sun"], ["--daylight"] + SUN), ids=("path", "extract", "daylight"))
def test_cli_sdf_shadows_go_with_every_way_of_getting_a_sun(sun):
    _, (mode, trace), _ = _parse("--sun-shadows", "sdf", *sun)
    assert mode == "sdf" and trace["steps"] == 96


def test_package_defaults_are_the_rule_s():
    from neusky_amd.relight import SHADOW_DEFAULTS, TRACE_DEFAULTS, shadows
    assert (shadows.ALIVE, shadows.HIT, shadows.ESCAPED, shadows.EXHAUSTED) == (ST.ALIVE, ST.HIT, ST.ESCAPED, ST.EXHAUSTED)
    assert {k: TRACE_DEFAULTS[k] for k in ST.DEFAULTS} == ST.DEFAULTS and TRACE_DEFAULTS["angular_diameter_deg"] == 0.0
    assert SHADOW_DEFAULTS["bias"] == 1e-2 and SHADOW_DEFAULTS["angular_diameter_deg"] == 0.533
    p = shadows.trace_params(shadows.trace_settings({"angular_diameter_deg": 4.0}, SHADOW_DEFAULTS))
    assert p.shape == (6,) and abs(float(p[3]) - ST.tan_half(4.0)) < 1e-8 and float(p[4]) == 1.0 and abs(float(p[5]) - 1e-2) < 1e-9
    with pytest.raises(ValueError):
        shadows.trace_settings({"step": 3}, SHADOW_DEFAULTS)
