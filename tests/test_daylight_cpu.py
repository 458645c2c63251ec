"""The clear-sky daylight model on the CPU: the float64 restatement (daylight_cpu.py) against the values the model's definitions were
pinned with, its edge rules (zenith, set sun, below the horizon), relight.DaylightSky's host side against the restatement, and the
`--daylight` command line's argument errors."""
import math

import numpy as np
import pytest

import daylight_cpu as DC
from neusky_amd.relight import DaylightSky, SunLight
from neusky_amd.relight.__main__ import build_parser, parse_daylight, parse_suns

PIN = 1e-3  # the pins were printed to 3 or 4 digits


def _close(got, want):
    np.testing.assert_allclose(np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1), rtol=PIN, atol=0.0)


@pytest.mark.parametrize("elevation, d, Yxy, rgb", [
    (45.0, (0.0, 0.0, 1.0), (7.320, 0.2457, 0.2515), (4.625, 7.410, 14.38)),
    (45.0, (-0.6, 0.0, 0.8), (5.100, 0.2358, 0.2467), (2.626, 5.286, 10.54)),
    (10.0, (1.0, 0.0, 1e-3), (21.135, 0.4106, 0.4146), (30.90, 19.73, 6.273)),
])
def test_sky_pins(elevation, d, Yxy, rgb):
    s = DC.sun_direction(0.0, elevation)
    Y, x, y, below = DC.sky_Yxy(3.0, s, [d])
    assert not below[0]
    _close([Y[0], x[0], y[0]], Yxy)
    _close(DC.radiance(3.0, [s], [d]), rgb)


@pytest.mark.parametrize("elevation, tau", [(20.0, (0.4967, 0.4176, 0.2723)), (60.0, (0.7570, 0.7066, 0.5960))])
def test_transmittance_pins(elevation, tau):
    _close(DC.transmittance(3.0, elevation), tau)
    _close(DaylightSky(3.0).transmittance(elevation), tau)
    _close(DaylightSky(3.0, exposure=1.0).sun_colour(0.0, elevation), 133.1 / (2.0 * math.pi) * np.array(tau))


@pytest.mark.parametrize("T", [2.0, 3.0, 6.0, 10.0])
@pytest.mark.parametrize("elevation", [2.0, 10.0, 45.0, 90.0])
def test_sky_at_the_zenith_is_the_zenith_value(T, elevation):
    s = DC.sun_direction(30.0, elevation)
    Y, x, y, _ = DC.sky_Yxy(T, s, [(0.0, 0.0, 2.5)])
    Yz, xz, yz = DC.zenith(T, np.arccos(s[2]))
    np.testing.assert_allclose([Y[0], x[0], y[0]], [Yz, xz, yz], rtol=1e-12)


@pytest.mark.parametrize("T", [2.0, 3.0, 6.0, 10.0])
@pytest.mark.parametrize("elevation", [2.0, 10.0, 45.0, 90.0])
def test_sky_is_finite_and_not_negative(T, elevation):
    d = np.random.default_rng(11).normal(size=(4000, 3))
    rgb = DC.radiance(T, [DC.sun_direction(75.0, elevation)], d, exposure=0.7, ground=(0.3, 0.2, 0.1))
    assert rgb.shape == (1, 4000, 3) and np.isfinite(rgb).all() and (rgb >= 0.0).all() and rgb.max() > 0.0
    raw = DC.radiance(T, [DC.sun_direction(75.0, elevation)], d, clamp=False)
    assert (raw > 0.0).all()  # from 2 degrees of elevation up the clamp has nothing to do


def test_a_set_sun_has_no_sky_and_no_colour():
    d = np.random.default_rng(12).normal(size=(100, 3))
    suns = [DC.sun_direction(10.0, 0.0), DC.sun_direction(10.0, -20.0), DC.sun_direction(10.0, 5.0)]
    suns[0][2] = 0.0  # exactly on the horizon
    rgb = DC.radiance(3.0, suns, d)
    assert (rgb[0] == 0.0).all() and (rgb[1] == 0.0).all() and rgb[2].min() > 0.0
    sky = DaylightSky(3.0)
    assert sky.sun_colour(10.0, 0.0) == (0.0, 0.0, 0.0) and sky.sun_colour(10.0, -20.0) == (0.0, 0.0, 0.0)
    assert (DC.sun_colour(3.0, -20.0) == 0.0).all() and (DC.sun_colour(3.0, 0.0) == 0.0).all()


def test_below_the_horizon_is_ground_times_the_horizon_point():
    g = np.random.default_rng(13)
    d = g.normal(size=(200, 3))
    d[:, 2] = -np.abs(d[:, 2]) - 1e-3
    horizon = d.copy()
    horizon[:, 2] = 0.0
    ground = np.array([0.3, 0.2, 0.1])
    s = [DC.sun_direction(200.0, 25.0)]
    np.testing.assert_allclose(DC.radiance(4.0, s, d, ground=ground), DC.radiance(4.0, s, horizon) * ground, rtol=1e-13)
    np.testing.assert_allclose(DC.radiance(4.0, s, [(0.0, 0.0, -3.0)], ground=ground), DC.radiance(4.0, s, [(0.0, 0.0, 1.0)]) * ground, rtol=1e-13)
    np.testing.assert_allclose(DC.radiance(4.0, s, 7.0 * horizon), DC.radiance(4.0, s, horizon), rtol=1e-12)  # any length


def test_daylight_sky_host_side():
    with pytest.raises(ValueError, match="turbidity"):
        DaylightSky(1.9)
    with pytest.raises(ValueError, match="turbidity"):
        DaylightSky(10.5)
    with pytest.raises(ValueError, match="ground"):
        DaylightSky(3.0, ground=(1.0, 1.0))
    sky = DaylightSky(turbidity=6.0, exposure=0.2)
    assert sky.ground == (0.25, 0.25, 0.25) and DaylightSky().turbidity == 3.0 and DaylightSky().exposure == 0.1
    for el in (0.5, 5.0, 33.0, 90.0):
        np.testing.assert_allclose(sky.sun_colour(12.0, el), DC.sun_colour(6.0, el, 0.2), rtol=1e-12)
    one = sky.sun(12.0, 33.0)
    assert isinstance(one, SunLight) and one.colour == sky.sun_colour(12.0, 33.0) and one.elevation_deg == 33.0
    path = sky.sun_path(90.0, 4.0, 180.0, 60.0, 5)
    assert [s.elevation_deg for s in path] == [4.0, 18.0, 32.0, 46.0, 60.0] and path[0].azimuth_deg == 90.0 and path[-1].azimuth_deg == 180.0
    assert all(s.colour == sky.sun_colour(s.azimuth_deg, s.elevation_deg) for s in path)
    assert path[0].colour[2] / path[0].colour[0] < path[-1].colour[2] / path[-1].colour[0]  # a low sun is redder
    assert sum(path[0].colour) < sum(path[-1].colour)  # and weaker


BASE = ["--checkpoint", "c.ckpt", "--camera-path", "p.json", "--output-dir", "o"]
SUN = ["--sun-azimuth", "10", "--sun-elevation", "20"]


def _parse(*extra):
    ap = build_parser()
    args = ap.parse_args(BASE + list(extra))
    daylight = parse_daylight(ap, args)
    return daylight, parse_suns(ap, args, daylight), args


ERRORS = {
    "no sun": (["--daylight"], "sun"),
    "one angle": (["--daylight", "--sun-azimuth", "10"], "sun"),
    "envmap": (["--daylight", "--envmap", "a.hdr"] + SUN, "--envmap"),
    "turntable": (["--daylight", "--turntable", "2"] + SUN, "--turntable"),
    "exposure": (["--daylight", "--exposure", "2"] + SUN, "--sky-exposure"),
    "rotation": (["--daylight", "--rotation-deg", "20"] + SUN, "--rotation-deg"),
    "transfer": (["--daylight", "--transfer", "fp16"] + SUN, "--transfer"),
    "extract-sun": (["--daylight", "--extract-sun"], "--extract-sun"),
    "turbidity 1": (["--daylight", "--turbidity", "1"] + SUN, "turbidity"),
    "turbidity without the flag": (["--latent-index", "0", "--turbidity", "4"], "--daylight"),
}


@pytest.mark.parametrize("extra, names", list(ERRORS.values()), ids=list(ERRORS))
def test_cli_argument_errors(extra, names, capsys):
    with pytest.raises(SystemExit) as e:
        _parse(*extra)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "error:" in err and names in err


def test_cli_main_rejects_before_it_loads_anything(capsys):
    from neusky_amd.relight.__main__ import main
    with pytest.raises(SystemExit) as e:
        main(BASE + ["--daylight", "--exposure", "2"] + SUN)
    assert e.value.code == 2 and "--sky-exposure" in capsys.readouterr().err


def test_cli_daylight_suns_take_the_models_colour():
    daylight, suns, args = _parse("--daylight", "--turbidity", "5", "--sky-exposure", "0.2", "--ground", "0.1", "0.2", "0.3",
                                  "--sun-path", "90", "5", "180", "50", "--sun-steps", "4", "--shadow-map", "--save-hdr")
    assert (daylight.turbidity, daylight.exposure, daylight.ground) == (5.0, 0.2, (0.1, 0.2, 0.3))
    assert suns == DaylightSky(5.0, 0.2).sun_path(90.0, 5.0, 180.0, 50.0, 4) and len(suns) == 4
    daylight, suns, _ = _parse("--daylight", *SUN)
    assert suns == [DaylightSky().sun(10.0, 20.0)]
    _, suns, _ = _parse("--daylight", "--sun-colour", "1", "2", "3", *SUN)  # a colour of the user's own stands
    assert suns == [SunLight(10.0, 20.0, (1.0, 2.0, 3.0))]
    daylight, suns, _ = _parse("--latent-index", "0", *SUN)  # and without the flag nothing changed
    assert daylight is None and suns == [SunLight(10.0, 20.0)]
