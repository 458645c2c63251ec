"""The directional sun off the GPU: direction, colour and sweep of neusky_amd.relight.sun against the float64 restatement (sun_cpu.py),
the claim behind the colour's normalisation, and the command line's argument errors."""
import math

import numpy as np
import pytest

import sun_cpu as SC
from neusky_amd.relight.sun import SunLight, sun_direction, sun_path, sun_solid_angle


def test_sun_direction():
    assert np.allclose(sun_direction(90.0, 45.0), (0.0, math.sqrt(0.5), math.sqrt(0.5)), atol=1e-15)
    assert np.allclose(sun_direction(0.0, 0.0), (1.0, 0.0, 0.0), atol=1e-15)
    for az, el in ((13.0, 71.0), (200.0, -4.0), (-75.0, 0.5)):
        d = np.array(sun_direction(az, el))
        assert np.allclose(d, SC.sun_direction(az, el), atol=1e-15) and abs(np.linalg.norm(d) - 1.0) < 1e-15
        assert SunLight(az, el).direction == sun_direction(az, el)


def test_from_radiance_closed_form():
    L = (2.0e4, 1.8e4, 1.5e4)
    for diameter in (0.533, 1.0, 10.0):
        omega = 2.0 * math.pi * (1.0 - math.cos(math.radians(diameter) / 2.0))
        assert abs(sun_solid_angle(diameter) - omega) < 1e-9 * omega  # (the closed form cancels: 1 - cos of a quarter degree)
        got = SunLight.from_radiance(30.0, 40.0, L, angular_diameter_deg=diameter)
        assert np.allclose(got.colour, [x * omega / (2.0 * math.pi) for x in L], rtol=1e-9)
        assert np.allclose(got.colour, SC.colour_from_radiance(L, diameter), rtol=1e-9)
    assert abs(sun_solid_angle(0.533) - 6.8e-5) < 1e-6  # the sun
    assert SunLight.from_radiance(1.0, 2.0, L).colour == SunLight.from_radiance(1.0, 2.0, L, angular_diameter_deg=0.533).colour


def test_sun_path_endpoints_and_spacing():
    p = sun_path(100.0, 5.0, 260.0, -5.0, 6, colour=(1.0, 0.9, 0.8))
    assert len(p) == 6 and (p[0].azimuth_deg, p[0].elevation_deg) == (100.0, 5.0) and (p[-1].azimuth_deg, p[-1].elevation_deg) == (260.0, -5.0)
    assert np.allclose(np.diff([s.azimuth_deg for s in p]), 32.0) and np.allclose(np.diff([s.elevation_deg for s in p]), -2.0)
    assert all(s.colour == (1.0, 0.9, 0.8) for s in p)
    one = sun_path(10.0, 20.0, 30.0, 40.0, 1)
    assert len(one) == 1 and (one[0].azimuth_deg, one[0].elevation_deg) == (10.0, 20.0)
    with pytest.raises(ValueError):
        sun_path(0.0, 0.0, 1.0, 1.0, 0)


def test_colour_normalisation_against_the_direction_set():
    """A radiance L on the ONE direction of the model's 512 nearest to s lights a constant normal n through the hemisphere term by
    L clamp(<n,d>) / cnt (cnt = the directions of n's hemisphere); the sun of the same radiance and the cell's solid angle 4 pi / 512
    has C = L (4 pi / 512) / (2 pi) = L / 256 and lights it by C clamp(<n,s>).  With s = d the two agree to cnt / 256."""
    from neusky_amd.model_components.illumination import IcosahedronSamplerConfig
    dirs = IcosahedronSamplerConfig().setup().directions.double().numpy()
    assert dirs.shape == (512, 3)
    L = 7.0
    for az, el, n in ((40.0, 55.0, (0.0, 0.0, 1.0)), (200.0, 20.0, (-0.6, -0.3, 0.74)), (310.0, 70.0, (0.2, -0.1, 0.97))):
        n = np.array(n) / np.linalg.norm(n)
        s = SC.sun_direction(az, el)
        d = dirs[np.argmax(dirs @ s)]
        cos = np.clip(dirs @ n, 0.0, 1.0)
        cnt = int((cos > 0.0).sum())
        sky = L * np.clip(n @ d, 0.0, 1.0) / cnt
        C = L * (4.0 * math.pi / 512) / (2.0 * math.pi)
        sun = C * np.clip(n @ d, 0.0, 1.0)
        assert sky > 0.0 and abs(sun / sky - cnt / 256.0) < 1e-12
        assert abs(cnt - 256) <= 16  # half of an even set, up to the directions on the normal's horizon
        # and the sun at its true position differs from the snapped one by the cell's width only
        assert abs(np.clip(n @ s, 0.0, 1.0) - np.clip(n @ d, 0.0, 1.0)) < math.sqrt(4.0 * math.pi / 512)


@pytest.mark.parametrize("extra", [["--sun-steps", "3"],
                                   ["--sun-azimuth", "10", "--sun-elevation", "20", "--transfer", "fp16"],
                                   ["--sun-path", "0", "10", "90", "10", "--sun-steps", "3", "--turntable", "2"]])
def test_parser_errors(extra, capsys):
    from neusky_amd.relight.__main__ import main
    with pytest.raises(SystemExit) as e:
        main(["--checkpoint", "none.ckpt", "--camera-path", "none.json", "--output-dir", "none", "--latent-index", "0"] + extra)
    assert e.value.code == 2
    assert "error:" in capsys.readouterr().err
