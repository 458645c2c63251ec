"""The sun extraction's definitions on the CPU: the float64 restatement (envmap_sun_cpu.py) recovers a synthetic sun's direction and
colour and conserves the map's flux; and the host side of relight.extract_sun that needs no device: SunLight.from_direction,
SunExtraction.sun, the argument checks and the command line's."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import envmap_sun_cpu as EC
from neusky_amd.relight import SunExtraction, SunLight, extract_sun, sun_direction, z_rotation
from neusky_amd.relight.__main__ import build_parser, parse_suns


@pytest.fixture(scope="module")
def extractions():
    out = {}
    for c in EC.CASES:
        H, W, conv, az, el, sigma, rho = c
        m = EC.synthetic_map(H, W, conv, az, el, sigma)
        out[c] = (m, EC.extract(m, conv, rho))
    return out


@pytest.mark.parametrize("case", EC.CASES, ids=EC.case_id)
def test_preconditions(extractions, case):
    """no texel within 1e-9 of a cap or ring boundary and a unique maximum: set membership does not depend on rounding"""
    _, ref = extractions[case]
    assert ref.found
    assert EC.boundary_margin(ref, case[6]) > 1e-9
    assert EC.peak_margin(ref) > 1e-6


@pytest.mark.parametrize("case", EC.CASES, ids=EC.case_id)
def test_direction_within_a_quarter_texel(extractions, case):
    H, W, conv, az, el, sigma, rho = case
    _, ref = extractions[case]
    err = EC.angle_deg(ref.m, EC.direction(az, el))
    print(f"{EC.case_id(case)}: direction error {err:.4f} degrees (bar {45.0 / H:.4f}), peak texel off by "
          f"{EC.angle_deg(ref.e_p, EC.direction(az, el)):.3f}")
    assert err < 45.0 / H
    assert abs(np.linalg.norm(ref.m) - 1.0) < 1e-14


def _cut_at_three_sigma(case):
    return case[6] == 3.0 * case[5]


@pytest.mark.parametrize("case", list(filter(_cut_at_three_sigma, EC.CASES)), ids=EC.case_id)
def test_colour_is_the_lobe_integral(extractions, case):
    """C = (1 / 2 pi) int A exp(-a^2 / 2 sigma^2) = A sigma^2 per unit tint; the cut at 3 sigma loses exp(-4.5) = 1.1 %, the clamp to
    the sky level a little more"""
    H, W, conv, az, el, sigma, rho = case
    _, ref = extractions[case]
    want = EC.SUN_PEAK * math.radians(sigma) ** 2 * EC.SUN_TINT
    rel = np.abs(ref.C - want).max() / want.max()
    print(f"{EC.case_id(case)}: C {ref.C}, A sigma^2 tint {want}, rel {rel:.4f}")
    assert np.all(np.abs(ref.C - want) <= 0.03 * want)


@pytest.mark.parametrize("case", EC.CASES, ids=EC.case_id)
def test_flux_is_conserved(extractions, case):
    H, W, conv = case[:3]
    m, ref = extractions[case]
    before, after = EC.flux(m, H, W, conv), EC.flux(ref.residual, H, W, conv) + 2.0 * np.pi * ref.C
    rel = np.abs(before - after).max() / np.abs(before).max()
    print(f"{EC.case_id(case)}: conservation {rel:.2e}")
    assert rel <= 1e-12
    # the residual differs from the map on the excess set only, and its luminance there is the sky level
    assert np.array_equal(ref.residual[~ref.excess], m[~ref.excess])
    np.testing.assert_allclose(EC.luminance(ref.residual[ref.excess].astype(np.float64)), ref.tau, rtol=1e-6)
    assert ref.excess.sum() >= 4 and ref.solid_angle > 0.0


def test_overcast_map_has_no_sun():
    m = EC.sky_map(64, 128, "blender").astype(np.float32)
    ref = EC.extract(m, "blender", 6.0)
    assert not ref.found and np.array_equal(ref.residual, m) and not ref.C.any() and np.array_equal(ref.m, ref.e_p)


def test_from_direction_round_trip():
    for az, el in ((37.3, 41.7), (-120.0, 55.0), (179.6, 20.2), (10.0, 88.9), (0.0, 0.0), (200.0 - 360.0, -12.0)):
        s = SunLight.from_direction(tuple(2.5 * x for x in sun_direction(az, el)), (3.0, 2.0, 1.0))
        assert abs(s.azimuth_deg - az) < 1e-9 and abs(s.elevation_deg - el) < 1e-9 and s.colour == (3.0, 2.0, 1.0)
        np.testing.assert_allclose(s.direction, sun_direction(az, el), atol=1e-14)
    assert SunLight.from_direction((0.0, 0.0, 4.0)).elevation_deg == 90.0
    with pytest.raises(ValueError):
        SunLight.from_direction((0.0, 0.0, 0.0))


def _extraction(found=True, exposure=1.0):
    m = EC.direction(37.3, 41.7)
    return SunExtraction(envmap=SimpleNamespace(exposure=exposure), found=found, direction=tuple(m), colour=(0.5, 0.4, 0.3), peak_luminance=400.0,
                         sky_luminance=0.6, solid_angle=0.01, flux_fraction=0.3)


def test_sun_is_the_map_direction_turned_back():
    ext = _extraction()
    m = np.array(ext.direction)
    np.testing.assert_allclose(ext.sun().direction, m, atol=1e-14)
    np.testing.assert_allclose(ext.sun(None).colour, ext.colour)
    for angle in (0.3, -2.0, math.pi):
        R = z_rotation(angle)
        np.testing.assert_allclose(ext.sun(R).direction, R.double().numpy().T @ m, atol=1e-14)
        # R^T: the sun turns by -angle.  The matrix is fp32: its entries are off by 2^-24, the angles by up to 1e-5 degrees
        assert abs((ext.sun(R).azimuth_deg - (37.3 - math.degrees(angle)) + 180.0) % 360.0 - 180.0) < 1e-5
        assert abs(ext.sun(R).elevation_deg - 41.7) < 1e-5
    g = torch.Generator().manual_seed(0)
    Q, _ = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))  # any rotation, as a tensor or an array
    np.testing.assert_allclose(ext.sun(Q).direction, Q.numpy().T @ m, atol=1e-14)
    np.testing.assert_allclose(ext.sun(Q.numpy()).direction, Q.numpy().T @ m, atol=1e-14)
    with pytest.raises(ValueError):
        ext.sun(np.eye(4))
    assert _extraction(found=False).sun() is None and _extraction(found=False).sun(z_rotation(1.0)) is None


def test_exposure_scales_the_sun():
    ext = _extraction(exposure=2.5)
    np.testing.assert_allclose(ext.sun().colour, [2.5 * c for c in ext.colour], rtol=1e-15)
    ext.envmap.exposure = 0.5  # the map's CURRENT exposure
    np.testing.assert_allclose(ext.sun(z_rotation(0.7)).colour, [0.5 * c for c in ext.colour], rtol=1e-15)
    assert ext.colour == (0.5, 0.4, 0.3)


def test_radius_errors_need_no_device():
    env = SimpleNamespace(shape=(64, 128))
    with pytest.raises(ValueError, match="ring"):
        extract_sun(env, radius_deg=180.0 / 64 - 1e-6)
    with pytest.raises(ValueError, match="45"):
        extract_sun(env, radius_deg=45.0)
    with pytest.raises(ValueError):
        extract_sun(env, radius_deg=float("nan"))


BASE = ["--checkpoint", "c.ckpt", "--camera-path", "p.json", "--output-dir", "o"]


def _parse(*extra):
    ap = build_parser()
    args = ap.parse_args(BASE + list(extra))
    return parse_suns(ap, args), args


@pytest.mark.parametrize("extra", [
    ("--latent-index", "0", "--extract-sun"),  # needs --envmap
    ("--envmap", "a.hdr", "--extract-sun", "--transfer", "fp16"),
    ("--envmap", "a.hdr", "--extract-sun", "--sun-azimuth", "10", "--sun-elevation", "20"),
    ("--envmap", "a.hdr", "--extract-sun", "--sun-elevation", "20"),
    ("--envmap", "a.hdr", "--extract-sun", "--sun-path", "0", "10", "90", "10", "--sun-steps", "3"),
    ("--envmap", "a.hdr", "--extract-sun", "--sun-steps", "3"),
    ("--envmap", "a.hdr", "--extract-sun", "--sun-colour", "1", "1", "1"),
    ("--envmap", "a.hdr", "--extract-sun", "--sun-radiance", "1", "1", "1"),
    ("--envmap", "a.hdr", "--extract-sun", "--sun-angular-diameter", "1.0"),
    ("--envmap", "a.hdr", "--extract-sun", "--sun-search-radius", "45"),
    ("--envmap", "a.hdr", "--extract-sun", "--sun-search-radius", "0"),
    ("--envmap", "a.hdr", "--extract-sun", "--sun-min-peak-ratio", "-1"),
    ("--envmap", "a.hdr", "--sun-search-radius", "3"),  # need --extract-sun
    ("--envmap", "a.hdr", "--sun-min-peak-ratio", "20"),
    ("--envmap", "a.hdr", "--shadow-map"),  # still needs a sun
], ids=" ".join)
def test_cli_argument_errors(extra, capsys):
    with pytest.raises(SystemExit) as e:
        _parse(*extra)
    assert e.value.code == 2
    assert "error:" in capsys.readouterr().err


def test_cli_extract_sun_counts_as_a_sun():
    suns, args = _parse("--envmap", "a.hdr", "--extract-sun", "--shadow-map", "--shadow-threshold", "0.1", "--shadow-sigmoid-scale", "30",
                        "--turntable", "4", "--rotation-deg", "15", "--exposure", "2", "--sun-search-radius", "3", "--sun-min-peak-ratio", "20")
    assert suns is None and args.extract_sun and args.shadow_map and args.sun_search_radius == 3.0 and args.sun_min_peak_ratio == 20.0
    suns, args = _parse("--envmap", "a.hdr", "--extract-sun")
    assert suns is None and args.sun_search_radius is None and args.sun_min_peak_ratio is None
    suns, args = _parse("--envmap", "a.hdr")  # and without the flag nothing changed
    assert suns is None and not args.extract_sun
    suns, _ = _parse("--envmap", "a.hdr", "--sun-azimuth", "10", "--sun-elevation", "20")
    assert suns == [SunLight(10.0, 20.0)]
