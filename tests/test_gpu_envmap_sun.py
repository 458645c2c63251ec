"""The sun-extraction kernels (csrc/envmap_sun.hip: peak, ring, split) against the float64 restatement of their definitions
(envmap_sun_cpu.py) on synthetic skies with a Gaussian sun, and the properties the definitions promise: ties, the lower hemisphere,
non-finite texels, an overcast map, bitwise repeatability."""
import math

import numpy as np
import pytest
import torch

import envmap_sun_cpu as EC
from neusky_amd import hip
from neusky_amd.relight import EnvironmentMap, extract_sun

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# the cases of the CPU test, and a map large enough for several workgroups in every pass (16 in the peak's, 20 in the ring's, 96 in the
# split's: both reduction stages) and several steps of every strided loop (a thread takes about 4)
CASES = EC.CASES + [(256, 512, "blender", -75.3, 33.3, 2.0, 6.0)]


def _device_map(map32, offset):
    """the map in device memory, `offset` floats past a 16-byte boundary"""
    flat = torch.empty(map32.size + offset, dtype=torch.float32, device=DEV)
    data = flat[offset:].view(map32.shape)
    data.copy_(torch.from_numpy(np.ascontiguousarray(map32)))
    assert data.data_ptr() % 16 == 4 * offset
    return data


def run_kernels(map32, convention, rho_deg, ratio=10.0, offset=0):
    """(peak index, Y_p, ring [2], residual [H, W, 3] fp32, stats [12]) as numpy, from the three entry points on one stream"""
    data = _device_map(map32, offset)
    conv = hip.ENVMAP_BLENDER if convention == "blender" else hip.ENVMAP_NEUSKY
    scratch = torch.full((hip.ENVMAP_SUN_SCRATCH_BYTES // 8,), float("nan"), dtype=torch.float64, device=DEV)
    peak = torch.empty(2, dtype=torch.int64, device=DEV)
    ring = torch.empty(2, dtype=torch.float64, device=DEV)
    stats = torch.empty(12, dtype=torch.float64, device=DEV)
    residual = torch.full_like(data, float("nan"))
    hip.envmap_peak(data, conv, scratch, peak)
    hip.envmap_sun_ring(data, conv, peak, math.radians(rho_deg), scratch, ring)
    hip.envmap_sun_split(data, conv, peak, ring, math.radians(rho_deg), ratio, scratch, residual, stats)
    torch.cuda.synchronize()
    return int(peak[0].item()), float(peak.view(torch.float64)[1].item()), ring.cpu().numpy(), residual.cpu().numpy(), stats.cpu().numpy()


@pytest.fixture(scope="module")
def runs():
    out = {}
    for c in CASES:
        H, W, conv, az, el, sigma, rho = c
        m = EC.synthetic_map(H, W, conv, az, el, sigma)
        out[c] = (m, EC.extract(m, conv, rho), run_kernels(m, conv, rho))
    return out


def _rel(a, b):
    return abs(a - b) / abs(b)


def _ulps(a, b):
    """the distance of two finite fp32 arrays in units in the last place"""
    def key(x):
        i = x.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


@pytest.mark.parametrize("case", CASES, ids=EC.case_id)
def test_kernels_match_the_definitions(runs, case):
    H, W, conv, az, el, sigma, rho = case
    m, ref, (p, Yp, ring, residual, stats) = runs[case]
    assert ref.found and EC.boundary_margin(ref, rho) > 1e-9 and EC.peak_margin(ref) > 1e-6  # the precondition
    assert p == ref.peak
    assert stats[10] == ref.peak_row and stats[11] == ref.peak_col and stats[9] == 1.0
    err_m = np.abs(stats[0:3] - ref.m).max()
    err_c = (np.abs(stats[3:6] - ref.C) / ref.C).max()
    ulps = _ulps(residual, ref.residual)
    print(f"{EC.case_id(case)}: m {err_m:.2e} C {err_c:.2e} Y_p {_rel(Yp, ref.Y_p):.2e} tau {_rel(stats[7], ref.tau):.2e} "
          f"Omega {_rel(stats[8], ref.solid_angle):.2e} ring {_rel(ring[0], ref.ring_omega):.2e} {_rel(ring[1], ref.ring_omega_Y):.2e} "
          f"residual ulps max {ulps.max()} (differing {int((ulps > 0).sum())} of {int(ref.excess.sum()) * 3})")
    assert err_m <= 1e-9
    assert _rel(Yp, ref.Y_p) <= 1e-12 and stats[6] == Yp
    assert _rel(stats[7], ref.tau) <= 1e-12
    assert _rel(stats[8], ref.solid_angle) <= 1e-12
    assert _rel(ring[0], ref.ring_omega) <= 1e-12 and _rel(ring[1], ref.ring_omega_Y) <= 1e-12
    assert ulps.max() <= 1
    assert np.array_equal(residual[~ref.excess].view(np.int32), m[~ref.excess].view(np.int32))  # bitwise outside the excess set
    assert err_c <= 1e-6
    # conservation from the GPU's own outputs, in float64
    before, after = EC.flux(m, H, W, conv), EC.flux(residual, H, W, conv) + 2.0 * np.pi * stats[3:6]
    cons = np.abs(before - after).max() / np.abs(before).max()
    print(f"conservation {cons:.2e}")
    assert cons <= 1e-12


def test_overcast_map_is_copied():
    m = EC.sky_map(96, 200, "neusky").astype(np.float32)  # 3 H W is a multiple of 4; see the odd-sized copy below
    ref = EC.extract(m, "neusky", 6.0)
    p, Yp, ring, residual, stats = run_kernels(m, "neusky", 6.0)
    assert not ref.found and p == ref.peak and stats[9] == 0.0
    assert np.array_equal(residual.view(np.int32), m.view(np.int32))
    assert not stats[3:6].any() and stats[8] == 0.0
    np.testing.assert_allclose(stats[0:3], ref.e_p, atol=1e-15)
    assert _rel(stats[7], ref.tau) <= 1e-12


@pytest.mark.parametrize("shape", [(37, 91), (5, 3), (2, 1)])
def test_odd_sized_copy(shape):
    """3 H W not a multiple of 4: the tail of the streamed copy"""
    H, W = shape
    m = EC.sky_map(H, W, "blender").astype(np.float32)
    _, _, _, residual, stats = run_kernels(m, "blender", 40.0)
    assert stats[9] == 0.0 and np.array_equal(residual.view(np.int32), m.view(np.int32))


def test_unaligned_map_takes_the_scalar_loads(runs):
    """a map that does not start on a 16-byte boundary: same outputs, bit for bit"""
    case = CASES[3]  # 37 x 91
    m, _, (p, Yp, ring, residual, stats) = runs[case]
    p2, Yp2, ring2, residual2, stats2 = run_kernels(m, case[2], case[6], offset=1)
    assert p2 == p and Yp2 == Yp and ring2.tobytes() == ring.tobytes() and stats2.tobytes() == stats.tobytes()
    assert residual2.tobytes() == residual.tobytes()
    _, _, _, copied, _ = run_kernels(EC.sky_map(37, 91, "blender").astype(np.float32), "blender", 15.0, offset=3)
    assert np.array_equal(copied, EC.sky_map(37, 91, "blender").astype(np.float32))


def test_equal_maxima_give_the_lower_index():
    H, W = 128, 256
    m = EC.sky_map(H, W, "blender").astype(np.float32)
    spots = [(40, 200), (17, 31), (17, 30), (63, 255), (5, 77)]  # several workgroups and both reduction stages apart
    for i, j in spots:
        m[i, j] = (300.0, 300.0, 300.0)
    p, Yp, _, _, stats = run_kernels(m, "blender", 6.0)
    assert p == 5 * W + 77 and stats[10] == 5 and stats[11] == 77
    m[5, 77] = m[5, 78]
    p, _, _, _, _ = run_kernels(m, "blender", 6.0)
    assert p == 17 * W + 30


def test_lower_hemisphere_is_ignored():
    H, W, conv = 128, 256, "neusky"
    m = EC.synthetic_map(H, W, conv, 50.0, 35.0, 2.0)
    ref = EC.extract(m, conv, 6.0)
    bright = m.copy()
    bright[64, 10] = (9000.0, 9000.0, 9000.0)  # the first row below the horizon
    bright[100, 100] = (9000.0, 9000.0, 9000.0)
    p, Yp, _, residual, stats = run_kernels(bright, conv, 6.0)
    assert p == ref.peak and p // W < 64
    assert np.array_equal(residual[64:].view(np.int32), bright[64:].view(np.int32))
    np.testing.assert_allclose(stats[0:3], ref.m, atol=1e-9)
    H, W = 37, 91  # an odd height: row 18 straddles the horizon, (18 + 0.5) / 37 = 0.5 is not below it
    m = EC.sky_map(H, W, conv).astype(np.float32)
    m[18, 5] = (50.0, 50.0, 50.0)
    m[17, 80] = (20.0, 20.0, 20.0)
    p, _, _, _, _ = run_kernels(m, conv, 15.0)
    assert p == 17 * W + 80


def test_non_finite_texels_are_skipped_and_copied():
    H, W, conv, rho = 128, 256, "blender", 6.0
    m = EC.synthetic_map(H, W, conv, 37.3, 41.7, 2.0)
    clean = EC.extract(m, conv, rho)
    i, j = clean.peak_row, clean.peak_col
    m[i, j + 1] = (np.nan, 1.0, 1.0)  # next to the sun, in the cap
    m[i - 1, j] = (1.0, np.inf, 1.0)
    m[i + 6, j] = (1.0, 1.0, -np.inf)  # in the ring (8.4 degrees away)
    m[3, 3] = (np.nan, np.nan, np.nan)  # far away, in the streamed copy
    ref = EC.extract(m, conv, rho)
    assert ref.found and ref.peak == clean.peak and 6.0 < EC.angle_deg(EC.texel_directions(H, W, conv)[0][i + 6, j], ref.e_p) < 12.0
    p, Yp, ring, residual, stats = run_kernels(m, conv, rho)
    assert p == ref.peak and np.isfinite(stats).all() and np.isfinite(ring).all()
    assert np.array_equal(residual.view(np.int32)[~ref.excess], m.view(np.int32)[~ref.excess])  # the NaN payloads included
    assert not ref.excess[i, j + 1] and not ref.excess[i - 1, j]
    assert _ulps(np.nan_to_num(residual), np.nan_to_num(ref.residual)).max() <= 1
    np.testing.assert_allclose(stats[0:3], ref.m, atol=1e-9)
    np.testing.assert_allclose(stats[3:6], ref.C, rtol=1e-6)
    assert _rel(stats[7], ref.tau) <= 1e-12 and _rel(stats[8], ref.solid_angle) <= 1e-12
    m[:64] = np.nan  # no finite texel above the horizon: no peak
    p, Yp, _, residual, stats = run_kernels(m, conv, rho)
    assert p == -1 and Yp == 0.0 and stats[9] == 0.0 and stats[10] == -1 and stats[11] == -1 and list(stats[0:3]) == [0.0, 0.0, 1.0]
    assert np.array_equal(residual.view(np.int32), m.view(np.int32))


def test_two_runs_are_bitwise_equal(runs):
    case = CASES[-1]
    m, _, (p, Yp, ring, residual, stats) = runs[case]
    p2, Yp2, ring2, residual2, stats2 = run_kernels(m, case[2], case[6])
    assert p2 == p and Yp2 == Yp
    assert ring2.tobytes() == ring.tobytes() and stats2.tobytes() == stats.tobytes() and residual2.tobytes() == residual.tobytes()


def test_extract_sun_wraps_the_kernels(runs):
    case = CASES[0]
    H, W, conv, az, el, sigma, rho = case
    m, ref, (p, Yp, ring, residual, stats) = runs[case]
    env = EnvironmentMap(m, conv, exposure=1.5)
    before = env.data.clone()
    ext = extract_sun(env, radius_deg=rho)
    assert torch.equal(env.data, before) and ext.envmap is not env and ext.envmap.data.data_ptr() != env.data.data_ptr()
    assert ext.envmap.convention == conv and ext.envmap.exposure == 1.5 and ext.envmap.device == env.device
    assert ext.found and list(ext.direction) == list(stats[0:3]) and list(ext.colour) == list(stats[3:6])
    assert ext.peak_luminance == Yp and ext.sky_luminance == stats[7] and ext.solid_angle == stats[8]
    assert np.array_equal(ext.envmap.data.cpu().numpy().view(np.int32), residual.view(np.int32))
    total = float((EC.flux(m, H, W, conv) * EC.LUM).sum())
    assert abs(ext.flux_fraction - 2.0 * np.pi * float((ref.C * EC.LUM).sum()) / total) < 1e-9
    sun = ext.sun()
    assert EC.angle_deg(sun.direction, EC.direction(az, el)) < 45.0 / H
    np.testing.assert_allclose(sun.colour, 1.5 * stats[3:6], rtol=1e-15)
    assert extract_sun(env, radius_deg=rho, min_peak_ratio=1e6).found is False
    with pytest.raises(ValueError):
        extract_sun(env, radius_deg=1.0)
    with pytest.raises(ValueError):
        extract_sun(env, radius_deg=45.0)
