"""The sun kernels (csrc/sun.hip: nsky_sun_transfer, nsky_sun_composite) against the float64 restatement of their definitions (sun_cpu.py)."""
import numpy as np
import pytest
import torch

import sun_cpu as SC
from neusky_amd import hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 1, 1), (3, 5, 1), (5, 67, 9), (130, 96, 8)]  # (R, S, K): smallest; S below a wave; S across 64 lanes and K across the 8-sun
#                                                             pass; the workload's S with R no multiple of the 4 waves of a workgroup
# the pass rule and the ray loop the kernel shares with the lamps': a full pass, a pass of one behind it, two passes and one; R = 5: a second
# workgroup with one live wave; S = 65: one sample behind a full lane stride
SHAPES += [(5, 65, 8), (5, 65, 9), (5, 65, 17)]


def _unit(rng, n):
    v = rng.standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _suns(rng, K):
    s = _unit(rng, K)
    s[:, 2] = np.abs(s[:, 2]) + 0.05
    s /= np.linalg.norm(s, axis=1, keepdims=True)
    s[0] = (0.6, 0.0, 0.8)
    return s.astype(np.float32)


def _inputs(R, S, K, seed):
    rng = np.random.default_rng(seed)
    suns = _suns(rng, K)
    normals = _unit(rng, R * S).reshape(R, S, 3)  # about half of them face away from any one sun
    normals[0, 0] = (0.0, 1.0, 0.0)  # exactly perpendicular to sun 0: <n, s> = 0
    normals[R // 2, S // 2] = 1.5 * suns[0].astype(np.float64)  # <n, s> = 1.5: the clamp at 1
    normals[::2, 1::3] *= 1.5
    albedo = rng.uniform(0.0, 1.0, (R, S, 3))
    weights = rng.uniform(0.0, 1.0, (R, S)) ** 4
    weights[:, 2::5] = 0.0
    if R > 1:
        weights[R - 1] = 0.0  # a ray that met nothing
    return tuple(x.astype(np.float32) for x in (albedo, normals, weights)) + (suns,)


def _transfer(albedo, normals, weights, suns):
    dv = [torch.from_numpy(x).to(DEV) for x in (albedo, normals, weights, suns)]
    out = torch.full((suns.shape[0], albedo.shape[0], 3), float("nan"), device=DEV)
    hip.sun_transfer(*dv, out)
    return out


@pytest.mark.parametrize("R,S,K", SHAPES)
def test_sun_transfer(R, S, K):
    albedo, normals, weights, suns = _inputs(R, S, K, seed=R + S)
    got = _transfer(albedo, normals, weights, suns)
    again = _transfer(albedo, normals, weights, suns)
    assert torch.equal(got, again)  # no atomics, one reduction order
    ref, scale = SC.transfer(albedo, normals, weights, suns)
    # every term is rounded a bounded number of times and the sum has at most S roundings: 4 S u sum_s |w a|, u = 2^-24
    tol = 4.0 * S * 2.0 ** -24 * scale[None]
    err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
    print(f"sun_transfer {(R, S, K)}: max err / tol = {np.max(err / np.maximum(tol, 1e-300)):.3f}")
    assert np.all(err <= tol), float(np.max(err - tol))
    if R > 1:
        assert np.all(got[:, R - 1].cpu().numpy() == 0.0)


def _sun_sets(K, seed):
    rng = np.random.default_rng(seed)
    if K == 1:
        return [_suns(rng, 1), np.array([[0.8, 0.6, 0.0]], np.float32), np.array([[0.0, 0.8, -0.6]], np.float32)]
    s = _suns(rng, K)
    s[1] = (0.8, 0.6, 0.0)  # on the horizon: set
    s[2] = (0.0, 0.8, -0.6)  # below it
    return [s]


@pytest.mark.parametrize("with_vis", [True, False])
@pytest.mark.parametrize("R,K", [(1, 1), (3, 1), (5, 9), (130, 8)])  # the R and K of SHAPES
def test_sun_composite(R, K, with_vis):
    rng = np.random.default_rng(100 + R + K)
    thr = np.float32(0.25)
    for suns in _sun_sets(K, R):
        lin_sky = (rng.uniform(0.0, 1.5, (R, 3)) ** 3).astype(np.float32)
        lin_sky[0, 0] = 0.0
        t = rng.uniform(0.0, 1.0, (K, R, 3)).astype(np.float32)
        vis = rng.uniform(0.0, 1.0, (K, R)).astype(np.float32) if with_vis else None
        acc = rng.uniform(0.0, 1.0, R).astype(np.float32)
        acc[0] = thr  # equal to the threshold: masked
        if R > 2:
            acc[1], acc[2] = 0.0, 1.0
        colours = rng.uniform(0.0, 3.0, (K, 3)).astype(np.float32)
        dv = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)  # noqa: E731
        rgb, lin, shadow = (torch.full(s, float("nan"), device=DEV) for s in ((K, R, 3), (K, R, 3), (K, R)))
        hip.sun_composite(dv(lin_sky), dv(t), dv(vis), dv(acc), dv(np.array([thr])), dv(suns), dv(colours), rgb, lin, shadow)
        rgb_only = torch.full((K, R, 3), float("nan"), device=DEV)
        hip.sun_composite(dv(lin_sky), dv(t), dv(vis), dv(acc), dv(np.array([thr])), dv(suns), dv(colours), rgb_only)
        assert torch.equal(rgb, rgb_only)
        rgb, lin, shadow = rgb.cpu().numpy(), lin.cpu().numpy(), shadow.cpu().numpy()
        ref_rgb, ref_lin, ref_v = SC.composite(lin_sky, t, vis, acc, thr, suns, colours)
        off = ref_v == 0.0
        assert np.all(off[suns[:, 2] <= 0.0]) and np.all(off[:, acc <= thr]) and off[:, 0].all()
        assert np.array_equal(shadow, ref_v.astype(np.float32))  # V is vis itself, or exactly 0
        assert np.array_equal(lin[off], np.broadcast_to(lin_sky, lin.shape)[off])  # no light: the sky's value, bit for bit
        ref32 = ref_lin.astype(np.float32)
        assert np.all(np.abs(lin.astype(np.float64) - ref32) <= 2.0 * np.spacing(np.abs(ref32)).astype(np.float64))
        np.testing.assert_allclose(rgb, ref_rgb, rtol=1e-4, atol=1e-6)  # the srgb_fwd bar of test_gpu_render.py
        assert rgb.min() >= 0.0 and rgb.max() <= 1.0


@pytest.mark.parametrize("sky", [(4, 5, 3), (5, 4), (1, 5, 3), (15,)], ids=("K+1 skies", "R x 4", "one of K skies", "flat"))
def test_sun_composite_rejects_a_sky_of_another_shape(sky):
    """lin_sky is [R, 3] or [K, R, 3] (here K = 3, R = 5): [K + 1, R, 3], [R, 4] and their like never reach the kernel"""
    K, R = 3, 5
    z = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
    rgb = torch.full((K, R, 3), 7.0, device=DEV)
    with pytest.raises(AssertionError):
        hip.sun_composite(z(*sky), z(K, R, 3), None, z(R), z(1), z(K, 3), z(K, 3), rgb)
    assert (rgb == 7.0).all()
    for good in ((R, 3), (K, R, 3)):
        hip.sun_composite(z(*good), z(K, R, 3), None, z(R), z(1), z(K, 3), z(K, 3), rgb)
