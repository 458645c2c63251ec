"""nsky_daylight_eval (csrc/daylight.hip) against the float64 restatement of the model (daylight_cpu.py) on the same fp32 inputs, at
the lane and tail sizes, with the directions and suns where the definition branches; repeatability; parameters read from device memory;
and nsky_sun_composite on a sky [R, 3] against its [K, R, 3] expansion."""
import numpy as np
import pytest
import torch

import daylight_cpu as DC
from neusky_amd import hip
from neusky_amd.relight import DaylightSky, SunLight

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LIN_BAR = 1e-5  # the project's bar on a linear image (test_gpu_relight_frame.py, test_gpu_sun_frame.py), here per sun of its brightest entry
# A second bar, so that the dim parts of a sky (below the horizon after `ground`, far from a low sun) are not checked against the aureole
# alone: an entry against the brightest CHANNEL OF ITS OWN DIRECTION.  A channel is a sum of X, Y, Z terms of at most 3.3 times the
# luminance, each out of about ten fp32 roundings (6e-8 apiece): some 3e-6 of the luminance.  1e-4 leaves that a factor of 30 and is still
# 1e3 times finer than a wrong ground channel or gradient factor.  (Relative to the entry itself it could not hold: a channel may cancel to 0.)
OWN_BAR = 1e-4
GROUND = (0.3, 0.2, 0.1)
EXPOSURE = 0.7


def suns_f32(K):
    """[K, 3] fp32.  K = 1: a sun at 2 degrees; K >= 3: also one at 90 degrees and one that has set; K = 9: one exactly on the horizon"""
    el = [2.0, 90.0, -5.0, 33.0, 10.0, 61.0, 0.0, 5.0, 80.0]
    suns = [DC.sun_direction(37.0 * i, el[i] if i < len(el) else 1.0 + 88.0 * (i % 97) / 97.0) for i in range(K)]
    return np.asarray(suns, np.float64).astype(np.float32)


def directions_f32(N, suns, seed):
    """[N, 3] fp32: the special directions first (as many as fit), random ones of random length after"""
    s = suns[0].astype(np.float64)
    special = [(0.0, 0.0, 1.0), tuple(s), tuple(-s), (0.6, -0.8, 0.0), (0.6, 0.8, 1e-6), (0.3, 0.4, -0.5), (0.0, 0.0, -1.0), (30.0, -40.0, 12.0),
               (0.0, 0.0, 3.0), tuple(suns[min(1, len(suns) - 1)].astype(np.float64)), (1.0, 0.0, 1e-3), (-2e-3, 1e-3, -1e-7), (0.0, 0.0, 0.0)]
    g = np.random.default_rng(seed)
    rand = g.normal(size=(N, 3)) * np.exp(g.uniform(-3.0, 3.0, size=(N, 1)))
    d = np.concatenate([np.asarray(special, np.float64), rand])
    if N < len(special):  # a short case takes the specials in turn, by its seed
        d = np.roll(d[:len(special)], -seed % len(special), axis=0)
    return d[:N].astype(np.float32)


def device_eval(d, s, T, exposure=EXPOSURE, ground=GROUND):
    out = torch.empty(s.shape[0], d.shape[0], 3, device=DEV)
    params = [torch.tensor(v, dtype=torch.float32, device=DEV) for v in ([T], [exposure], list(ground))]
    hip.daylight_eval(torch.from_numpy(d).to(DEV), torch.from_numpy(s).to(DEV), *params, out)
    return out, params


@pytest.mark.parametrize("T", [2.0, 10.0])
@pytest.mark.parametrize("K", [1, 3, 9])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_kernel_matches_the_definition(N, K, T):
    s = suns_f32(K)
    d = directions_f32(N, s, seed=N + K)
    got, _ = device_eval(d, s, T)
    again, _ = device_eval(d, s, T)
    assert torch.equal(got, again)  # two calls are bitwise equal
    got = got.cpu().double().numpy()
    ref = DC.radiance(np.float64(np.float32(T)), s.astype(np.float64), d.astype(np.float64), exposure=np.float64(np.float32(EXPOSURE)),
                      ground=np.asarray(GROUND, np.float32).astype(np.float64))
    assert got.shape == ref.shape == (K, N, 3) and np.isfinite(got).all() and (got >= 0.0).all()
    worst = own = 0.0
    for k in range(K):
        if not s[k, 2] > 0.0:
            assert (got[k] == 0.0).all() and (ref[k] == 0.0).all(), k
            continue
        worst = max(worst, np.abs(got[k] - ref[k]).max() / ref[k].max())
        top = ref[k].max(axis=1, keepdims=True)
        lit = top[:, 0] > 0.0
        assert (got[k][~lit] == 0.0).all()
        if lit.any():
            own = max(own, (np.abs(got[k] - ref[k])[lit] / top[lit]).max())
    print(f"N {N} K {K} T {T}: worst |gpu - f64| / brightest entry of the sun's sky = {worst:.3e} (bar {LIN_BAR:.0e}); "
          f"/ brightest channel of the entry's own direction = {own:.3e} (bar {OWN_BAR:.0e})")
    assert worst <= LIN_BAR and own <= OWN_BAR


def test_more_suns_than_one_launch_holds():
    """the table of a launch holds 256 suns: 257 take two"""
    s = suns_f32(257)
    d = directions_f32(65, s, seed=4)
    got, _ = device_eval(d, s, 3.0)
    ref = DC.radiance(3.0, s.astype(np.float64), d.astype(np.float64), exposure=np.float64(np.float32(EXPOSURE)),
                      ground=np.asarray(GROUND, np.float32).astype(np.float64))
    top = np.maximum(ref.reshape(257, -1).max(axis=1), 1e-300)
    worst = (np.abs(got.cpu().double().numpy() - ref).reshape(257, -1).max(axis=1) / top).max()
    print(f"257 suns: worst ratio {worst:.3e}")
    assert worst <= LIN_BAR
    assert torch.equal(got[256], device_eval(d, s[256:], 3.0)[0][0])


def test_parameters_are_read_from_device_memory():
    s = suns_f32(3)
    d = directions_f32(65, s, seed=2)
    out, (turbidity, exposure, ground) = device_eval(d, s, 3.0)
    first = out.clone()
    dd, ss = torch.from_numpy(d).to(DEV), torch.from_numpy(s).to(DEV)
    turbidity.fill_(7.0)
    exposure.fill_(0.25)
    hip.daylight_eval(dd, ss, turbidity, exposure, ground, out)
    assert not torch.equal(out, first)
    assert torch.equal(out, device_eval(d, s, 7.0, exposure=0.25)[0])
    ss[0].copy_(ss[1])  # and so are the suns
    hip.daylight_eval(dd, ss, turbidity, exposure, ground, out)
    assert torch.equal(out[0], out[1])


def test_daylight_sky_radiance():
    sky = DaylightSky(turbidity=4.0, exposure=0.5, ground=GROUND)
    suns = [SunLight(20.0, 30.0), SunLight(200.0, -3.0)]
    d = directions_f32(65, suns_f32(1), seed=9)
    got = sky.radiance(torch.from_numpy(d).to(DEV), suns)
    s32 = np.asarray([s.direction for s in suns], np.float64).astype(np.float32)
    assert got.shape == (2, 65, 3) and torch.equal(got, device_eval(d, s32, 4.0, exposure=0.5)[0])
    assert torch.equal(sky.radiance(torch.from_numpy(d).to(DEV), torch.from_numpy(s32)), got)
    assert got[0].max().item() > 0.0 and got[1].abs().max().item() == 0.0


@pytest.mark.parametrize("with_vis", [True, False])
def test_composite_with_copies_of_one_sky_is_the_composite_on_that_sky(with_vis):
    K, R = 9, 257
    g = torch.Generator().manual_seed(21)
    lin_sky = (torch.rand(R, 3, generator=g) * 2.0).to(DEV)
    t = torch.rand(K, R, 3, generator=g).to(DEV)
    vis = torch.rand(K, R, generator=g).to(DEV) if with_vis else None
    acc = torch.rand(R, generator=g).to(DEV)
    thr = torch.tensor([0.2], device=DEV)
    suns = torch.from_numpy(suns_f32(K)).to(DEV)
    colours = (torch.rand(K, 3, generator=g) * 3.0).to(DEV)
    one = [torch.empty(K, R, 3, device=DEV), torch.empty(K, R, 3, device=DEV), torch.empty(K, R, device=DEV)]
    many = [torch.empty_like(x) for x in one]
    hip.sun_composite(lin_sky, t, vis, acc, thr, suns, colours, *one)
    hip.sun_composite(lin_sky[None].expand(K, R, 3).contiguous(), t, vis, acc, thr, suns, colours, *many)
    for a, b in zip(one, many):
        assert torch.equal(a, b)
    skies = (torch.rand(K, R, 3, generator=g) * 2.0).to(DEV)  # and each sun meets its own sky
    hip.sun_composite(skies, t, vis, acc, thr, suns, colours, *many)
    for k in range(K):
        hip.sun_composite(skies[k].contiguous(), t, vis, acc, thr, suns, colours, *one)
        assert torch.equal(one[1][k], many[1][k]) and torch.equal(one[0][k], many[0][k])
