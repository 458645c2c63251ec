"""nsky_atmosphere_apply and nsky_atmosphere_rows (csrc/atmosphere.hip) against the float64 restatement, atmosphere_cpu.py, on hand-made
rows: every ray count about a workgroup's edge, one base and three (a shared and a per-base background, one sun of the three set), no
shafts, one and five with random visibilities, a homogeneous medium and a height fog, rays that look level, barely up or down, and
straight up or down, surfaces at the camera, inside the medium, at `far` and beyond it, every accumulation, no density, a grey and a
coloured one, both phase functions, with and without the lamps' image, and a frame of K suns as it lies in memory, ray-major.

The bar.  The rule's own float32 noise: the restatement run in float32 numpy on these same inputs deviates from float64 by at most
F32_RESTATEMENT_WORST of the pixel's scale max(|lin|, |B|, J); four times that, BAR_F32, would be the bar of a float32 kernel (the
margin covers the device's expf / expm1f against numpy's and fused multiply-adds).  The kernel does better: it forms everything in
float64 from the float32 inputs and rounds each output once.  Its error is then half an ulp of the output, at most 2^-24 |out|, plus
float64 noise some 1e-9 of that; and |out| <= 2 scale (T (lin - (1 - A) B) is at most one scale for the non-negative images here, and
A S + (1 - A) X at most another, S and X being means of J and B).  KERNEL_BAR = 4 * 2^-24 is twice that bound, 90 times tighter than
BAR_F32, and the one the tests hold the kernel to.  Neither number is taken from the kernel's output; the unmarked test below measures
the first again wherever the suite runs.  atmosphere_transmittance has no pixel scale: it is compared on the scale 1."""
import itertools

import numpy as np
import pytest
import torch

import atmosphere_cpu as AC
import sun_cpu as SC

gpu = pytest.mark.gpu
DEV = "cuda:0"
F32_RESTATEMENT_WORST = 5.5e-6  # measured on the development machine's CPU over every case below (test_the_float32_restatement_sets_the_bar)
BAR_F32 = 4.0 * F32_RESTATEMENT_WORST
KERNEL_BAR = 4.0 * 2.0 ** -24  # 2.4e-7: float64 with one rounding (above)
FAR = 2.0
RS, KBS = (1, 63, 64, 65, 257), (1, 3)
# M, H, density, whether the Kb bases share one background: 36 media per size.  g, the lamps' image and the ray-major layout walk through
# their eight combinations along the media, from a start that differs from size to size, so that at every size each of them meets each
# background layout and each other under a density (the test asserts it), and no option stays tied to one M, H or density across the
# sizes; the background flag and a sky frame without suns are drawn per case
MEDIA = list(itertools.product((0, 1, 5), (None, 0.3), (0.0, 1.5, (0.5, 1.0, 2.0)), (False, True)))


def _case(R, Kb, i):
    """the i-th of the media at this size: inputs in float32 (as the device holds them), as float64 arrays; `ray_major`: the layout"""
    M, H, density, shared = MEDIA[i]
    g = np.random.default_rng(1000 * R + 100 * Kb + i)
    turn = (i // 2 + 3 * RS.index(R) + 5 * (Kb - 1) // 2) % 8
    forward, lamps, ray_major = bool(turn & 1), bool(turn & 2), bool(turn & 4)
    no_suns, fog_background = bool(g.integers(0, 2)), bool(g.integers(0, 4))  # one case in four leaves the background clear
    f32 = lambda x: np.asarray(x, np.float64).astype(np.float32)  # noqa: E731
    dz = g.choice([0.0, 1e-7, -1e-7, 0.5, -0.5, 1.0, -1.0], R)
    az = g.uniform(0.0, 2.0 * np.pi, R)
    h = np.sqrt(np.maximum(1.0 - dz * dz, 0.0))
    suns = Kb > 1 or M > 0 or not no_suns  # (a sky frame, Kb = 1 without suns, has no shafts)
    s = g.normal(size=(Kb, 3))
    s[:, 2] = np.abs(s[:, 2]) + 0.2
    if Kb == 3:
        s[1, 2] = -s[1, 2]  # one sun has set
    s /= np.linalg.norm(s, axis=1, keepdims=True)
    c = dict(origins=f32(g.uniform(-0.5, 0.5, (R, 3))), directions=f32(np.stack([h * np.cos(az), h * np.sin(az), dz], 1)),
             depth=f32(g.choice([0.0, 0.4, FAR, 2.0 * FAR], R)), accumulation=f32(g.choice([0.0, 0.5, 1.0], R)),
             lin=f32(g.uniform(0.0, 2.0, (Kb, R, 3))), background=f32(g.uniform(0.0, 1.0, (R, 3) if shared else (Kb, R, 3))),
             abar=f32(g.uniform(0.1, 0.6, (Kb, 3))), sun_dirs=f32(s) if suns else None, sun_colours=f32(g.uniform(0.5, 2.0, (Kb, 3))) if suns else None,
             vis=f32(g.uniform(0.0, 1.0, (M, Kb, R))) if M > 0 else None,
             params=AC.block(density, H, base_height=0.1, albedo=(0.9, 0.8, 1.0), anisotropy=0.8 if forward else 0.0, far=FAR, background=fog_background),
             M=M, light_lin=f32(g.uniform(0.0, 1.0, (R, 3))) if lamps else None)
    return {k: (v.astype(np.float64) if isinstance(v, np.ndarray) else v) for k, v in c.items()}, ray_major


SHAFTS_5 = MEDIA.index((5, 0.3, (0.5, 1.0, 2.0), True))  # five shaft samples in a coloured height fog, one background under all bases


def _relative(got, ref, scale):
    return float((np.abs(np.asarray(got, np.float64) - ref) / scale).max())


def test_the_float32_restatement_sets_the_bar():
    """steps 1 to 3 of the bar's derivation, on the CPU: no kernel runs here"""
    worst = 0.0
    for R, Kb in itertools.product(RS, KBS):
        for i in range(len(MEDIA)):
            c, _ = _case(R, Kb, i)
            ref, f32 = AC.apply(**c), AC.apply(**c, dtype=np.float32)
            for k in ("lin", "inscatter"):
                worst = max(worst, _relative(f32[k], ref[k], ref["scale"]))
            worst = max(worst, _relative(f32["transmittance"], ref["transmittance"], 1.0))
    print(f"float32 restatement against float64: worst {worst:.3e} of the pixel's scale (recorded {F32_RESTATEMENT_WORST:.1e}); "
          f"BAR_F32 {BAR_F32:.2e}, KERNEL_BAR {KERNEL_BAR:.2e}")
    assert F32_RESTATEMENT_WORST / 2.0 <= worst <= F32_RESTATEMENT_WORST * 2.0  # (numpy's expf may differ from one machine to the next)
    assert KERNEL_BAR < BAR_F32


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(DEV)


def _run(c, ray_major):
    from neusky_amd import hip
    Kb, R = c["lin"].shape[0], c["lin"].shape[1]
    if ray_major:  # [R, Kb, 3] in memory, Kb leading in the shape alone: a frame of K suns
        lin_in = _dev(c["lin"].transpose(1, 0, 2)).permute(1, 0, 2)
        lin, rgb, ins = (torch.full((R, Kb, 3), float("nan"), device=DEV).permute(1, 0, 2) for _ in range(3))
    else:
        lin_in = _dev(c["lin"])
        lin, rgb, ins = (torch.full((Kb, R, 3), float("nan"), device=DEV) for _ in range(3))
    vis = _dev(c["vis"])
    if vis is not None and ray_major:  # [M, R, Kb] in memory: what the DDF's rows give
        vis = _dev(c["vis"].transpose(0, 2, 1)).permute(0, 2, 1)
    T, light_lin = torch.full((R, 3), float("nan"), device=DEV), _dev(c["light_lin"])
    hip.atmosphere_apply(_dev(c["origins"]), _dev(c["directions"]), _dev(c["depth"]), _dev(c["accumulation"]), lin_in, _dev(c["background"]),
                         _dev(c["abar"]), _dev(c["sun_dirs"]), _dev(c["sun_colours"]), vis, _dev(c["params"]), c["M"], lin, rgb, ins, T, light_lin)
    f64 = lambda t: None if t is None else t.cpu().double().numpy()  # noqa: E731
    return {"lin": f64(lin), "rgb": f64(rgb), "inscatter": f64(ins), "transmittance": f64(T), "light_lin": f64(light_lin)}


@gpu
@pytest.mark.parametrize("Kb", KBS)
@pytest.mark.parametrize("R", RS)
def test_apply_is_the_restatement(R, Kb):
    worst = {"lin": 0.0, "inscatter": 0.0, "transmittance": 0.0, "light_lin": 0.0}
    seen = set()  # (a density, a shared background, g = 0.8, the lamps' image, ray-major)
    for i in range(len(MEDIA)):
        c, ray_major = _case(R, Kb, i)
        ref, got = AC.apply(**c), _run(c, ray_major)
        assert all(np.isfinite(v).all() for v in got.values() if v is not None), (R, Kb, i)
        worst["lin"] = max(worst["lin"], _relative(got["lin"], ref["lin"], ref["scale"]))
        worst["inscatter"] = max(worst["inscatter"], _relative(got["inscatter"], ref["inscatter"], ref["scale"]))
        worst["transmittance"] = max(worst["transmittance"], _relative(got["transmittance"], ref["transmittance"], 1.0))
        if c["light_lin"] is not None:
            worst["light_lin"] = max(worst["light_lin"], _relative(got["light_lin"], ref["light_lin"], 1.0))
        else:
            assert got["light_lin"] is None
        np.testing.assert_allclose(got["rgb"], SC.linear_to_srgb(got["lin"]), rtol=1e-4, atol=1e-6)
        seen.add((MEDIA[i][2] != 0.0, c["background"].ndim == 2, bool(c["params"][8]), c["light_lin"] is not None, ray_major))
        if MEDIA[i][2] == 0.0:  # no density: the frame's own bits
            assert np.array_equal(got["lin"], c["lin"])
            assert (got["transmittance"] == 1.0).all() and (got["inscatter"] == 0.0).all()
    print(f"R {R} Kb {Kb}: worst deviation from float64, of the pixel's scale: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items())
          + f" (bar {KERNEL_BAR:.2e})")
    assert max(worst.values()) <= KERNEL_BAR, worst
    # with a density, every pairing of the drawn options was run at this size
    assert {t[1:] for t in seen if t[0]} == set(itertools.product((False, True), repeat=4)), sorted(seen)


@gpu
def test_segments_without_visibilities_are_unshadowed():
    """M > 0 and no visibilities (a model without a visibility network under "ddf"): V = 1 in every segment"""
    c = {**_case(65, 3, SHAFTS_5)[0], "vis": None}
    ref, got = AC.apply(**c), _run(c, ray_major=False)
    assert c["M"] == 5 and max(_relative(got[k], ref[k], ref["scale"]) for k in ("lin", "inscatter")) <= KERNEL_BAR


@gpu
@pytest.mark.parametrize("Kb", (8, 9, 17))
def test_more_bases_than_a_thread_keeps_in_registers(Kb):
    """the kernel walks the segments once per 8 bases: a full pass, one base into the second, one into the third"""
    for shared in (False, True):
        c, ray_major = _case(65, Kb, MEDIA.index((5, 0.3, (0.5, 1.0, 2.0), shared)))
        ref, got = AC.apply(**c), _run(c, ray_major)
        worst = max(_relative(got[k], ref[k], ref["scale"]) for k in ("lin", "inscatter"))
        print(f"Kb {Kb}, shared background {shared}: worst deviation {worst:.2e} (bar {KERNEL_BAR:.2e})")
        assert worst <= KERNEL_BAR


@gpu
def test_two_runs_agree_to_the_bit():
    c = _case(257, 3, SHAFTS_5)[0]
    a, b = _run(c, True), _run(c, True)
    assert all(np.array_equal(a[k], b[k]) for k in ("lin", "rgb", "inscatter", "transmittance"))


@gpu
@pytest.mark.parametrize("R,M", ((1, 1), (65, 5), (257, 64)))
def test_rows_are_the_rays_at_the_midpoints(R, M):
    from neusky_amd import hip
    g = np.random.default_rng(R + M)
    far = np.float32(1.7)
    o, d = g.uniform(-0.5, 0.5, (R, 3)).astype(np.float32), g.normal(size=(R, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    params = AC.block(1.5, 0.3, far=far)
    ro, rd, rt = (torch.full(s, float("nan"), device=DEV) for s in ((M * R, 3), (M * R, 3), (M * R,)))
    hip.atmosphere_rows(_dev(o), _dev(d), _dev(params), M, ro, rd, rt)
    ro, rd, rt = ro.cpu().numpy(), rd.cpu().numpy(), rt.cpu().numpy()
    assert np.array_equal(ro, np.tile(o, (M, 1))) and np.array_equal(rd, np.tile(d, (M, 1)))  # row m R + r is ray r
    mid = AC.midpoints(far, M)  # float64
    assert np.array_equal(rt.reshape(M, R), np.broadcast_to(mid.astype(np.float32)[:, None], (M, R)))  # the float32 rounding, exactly
    # the point a shadow query then starts at is the float64 midpoint to half an ulp of the depth's rounding
    x = ro.astype(np.float64) + rt.astype(np.float64)[:, None] * rd.astype(np.float64)
    want = np.tile(o, (M, 1)).astype(np.float64) + np.repeat(mid, R)[:, None] * np.tile(d, (M, 1)).astype(np.float64)
    ulp = np.spacing(np.repeat(mid, R).astype(np.float32)).astype(np.float64)[:, None]
    # (a midpoint may be an exact tie of two float32 values; the float64 sums here then add their own last bits)
    assert (np.abs(x - want) <= 0.5 * ulp * np.abs(np.tile(d, (M, 1))) + 4.0 * np.spacing(np.abs(want))).all()


@gpu
def test_what_the_binding_refuses():
    from neusky_amd import hip
    c = _case(64, 3, SHAFTS_5)[0]
    with pytest.raises((AssertionError, ValueError)):
        _run({**c, "vis": c["vis"][:, :2]}, False)  # visibilities of two of three suns
    with pytest.raises((AssertionError, ValueError)):
        _run({**c, "sun_colours": None}, False)
    with pytest.raises((AssertionError, ValueError)):
        _run({**c, "M": 65}, False)
    with pytest.raises(hip.NeuSkyHipError):  # host tensors: there is no CPU path
        hip.atmosphere_rows(torch.zeros(4, 3), torch.zeros(4, 3), _dev(c["params"]), 1, torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(4))
