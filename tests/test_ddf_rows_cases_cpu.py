"""What the GPU tests of the DDF query rows (test_gpu_ddf_rows.py) rest on, proved on the CPU from ddf_rows_cases.py: the case lists
hold every value the kernels' paths depend on; no parity row is near a pole of the local frame; no multi-view ray is short enough
for 1 / len to amplify float32 noise; every sky ray meets the sphere; no `norm < radius` decision is close enough to be taken
differently in float32, except the one that is exact; every case is well conditioned (its float32 restatement agrees with its
float64 one, so a parity assertion on it means something); the restatements added here equal the oracle functions they stand
for; and the statistical bounds put on the kernel's own draws hold for the reference's construction alone."""
import os

import numpy as np
import pytest
import torch

import ddf_rows_cases as DC
import inputs as gi
from oracle import neusky_oracle as O

# conditions on the INPUTS, not tolerances on a kernel: a case past them is re-seeded
POLE_MARGIN, FORWARD_LIMIT, GRAD_LIMIT = 1e-3, 1e-4, 1e-3
FIT_KEYS = sorted({(N, Ns, r) for N, Ns, _, r, _ in DC.FIT_CASES} | {(N, 100, r) for N, r, _ in DC.BWD_CASES} | {DC.NODE_FIT})


def _ids(cases):
    return ["-".join(str(v) for v in c) for c in cases]


def test_case_lists_hold_every_axis_value_and_both_launch_edges():
    c = DC.FIT_CASES
    assert len(set(c)) == len(c)
    assert {x[0] for x in c} == {1, 63, 257, 1312} and {x[1] for x in c} >= {0, 1, 100}
    assert {x[2] for x in c} == {True, False} and {x[3] for x in c} == set(DC.RADII) and {x[4] for x in c} == {16, 20}
    E = [DC.fit_launch_rows(N, Ns, mv) for N, Ns, mv, _, _ in c]
    assert any(e < 256 for e in E) and any(e > 256 and e % 256 == 1 for e in E) and max(E) <= 4096
    assert {x[0] for x in DC.BWD_CASES} == {1, 257, 1312} and {x[2] for x in DC.BWD_CASES} == {16, 20}
    assert all({x[1] for x in DC.BWD_CASES if x[0] == N} == set(DC.RADII) for N in (1, 257, 1312))
    assert sorted(sum((list(cols) for _, cols in DC.COLUMN_GROUPS), [])) == list(range(15)) and len(DC.COLUMN_GROUPS) == 9
    assert set(DC.WEIGHT_MODES) == {(z, e) for z in (False, True) for e in (3.0, 1.0, 2.5)}
    assert {(R, Dv) for R, Dv, _ in DC.vis_cases()} == {(1, 1), (5, 51), (37, 7), (16, 256)}
    assert all({r for R, Dv, r in DC.vis_cases() if (R, Dv) == s} == set(DC.RADII) for s in DC.VIS_SHAPES)
    assert max(R * Dv for R, Dv, _ in DC.vis_cases()) <= 4096
    (N, Ns, r), (R, Dv, rv) = DC.NODE_FIT, DC.NODE_VIS  # a slipped section offset of a node lands in another section
    assert r == rv and (R * Dv) % N != 0 and N != Ns and (R, Dv, rv) in DC.vis_cases()
    assert (DC.READOUT != 0).all() and DC.READOUT.unique().numel() == 15


def _off_pole(pos, radius, what):
    """|cross(up, y)| with y = -pos is the length of pos's (x, y) part: the divisor of the frame's x axis"""
    if pos.numel():
        m = pos[:, :2].norm(dim=-1).min().item()
        assert m >= POLE_MARGIN, (what, m)


@pytest.mark.parametrize("case", FIT_KEYS, ids=_ids(FIT_KEYS))
def test_fit_case_inputs_are_fit_to_test_with(case):
    N, Ns, radius = case
    inp, ref, ref32 = DC.fit_case(*case)
    assert all(v.dtype == torch.float32 and not v.requires_grad for v in inp.values())  # (the references leave the cached inputs alone)
    pos, mv = inp["positions"].double(), inp["mv"].double()
    assert ((pos.norm(dim=-1) - radius).abs() <= 4e-7 * radius).all() and (pos[:, 2] >= 0).all()
    assert ((inp["directions"].double().norm(dim=-1) - 1).abs() <= 4e-7).all()
    inner = pos + inp["directions"].double() * inp["t"].double()[:, None]
    assert (inner.norm(dim=-1) <= 0.7 * radius * (1 + 1e-6)).all()
    # the reference's quirk: unit multi-view points whatever the radius; some below the equator, so the fold has work to do
    assert ((mv.norm(dim=-1) - 1).abs() <= 4e-7).all() and (N < 63 or (mv[:, 2] < 0).any())
    assert torch.equal(ref["pos_mv"], DC.fold(inp["mv"]).double())
    assert (inp["sky_o"].double().norm(dim=-1) <= 0.5 * radius * (1 + 1e-6)).all()
    assert ((inp["sky_d"].double().norm(dim=-1) - 1).abs() <= 4e-7).all()
    for s in DC.FIT_SECTIONS:
        _off_pole(ref["pos_" + s], radius, (case, s))
        assert ref["rows_" + s].shape == (Ns if s == "sky" else N, 15) and torch.isfinite(ref["rows_" + s]).all()
    assert ref["mv_len"].min().item() >= DC.MV_MIN_LEN * radius, ref["mv_len"].min().item()
    o, d = inp["sky_o"].double(), inp["sky_d"].double()
    b, c = 2 * (o * d).sum(-1), (o * o).sum(-1) - radius ** 2
    assert (b * b - 4 * c > 0).all()
    # far root: the sky point lies on the sphere (as far as sky_d is a unit vector: float32) AHEAD of the origin; sky_gt is the distance
    assert ((ref["pos_sky"].norm(dim=-1) - radius).abs() <= 1e-6 * radius).all() and (((ref["pos_sky"] - o) * d).sum(-1) > 0).all()
    assert torch.equal(ref["sky_gt"], (o - ref["pos_sky"]).norm(dim=-1))
    # the restatement of the weight is the oracle's, in the one mode the oracle has
    assert torch.equal(DC.distance_weight(inp["positions"], radius, 3.0, False, torch.float64), ref["distance_weight"])
    # the differentiable multi-view row is the captured one
    assert torch.equal(DC.mv_rows_of_t(inp, inp["t"].double(), torch.float64), ref["rows_mv"])
    assert torch.equal(DC.mv_t_gradient(inp, inp["d_xrow"], torch.float64), ref["d_t"])
    worst = {}
    for k in ("pos_fit", "rows_fit", "pos_mv", "rows_mv", "pos_sky", "rows_sky", "sky_gt", "distance_weight"):
        worst[k] = DC.max_err(ref32[k], ref[k])
        assert worst[k] <= FORWARD_LIMIT, (case, k, worst[k])
    scale = ref["d_t"].abs().max().item()
    worst["d_t / max"] = DC.max_err(ref32["d_t"], ref["d_t"]) / scale
    assert scale > 0 and worst["d_t / max"] <= GRAD_LIMIT, (case, worst["d_t / max"])
    for name, cols in DC.COLUMN_GROUPS:  # each column group alone reaches t: a factor wrong on one of them has a gradient to spoil
        probe = DC.group_probe(inp, cols)
        g64, g32 = DC.mv_t_gradient(inp, probe, torch.float64), DC.mv_t_gradient(inp, probe, torch.float32)
        assert g64.abs().max().item() > 0 and DC.max_err(g32, g64) <= GRAD_LIMIT * g64.abs().max().item(), (case, name)
    print(case, f"shortest mv ray {ref['mv_len'].min().item() / radius:.3f} radius;",
          "float32 - float64:", {k: f"{v:.1e}" for k, v in worst.items()})


@pytest.mark.parametrize("include_z,exp", DC.WEIGHT_MODES)
def test_distance_weight_modes_differ(include_z, exp):
    """on the sphere the weight with z is 0 to rounding and the one without is not: ignoring include_z cannot pass"""
    for radius in DC.RADII:
        inp = DC.fit_inputs(257, 100, radius)
        w = DC.distance_weight(inp["positions"], radius, exp, include_z, torch.float64)
        other = DC.distance_weight(inp["positions"], radius, exp, not include_z, torch.float64)
        assert (w - other).abs().max().item() > 0.5 and torch.isfinite(w).all()
        assert (w.abs().max().item() < 1e-5) == include_z


@pytest.mark.parametrize("case", DC.vis_cases(), ids=_ids(DC.vis_cases()))
def test_visibility_case_inputs_are_fit_to_test_with(case):
    R, Dv, radius = case
    inp, ref, ref32, fin = DC.vis_case(*case)
    sel, D = inp["sel_index"], inp["dirs"].shape[0]
    assert sel.numel() == Dv and Dv < D and (sel[1:] > sel[:-1]).all()  # a strict subset, ascending
    lengths = inp["dirs"].norm(dim=-1)
    assert (lengths - 1).abs().max().item() > 0.05 and lengths.min().item() >= 0.5  # non-unit: the kernel has to normalise
    # the boundary ray is ON the sphere in both precisions; every other decision is clear of it
    for dt in (torch.float32, torch.float64):
        end = inp["origins"][0].to(dt) + inp["ray_dirs"][0].to(dt) * inp["depth"][0].to(dt)
        assert end.norm().item() == radius
    margin = (ref["end_norm"][1:] - radius).abs()
    assert R == 1 or margin.min().item() >= DC.BOUNDARY_MARGIN
    outside = int((ref["end_norm"][1:] > radius).sum())
    assert outside == inp["n_outside"] and (R == 1 or (outside >= 1 and outside < R - 1))
    assert torch.equal(ref32["end_norm"] < radius, ref["end_norm"] < radius)
    _off_pole(ref["sphere_points"], radius, case)
    assert ((ref["sphere_points"].norm(dim=-1) - radius).abs() <= 1e-12 * radius).all()
    assert (ref["surf_dist"] <= 2 * radius).all() and torch.isfinite(ref["rows"]).all()
    worst = {k: DC.max_err(ref32[k], ref[k]) for k in ("sphere_points", "termination_dist", "surf_dist", "rows")}
    assert all(v <= FORWARD_LIMIT for v in worst.values()), (case, worst)
    # the finish formulation IS the oracle's visibility on the selected directions, and 1 (the lower value) elsewhere
    f = DC.finish_reference(ref["t_hat"], ref["surf_dist"], inp, torch.float64)
    assert torch.allclose(f["vis"], ref["visibility"][:, sel], rtol=0, atol=1e-14)
    rest = torch.ones(D, dtype=torch.bool)
    rest[sel] = False
    assert (ref["visibility"][:, rest] == 1).all()
    r64, r32 = fin["ref"], fin["ref32"]
    assert not fin["t_hat"].requires_grad and not fin["surf_dist"].requires_grad
    worst["vis"] = DC.max_err(r32["vis"], r64["vis"])
    assert worst["vis"] <= FORWARD_LIMIT
    scale = r64["d_t_hat"].abs().max().item()
    worst["d_t_hat / max"] = DC.max_err(r32["d_t_hat"], r64["d_t_hat"]) / scale
    assert scale > 0 and worst["d_t_hat / max"] <= GRAD_LIMIT
    # the sigmoid is not saturated everywhere: the backward has something to get wrong, and the threshold's gradient is a real sum
    assert (r64["vis"] > 1e-3).any() and (r64["vis"] < 1 - 1e-3).any()
    assert abs(r64["d_threshold"].item()) > 0 and DC.threshold_bar(r64["d_threshold_terms"]) < 1e-3 * r64["d_threshold_terms"].abs().sum().item()
    print(case, f"scale {inp['scale']:.2f};", "float32 - float64:", {k: f"{v:.1e}" for k, v in worst.items()})


def test_g6_inputs_are_the_golden_generator_s():
    g = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "g6_ddf.npz")))
    inp = gi.sphere_rays(seed=6, M=40, radius=1.0)
    out64, out32 = DC.g6_oracle(g, inp, torch.float64), DC.g6_oracle(g, inp, torch.float32)
    for k in DC.G6_OUTPUTS:  # test_g6_ddf_model_plumbing's own assertion, through this module's statement of it
        np.testing.assert_allclose(out32[k].numpy(), g["out_" + k], rtol=DC.G6_RTOL, atol=DC.G6_ATOL)
        print(k, f"float32 - float64 oracle distance {DC.max_err(out32[k], out64[k]):.2e}")
        assert DC.max_err(out32[k], out64[k]) <= 1e-3  # (two of G6's 40 positions sit 2e-3 off a pole on purpose)


def test_reference_construction_meets_the_statistical_bounds():
    """the bounds test_gpu_ddf_rows puts on the kernel's draws, on float64 draws of the oracle's construction alone"""
    pts = DC.oracle_hemisphere_draws(DC.DRAW_CALLS, DC.DRAW_N, seed=2024)
    assert pts.shape == (64, 4096, 3) and ((pts.norm(dim=-1) - 1).abs() <= 1e-12).all() and (pts[..., 2] >= 0).all()
    stats = DC.hemisphere_statistics(pts)
    assert len(stats) == 7
    for name, value, expected, bound in stats:
        print(f"{name}: {value:.6g}, expected {expected:.6g} +- {bound:.3g}")
        assert abs(value - expected) <= bound, (name, value, expected, bound)
    # the bounds bite: z that is not uniform (cos(phi) = u instead of 2 u - 1 without the fold is uniform too, but a square root
    # law is not), and a repeated call
    skew = pts.clone()
    skew[..., 2] = skew[..., 2] ** 0.9
    assert any(abs(v - e) > b for _, v, e, b in DC.hemisphere_statistics(skew)[:2])
    again = pts.clone()
    again[1::2] = again[0::2]
    assert abs(DC.hemisphere_statistics(again)[5][1]) > DC.hemisphere_statistics(again)[5][3]


def test_philox_restatement_gives_the_published_vectors():
    """the known-answer vectors of Philox4x32-10 distributed with Random123 (kat_vectors): zeros, ones and the digits of pi"""
    h = lambda *w: np.array(w, dtype=np.uint32)  # noqa: E731
    for ctr, key, out in ((h(0, 0, 0, 0), h(0, 0), h(0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
                          (h(*[0xffffffff] * 4), h(*[0xffffffff] * 2), h(0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
                          (h(0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), h(0xa4093822, 0x299f31d0),
                           h(0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))):
        assert (DC.philox4x32_10(ctr[None], key)[0] == out).all()
    p64, p32 = DC.philox_mv_points(1234, 63, DC.DRAW_N, torch.float64), DC.philox_mv_points(1234, 63, DC.DRAW_N, torch.float32)
    assert p32.dtype == torch.float32 and ((p64.norm(dim=-1) - 1).abs() <= 1e-12).all() and (p64[:, 2] > 0).all() and (p64[:, 2] < 1).all()
    assert torch.equal(p32[:, 2].double(), p64[:, 2])  # z = |2 u - 1| is exact in float32
    assert DC.max_err(p32, p64) <= 1e-5
    assert not torch.equal(p64, DC.philox_mv_points(1234, 62, DC.DRAW_N, torch.float64))
