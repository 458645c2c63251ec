"""What the GPU edge tests of the render kernels (test_gpu_render_edges.py) rest on, proved on the CPU from render_cases.py: the
case matrix covers every axis value under every anneal; every case is well conditioned (its float32 restatement agrees with its
float64 one, so a parity assertion on it means something); the coarse family really saturates; the kink case really sits on the
kinks; and no discontinuity of a reference (a count of positive dots, an sRGB segment, an active interlevel interval) is close
enough to be decided differently in float32."""
import pytest
import torch

import render_cases as RC

GRAD_LIMIT, FORWARD_LIMIT = 1e-3, 1e-5  # conditions on the INPUTS, not tolerances on a kernel: a case past them is re-seeded


def _ids(cases):
    return ["-".join(str(v) for v in c) for c in cases]


def test_matrix_covers_every_axis_under_every_anneal():
    cases = RC.neus_cases()
    assert len(set(cases)) == len(cases)
    for an in RC.ANNEALS:
        mine = [c for c in cases if c[2] == an]
        assert {c[1] for c in mine} == set(RC.VARIANCES)
        assert {c[4] for c in mine} == set(RC.NEUS_S)
        assert {1, 9} <= {c[3] for c in mine}
        assert {c[1] for c in mine if c[0] == "coarse"} == {0.6, 0.9}
        pts = [c for c in RC.point_cases() if c[1] == an]
        assert {c[0] for c in pts} == set(RC.VARIANCES) and {c[2] for c in pts} == set(RC.POINT_P)
    for family in ("resolved", "coarse"):
        S = {c[4] for c in cases if c[0] == family}
        assert 256 in S and any(129 <= s <= 192 for s in S)  # CH = 3 and the limit, in both families
    assert max(c[3] for c in cases) == 37 and max(c[4] for c in cases) == 256
    assert RC.inv_s_of(1.5) == 1e6 and RC.inv_s_of(1.2) < 1e6  # 1.5 is past the kernel's clamp, 1.2 is not


def _assert_conditioned(err, what):
    print(what, {k: f"{v:.2e}" for k, v in err.items()})
    for k, v in err.items():
        limit = GRAD_LIMIT if k.startswith("d_") else FORWARD_LIMIT
        assert v <= limit, (what, k, v)


@pytest.mark.parametrize("case", RC.neus_cases(), ids=_ids(RC.neus_cases()))
def test_neus_case_is_well_conditioned(case):
    inp, ref, err = RC.neus_case(*case)
    R, S = case[3], case[4]
    assert inp["sdf"].shape == (R, S) and inp["sdf"].dtype == torch.float32
    assert all(torch.isfinite(v).all() for v in ref.values())
    assert (inp["ends"] > inp["starts"]).all()  # no interval collapses in float32, however sharp the case
    assert ((inp["dirs"].norm(dim=-1) - 1).abs() < 1e-6).all() and ((inp["grad"].norm(dim=-1) - 1).abs() < 0.1 + 1e-6).all()
    cos = (inp["grad"] * inp["dirs"][:, None, :]).sum(-1)
    assert (cos < 0).any() and (R * S < 63 or (cos > 0).any())  # both sides of relu(-cos)
    if case[1] == 1.5:
        assert ref["d_variance"].item() == 0.0  # the clamp of inv_s passes no gradient
    else:
        assert ref["d_variance"].abs().item() > 0
    if case[0] == "resolved":
        # from 63 samples on the crossing is resolved: no sample saturates, and every ray is opaque behind it
        assert S < 63 or (ref["alpha"].max() < 0.999 and ref["accumulation"].min() > 0.9)
    _assert_conditioned(err, case)
    ref0, err0 = RC.neus_case_without_gT(*case)  # the GPU test's run with a null d_trans_bg
    assert (ref0["d_variance"].item() == 0.0) == (case[1] == 1.5)
    _assert_conditioned(err0, ("gT = 0",) + case)


_COARSE = [case for case in RC.neus_cases() if case[0] == "coarse"]


@pytest.mark.parametrize("case", _COARSE, ids=_ids(_COARSE))
def test_coarse_case_saturates(case):
    _, ref, _ = RC.neus_case(*case)
    share = (ref["alpha"] >= 0.999).double().mean().item()
    print(case, f"alpha >= 0.999 on {share:.1%} of the samples, smallest T_bg {ref['T_bg'].min().item():.2e}")
    assert share >= 0.10
    assert (ref["T_bg"] < 1e-30).any()
    assert (ref["alpha"] == 1.0).any() or ref["alpha"].max() > 1 - 1e-6  # 1 - alpha + 1e-7 at its floor in the backward's divisor


@pytest.mark.parametrize("anneal", RC.ANNEALS)
def test_kink_case_sits_on_the_kinks(anneal):
    inp, ref, err = RC.kink_case(anneal)
    cos = (inp["grad"] * inp["dirs"][:, None, :]).sum(-1)  # float32
    want = torch.tensor([1.0, 0.0, -1.0])[torch.arange(RC.KINK_S) % 3].expand(RC.KINK_R, RC.KINK_S)
    assert torch.equal(cos, want)
    g = ref["d_grad"]
    # relu'(0) = 0 in torch: at cos = 1 neither term passes; at cos = 0 only relu(-cos / 2 + 1 / 2), weighted (1 - anneal) / 2
    assert (g[cos == 1] == 0).all()
    assert (g[cos == 0] == 0).all() == (anneal == 1.0)
    assert (g[cos == -1][:, 2] != 0).all() and (g[..., :2] == 0).all()
    _assert_conditioned(err, ("kink", anneal))


@pytest.mark.parametrize("case", RC.point_cases(), ids=_ids(RC.point_cases()))
def test_point_case_is_well_conditioned(case):
    inp, ref, err = RC.point_case(*case)
    assert ref["alpha"].shape == (case[2], 3) and all(torch.isfinite(v).all() for v in ref.values())
    assert 0 < inp["gaps"][0] < inp["gaps"][1] < inp["gaps"][2]
    assert (ref["d_variance"].item() == 0.0) == (case[0] == 1.5)
    _assert_conditioned(err, case)


def test_hemisphere_cases_reach_every_srgb_regime_away_from_every_discontinuity():
    linear = power = clamped = 0
    assert set(RC.HEMI_OPTIONAL) <= set(RC.hemi_cases())
    for case, with_vis in [(c, True) for c in RC.hemi_cases()] + [(c, False) for c in RC.HEMI_OPTIONAL]:
        R, S, D, U, scale = case
        inp, ref = RC.hemi_case(*case, with_vis=with_vis)
        assert ("vis" in ref["grads"]) == with_vis
        assert U < R and torch.bincount(inp["cam_of_ray"], minlength=U).max() >= 2  # d_cam_colours atomics collide
        # count = #(n.l > 0) and the clamp to [0, 1] are discontinuous: float32 must not be able to decide a dot differently
        assert ref["dot"].abs().min().item() >= 1e-5, (case, ref["dot"].abs().min().item())
        assert ref["dot"].abs().max().item() <= 1 - 1e-6, case
        lin = ref["lin"]
        assert (lin > 0).all()
        # ... nor a channel's segment of the curve (knee) or its clamp (1.0)
        assert ((lin - RC.SRGB_KNEE).abs() > 1e-6).all() and ((lin - 1).abs() > 1e-5).all(), case
        linear += int((lin <= RC.SRGB_KNEE).sum())
        clamped += int((lin > 1).sum())
        power += int(((lin > RC.SRGB_KNEE) & (lin < 1)).sum())
        assert torch.equal(ref["rgb"] == 1.0, lin > 1)
        # a clamped channel passes nothing back: bg's gradient is that channel's alone
        assert (ref["grads"]["bg"][lin > 1] == 0).all()
    print(f"output channels on the linear segment {linear}, the power segment {power}, the clamp {clamped}")
    assert linear > 0 and power > 0 and clamped > 0


def test_density_edge_entries_sit_in_last_owned_slots():
    for n, R, ld in RC.density_cases():
        CH = (n + 63) // 64
        inp, ref = RC.density_case(n, R, ld)
        raw = inp["raw"][:, 0].view(R, n)
        assert ref["weights"].shape == (R, n) and ref["d_raw"].shape == (R * n,)
        assert torch.isfinite(ref["weights"]).all() and torch.isfinite(ref["d_raw"]).all()
        for r, (low, sat) in enumerate(RC.density_edge_slots(n, R, ld)):
            for i in (low, sat):
                if i is not None:
                    assert 0 <= i < n and (i % CH == CH - 1 or i == n - 1)  # the last slot its lane owns
            if low is not None:
                assert raw[r, low] == -30.0
            if sat is not None:
                assert raw[r, sat] == 40.0 and (ref["weights"][r, sat + 1:] == 0).all()
            if low is not None and sat is not None:
                assert low < sat and ref["d_raw"][r * n + low] != 0  # the entry below the clamp still has a gradient to get wrong
        lows = [s[0] is not None for s in RC.density_edge_slots(n, R, ld)]
        sats = [s[1] is not None for s in RC.density_edge_slots(n, R, ld)]
        assert any(lows) or any(sats)
    assert any(RC.density_edge_slots(1, 1, ld)[0][0] is not None for ld in (1, 4))
    assert any(RC.density_edge_slots(1, 1, ld)[0][1] is not None for ld in (1, 4))


@pytest.mark.parametrize("case", RC.interlevel_cases(), ids=_ids(RC.interlevel_cases()))
def test_interlevel_case_has_decided_intervals(case):
    R, S, n, ties = case
    inp, ref = RC.interlevel_case(*case)
    assert (inp["c"][:, 1:] >= inp["c"][:, :-1]).all() and (inp["sb"][:, 1:] >= inp["sb"][:, :-1]).all()
    # max(w - w_outer, 0): no interval close enough to the kink for float32 to put it on the other side
    assert ref["margin"].abs().min().item() > 1e-6
    assert (ref["per_ray"] > 0).all()
    covered, g = ref["covered"], ref["d_wp"]
    scale = g.abs().max().item()
    assert covered.any() and (g[covered] < -1e-6 * scale).all() and (g[~covered].abs() <= 1e-14 * scale).all()
    if n > 1:
        assert (~covered).any()  # bins whose gradient must be exactly 0
    if n > 5:
        assert (ref["margin"] > 0).any() and (ref["margin"] < 0).any()
    hits = (inp["c"][:, 1:-1, None] == inp["sb"][:, None, 1:-1]).any(-1).sum().item()
    assert hits == (R * len(range(4, n, 4)) if ties else 0)  # final-level edges ON inner proposal edges, away from 0 and 1
