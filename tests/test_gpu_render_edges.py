"""The render kernels (neusky_amd/csrc/render.hip) against the float64 oracle at trained sharpness and at every edge of their
chunking: NeuS weights, point alphas, the hemisphere composite, the proposal density weights and the interlevel loss.  The cases
and their references come from render_cases.py; test_render_cases_cpu.py proves what each case reaches and that it is well
conditioned.  Gradients are held to a bar relative to the reference tensor's largest entry."""
import numpy as np
import pytest
import torch

import render_cases as RC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS32 = float(np.finfo(np.float32).eps)


def _ids(cases):
    return ["-".join(str(v) for v in c) for c in cases]


def _grad_bar(err32):
    """the existing 5e-4 of the reference's largest entry, or 4 x what plain float32 arithmetic makes of the same inputs where that
    is more: the kernels' hardware exp / reciprocal and wave-scan order differ from torch's float32 by a small multiple of its
    rounding.  The cases are conditioned to err32 <= 1e-3 (test_render_cases_cpu.py), so the bar never passes 4e-3."""
    return max(5e-4, 4.0 * err32)


def _check_grad(name, got, ref, err32, what):
    e = RC.rel_to_max(got.cpu(), ref)
    if err32 > 0:
        print(f"RATIO {what[0]} {name} kernel {e:.3e} restatement {err32:.3e} ratio {e / err32:.2f} {what}")
    assert e <= _grad_bar(err32), (what, name, e, err32)


def _check_d_variance(dvar, ref, err32, variance, terms, what):
    """the kernels ADD into d_variance: the buffer held 3.0.  Past the clamp of inv_s (variance 1.5) nothing may be added at all.
    Below it the sum is 3.0 + reference, within the gradient bar on the reference plus the float32 rounding of `terms` atomic
    additions onto a value of that size."""
    if variance == 1.5:
        assert torch.equal(dvar.cpu(), torch.tensor([3.0])), (what, dvar.item())
        return
    r = ref.item()
    e = abs(dvar.double().item() - 3.0 - r)
    slack = terms * EPS32 * (3.0 + abs(r))
    if err32 > 0:
        print(f"RATIO {what[0]} d_variance kernel {e / abs(r):.3e} restatement {err32:.3e} ratio {e / abs(r) / err32:.2f} {what}")
    assert e <= _grad_bar(err32) * abs(r) + slack, (what, "d_variance", e, r, err32)


# ---- NeuS weights ----------------------------------------------------------------------------------------------------------------
_NEUS_OPTIONAL_FWD = ("alpha", "T_bg", "accumulation", "depth")


def _neus_args(inp):
    return tuple(inp[k].to(DEV) for k in ("sdf", "grad", "dirs", "starts", "ends", "variance")) + (inp["anneal"],)


def _neus_fwd(args, R, S, without=()):
    from neusky_amd import hip
    out = {k: None if k in without else torch.full((R, S) if k in ("alpha", "weights") else (R,), float("nan"), device=DEV)
           for k in ("alpha", "weights", "T_bg", "accumulation", "depth")}
    hip.neus_weights_fwd(*args, out["alpha"], out["weights"], out["T_bg"], out["accumulation"], out["depth"])
    return out


def _neus_bwd(args, gw, gT, R, S, with_variance=True):
    from neusky_amd import hip
    out = dict(d_sdf=torch.full((R, S), float("nan"), device=DEV), d_grad=torch.full((R, S, 3), float("nan"), device=DEV),
               d_variance=torch.full((1,), 3.0, device=DEV) if with_variance else None)
    hip.neus_weights_bwd(*args, gw, gT, out["d_sdf"], out["d_grad"], out["d_variance"])
    return out


def _check_neus_forward(out, ref, what):
    for k in ("alpha", "weights", "T_bg", "accumulation"):
        e = (out[k].cpu().double() - ref[k]).abs().max().item()
        assert e < 2e-5, (what, k, e)
    dep, on = out["depth"].cpu().double(), ref["accumulation"] > RC.DEPTH_MIN_ACC
    if on.any():
        e = (dep[on] - ref["depth"][on]).abs().max().item()
        assert e < 5e-5, (what, "depth", e)
    # a ray that accumulates next to nothing: depth = sum(w mid) / (sum(w) + 1e-10) is a mean of its mid points, short of one by
    # 1e-10 / sum(w) at the most, and sum(w) >= the smallest alpha there is, 1e-5 / (1 + 1e-5)
    mid = ref["mid"]
    assert torch.isfinite(dep).all()
    assert (dep >= mid.min(1).values * (1 - 2e-5)).all() and (dep <= mid.max(1).values * (1 + 1e-6)).all(), what


@pytest.mark.parametrize("case", RC.neus_cases(), ids=_ids(RC.neus_cases()))
def test_neus_weights_at_every_sharpness_anneal_and_chunk_edge(case):
    """nsky_neus_weights_fwd/bwd against O.neus_alpha + O.weights_from_alphas in float64, over render_cases.neus_cases().

    Largest kernel error / float32-restatement error seen on an MI355X (the bar allows 4, or 5e-4 of the reference's largest entry
    where that is more), per family:
      resolved  d_sdf 40.8   d_grad 1.40   d_variance 3.0
      coarse    d_sdf 1.48   d_grad 1.63   d_variance 1.65
    The 40.8 is one sample of one ray (S = 1, R = 1) whose restatement happens to land within 8e-9; the kernel is within 3.4e-7
    there, and among the cases with a restatement error of 1e-6 or more the largest ratio is 1.04 (d_sdf), 1.13 (d_grad), 1.57
    (d_variance).  d_variance is summed with float atomics onto the 3.0 the buffer held: its figure moves with their order from
    run to run (2.0 .. 3.0).  The largest errors themselves: d_sdf 2.0e-5, d_grad 2.3e-5 (both coarse, variance 0.9, S = 256, where
    the restatement has the same), d_variance 6.2e-4 (resolved, variance 0.9, R = 1, S = 63: restatement 6.0e-4)."""
    family, variance, anneal, R, S = case
    inp, ref, err = RC.neus_case(*case)
    args = _neus_args(inp)
    gw, gT = inp["gw"].to(DEV), inp["gT"].to(DEV)
    out = _neus_fwd(args, R, S)
    _check_neus_forward(out, ref, case)
    grads = _neus_bwd(args, gw, gT, R, S)
    if family == "coarse":  # alphas of exactly 1 and a transmittance below the normal float32 range
        assert all(torch.isfinite(v).all() for v in list(out.values()) + list(grads.values())), case
    _check_grad("d_sdf", grads["d_sdf"], ref["d_sdf"], err["d_sdf"], case)
    _check_grad("d_grad", grads["d_grad"], ref["d_grad"], err["d_grad"], case)
    _check_d_variance(grads["d_variance"], ref["d_variance"], err["d_variance"], variance, R, case)
    # every optional pointer may be null, and the other outputs do not notice
    for k in _NEUS_OPTIONAL_FWD:
        part = _neus_fwd(args, R, S, without=(k,))
        assert all(torch.equal(part[j], out[j]) for j in out if j != k), (case, k)
    part = _neus_bwd(args, gw, gT, R, S, with_variance=False)
    assert torch.equal(part["d_sdf"], grads["d_sdf"]) and torch.equal(part["d_grad"], grads["d_grad"]), case
    # no d_trans_bg is a d_trans_bg of zeros: the reference of the same inputs with gT = 0
    ref0, err0 = RC.neus_case_without_gT(*case)
    zeros, null = _neus_bwd(args, gw, torch.zeros(R, device=DEV), R, S), _neus_bwd(args, gw, None, R, S)
    assert torch.equal(null["d_sdf"], zeros["d_sdf"]) and torch.equal(null["d_grad"], zeros["d_grad"]), case
    _check_grad("d_sdf", null["d_sdf"], ref0["d_sdf"], err0["d_sdf"], ("gT=None",) + case)
    _check_grad("d_grad", null["d_grad"], ref0["d_grad"], err0["d_grad"], ("gT=None",) + case)
    _check_d_variance(null["d_variance"], ref0["d_variance"], err0["d_variance"], variance, R, ("gT=None",) + case)
    if R == 1:  # one atomic addition: nothing about its order can differ
        assert torch.equal(null["d_variance"], zeros["d_variance"]), case


@pytest.mark.parametrize("anneal", RC.ANNEALS)
def test_neus_weights_on_the_relu_kinks(anneal):
    """cos = 1, 0, -1 exactly: torch's relu has derivative 0 at 0, and so must the kernel's strict comparisons"""
    inp, ref, err = RC.kink_case(anneal)
    R, S = RC.KINK_R, RC.KINK_S
    args = _neus_args(inp)
    _check_neus_forward(_neus_fwd(args, R, S), ref, ("kink", anneal))
    grads = _neus_bwd(args, inp["gw"].to(DEV), inp["gT"].to(DEV), R, S)
    zero = ref["d_grad"] == 0
    assert zero.any() and (grads["d_grad"].cpu()[zero] == 0).all(), grads["d_grad"].cpu()[zero].abs().max().item()
    for k in ("d_sdf", "d_grad"):
        _check_grad(k, grads[k], ref[k], err[k], ("kink", anneal))
    _check_d_variance(grads["d_variance"], ref["d_variance"], err["d_variance"], 0.32, R, ("kink", anneal))


# ---- point alphas ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", RC.point_cases(), ids=_ids(RC.point_cases()))
def test_point_alphas_match_the_oracle(case):
    """nsky_point_alphas_fwd/bwd against O.neus_alpha itself (sdf [P,1], deltas = gaps[None,:]) in float64: not against
    nsky_neus_weights, which shares neus_alpha_terms with it.

    Largest kernel error / float32-restatement error seen on an MI355X: d_sdf 1.30, d_grad 1.65, d_variance 55 -- the last where
    the restatement lands within 3e-8 (variance 0.6, P = 257) and the kernel's sum, rounded onto the 3.0 the buffer held, within
    1.6e-6; 1.21 among the cases with a restatement error of 1e-6 or more.  Largest errors: 1.2e-5, 4.0e-5, 4.5e-5."""
    from neusky_amd import hip
    variance, anneal, P = case
    inp, ref, err = RC.point_case(*case)
    sdf, grad, dirs, var = (inp[k].to(DEV) for k in ("sdf", "grad", "dirs", "variance"))
    alphas = torch.full((P, 3), float("nan"), device=DEV)
    hip.point_alphas_fwd(sdf, grad, dirs, inp["gaps"], var, inp["anneal"], alphas)
    e = (alphas.cpu().double() - ref["alpha"]).abs().max().item()
    assert e < 2e-5, (case, e)
    d_sdf, d_grad = torch.full((P,), float("nan"), device=DEV), torch.full((P, 3), float("nan"), device=DEV)
    d_var = torch.full((1,), 3.0, device=DEV)
    hip.point_alphas_bwd(sdf, grad, dirs, inp["gaps"], var, inp["anneal"], inp["probe"].to(DEV), d_sdf, d_grad, d_var)
    what = ("point",) + case
    _check_grad("d_sdf", d_sdf, ref["d_sdf"], err["d_sdf"], what)
    _check_grad("d_grad", d_grad, ref["d_grad"], err["d_grad"], what)
    _check_d_variance(d_var, ref["d_variance"], err["d_variance"], variance, (P + 63) // 64, what)
    # d_variance is optional here too
    d_sdf2, d_grad2 = torch.empty_like(d_sdf), torch.empty_like(d_grad)
    hip.point_alphas_bwd(sdf, grad, dirs, inp["gaps"], var, inp["anneal"], inp["probe"].to(DEV), d_sdf2, d_grad2, None)
    assert torch.equal(d_sdf2, d_sdf) and torch.equal(d_grad2, d_grad)


# ---- hemisphere composite --------------------------------------------------------------------------------------------------------
def _hemi_run(inp, with_vis=True, without=()):
    """forward + backward; gradient buffers named in `without` are passed as null"""
    from neusky_amd import hip
    R, S, _ = inp["albedo"].shape
    D, U = inp["dirs"].shape[0], inp["cam_colours"].shape[0]
    d = {k: inp[k].to(DEV) for k in ("albedo", "normals", "weights", "dirs", "cam_colours", "bg", "d_rgb")}
    cam = inp["cam_of_ray"].to(torch.int32).to(DEV)
    vis = inp["vis"].to(DEV) if with_vis else None
    rgb, lin = torch.full((R, 3), float("nan"), device=DEV), torch.full((R, 3), float("nan"), device=DEV)
    hip.hemi_composite_fwd(d["albedo"], d["normals"], d["weights"], d["dirs"], d["cam_colours"], cam, vis, d["bg"], rgb, lin)
    nan = lambda *shape: torch.full(shape, float("nan"), device=DEV)  # noqa: E731
    out = {"albedo": nan(R, S, 3), "normals": nan(R, S, 3), "weights": nan(R, S), "cam_colours": torch.zeros(U, D, 3, device=DEV),
           "vis": nan(R, D), "bg": nan(R, 3)}
    for k in without:
        out[k] = None
    hip.hemi_composite_bwd(d["albedo"], d["normals"], d["weights"], d["dirs"], d["cam_colours"], cam, vis, d["bg"], lin, d["d_rgb"],
                           out["albedo"], out["normals"], out["weights"], out["cam_colours"], out["vis"], out["bg"])
    return rgb, lin, out


def _check_hemi(rgb, lin, out, ref, what):
    # forward bar of the golden tests; gradients at their 2e-4 of the reference's largest entry
    np.testing.assert_allclose(rgb.cpu().numpy(), ref["rgb"].numpy(), rtol=1e-4, atol=2e-6, err_msg=str(what))
    np.testing.assert_allclose(lin.cpu().numpy(), ref["lin"].numpy(), rtol=1e-4, atol=2e-6, err_msg=str(what))
    for k, gref in ref["grads"].items():
        if out[k] is None:
            continue
        e = RC.rel_to_max(out[k].cpu(), gref)
        assert e < 2e-4, (what, k, e)
    # a channel the curve clamps (composite > 1) passes nothing back: exactly zero to that channel's background and albedo, and
    # to every input of a ray whose three channels are all clamped
    clamped = ref["lin"] > 1
    assert (out["bg"].cpu()[clamped] == 0).all(), what
    assert (out["albedo"].cpu().transpose(1, 2)[clamped] == 0).all(), what
    dark = clamped.all(-1)
    for k in ("normals", "weights", "vis"):
        if out.get(k) is not None:
            assert (out[k].cpu()[dark] == 0).all(), (what, k)


@pytest.mark.parametrize("case", RC.hemi_cases(), ids=_ids(RC.hemi_cases()))
def test_hemi_composite_at_every_shape_and_brightness(case):
    """nsky_hemi_composite_fwd/bwd against O.lambertian_render in float64: one direction, fewer samples than waves, D on both
    sides of a lane stride, all 16 register slots per lane (D = 1024), rays that share a camera, and light that puts output
    channels on the curve's linear segment, on its power segment and above its clamp"""
    inp, ref = RC.hemi_case(*case)
    rgb, lin, out = _hemi_run(inp)
    _check_hemi(rgb, lin, out, ref, case)


@pytest.mark.parametrize("case", RC.HEMI_OPTIONAL, ids=_ids(RC.HEMI_OPTIONAL))
def test_hemi_composite_optional_pointers(case):
    inp, ref = RC.hemi_case(*case)
    rgb, lin, full = _hemi_run(inp)
    # d_cam_colours is summed with float atomics by the rays that share a camera, in no fixed order: it is held to the reference
    # in every run, the outputs with one writer each to equality with the full run
    fixed = ("albedo", "normals", "weights", "vis", "bg")
    for k in ("vis", "cam_colours"):
        rgb2, lin2, part = _hemi_run(inp, without=(k,))
        assert torch.equal(rgb2, rgb) and torch.equal(lin2, lin)
        assert all(torch.equal(part[j], full[j]) for j in fixed if j != k), (case, k)
        _check_hemi(rgb2, lin2, part, ref, case + ("no d_" + k,))
    inp, ref = RC.hemi_case(*case, with_vis=False)
    rgb, lin, out = _hemi_run(inp, with_vis=False, without=("vis",))
    _check_hemi(rgb, lin, out, ref, case + ("vis=None",))


# ---- proposal density weights ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", RC.density_cases(), ids=_ids(RC.density_cases()))
def test_density_weights_at_every_chunk_edge(case):
    """nsky_density_weights_fwd/bwd against trunc_exp + ray_samplers.weights_from_density in float64 at the bars of
    test_gpu_render.test_density_weights_matches_torch_formulation, with the saturated entry and the entry below trunc_exp's
    backward clamp in the last slot a lane owns"""
    from neusky_amd import ops
    n, R, ld = case
    inp, ref = RC.density_case(*case)
    raw = inp["raw"].to(DEV).requires_grad_(True)
    w = ops.DensityWeightsFn.apply(raw, inp["ebins"].to(DEV))
    assert w.shape == (R, n)
    assert (w.detach().cpu().double() - ref["weights"]).abs().max().item() < 2e-6
    (w * inp["probe"].to(DEV)).sum().backward()
    assert (raw.grad[:, 1:] == 0).all()
    gref = ref["d_raw"]
    e = (raw.grad[:, 0].cpu().double() - gref).abs().max().item()
    assert e < 1e-5 * max(gref.abs().max().item(), 1.0), (case, e)


# ---- interlevel loss -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", RC.interlevel_cases(), ids=_ids(RC.interlevel_cases()))
def test_interlevel_at_its_limits_and_on_ties(case):
    """nsky_interlevel_fwd/bwd against O._outer in float64: one sample and one bin, S past one lane stride, the LDS limit
    n = 1023, a partly filled last workgroup, and final-level edges that equal proposal edges"""
    from neusky_amd import ops
    R, S, n, ties = case
    inp, ref = RC.interlevel_case(*case)
    wp = inp["wp"].to(DEV).requires_grad_(True)
    per_ray = ops.InterlevelFn.apply(inp["c"].to(DEV), inp["w"].to(DEV), inp["sb"].to(DEV), wp)
    got = per_ray.detach().cpu().double()
    assert abs(got.sum().item() - ref["per_ray"].sum().item()) < 2e-5 * ref["per_ray"].sum().item()
    assert (got - ref["per_ray"]).abs().max().item() < 2e-5 * ref["per_ray"].max().item()
    (per_ray * inp["probe"].to(DEV)).sum().backward()
    g = wp.grad.cpu()
    assert (g.double() - ref["d_wp"]).abs().max().item() < 2e-5 * ref["d_wp"].abs().max().item()
    assert (g[~ref["covered"]] == 0).all()  # bins no active interval covers: exactly zero, not a residue of the prefix sum
