"""The small kernels on the step's critical path whose launch geometry was rebuilt around their serial parts (render.hip: hemisphere
composite, visibility finish backward, ray reduce, interlevel; losses.hip: main and DDF loss terms), each against a float64 torch
formulation at the smallest shapes where the new geometry can go wrong: one lane group / wave / workgroup and just past it, more
rows than one grid-stride pass covers, every register-slot count of the hemisphere kernels, absent optional inputs.  References and
bars are those of the existing tests of the same quantities (render_cases.py, ddf_rows_cases.py, test_gpu_losses.py,
test_gpu_ray_reduce.py, test_gpu_render_edges.py); nothing here is wider."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ddf_rows_cases as DC
import render_cases as RC
from test_gpu_losses import _oracle_main_terms
from test_gpu_ray_reduce import _ref as ray_reduce_reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(t):
    return None if t is None else t.to(DEV).contiguous()


# ---- hemisphere composite ----------------------------------------------------------------------------------------------------------
def _hemi_inputs(R, S, D):
    """render_cases.hemi_inputs inside the sRGB curve; with R = 5 the directions are folded into the upper hemisphere and every normal
    of ray 2 points straight down (no direction in its hemisphere: cnt = 0), and rays 3 and 4 share a camera.  Normals whose cosine
    to some direction is within 1e-5 of the clamp's kink are turned away from it (the margin render_cases conditions its own cases to)."""
    inp = {k: v.clone() for k, v in RC.hemi_inputs(R, S, D, 1 if R == 1 else 2, 0.05).items()}
    # d_bg = g (1 - sum_s w): at S = 96 the drawn weights sum to 1 - 1e-7 and the float32 difference is all rounding; half the weights
    # keep every ray's background visible (render_cases' own shapes stop at S = 5)
    inp["weights"] *= 0.5
    if R == 5:
        d = inp["dirs"].double()
        d[:, 2] = d[:, 2].abs() + 0.05
        inp["dirs"] = F.normalize(d, dim=-1).float()
        inp["cam_of_ray"][4] = inp["cam_of_ray"][3]
    for k in range(1, 20):
        bad = (torch.einsum("rsi,ji->rsj", inp["normals"].double(), inp["dirs"].double()).abs() < 1e-5).any(-1)
        if not bad.any():
            break
        inp["normals"][bad] = F.normalize(inp["normals"][bad] + 0.01 * k * torch.tensor([1.0, -2.0, 3.0]), dim=-1)
    if R == 5:
        inp["normals"][2] = torch.tensor([0.0, 0.0, -1.0])
    return inp


@pytest.mark.parametrize("with_vis", [True, False], ids=["vis", "novis"])
@pytest.mark.parametrize("D", [1, 63, 65, 512, 1024])
def test_hemi_composite_register_resident_directions(D, with_vis):
    """D on both sides of a lane stride and of the three register-slot counts (4, 8, 16 directions per lane); S = 1 (three idle
    waves), 5 (two samples for wave 0), 96 (the step's); a ray with cnt = 0; two rays adding into one camera's colours"""
    from test_gpu_render_edges import _hemi_run
    for R in (1, 5):
        for S in (1, 5, 96):
            inp = _hemi_inputs(R, S, D)
            ref = RC.hemi_reference(inp, torch.float64, with_vis)
            if R == 5:
                assert (ref["dot"][2] <= 0).all()
            rgb, lin, out = _hemi_run(inp, with_vis=with_vis, without=() if with_vis else ("vis",))
            what = (R, S, D, with_vis)
            np.testing.assert_allclose(rgb.cpu().numpy(), ref["rgb"].numpy(), rtol=1e-4, atol=2e-6, err_msg=str(what))
            np.testing.assert_allclose(lin.cpu().numpy(), ref["lin"].numpy(), rtol=1e-4, atol=2e-6, err_msg=str(what))
            for k, gref in ref["grads"].items():
                e = RC.rel_to_max(out[k].cpu(), gref)
                print(f"hemi {what} d_{k}: {e:.2e} of the largest entry (bar 2e-4)")
                assert e < 2e-4, (what, k, e)


# ---- main losses -------------------------------------------------------------------------------------------------------------------
MAIN_INPUTS = ("rgb", "eik", "weights", "normal", "hdr", "grid", "sdf", "thr")
MAIN_TERM_OF = {"rgb": 0, "eik": 1, "weights": 2, "grid": 3, "normal": 4, "hdr": 5, "thr": 6, "sdf": 7}


@pytest.mark.parametrize("R,S", [(1, 1), (5, 65), (64, 96)])
def test_main_losses_lane_groups_per_ray(R, S):
    """the inputs of test_gpu_losses.test_main_loss_terms_and_gradients at one ray, at S past four passes of a 16-lane group with a
    last partly filled workgroup, and at the step's S; then with each optional input absent once: its term is exactly 0, the
    others and their gradients stay at the bars"""
    from neusky_amd import ops
    g = torch.Generator().manual_seed(R + S)
    rnd = lambda *s: torch.rand(*s, generator=g)  # noqa: E731
    rgb, image = rnd(R, 3), rnd(R, 3)
    mask = (rnd(R, 4) > 0.5).float()
    mask[:, 1] = mask[:, 1] * (1 - mask[:, 3])
    eik = torch.randn(R, S, 3, generator=g)
    eik[0, 0] = 0.0
    scale = torch.tensor([0.5, 1.5, 0.0])[torch.arange(R) % 3]  # weight sums inside, above and below the BCE clip interval
    weights = rnd(R, S) * (2.0 / S) * scale[:, None]
    normal = torch.randn(R, 3, generator=g) * 0.7
    hdr = torch.exp(torch.randn(R, 3, generator=g) * 2 - 2)
    grid = torch.randn(50, 3, generator=g)
    sdf = torch.randn(777, 1, generator=g) * 0.1
    thr = torch.tensor([1.7])
    alpha, target = 0.1, 0.1
    cpu = dict(zip(MAIN_INPUTS, (rgb, eik, weights, normal, hdr, grid, sdf, thr)))
    ins64 = {k: t.double().requires_grad_(True) for k, t in cpu.items()}
    ref = _oracle_main_terms(ins64["rgb"], image.double(), mask.double(), *[ins64[k] for k in MAIN_INPUTS[1:]], alpha, target)
    wts = torch.linspace(0.5, 1.5, 8).double()
    gref = dict(zip(MAIN_INPUTS, torch.autograd.grad((ref * wts).sum(), [ins64[k] for k in MAIN_INPUTS])))
    for absent in (None,) + MAIN_INPUTS:
        insg = {k: None if k == absent else t.to(DEV).requires_grad_(True) for k, t in cpu.items()}
        out = ops.MainLossesFn.apply(insg["rgb"], image.to(DEV), mask.to(DEV), *[insg[k] for k in MAIN_INPUTS[1:]], alpha, target)
        want = ref.detach().clone()
        if absent is not None:
            assert out[MAIN_TERM_OF[absent]].item() == 0.0, (absent, out)
            want[MAIN_TERM_OF[absent]] = 0.0
        print(f"main losses ({R}, {S}) without {absent}: terms rel err {((out.cpu().double() - want).abs() / want.abs().clamp(min=1e-30)).max():.2e}")
        assert torch.allclose(out.cpu().double(), want, rtol=2e-5, atol=1e-7), (absent, out.cpu(), want)
        present = [k for k in MAIN_INPUTS if k != absent]
        ggpu = torch.autograd.grad((out * wts.float().to(DEV)).sum(), [insg[k] for k in present])
        for k, a in zip(present, ggpu):
            b = gref[k]
            assert a.shape == b.shape
            err = (a.cpu().double() - b).abs().max().item()
            assert err <= 2e-5 * max(b.abs().max().item(), 1e-12), (absent, k, err, b.abs().max().item())


# ---- DDF losses --------------------------------------------------------------------------------------------------------------------
def _ddf_terms(e, s, me, se, tm, mvt, mask, dw, sky_t, circ, inv, radius):
    """ddf_model.py:413-490 as test_gpu_losses.test_ddf_loss_terms_and_gradients writes it out; an absent section's term is 0"""
    zero = torch.zeros((), dtype=torch.float64)
    if circ:
        ex = e.unsqueeze(1); gt = tm.clone(); gt[mask == 0] = radius * 2
    else:
        ex = e.unsqueeze(1) * mask; gt = tm * mask
    iw = 1.0 / (gt + 1e-6) if inv else 1.0
    t0 = torch.mean(torch.abs(ex - gt) * dw.unsqueeze(-1) * iw)
    t1 = F.mse_loss(s * mask, torch.zeros_like(s) * mask)
    t2 = F.l1_loss(s * mask, torch.zeros_like(s) * mask)
    t3 = torch.mean(F.relu(me - mvt) ** 2) if me is not None else zero  # [Mm] - [Mm,1] -> [Mm,Mm] (sic)
    t4 = F.l1_loss(se, sky_t) if se is not None else zero
    return torch.stack([t0, t1, t2, t3, t4])


@pytest.mark.parametrize("circ,inv", [(False, False), (True, False), (False, True)])
def test_ddf_losses_wave_per_multi_view_row(circ, inv):
    """Mr of one row, just past a workgroup, and past one pass of the 256-workgroup grid; Mm absent, one row, one lane past a wave's
    stride, and more rows than the small grids have waves; with and without sky rows"""
    from neusky_amd import ops
    radius = 1.0
    wts = torch.tensor([1.0, 0.7, 1.3, 2.0, 0.5]).double()
    names = ("expected", "sdf", "mv", "sky", "term", "mv_term")
    for Mr in (1, 257, 70001):
        for Mm in (0, 1, 65, 300):
            for Ms in (0, 33):
                g = torch.Generator().manual_seed(3 + Mr + 7 * Mm + Ms)
                expected = torch.rand(Mr, generator=g) * 2
                term = torch.rand(Mr, 1, generator=g) * 2
                mask = (torch.rand(Mr, 1, generator=g) > 0.3).float()
                dw = torch.rand(Mr, generator=g)
                sdf = torch.randn(Mr, 1, generator=g) * 0.1
                mv_e = torch.rand(Mm, generator=g) * 2 if Mm else None
                mv_t = torch.rand(Mm, 1, generator=g) * 2 if Mm else None
                sky_e = torch.rand(Ms, generator=g) * 2 if Ms else None
                sky_t = torch.rand(Ms, generator=g) * 2 if Ms else None
                cpu = dict(zip(names, (expected, sdf, mv_e, sky_e, term, mv_t)))
                i64 = {k: None if t is None else t.double().requires_grad_(True) for k, t in cpu.items()}
                ref = _ddf_terms(i64["expected"], i64["sdf"], i64["mv"], i64["sky"], i64["term"], i64["mv_term"], mask.double(), dw.double(),
                                 None if sky_t is None else sky_t.double(), circ, inv, radius)
                present = [k for k in names if cpu[k] is not None]
                gref = dict(zip(present, torch.autograd.grad((ref * wts).sum(), [i64[k] for k in present])))
                ig = {k: None if t is None else t.to(DEV).requires_grad_(True) for k, t in cpu.items()}
                flags = dict(want_depth=1, want_sdf_l2=1, want_sdf_l1=1, mask_to_circumference=int(circ), inverse_depth_weight=int(inv), radius=radius)
                out = ops.DDFLossesFn.apply(ig["expected"], ig["term"], mask.to(DEV), dw.to(DEV), ig["sdf"], ig["mv"], ig["mv_term"], ig["sky"],
                                            _dev(sky_t), flags)
                what = (circ, inv, Mr, Mm, Ms)
                assert torch.allclose(out.cpu().double(), ref.detach(), rtol=3e-5, atol=1e-7), (what, out.cpu(), ref)
                ggpu = torch.autograd.grad((out * wts.float().to(DEV)).sum(), [ig[k] for k in present])
                for k, a in zip(present, ggpu):
                    b = gref[k]
                    assert a.shape == b.shape
                    err = (a.cpu().double() - b).abs().max().item()
                    assert err <= 3e-5 * max(b.abs().max().item(), 1e-12), (what, k, err)


# ---- visibility finish backward ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_thr", [True, False], ids=["d_threshold", "null"])
@pytest.mark.parametrize("R,Dv", [(1, 1), (5, 51), (70001, 1)])
def test_visibility_finish_bwd_one_atomic_per_workgroup(R, Dv, with_thr):
    """R Dv = 1, one short of a workgroup, and past one pass of the 256-workgroup grid; d_t_hat at ddf_rows_cases.bar, d_threshold at
    ddf_rows_cases.threshold_bar, and nothing written to a null d_threshold"""
    from neusky_amd import hip
    g = torch.Generator().manual_seed(R + Dv)
    D, M = Dv + Dv // 2 + 1, R * Dv
    sel = torch.sort(torch.randperm(D, generator=g)[:Dv]).values
    inp = dict(origins=torch.zeros(R, 3), sel_index=sel, threshold=RC.F32(0.35), scale=2.0 if R == 1 else 25.0, d_vis=torch.randn(R, D, generator=g))
    surf = torch.rand(M, generator=g) * 2
    t_hat = surf - 0.35 + torch.randn(M, generator=g) * 0.1  # a share of the rows off the sigmoid's saturation at scale 25
    r64, r32 = DC.finish_reference(t_hat, surf, inp, torch.float64), DC.finish_reference(t_hat, surf, inp, torch.float32)
    d_t = torch.full((M + 64,), float("nan"), device=DEV)
    d_thr = torch.zeros(1, device=DEV) if with_thr else None
    hip.visibility_finish_bwd(_dev(t_hat), _dev(surf), torch.tensor([inp["threshold"]], device=DEV), inp["scale"], _dev(sel.to(torch.int32)), R, Dv, D,
                              _dev(inp["d_vis"]), d_t[:M], d_thr)
    torch.cuda.synchronize()
    assert torch.isnan(d_t[M:]).all(), "a guard row was written"
    err, bar = DC.max_err(d_t[:M].cpu(), r64["d_t_hat"]), DC.bar(r32["d_t_hat"], r64["d_t_hat"])
    print(f"visibility finish ({R}, {Dv}) d_t_hat: error {err:.2e}, bar {bar:.2e}")
    assert err <= bar
    if with_thr:
        err, bar = abs(d_thr.item() - r64["d_threshold"].item()), DC.threshold_bar(r64["d_threshold_terms"])
        print(f"visibility finish ({R}, {Dv}) d_threshold: error {err:.2e}, bar {bar:.2e}")
        assert err <= bar


# ---- ray reduce --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,S", [(1, 1), (1, 65), (5, 1), (5, 65), (1024, 1), (1024, 65)])
def test_ray_reduce_bounds_meet_in_the_workgroup(R, S):
    """one ray, fewer rays than a workgroup's waves, and two rays per wave of a full grid; S of one sample and past a lane stride.  The
    last ray holds both the smallest and the largest mid point of the batch (with S > 1), so both clip bounds come out of one wave of
    the last workgroup; the clip is active on rays with no weight (depth 0 below the smallest mid point)"""
    from neusky_amd import ops
    g = torch.Generator().manual_seed(R + S)
    w = torch.rand(R, S, 1, generator=g) * (2.0 / S)
    w[0] = 0.0
    st = torch.cumsum(torch.rand(R, S, 1, generator=g) * 0.1, dim=1) + 0.5
    st[-1, 0] = 0.01
    st[-1, -1] = st.max() + 1.0
    en = st + 0.05
    nr = F.normalize(torch.randn(R, S, 3, generator=g), dim=-1)
    al = torch.rand(R, S, 3, generator=g)
    wd = w.to(DEV).requires_grad_(True)
    p2p, acc, normal, alb = ops.RayReduceFn.apply(wd, st.to(DEV), en.to(DEV), nr.to(DEV), al.to(DEV), 0.0)
    w64 = w.double().requires_grad_(True)
    rp, ra, rn, rb = ray_reduce_reference(w64, st.double(), en.double(), nr.double(), al.double(), 0.0)
    mids = (st + en) / 2
    assert p2p[0].item() == mids.min().item()  # the empty ray's depth is the lower bound itself, bit for bit
    for got, want in ((p2p, rp), (acc, ra), (normal, rn), (alb, rb)):
        assert torch.allclose(got.cpu().double(), want, atol=2e-6, rtol=1e-5), (R, S)
    gp, ga = torch.randn(R, 1, generator=g), torch.randn(R, 1, generator=g)
    ((p2p * gp.to(DEV)).sum() + (acc * ga.to(DEV)).sum()).backward()
    ((rp * gp.double()).sum() + (ra * ga.double()).sum()).backward()
    assert float((wd.grad.cpu().double() - w64.grad).abs().max()) < 2e-5 * float(w64.grad.abs().max())


# ---- interlevel --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 65])
@pytest.mark.parametrize("n", [1, 64, 257])
def test_interlevel_rows_through_lds(n, S):
    """the proposal weights of a row reach LDS and d_wp leaves it with all lanes: n of one bin, of one pass of the wave, and of four
    passes and one lane; R = 5 leaves the second workgroup with one ray.  Bars of test_gpu_render_edges."""
    from neusky_amd import ops
    inp, ref = RC.interlevel_case(5, S, n, False)
    wp = inp["wp"].to(DEV).requires_grad_(True)
    per_ray = ops.InterlevelFn.apply(inp["c"].to(DEV), inp["w"].to(DEV), inp["sb"].to(DEV), wp)
    got = per_ray.detach().cpu().double()
    assert abs(got.sum().item() - ref["per_ray"].sum().item()) < 2e-5 * ref["per_ray"].sum().item()
    assert (got - ref["per_ray"]).abs().max().item() < 2e-5 * ref["per_ray"].max().item()
    (per_ray * inp["probe"].to(DEV)).sum().backward()
    grad = wp.grad.cpu()
    assert (grad.double() - ref["d_wp"]).abs().max().item() < 2e-5 * ref["d_wp"].abs().max().item()
    assert (grad[~ref["covered"]] == 0).all()
