"""The one-column path of the NeuS weights kernels (nsky_neus_weights_cos_fwd / _bwd: the gradient arrives as the precomputed cosine
cos = ray_dir . grad(sdf), the backward writes d_cos) against the three-column path fed g = cos d, forward and backward, at the
bars test_gpu_render_edges.py holds that kernel to: 2e-5 on alpha / weights / T_bg / accumulation, 5e-5 on the depth, 5e-4 of the
largest entry on the gradients.  R = 1, 33 (a ninth workgroup holding one ray), S = 1, 96 (the step's: two samples per lane in 48
lanes)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _inputs(R, S, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.linspace(0.0, 1.0, S + 1)[None].repeat(R, 1) * (1.0 + 0.2 * torch.rand(R, 1, generator=g)) + 0.05
    starts, ends = t[:, :-1].contiguous(), t[:, 1:].contiguous()
    mid = 0.5 * (starts + ends)
    sdf = (0.6 * torch.rand(R, 1, generator=g) + 0.2 - mid) * 0.5 + 0.02 * torch.randn(R, S, generator=g)  # crosses zero along the ray
    cos = torch.rand(R, S, generator=g) * 2 - 1  # both sides of the two ReLU kinks
    d = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1)
    variance = torch.tensor([0.3])
    gw, gT = torch.randn(R, S, generator=g), torch.randn(R, generator=g)
    return [v.to(DEV) for v in (sdf, cos, d, starts, ends, variance, gw, gT)]


@pytest.mark.parametrize("anneal", [0.0, 0.4, 1.0])
@pytest.mark.parametrize("R,S", [(1, 1), (1, 96), (33, 1), (33, 96)])
def test_cosine_column_equals_the_three_column_path(R, S, anneal):
    from neusky_amd import hip
    sdf, cos, d, starts, ends, variance, gw, gT = _inputs(R, S, 100 * R + S)
    grad3 = (cos[:, :, None] * d[:, None, :]).contiguous()  # g = cos d: d . g = cos |d|^2
    new = lambda *s: torch.full(s, float("nan"), device=DEV)  # noqa: E731
    out3 = dict(alpha=new(R, S), weights=new(R, S), T_bg=new(R), accumulation=new(R), depth=new(R))
    out1 = {k: v.clone() for k, v in out3.items()}
    hip.neus_weights_fwd(sdf, grad3, d, starts, ends, variance, anneal, out3["alpha"], out3["weights"], out3["T_bg"], out3["accumulation"], out3["depth"])
    hip.neus_weights_cos_fwd(sdf, cos, starts, ends, variance, anneal, out1["alpha"], out1["weights"], out1["T_bg"], out1["accumulation"], out1["depth"])
    b3 = dict(d_sdf=new(R, S), d_grad=new(R, S, 3), d_variance=torch.zeros(1, device=DEV))
    b1 = dict(d_sdf=new(R, S), d_cos=new(R, S), d_variance=torch.zeros(1, device=DEV))
    hip.neus_weights_bwd(sdf, grad3, d, starts, ends, variance, anneal, gw, gT, b3["d_sdf"], b3["d_grad"], b3["d_variance"])
    hip.neus_weights_cos_bwd(sdf, cos, starts, ends, variance, anneal, gw, gT, b1["d_sdf"], b1["d_cos"], b1["d_variance"])
    torch.cuda.synchronize()
    for k in ("alpha", "weights", "T_bg", "accumulation", "depth"):
        assert torch.isfinite(out1[k]).all(), k
        e = (out1[k].double() - out3[k].double()).abs().max().item()
        print(f"R {R} S {S} anneal {anneal}: {k} {e:.3e}")
        assert e < (5e-5 if k == "depth" else 2e-5), (k, e)
    want_dcos = (b3["d_grad"].double() * d.double()[:, None, :]).sum(-1)  # d_cos = sum_a d_a d_grad_a
    for k, got, want in (("d_sdf", b1["d_sdf"], b3["d_sdf"].double()), ("d_cos", b1["d_cos"], want_dcos),
                         ("d_variance", b1["d_variance"], b3["d_variance"].double())):
        assert torch.isfinite(got).all(), k
        e, s = (got.double() - want).abs().max().item(), want.abs().max().item()
        print(f"R {R} S {S} anneal {anneal}: {k} {e:.3e} of {s:.3e}")
        assert e <= 5e-4 * s, (k, e, s)
    # optional outputs may be null, and the autograd node takes the [R, S, 1] column
    w_only = new(R, S)
    hip.neus_weights_cos_fwd(sdf, cos, starts, ends, variance, anneal, None, w_only, None, None, None)
    assert torch.equal(w_only, out1["weights"])


def test_autograd_node_dispatches_on_the_column_count():
    from neusky_amd import ops
    R, S = 33, 96
    sdf, cos, d, starts, ends, variance, gw, gT = _inputs(R, S, 7)
    res = {}
    for name, grad in (("one", cos[:, :, None].clone()), ("three", (cos[:, :, None] * d[:, None, :]).contiguous())):
        s, g, v = sdf.clone().requires_grad_(True), grad.requires_grad_(True), variance.clone().requires_grad_(True)
        w, tb, acc, dep = ops.NeusWeightsFn.apply(s, g, d, starts, ends, v, 0.7)
        ((w * gw).sum() + (tb * gT).sum()).backward()
        res[name] = (w.detach(), s.grad, g.grad, v.grad)
    torch.cuda.synchronize()
    assert res["one"][2].shape == (R, S, 1) and res["three"][2].shape == (R, S, 3)
    assert (res["one"][0] - res["three"][0]).abs().max().item() < 2e-5
    want = (res["three"][2].double() * d.double()[:, None, :]).sum(-1, keepdim=True)
    for got, ref in ((res["one"][1].double(), res["three"][1].double()), (res["one"][2].double(), want), (res["one"][3].double(), res["three"][3].double())):
        assert (got - ref).abs().max().item() <= 5e-4 * ref.abs().max().item()
