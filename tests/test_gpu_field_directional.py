"""The directional mode of the fused geometry kernels (csrc/field_chain.hip, pair layout: a point is two row-sets {value, tangent
along d}; ops.FieldChainFn(..., directional=True)) against the float64 restatement of test_gpu_field_chain.py fed the gradient
g_grad = g_cos d, and against the quad kernels on the same inputs.  Bars as there: 3e-6 of the largest entry for outputs, 4e-5 for
gradients.

Sizes: one partial pair tile (1), a tile edge (17 = 16 + 1), many tiles (5003), a second persistent round (33001)."""
import functools

import pytest
import torch

from test_gpu_field_chain import BETA, DEV, GF, KIN, NAMES, _crop, _err, _inputs, _reference, _run, _weights

pytestmark = pytest.mark.gpu
SIZES = [1, 17, 5003, 33001]


@functools.lru_cache(maxsize=None)
def _case(N):
    """inputs, float64 reference and both kernels' results for one size, computed once and shared (nothing below writes to them)"""
    from neusky_amd import ops
    g = torch.Generator().manual_seed(N)
    ET = _inputs(N, N + 1)
    ws = _weights(seed=N)
    d = torch.nn.functional.normalize(torch.randn(N, 3, generator=g).double(), dim=-1)
    g_sdf, g_cos = torch.randn(N, generator=g).to(DEV), torch.randn(N, generator=g).to(DEV)
    g_grad64 = g_cos.double().cpu()[:, None] * d  # [N, 3]
    # [E; sum_a d_a T_a], contracted in float64
    Td = (ET[N:].double().cpu().view(3, N, KIN) * d.t()[:, :, None]).sum(0)
    ETd = torch.cat([ET[:N], Td.float().to(DEV)], 0).contiguous()
    want_sdf, want_grad, _, want = _reference(ET, ws, g_sdf, g_grad64, None)
    want_cos = (want_grad * d).sum(-1)
    dET = want[0]
    want_dE = dET[:N]
    want_dTd = (dET[N:].view(3, N, KIN) * d.t()[:, :, None]).sum(0)
    # ---- directional kernels
    ops.begin_step(DEV)
    Eg = ETd.clone().requires_grad_(True)
    sdf, cos, alb = ops.FieldChainFn.apply(Eg, *ws, BETA, False, True)
    assert sdf.shape == (N,) and cos.shape == (N, 1) and float(alb.abs().max()) == 0.0
    loss = (sdf * g_sdf).sum() + (cos[:, 0] * g_cos).sum()
    got = torch.autograd.grad(loss, [Eg] + list(ws), allow_unused=True)
    torch.cuda.synchronize()
    # ---- quad kernels on the same inputs
    quad = _run(ops.FieldChainFn, ET, ws, g_sdf, g_grad64.float().to(DEV), None)
    return dict(N=N, d=d, sdf=sdf.detach(), cos=cos.detach()[:, 0], got=got, quad=quad, want_sdf=want_sdf, want_cos=want_cos,
                want_dE=want_dE, want_dTd=want_dTd, want=want)


def _sdf_row(n, t):
    """geometry-only passes train the sdf row of the last layer alone"""
    return t[GF] if n in ("dW2", "db2") else _crop(n, t)


@pytest.mark.parametrize("N", SIZES)
def test_pair_kernels_match_float64(N):
    c = _case(N)
    for what, a, b in (("sdf", c["sdf"], c["want_sdf"]), ("cos", c["cos"], c["want_cos"])):
        e, s = _err(a, b)
        print(f"N {N}: {what} {e:.3e} of {s:.3e} = {e / s:.3e}")
        assert e <= 3e-6 * s, f"{what}: {e:.3e} of {s:.3e}"
    dETd = c["got"][0]
    assert dETd.shape == (2 * N, KIN)
    for what, a, b in (("dE", dETd[:N], c["want_dE"]), ("dTd", dETd[N:], c["want_dTd"])):
        e, s = _err(a[:, :KIN - 1], b[:, :KIN - 1])
        print(f"N {N}: {what} {e:.3e} of {s:.3e} = {e / s:.3e}")
        assert e <= 4e-5 * s, f"{what}: {e:.3e} of {s:.3e}"
    for n, a, b in list(zip(NAMES, c["got"], c["want"]))[1:7]:
        e, s = _err(_sdf_row(n, a), _sdf_row(n, b))
        print(f"N {N}: {n} {e:.3e} of {s:.3e} = {e / s:.3e}")
        assert e <= 4e-5 * s, f"{n}: max err {e:.3e} of {s:.3e}"
    for n, a in list(zip(NAMES, c["got"]))[7:]:  # the colour net takes no gradient
        assert a is None or float(a.abs().max()) == 0.0, n


@pytest.mark.parametrize("N", SIZES)
def test_pair_and_quad_kernels_agree(N):
    """same points, g_grad = g_cos d: the value rows go through the same products in both layouts"""
    c = _case(N)
    q_sdf, q_grad, _, q = c["quad"]
    e, s = _err(c["sdf"], q_sdf.double().cpu())
    print(f"N {N}: sdf pair vs quad {e:.3e} of {s:.3e}; bit-equal: {bool(torch.equal(c['sdf'], q_sdf))}")
    assert e <= 3e-6 * s, f"sdf: {e:.3e} of {s:.3e}"
    e, s = _err(c["cos"], (q_grad.double().cpu() * c["d"]).sum(-1))
    assert e <= 3e-6 * s, f"cos: {e:.3e} of {s:.3e}"
    for n, a, b in list(zip(NAMES, c["got"], q))[1:7]:
        e, s = _err(_sdf_row(n, a), _sdf_row(n, b).double().cpu())
        print(f"N {N}: {n} pair vs quad {e:.3e} of {s:.3e} = {e / s:.3e}")
        assert e <= 4e-5 * s, f"{n}: {e:.3e} of {s:.3e}"


def test_pair_form_of_the_weighted_column_sum_and_the_masked_bias():
    """the two helper paths of the parameter gradients in their pair forms: w(row) = g_sdf[row / 2] on even rows, g_cos[row / 2] on odd
    rows, bias from the even rows; the streaming weight gradient's bias over rows 2 n only (bars of the quad forms' test)"""
    from neusky_amd import hip
    g = torch.Generator().manual_seed(2)
    N = 3001
    rows = 2 * N
    X = torch.randn(rows, 256, generator=g)
    Xn = hip.film_rows_to_native(X.to(DEV), 256)
    g_sdf, g_cos = torch.randn(N, generator=g), torch.randn(N, generator=g)
    out, b = torch.zeros(256, device=DEV), torch.zeros(1, device=DEV)
    hip.native_weighted_colsum_pair(Xn, 8, rows, out, b, g_sdf=g_sdf.to(DEV), g_cos=g_cos.to(DEV))
    want = torch.stack([g_sdf, g_cos], 1).reshape(-1).double() @ X.double()  # row 2 n + j
    assert (out.cpu().double() - want).abs().max() <= 1e-4 * want.abs().max()
    assert abs(float(b) - float(g_sdf.double().sum())) <= 1e-4 * float(g_sdf.abs().sum())
    dZ = torch.randn(rows, 256, generator=g) * 0.01
    Xe = torch.zeros(rows, 128); Xe[:, :72] = torch.randn(rows, 72, generator=g)
    dW, db = torch.zeros(256, 72, device=DEV), torch.zeros(256, device=DEV)
    gm = dZ.abs().max().reshape(1).to(DEV)
    hip.wgrad_native_batch([hip.wgrad_problem(hip.film_rows_to_native(dZ.to(DEV), 256), 8, hip.film_rows_to_native(Xe.to(DEV), 128), 4, rows, dW, db, gm, 64.0,
                                              width_b=72, bias_row_mod=2)], rows)
    wantW, wantb = dZ.double().t() @ Xe[:, :72].double(), dZ.double()[0::2].sum(0)
    assert (dW.cpu().double() - wantW).abs().max() <= 3e-5 * wantW.abs().max()
    assert (db.cpu().double() - wantb).abs().max() <= 3e-5 * wantb.abs().max()
