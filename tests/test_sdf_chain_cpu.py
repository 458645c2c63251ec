"""sdf_chain_cpu.py, the CPU restatement of the sdf value chain that test_gpu_sdf_chain_parity.py holds the chain kernels to: (a) its float64
mode is torch float64 autograd of the three layers, (b) its restatement of the launch plan covers every wave tile exactly once and the row
counts of plan_rows land in the classes they name, (c) the noise-tied bars catch one lost split term in any of the four products and two
damaged constants, in an emulation of the kernels' split products, while the undamaged emulation passes at every case of the GPU suite."""
import functools

import pytest
import torch

import sdf_chain_cpu as SC

PLAN_CUS = (1, 8, 32, 256, 304)


@functools.lru_cache(maxsize=None)
def _case(in_dim, M, steep=False):
    E, g = SC.make_inputs(M, in_dim, steep)
    return SC.make_weights(in_dim, steep), E, g


@functools.lru_cache(maxsize=None)
def _ref_and_bars(in_dim, M, steep=False):
    return SC.reference_and_bars(*_case(in_dim, M, steep))


@pytest.mark.parametrize("in_dim", SC.DIM_EDGES)
def test_float64_restatement_is_torch_autograd(in_dim):
    ws, E, g = _case(in_dim, SC.DIM_M)
    w64 = [w.double().requires_grad_(True) for w in ws]
    W0, b0, W1, b1, w2, b2 = w64
    E64 = E.double().requires_grad_(True)
    sp = lambda z: torch.nn.functional.softplus(z, beta=SC.BETA)  # noqa: E731
    z0 = E64 @ W0.T + b0
    a0 = sp(z0)
    z1 = a0 @ W1.T + b1
    a1 = sp(z1)
    sdf = a1 @ w2 + b2
    z0.retain_grad(); z1.retain_grad()
    (sdf * g.double()).sum().backward()
    S = SC.sdf_chain(ws, E, g, SC.BETA, "float64")
    rel = lambda a, b: float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)  # noqa: E731
    want = {"sdf": sdf, "a0": a0, "a1": a1, "dz1": z1.grad, "dz0": z0.grad, "dE": E64.grad, "dw2": w2.grad, "db2": b2.grad}
    for k, v in want.items():
        assert S[k].shape == v.shape and rel(S[k], v.detach()) < 1e-12, k
    for k, v in {"dW1": W1.grad, "db1": b1.grad, "dW0": W0.grad, "db0": b0.grad}.items():
        assert rel(S["grads"][k], v) < 1e-12, k
    assert torch.equal(S["gmax"], torch.stack([S["dz1"].abs().max(), S["dz0"].abs().max()]))
    assert rel(S["sum_abs"]["dw2"], (g.double()[:, None] * a1.detach()).abs().sum(0)) < 1e-12


# ------------------------------------------------------------------------------------------------------------------ launch plans
@pytest.mark.parametrize("cus", PLAN_CUS)
def test_tail_plan_covers_every_tile_exactly_once(cus):
    """every n_tiles of 1 .. 17 cus; the walk is the kernels': every wave of every workgroup of the grid asks tail_tile for its tile"""
    counts = list(range(1, 17 * cus + 1))
    wave = torch.arange(8)
    for n in counts:
        full, tail, k = SC.tail_plan(n, cus)
        assert (tail == 0) == (k == 0) and 0 <= k <= 7
        # tail workgroups first: block b < tail holds tiles 8 full + b k + wave for wave < k; block b >= tail holds (b - tail) 8 + wave
        tb = torch.arange(tail)[:, None]
        t_tail = 8 * full + tb * k + wave[None, :]
        t_tail = t_tail[(wave[None, :] < k).expand_as(t_tail) & (t_tail < n)]
        t_full = (torch.arange(full)[:, None] * 8 + wave[None, :]).flatten()
        t_full = t_full[t_full < n]
        seen = torch.bincount(torch.cat([t_tail, t_full]), minlength=n)
        assert seen.numel() == n and bool((seen == 1).all()), (cus, n, full, tail, k)
    # the vectorised walk above is tail_tile's: compared wave by wave at the first counts
    for n in counts[:min(len(counts), 40)] + counts[-3:]:
        full, tail, k = SC.tail_plan(n, cus)
        walked = sorted(t for b in range(full + tail) for w in range(8) for t in [SC.tail_tile(full, tail, k, n, b, w)] if 0 <= t < n)
        assert walked == list(range(n)), (cus, n)


def test_production_plan():
    """263 456 DDF rows on 256 CUs: 1024 full workgroups behind 41 one-wave tail workgroups (chain.h)"""
    assert SC.tail_plan((263456 + 31) // 32, 256) == (1024, 41, 1)


@pytest.mark.parametrize("cus", PLAN_CUS)
def test_plan_rows_land_in_their_class(cus):
    rows = SC.plan_rows(cus)
    for name, (cls, M) in rows.items():
        n = (M + 31) // 32
        assert SC.plan_class(n, cus) == cls and name.startswith(cls[:2]), (cus, name, M, SC.tail_plan(n, cus))
        assert (M % 32 != 0) == (cls != "P4")
    assert set(rows) == ({"P1", "P2:2", "P2:5", "P2:7", "P3", "P4", "P5:1", "P5:41"} if cus >= 2 else {"P1", "P3", "P4", "P5:1", "P5:41"})
    n = lambda name: (rows[name][1] + 31) // 32  # noqa: E731
    assert n("P1") <= cus and 7 * cus <= n("P3") < 8 * cus and n("P3") % 8 and n("P4") == 8 * cus
    assert n("P5:1") == 8 * cus + 1 and n("P5:41") == 8 * cus + 41
    for k in (2, 5, 7):
        if cus >= 2:
            assert SC.tail_plan(n(f"P2:{k}"), cus)[2] == k and n(f"P2:{k}") % k
    assert (SC.chunk_rows(cus) + 31) // 32 <= cus and SC.plan_class((SC.chunk_rows(cus) + 31) // 32, cus) == "P1"
    if cus == 256:
        assert max(M for _, M in rows.values()) == 66843 and SC.tail_plan(n("P5:41"), cus) == (256, 41, 1)


# ------------------------------------------------------------------------------------------------------------------ the bars bite
def _fed(defect):
    """the quantity groups a defect feeds directly: the first stored downstream of it and the parameter gradients formed from them"""
    return {"fwd0": ["a0", "grad:dW1"], "fwd1": ["a1", "sdf", "dw2"], "bwd1": ["dz0", "grad:dW0", "grad:db0"], "bwd0": ["dE"],
            "beta": ["dz1", "dz0", "grad:dW1", "grad:db1", "grad:dW0", "grad:db0"], "threshold": ["a0", "a1", "sdf"]}[defect]


@pytest.mark.parametrize("in_dim,M,steep", SC.all_shapes())
def test_undamaged_emulation_is_below_every_bar(in_dim, M, steep):
    ws, E, g = _case(in_dim, M, steep)
    ref, bar = _ref_and_bars(in_dim, M, steep)
    r = SC.ratios(SC.sdf_chain(ws, E, g, SC.BETA, "split"), ref, bar)
    worst = max(r, key=r.get)
    print(f"undamaged emulation in_dim={in_dim} M={M} steep={steep}: worst err/bar {r[worst]:.3f} ({worst})")
    assert all(v < 1.0 for v in r.values()), {k: round(v, 3) for k, v in r.items() if not v < 1.0}


@pytest.mark.parametrize("defect", SC.PRODUCTS + SC.CONSTANT_DEFECTS)
def test_injected_defect_is_caught(defect):
    """the DDF-sized case.  A product loses its (weight residual) x (activation hi) term; beta is off by 1e-3 where the sigmoid is
    recovered from the saved output; the softplus is log(1 + exp(beta z)) / beta at every beta z (in float32 that is inf from beta z = 88.8
    on, and the case has pre-activations beyond it: a group that holds an inf or a NaN is over its bar).  The overflow-safe form without
    the branch, (max(beta z, 0) + log1p(exp(-|beta z|))) / beta, is NOT a defect these bars can see and is not asked of them: above the
    threshold it differs from z by exp(-20) / beta = 2e-11 and two float32 roundings; measured here a0 0.081 against 0.075 undamaged"""
    in_dim, M = SC.DEFECT_CASE
    ws, E, g = _case(in_dim, M)
    ref, bar = _ref_and_bars(in_dim, M)
    r = SC.ratios(SC.sdf_chain(ws, E, g, SC.BETA, "split", defect=defect), ref, bar)
    fed = {k: r[k] for k in _fed(defect)}
    over = {k: v for k, v in fed.items() if not v <= 1.0}
    print(f"defect {defect}: err/bar of the groups it feeds " + " ".join(f"{k}={v:.2f}" for k, v in fed.items()))
    assert over, (defect, fed)


def test_case_spans_both_softplus_branches():
    """beta z on either side of the threshold 20 and far into the exponential tail, in both hidden layers; the steep set beyond +-88"""
    for steep, reach in ((False, 20.0), (True, 88.8)):
        ws, E, g = _case(SC.DDF_DIM, 257, steep)
        W0, b0, W1, b1 = (t.double() for t in ws[:4])
        z0 = E.double() @ W0.T + b0
        z1 = torch.nn.functional.softplus(z0, beta=SC.BETA) @ W1.T + b1
        for z in (z0, z1):
            bz = SC.BETA * z
            assert float(bz.max()) > reach and float(bz.min()) < -reach and bool(((bz > 0) & (bz < 20)).any())
