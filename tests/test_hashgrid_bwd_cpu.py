"""The float64 restatement of the hash-grid table gradient (hashgrid_bwd_cpu.py) against the oracle's autograd, and the proofs
the GPU tests of the chunk-owner kernel (test_gpu_hashgrid_owner.py) rest on: their lattice inputs are exact in fp32, they reach
the owner's phase-shrinking branches, and their per-entry bound notices a skipped slice, a lost corner or one lost point."""
import functools

import numpy as np
import pytest
import torch

import hashgrid_bwd_cpu as HB
from oracle import neusky_oracle as O

P_CROWD = 66600


def _cfg8(smooth):
    return O.HashGridCfg(n_levels=8, log2_hashmap_size=14, max_res=256, smoothstep=smooth)


@pytest.mark.parametrize("geometry", ["g4", "l8"])
@pytest.mark.parametrize("with_t", [False, True])
@pytest.mark.parametrize("smooth", [False, True])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_restatement_equals_autograd(mode, smooth, with_t, geometry):
    cfg = HB.g4_cfg(smooth) if geometry == "g4" else _cfg8(smooth)
    g = torch.Generator().manual_seed(5)
    P, W = 64, 2 * cfg.n_levels
    x = ((torch.rand(P, 3, generator=g) * 2 - 1) * (1.0 if mode == 0 else 1.3)).double()
    # away from where the contraction is not differentiable: the unit sphere of its norm, and ties of the largest |x_i|
    m = x.abs().max(-1).values if mode == 1 else x.norm(dim=-1)
    assert mode == 0 or ((m - 1).abs().min() > 1e-4 and (m < 1).any() and (m > 1).any())
    srt = x.abs().sort(-1).values
    assert mode != 1 or (srt[:, 2] - srt[:, 1]).min() > 1e-5
    table = (torch.rand(cfg.n_params, 2, generator=g) * 2 - 1).double()
    dY = torch.randn(P, W, generator=g).double()
    dT = torch.randn(3, P, W, generator=g).double() if with_t else None
    G, A = HB.table_gradient(x, mode, cfg, dY, dT, smoothstep=smooth)
    ref, _ = HB.autograd_table_gradient(x, mode, cfg, table, dY, dT)
    assert (A >= G.abs() * (1 - 1e-12)).all()
    for l in range(cfg.n_levels):
        sl = slice(cfg.offsets[l], cfg.offsets[l + 1])
        scale = ref[sl].abs().max().item()
        assert scale > 0
        assert (G[sl] - ref[sl]).abs().max().item() <= 1e-10 * scale, (l, (G[sl] - ref[sl]).abs().max().item(), scale)


def test_g4_lattice_is_exact_in_fp32():
    """x = k / 2048: q = fmaf(scale, pos, 0.5) has no rounding at any of g4's four scales, so t is the same number on the GPU and
    here (mode 2: inside the unit ball, where the contraction is the identity)"""
    cfg = HB.g4_cfg(True)
    assert [float(np.float32(s)) for s in cfg.scales] == [15.0, 63.0, 255.0, 1023.0]
    assert cfg.resolutions == [16, 64, 256, 1024]
    assert [cfg.offsets[l + 1] - cfg.offsets[l] for l in range(4)] == [16 ** 3, 64 ** 3, 1 << 19, 1 << 19]
    k = torch.arange(-(HB.LATTICE - 1), HB.LATTICE)
    x1 = k.to(torch.float32) / HB.LATTICE
    assert torch.equal(x1.double() * HB.LATTICE, k.double())
    for f in (0.0, 0.7):
        x = HB.lattice_points(P_CROWD, f)
        assert x.abs().max() < 1 and torch.equal((x.double() * HB.LATTICE).round(), x.double() * HB.LATTICE)
        for mode in (0, 1, 2):
            xs = torch.cat([x, x1[:, None].expand(-1, 3)]) if mode != 2 else x[x.double().norm(dim=-1) < 1]
            assert xs.shape[0] > P_CROWD // 3
            pos32 = xs if mode == 0 else (xs + 2.0) * 0.25  # the kernel's fp32 arithmetic (no contraction inside the unit ball)
            pos64, _ = HB.grid_position(xs, mode)
            assert torch.equal(pos32.double(), pos64)
            for s in cfg.scales:
                q32 = (pos32.double() * float(np.float32(s)) + 0.5).to(torch.float32)  # exact product and sum, rounded once = fmaf
                assert torch.equal(q32.double(), pos64 * s + 0.5), (mode, s)


def test_owner_plan_on_g4():
    K = HB.owner_constants()
    assert K["OWN_CH"] == 1 << K["OWN_SHIFT"] and K["OWN_THREADS"] == 1024
    words, levels = HB.owner_plan(HB.g4_cfg(True), P_CROWD, K)
    assert words == 2112
    got = [(lv["level"], lv["dense"], lv["chunks"], lv["splits"]) for lv in levels]
    assert got == [(3, False, 32, 1), (2, False, 32, 2), (1, True, 16, 32), (0, True, 1, 64)]
    words, levels = HB.owner_plan(HB.g4_cfg(True), K["MIN_POINTS"], K)
    assert words == 1024 and levels[-1]["splits"] == 32  # the one-chunk level: capped by words / 32
    assert K["MIN_POINTS"] == 32768  # test_gpu_hashgrid_owner's P edges sit around it


@pytest.mark.parametrize("f,taken", [(0.0, {2048}), (0.35, {1024}), (0.7, {512}), (1.0, {256})])
def test_crowded_inputs_reach_the_phase_branches(f, taken):
    """the dispatch of encode_bwd_owner_kernel, restated, on the very inputs the GPU test runs (mode 1)"""
    ph = HB.owner_phases(HB.lattice_points(P_CROWD, f), 1, HB.g4_cfg(True))
    assert taken <= ph[3]["sizes"], ph[3]
    if f == 0.0:
        assert all(ph[l]["sizes"] == {2048} for l in range(4)), ph
    else:
        # a crowd leaves most z-slabs of the 64^3 level without a point: owners that return early, beside owners that work
        assert ph[1]["empty"] > 0 and ph[1]["busy"] > 0, ph[1]
    if f >= 0.7:  # the hashed level whose chunks' points are split over two workgroups shrinks too
        assert (512 if f == 0.7 else 256) in ph[2]["sizes"], ph[2]


def test_mode0_inputs_reach_the_carry_and_outside_paths():
    cfg, K = HB.g4_cfg(False), HB.owner_constants()
    x = HB.lattice_points(P_CROWD, 0.0)
    _, fl = O.hash_grid_indices(x.double(), cfg)
    pg = fl.to(torch.int64) & HB.M32
    for l in (2, 3):  # hashed: x + 1 carries into the chunk bits (cell -1)
        carry = (pg[:, l, 0] & (K["OWN_CH"] - 1)) == K["OWN_CH"] - 1
        assert carry.sum() > 0 and HB.owner_bitmaps(x, 0, cfg, l, K)[:, carry.numpy()].all()
    for l in (0, 1):  # dense: a negative cell is not inside
        outside = ~(pg[:, l] < cfg.resolutions[l] - 1).all(-1)
        assert 0 < outside.sum() < P_CROWD
    ph = HB.owner_phases(HB.lattice_points(P_CROWD, 1.0), 0, cfg, K)
    # mode 0 feeds x itself: the crowd spans 4 x 4 x 4 finest cells (more chunks, fewer points each) -- still shrunk phases
    assert 1024 in ph[3]["sizes"] and {512, 256} <= ph[2]["sizes"], ph


@functools.lru_cache(maxsize=None)
def _crowded_case(mode):
    smooth = with_t = mode == 1
    cfg = HB.g4_cfg(smooth)
    x = HB.lattice_points(P_CROWD, 0.7 if mode == 1 else 0.0)
    g = torch.Generator().manual_seed(7)
    dY = torch.randn(P_CROWD, 8, generator=g)
    dT = torch.randn(3, P_CROWD, 8, generator=g) if with_t else None
    return cfg, x, dY, dT, HB.table_gradient(x, mode, cfg, dY, dT)


@pytest.mark.parametrize("defect", ["slice", "tail", "carry_corner", "share_twice", "last_point"])
def test_the_bound_notices(defect):
    """defects an owner could have, injected into the restatement: each breaks the GPU test's per-entry bound tenfold somewhere"""
    mode = 0 if defect == "carry_corner" else 1
    cfg, x, dY, dT, (G, A) = _crowded_case(mode)
    K = HB.owner_constants()
    P = P_CROWD
    cs = torch.ones(P, 4, 8, dtype=torch.float64)
    if defect == "slice":           # one skipped 256-word slice of a phase on the finest level
        cs[8192:16384, 3] = 0
    elif defect == "tail":          # the points of the partial last bitmap word
        assert P % 32 > 0
        cs[P - P % 32:] = 0
    elif defect == "carry_corner":  # hashed levels: the x + 1 corner of a cell whose low 14 bits are all set (mode 0: cell -1)
        _, fl = O.hash_grid_indices(x.double(), cfg)
        pg0 = fl[..., 0].to(torch.int64) & HB.M32
        for l in (2, 3):
            hit = (pg0[:, l] & (K["OWN_CH"] - 1)) == K["OWN_CH"] - 1
            assert hit.any()
            for c in (1, 3, 5, 7):
                cs[hit, l, c] = 0
    elif defect == "share_twice":   # one workgroup's share of the points of the 64^3 level, counted twice
        words, levels = HB.owner_plan(cfg, P, K)
        lv = next(v for v in levels if v["level"] == 1)
        wper = -(-words // lv["splits"])
        cs[3 * wper * 32:4 * wper * 32, 1] = 2
    else:
        cs[P - 1] = 0
    Gd, _ = HB.table_gradient(x, mode, cfg, dY, dT, corner_scale=cs)
    excess = ((Gd - G).abs() - 10 * HB.C_LATTICE * A)
    assert (excess > 0).any(), defect
