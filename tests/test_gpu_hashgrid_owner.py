"""The hash-grid table gradient (nsky_encode_bwd: the chunk-owner kernel from 32 768 points on, the direct scatter below) against
the float64 restatement of hashgrid_bwd_cpu.py, entry by entry, accumulated into a table that is not zero.

The lattice cases run on the 4-level geometry g4 (integral scales: t has no fp32 rounding, test_hashgrid_bwd_cpu.py asserts it), so
what is measured is the kernel's weight arithmetic and its accumulation; the crowded ones drive the owner's phases down to 1024,
512 and 256 bitmap words (test_hashgrid_bwd_cpu.py asserts which input takes which).  Bound per entry e:
    |got_e - base_e - G_e| <= C_LATTICE * (A_e + |base_e|),    entries no point touches: bit-equal to base,
A_e the sum of the absolute values of the terms that entry received.  Off the lattice t carries ~scale * 2^-24 of a cell, so the
real geometry is judged per level: max_e |err_e| <= C_LEVEL * max_e A_e over the level's slab, each of the 16 levels by itself.
The bars are 4 x the largest figure measured on an MI355X against the restatement (the order of the LDS and L2 atomics changes
from run to run); measured figures stand beside them."""
import pytest
import torch

import hashgrid_bwd_cpu as HB
from oracle import neusky_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

C_LATTICE = HB.C_LATTICE  # 1.6e-6 = 4 x 4.00e-7 measured (shared with the CPU test that injects defects)
# Off the lattice a level's error is the fp32 rounding of t, ~scale_l * 2^-24 of a cell, so every level has its own bar: 4 x the
# larger of the two figures measured (modes 1 and 2), and never above test_gpu_hashgrid.py's 5e-4.  Measured, levels 0 .. 15:
MEASURED_LEVEL = [2.51e-7, 6.16e-7, 1.08e-6, 1.83e-6, 3.92e-6, 5.97e-6, 1.11e-5, 1.46e-5,
                  2.45e-5, 3.28e-5, 5.57e-5, 5.64e-5, 9.36e-5, 1.10e-4, 1.49e-4, 2.19e-4]
# (levels 14 and 15: 4 x the measurement would be 5.96e-4 and 8.6e-4 -- the ceiling holds, they keep 3.4 x and 2.3 x.  What is
# measured there is t's rounding, the same from run to run, not the order of the atomics.)
C_LEVEL = [min(4.0 * m, 5e-4) for m in MEASURED_LEVEL]
C_DX = 5e-4       # input gradient: test_gpu_hashgrid.py's bar, of the largest |dx| (measured: 8.3e-6 and below)


def _inputs(cfg, x, mode, with_t, seed):
    P = x.shape[0]
    g = torch.Generator().manual_seed(seed)
    table = (torch.rand(cfg.n_params, 2, generator=g) * 2 - 1) * 0.5
    pe = 6 if mode else 0  # the fields' rows: [x | PE6 | hash] (hash columns from the odd column 39) and the DDF's [x | hash]
    feat0 = 3 + 6 * pe
    width = feat0 + 2 * cfg.n_levels
    ldy = (width + 3) // 4 * 4
    dY = torch.zeros(P, ldy); dY[:, :width] = torch.randn(P, width, generator=g)
    dT = None
    if with_t:
        dT = torch.zeros(3, P, ldy); dT[:, :, :width] = torch.randn(3, P, width, generator=g)
    base = torch.randn(cfg.n_params, 2, generator=g) * 1e-3
    return table, pe, feat0, width, dY, dT, base


def _launch(cfg, x, mode, table, pe, dY, dT, base):
    """-> the table gradient accumulated into base, and dx (fp32, cpu)"""
    from neusky_amd import hip
    from neusky_amd.encoding import HashGridGeometry
    geom = HashGridGeometry(n_levels=cfg.n_levels, log2_hashmap_size=cfg.log2_hashmap_size, base_res=cfg.base_res, max_res=cfg.max_res,
                            smoothstep=cfg.smoothstep)
    assert geom.offsets == cfg.offsets and geom.resolutions == cfg.resolutions and geom.scales == cfg.scales
    got = base.to(DEV)
    dx = torch.full((x.shape[0], 3), float("nan"), device=DEV)
    hip.encode_bwd(geom, table.to(DEV), x.to(DEV), mode, True, pe, 5.0, dY.to(DEV), None if dT is None else dT.to(DEV), got, dx,
                   workspace="auto")
    return got.cpu(), dx.cpu()


def _run(cfg, x, mode, with_t, seed):
    """-> err [n_params,2] = got - base - G (float64), A, base, got (fp32, cpu); asserts the input gradient on the way"""
    table, pe, feat0, width, dY, dT, base = _inputs(cfg, x, mode, with_t, seed)
    got, dx = _launch(cfg, x, mode, table, pe, dY, dT, base)

    G, A = HB.table_gradient(x, mode, cfg, dY[:, feat0:width], None if dT is None else dT[:, :, feat0:width])

    xd = x.double().requires_grad_(True)
    pos = xd if mode == 0 else (O.scene_contraction(xd, float("inf") if mode == 1 else 2) + 2.0) / 4.0
    parts = [xd] + ([O.nerf_encoding(xd, 6, 0.0, 5.0, False)] if pe else []) + [O.hash_grid_encode(pos, table.double(), cfg)]
    gx = torch.autograd.grad((torch.cat(parts, -1) * dY[:, :width].double()).sum(), xd)[0]
    ex, sx = (dx.double() - gx).abs().max().item(), gx.abs().max().item()
    print(f"dx: max err {ex:.3e} = {ex / sx:.3e} of the largest entry")
    assert ex <= C_DX * sx, (ex, sx)
    return got.double() - base.double() - G, A, base, got


def _check_entries(err, A, base, got):
    room = A + base.double().abs()
    ratio = (err.abs()[room > 0] / room[room > 0]).max().item()
    print(f"table: max |err| / (A + |base|) = {ratio:.3e}; touched entries {int((A > 0).sum())}")
    assert (A > 0).any()
    assert torch.equal(got[A == 0], base[A == 0]), "an entry no point touches was written"
    bad = err.abs() > C_LATTICE * room
    assert not bad.any(), (int(bad.sum()), ratio)


def _lattice_case(P, f, mode):
    smooth = with_t = mode == 1
    return _run(HB.g4_cfg(smooth), HB.lattice_points(P, f), mode, with_t, seed=21)


# mode 1, smoothstep, tangents: the SDF field's call.  f = 0: 2048-word phases only; 0.35 / 0.7 / 1.0: down to 1024 / 512 / 256
@pytest.mark.parametrize("f", [0.0, 0.35, 0.7, 1.0])
def test_crowded_lattice_points_contracted_with_tangents(f):
    _check_entries(*_lattice_case(66600, f, 1))


# mode 0, no smoothstep, no tangents: the DDF's call.  Negative x: cell -1 (the x + 1 carry into the chunk bits) on the hashed
# levels, cells that are "not inside" on the dense ones
@pytest.mark.parametrize("f", [0.0, 1.0])
def test_crowded_lattice_points_raw(f):
    _check_entries(*_lattice_case(66600, f, 0))


# one point below the owner threshold (the direct scatter: same reference, same bound), the threshold, a partial 1024-point
# block, exactly one full phase, and one point into a second phase with a partial last bitmap word
@pytest.mark.parametrize("P", [32767, 32768, 32800, 65536, 65569])
def test_point_count_edges(P):
    _check_entries(*_lattice_case(P, 0.0, 1))


# the step's geometry (L = 16, T = 2^19, 16 -> 2048), points off the lattice, both contractions
@pytest.mark.parametrize("mode", [1, 2])
def test_real_geometry_per_level(mode):
    cfg = O.HashGridCfg(smoothstep=True)
    g = torch.Generator().manual_seed(22)
    x = (torch.rand(32808, 3, generator=g) * 2 - 1) * 1.3
    err, A, base, got = _run(cfg, x, mode, True, seed=23)
    worst = 0.0
    for l in range(cfg.n_levels):
        sl = slice(cfg.offsets[l], cfg.offsets[l + 1])
        e, a = err[sl].abs().max().item(), A[sl].max().item()
        assert a > 0
        print(f"level {l:2d}: max |err| {e:.3e} = {e / a:.3e} of max A")
        worst = max(worst, e / a)
    print(f"worst level: {worst:.3e}")
    for l in range(cfg.n_levels):
        sl = slice(cfg.offsets[l], cfg.offsets[l + 1])
        assert err[sl].abs().max().item() <= C_LEVEL[l] * A[sl].max().item(), l
