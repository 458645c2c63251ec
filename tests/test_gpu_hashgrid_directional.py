"""The directional mode of the hash-grid encode (nsky_encode_fwd_dir / nsky_encode_bwd_dir: ONE tangent row-set Td = sum_a d_a T_a
along a per-ray direction) against the existing three-row mode: forward, the float64 contraction of the three tangent rows that mode
writes (test_gpu_hashgrid.py's tangent bar: 5e-4 of the largest tangent entry); backward, the table gradient of the existing call fed
dT_a = d_a dTd (test_gpu_hashgrid_owner.py's bar per entry, C_LATTICE (A_e + |base_e|); the LDS / L2 atomics' order varies, so no bit
equality).  P = 1, 65 (a second 64-point block), 4099: the direct scatter; 33001: the chunk owners behind the directional pack."""
import pytest
import torch

import hashgrid_bwd_cpu as HB
from oracle import neusky_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODE, PE = 1, 6  # the SDF field's call: L-infinity contraction, smoothstep, [x | PE6 | hash]


def _setup(P, spr, seed):
    from neusky_amd.encoding import HashGridGeometry
    cfg = O.HashGridCfg(smoothstep=True)
    geom = HashGridGeometry(smoothstep=True)
    assert geom.offsets == cfg.offsets and geom.resolutions == cfg.resolutions
    g = torch.Generator().manual_seed(seed)
    table = (torch.rand(geom.n_params, 2, generator=g) * 2 - 1) * 0.5
    x = (torch.rand(P, 3, generator=g) * 2 - 1) * 1.3
    assert P % spr == 0
    dirs = torch.nn.functional.normalize(torch.randn(P // spr, 3, generator=g), dim=-1)
    width = 3 + 6 * PE + 2 * geom.n_levels
    return cfg, geom, g, table, x, dirs, width, (width + 3) // 4 * 4


@pytest.mark.parametrize("P,spr", [(1, 1), (65, 1), (65, 13), (4099, 1), (4096, 96 // 3)])
def test_directional_row_is_the_contraction_of_the_three_tangent_rows(P, spr):
    from neusky_amd import hip
    cfg, geom, g, table, x, dirs, width, ldy = _setup(P, spr, 31)
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)  # noqa: E731
    Y, T = nan(P, ldy), nan(3, P, ldy)
    hip.encode_fwd(geom, table.to(DEV), x.to(DEV), MODE, True, PE, 5.0, Y, T)
    both = nan(2 * P, ldy)
    hip.encode_fwd_dir(geom, table.to(DEV), x.to(DEV), MODE, True, PE, 5.0, dirs.to(DEV), both[:P], both[P:])
    torch.cuda.synchronize()
    assert torch.equal(both[:P], Y)  # the value rows: the same arithmetic
    d = dirs.double().repeat_interleave(spr, 0)  # point p takes direction p // spr
    want = (T.cpu().double() * d.t()[:, :, None]).sum(0)
    scale = T.cpu().double().abs().max().item()
    err = (both[P:].cpu().double() - want).abs().max().item()
    print(f"P {P}, spr {spr}: directional row max err {err:.3e} = {err / scale:.3e} of the largest tangent entry")
    assert err <= 5e-4 * scale, (err, scale)
    assert (both[P:, width:] == 0).all()


@pytest.mark.parametrize("P,spr", [(1, 1), (65, 1), (65, 5), (4099, 1), (33001, 1), (32800, 32)])
def test_directional_table_gradient_equals_the_three_row_call(P, spr):
    from neusky_amd import hip
    cfg, geom, g, table, x, dirs, width, ldy = _setup(P, spr, 32)
    feat0 = 3 + 6 * PE
    dY = torch.zeros(P, ldy); dY[:, :width] = torch.randn(P, width, generator=g)
    dTd = torch.zeros(P, ldy); dTd[:, :width] = torch.randn(P, width, generator=g)
    base = torch.randn(geom.n_params, 2, generator=g) * 1e-3
    d = dirs.repeat_interleave(spr, 0)
    dT = (d.t()[:, :, None] * dTd[None]).contiguous()  # dT_a = d_a dTd, one fp32 product each (as the kernels form it)
    a, b = base.to(DEV), base.to(DEV)
    hip.encode_bwd(geom, table.to(DEV), x.to(DEV), MODE, True, PE, 5.0, dY.to(DEV), dT.to(DEV), a, None)
    hip.encode_bwd_dir(geom, table.to(DEV), x.to(DEV), MODE, True, PE, 5.0, dirs.to(DEV), dY.to(DEV), dTd.to(DEV), b)
    torch.cuda.synchronize()
    _, A = HB.table_gradient(x, MODE, cfg, dY[:, feat0:width], dT[:, :, feat0:width])
    a, b = a.cpu(), b.cpu()
    # (off the lattice the fp32 position of a point on a cell face may land in the neighbouring cell of the float64 restatement: entries
    # with A = 0 can receive such a point's term, in both calls alike -- the same single fp32 term, so the two agree there to the bit)
    stray = (A == 0) & (b != base)
    print(f"P {P}, spr {spr}: entries outside the float64 footprint written: {int(stray.sum())}")
    assert (A > 0).any() and torch.equal(b[A == 0], a[A == 0]), "the two calls differ on an entry outside the float64 footprint"
    assert int(stray.sum()) <= 64, int(stray.sum())
    room = A + base.double().abs()
    diff = (a.double() - b.double()).abs()
    ratio = (diff[room > 0] / room[room > 0]).max().item()
    print(f"P {P}, spr {spr}: max |directional - three-row| / (A + |base|) = {ratio:.3e}; bit-equal: {bool(torch.equal(a, b))}")
    assert not (diff > HB.C_LATTICE * room).any(), ratio
