"""csrc/transfer_sh.hip against the float64 restatement (transfer_sh_cpu.py), with a random basis so that any D and J run: the
projection in every pair of storages, its corners, and one 1080p-sized input whose flat indices cross 2^31; the relight of coefficient
rows for J in {1, 9, 36, 81} and K in {1, 3, 8, 9}, and one 1080p-sized call."""
import numpy as np
import pytest
import torch

import transfer_cpu as TC
import transfer_sh_cpu as SC
from neusky_amd import hip
from neusky_amd.relight import pack_fp16, unpack_fp16

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -24
HALF = 2.0 ** -11


def _stored(x64: torch.Tensor, storage: str):
    """(stored tensor, exponents or None, the float64 values it holds)"""
    if storage == "fp16":
        half, exps = pack_fp16(x64)
        return half, exps, unpack_fp16(half, exps, torch.float64)
    x = x64.float()
    return x, None, x.double()


def _project(T, exps, B, out_storage, rows=None, row0=0, fill=0):
    R, J = T.shape[0], B.shape[1]
    C = torch.full((rows or R, J, 3), fill, dtype=torch.float32 if out_storage == "fp32" else torch.float16, device=DEV)
    cexps = torch.full((rows or R,), -7, dtype=torch.int32, device=DEV) if out_storage == "fp16" else None
    hip.transfer_project(T.to(DEV), None if exps is None else exps.to(DEV), B.to(DEV), C, row0, cexps)
    return C, cexps


def _transfer_rows(R, D, seed):
    g = torch.Generator().manual_seed(seed)
    T = torch.rand(R, D, 3, generator=g, dtype=torch.float64) ** 3 * 1e-3  # the size of a baked row: weights / cnt
    T[3] = 0.0
    T[5] *= 1e-6
    return T


@pytest.mark.parametrize("J", [1, 9, 36, 81])
@pytest.mark.parametrize("D", [32, 42, 512, 1024])
def test_projection_matches_the_restatement(D, J):
    R = 37  # one partial tile
    T64 = _transfer_rows(R, D, 300 + D + J)
    B = torch.randn(D, J, generator=torch.Generator().manual_seed(D * 131 + J))
    for storage in ("fp32", "fp16"):
        T, exps, dense = _stored(T64, storage)
        ref = torch.from_numpy(SC.project(dense.numpy(), B.numpy()))
        mag = torch.from_numpy(SC.project_magnitude(dense.numpy(), B.numpy()))
        row_max = ref.reshape(R, -1).abs().amax(1)
        live = row_max > 0
        assert live.sum() == R - 1
        # fp32 coefficients
        C, _ = _project(T, exps, B, "fp32")
        err = (C.cpu().double() - ref).abs()
        print(f"project {storage}->fp32 D={D} J={J}: worst error / sum |T||B| {(err / mag.clamp_min(1e-300)).max().item():.3e} "
              f"(bound {D * EPS:.3e})")
        assert (err <= D * EPS * mag).all()
        assert (C[3] == 0).all()
        assert torch.equal(_project(T, exps, B, "fp32")[0], C)
        # scaled fp16 coefficients
        Ch, cexps = _project(T, exps, B, "fp16")
        back = unpack_fp16(Ch.cpu(), cexps.cpu(), torch.float64)
        err = (back - ref).abs()
        bound = D * EPS * mag + HALF * row_max[:, None, None]
        print(f"project {storage}->fp16 D={D} J={J}: worst error / bound {(err / bound.clamp_min(1e-300)).max().item():.3f}")
        assert (err <= bound).all()
        scaled_max = Ch.cpu().double().reshape(R, -1).abs().amax(1)
        assert ((scaled_max[live] >= 0.5) & (scaled_max[live] <= 1.0)).all()
        assert (cexps.cpu()[~live] == 0).all() and (Ch.cpu()[~live] == 0).all()
        again = _project(T, exps, B, "fp16")
        assert torch.equal(again[0], Ch) and torch.equal(again[1], cexps)


@pytest.mark.parametrize("out_storage", ["fp32", "fp16"])
def test_projection_writes_its_rows_of_a_larger_buffer(out_storage):
    T64 = _transfer_rows(6, 48, 1)
    B = torch.randn(48, 9, generator=torch.Generator().manual_seed(2))
    T = T64.float()
    alone, alone_exps = _project(T, None, B, out_storage)
    C, cexps = _project(T, None, B, out_storage, rows=13, row0=4)
    assert torch.equal(C[4:10], alone) and (C[:4] == 0).all() and (C[10:] == 0).all()
    if cexps is not None:
        assert torch.equal(cexps[4:10], alone_exps) and (cexps[:4] == -7).all() and (cexps[10:] == -7).all()
    with pytest.raises(ValueError):
        _project(T, None, B, out_storage, rows=8, row0=4)


@pytest.mark.parametrize("J", [36, 49, 81])
def test_projection_in_chunks_gives_the_bits_of_the_projection_at_once(J):
    # more rows than 256 tiles of 64: the kernel then takes larger tiles with fewer waves per row (one at J = 36, two at J = 49),
    # and a chunk of a bake does not.  A coefficient's bits must not depend on it.
    R, D = 64 * 256 + 37, 32
    g = torch.Generator().manual_seed(J)
    T = (torch.rand(R, D, 3, generator=g) ** 3 * 1e-3).to(DEV)
    B = torch.randn(D, J, generator=g).to(DEV)
    for out_storage in ("fp32", "fp16"):
        whole, whole_exps = _project(T, None, B, out_storage)
        parts, part_exps = _project(T[:5000], None, B, out_storage, rows=R)
        hip.transfer_project(T[5000:], None, B, parts, 5000, part_exps)
        assert torch.equal(parts, whole) and (part_exps is None or torch.equal(part_exps, whole_exps))
    rows = torch.cat([torch.arange(0, 70), torch.arange(R - 70, R)])
    whole = _project(T, None, B, "fp32")[0]
    ref = torch.einsum("rdc,dj->rjc", T[rows].double(), B.double())
    mag = torch.einsum("rdc,dj->rjc", T[rows].double().abs(), B.double().abs())
    assert ((whole[rows].double() - ref).abs() <= D * EPS * mag).all()


def test_projection_refuses_more_than_128_coefficients():
    T = torch.rand(4, 160, 3)
    with pytest.raises(ValueError):
        _project(T, None, torch.randn(160, 129), "fp32")
    C, _ = _project(T, None, torch.randn(160, 128, generator=torch.Generator().manual_seed(0)), "fp32")
    assert torch.isfinite(C).all()


def test_projection_at_full_frame_size_crosses_two_to_the_31():
    R, D, J = 2_073_600, 512, 9
    torch.manual_seed(4)
    T = torch.rand(R, D, 3, dtype=torch.float16, device=DEV)
    exps = torch.randint(0, 12, (R,), dtype=torch.int32, device=DEV)
    B = torch.randn(D, J, device=DEV)
    C = torch.empty(R, J, 3, device=DEV)
    hip.transfer_project(T, exps, B, C, 0, None)
    cross = (1 << 31) // (D * 3)  # the row that holds element 2^31
    assert cross * D * 3 < (1 << 31) < (cross + 1) * D * 3 < R * D * 3
    rows = torch.cat([torch.arange(0, 9), torch.arange(cross - 4, cross + 5), torch.arange(R - 9, R)]).to(DEV)
    dense = torch.ldexp(T[rows].double(), -exps[rows].double()[:, None, None])
    ref = torch.einsum("rdc,dj->rjc", dense, B.double())
    mag = torch.einsum("rdc,dj->rjc", dense.abs(), B.double().abs())
    err = (C[rows].double() - ref).abs()
    print(f"full-size projection: worst error / sum |T||B| {(err / mag).max().item():.3e} (bound {D * EPS:.3e})")
    assert (err <= D * EPS * mag).all()


def _coefficient_rows(R, J, seed):
    g = torch.Generator().manual_seed(seed)
    C = torch.randn(R, J, 3, generator=g, dtype=torch.float64) * torch.rand(R, 1, 1, generator=g, dtype=torch.float64) * 1e-2
    C[4] = 0.0
    acc = torch.rand(R, generator=g)
    acc[0], acc[1] = 0.0, 1.0
    return C, acc


def _short_lights(K, J, R, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(K, J, 3, generator=g) * 20.0, torch.rand(K, R, 3, generator=g) * 1.5


@pytest.mark.parametrize("storage", ["fp32", "fp16"])
@pytest.mark.parametrize("K", [1, 3, 8, 9])
@pytest.mark.parametrize("J", [1, 9, 36, 81])
def test_relight_of_coefficient_rows_matches_the_restatement(J, K, storage):
    R = 37  # one partial tile; 3 R J is no multiple of 4 for odd J: the last 16-byte load is a partial one
    C64, acc = _coefficient_rows(R, J, 7 + J)
    C, exps, dense = _stored(C64, storage)
    l, bg = _short_lights(K, J, R, 21 + K)  # noqa: E741
    rgb = torch.empty(K, R, 3, device=DEV)
    lin = torch.empty(K, R, 3, device=DEV)
    args = (C.to(DEV), None if exps is None else exps.to(DEV), acc.to(DEV), l.to(DEV), bg.to(DEV))
    hip.transfer_relight_short(*args, rgb, lin)
    ref = torch.from_numpy(SC.relit_linear(dense.numpy(), acc.numpy(), l.numpy(), bg.numpy()))
    mag = torch.from_numpy(SC.relit_magnitude(dense.numpy(), l.numpy(), bg.numpy()))
    q = 0.0 if storage == "fp32" else HALF
    err = (lin.cpu().double() - ref).abs()
    print(f"short relight {storage} J={J} K={K}: worst error / magnitude {(err / mag).max().item():.3e} (bound {J * EPS + q:.3e})")
    assert (err <= (J * EPS + q) * mag).all()
    assert (rgb.cpu().double() - TC.linear_to_srgb(lin.cpu().double())).abs().max().item() <= 2e-6
    rgb2 = torch.empty_like(rgb)
    hip.transfer_relight_short(*args, rgb2, None)
    assert torch.equal(rgb2, rgb)
    again = torch.empty_like(lin)
    hip.transfer_relight_short(*args, torch.empty_like(rgb), again)
    assert torch.equal(again, lin)


def test_relight_of_coefficient_rows_refuses_more_than_128():
    R = 4
    z = torch.zeros(1, R, 3, device=DEV)
    with pytest.raises(ValueError):
        hip.transfer_relight_short(torch.zeros(R, 129, 3, device=DEV), None, torch.zeros(R, device=DEV), torch.zeros(1, 129, 3, device=DEV),
                                   z, z.clone())
    C = torch.rand(R, 128, 3, device=DEV)
    l = torch.rand(2, 128, 3, device=DEV)  # noqa: E741
    lin = torch.empty(2, R, 3, device=DEV)
    hip.transfer_relight_short(C, None, torch.ones(R, device=DEV), l, torch.zeros(2, R, 3, device=DEV), torch.empty(2, R, 3, device=DEV), lin)
    ref = torch.einsum("rjc,kjc->krc", C.double(), l.double())
    assert ((lin.double() - ref).abs() <= 128 * EPS * ref).all()


def test_relight_of_coefficient_rows_at_full_frame_size():
    R, J = 2_073_600, 81
    torch.manual_seed(5)
    C = torch.rand(R, J, 3, dtype=torch.float16, device=DEV)
    exps = torch.randint(0, 12, (R,), dtype=torch.int32, device=DEV)
    acc = torch.rand(R, device=DEV)
    l = torch.rand(1, J, 3, device=DEV) * 2.0  # noqa: E741
    bg = torch.rand(1, R, 3, device=DEV)
    rgb = torch.empty(1, R, 3, device=DEV)
    lin = torch.empty(1, R, 3, device=DEV)
    hip.transfer_relight_short(C, exps, acc, l, bg, rgb, lin)
    rows = torch.cat([torch.arange(0, 9), torch.arange(R // 2 - 4, R // 2 + 5), torch.arange(R - 9, R)]).to(DEV)
    dense = torch.ldexp(C[rows].double(), -exps[rows].double()[:, None, None])
    ref = torch.einsum("rjc,jc->rc", dense, l[0].double()) + bg[0, rows].double() * (1.0 - acc[rows].double())[:, None]
    mag = torch.einsum("rjc,jc->rc", dense, l[0].double()) + bg[0, rows].double()
    err = (lin[0, rows].double() - ref).abs()
    print(f"full-size short relight: worst error / magnitude {(err / mag).max().item():.3e} (bound {J * EPS + HALF:.3e})")
    assert (err <= (J * EPS + HALF) * mag).all()
    assert (rgb[0, rows].double() - TC.linear_to_srgb(lin[0, rows].double())).abs().max().item() <= 2e-6
    assert np.isfinite(rgb.sum().item())


@pytest.mark.parametrize("D", [6, 8])
def test_projection_of_short_rows_onto_five_coefficients(D):
    """J = 5 is no multiple of the 4 coefficients a lane reads at a time; D = 6 takes the scalar loads of a block, D = 8 the 8- and
    16-byte ones; both storages in and out, the restatement and the bars of test_projection_matches_the_restatement"""
    test_projection_matches_the_restatement(D, 5)


@pytest.mark.parametrize("storage", ["fp32", "fp16"])
def test_relight_of_five_coefficients_under_nine_lights(storage):
    """a pass of 8 lights and a pass of one behind it over rows of 15 numbers (padded to 24 in LDS); the restatement and the bars of
    test_relight_of_coefficient_rows_matches_the_restatement"""
    test_relight_of_coefficient_rows_matches_the_restatement(5, 9, storage)
