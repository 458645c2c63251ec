"""csrc/transfer.hip against the float64 restatement (transfer_cpu.py): the bake in both storages, every shape corner, bitwise
repeatability; the relight for K in {1, 3, 8, 9}; and one 1080p-sized relight whose flat indices cross 2^31."""
import pytest
import torch

import transfer_cpu as TC
from neusky_amd import hip
from neusky_amd.relight import pack_fp16, unpack_fp16

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -24
HALF = 2.0 ** -11


def _bake(inputs, storage, rows=None, row0=0):
    albedo, normals, weights, dirs, vis = (None if t is None else t.to(DEV) for t in inputs)
    R, D = albedo.shape[0], dirs.shape[0]
    T = torch.zeros(rows or R, D, 3, dtype=torch.float32 if storage == "fp32" else torch.float16, device=DEV)
    acc = torch.empty(R, device=DEV)
    exps = torch.empty(R, dtype=torch.int32, device=DEV) if storage == "fp16" else None
    hip.transfer_bake(albedo, normals, weights, dirs, vis, T, row0, exps, acc)
    return T, exps, acc


@pytest.mark.parametrize("with_vis", [True, False])
@pytest.mark.parametrize("S", [1, 96])
@pytest.mark.parametrize("D", [32, 42, 512, 1024])
def test_bake_matches_the_restatement(D, S, with_vis):
    R = 24
    inputs = TC.random_inputs(R, S, D, 100 + D + S, with_vis)
    ref, ref_acc = TC.transfer(*inputs)
    row_max = ref.reshape(R, -1).abs().amax(1)
    assert (row_max[2:] > 0).any()
    # fp32 storage
    T, _, acc = _bake(inputs, "fp32")
    err = (T.cpu().double() - ref).abs().reshape(R, -1).amax(1)
    worst = (err / row_max.clamp_min(1e-300)).max().item()
    acc_err = (acc.cpu().double() - ref_acc).abs().max().item()
    print(f"bake fp32 D={D} S={S} vis={with_vis}: worst element error / row maximum {worst:.3e} (bound {S * EPS:.3e}), acc {acc_err:.3e}")
    assert (err <= S * EPS * row_max).all()
    assert acc_err <= S * EPS
    again = _bake(inputs, "fp32")
    assert torch.equal(again[0], T) and torch.equal(again[2], acc)
    # scaled fp16 storage
    Th, exps, acc_h = _bake(inputs, "fp16")
    assert torch.equal(acc_h, acc)
    back = unpack_fp16(Th.cpu(), exps.cpu(), torch.float64)
    err = (back - ref).abs().reshape(R, -1).amax(1)
    worst = (err / row_max.clamp_min(1e-300)).max().item()
    print(f"bake fp16 D={D} S={S} vis={with_vis}: worst element error / row maximum {worst:.3e} (bound {HALF + S * EPS:.3e})")
    assert (err <= (HALF + S * EPS) * row_max).all()
    scaled_max = Th.cpu().double().reshape(R, -1).abs().amax(1)
    live = row_max > 0
    assert ((scaled_max[live] >= 0.5) & (scaled_max[live] <= 1.0)).all()
    assert (exps.cpu()[~live] == 0).all() and (Th.cpu()[~live] == 0).all()  # (ray 0 has zero weights: a row of zeros)
    again = _bake(inputs, "fp16")
    assert torch.equal(again[0], Th) and torch.equal(again[1], exps)


def test_bake_writes_its_rows_of_a_larger_buffer():
    inputs = TC.random_inputs(5, 7, 48, 1)
    alone = _bake(inputs, "fp32")[0]
    T, _, _ = _bake(inputs, "fp32", rows=12, row0=4)
    assert torch.equal(T[4:9], alone) and (T[:4] == 0).all() and (T[9:] == 0).all()
    with pytest.raises(ValueError):
        _bake(inputs, "fp32", rows=8, row0=4)


@pytest.mark.parametrize("storage", ["fp32", "fp16"])
@pytest.mark.parametrize("K", [1, 3, 8, 9])
@pytest.mark.parametrize("D", [42, 512, 1024])
def test_relight_matches_the_restatement(D, K, storage):
    R = 37  # not a multiple of the rows a wave takes
    inputs = TC.random_inputs(R, 9, D, 7 + D)
    T64, acc64 = TC.transfer(*inputs)
    exps = None
    if storage == "fp16":
        T, exps = pack_fp16(T64)
        dense = unpack_fp16(T, exps, torch.float64)
    else:
        T = T64.float()
        dense = T.double()
    acc = acc64.float()
    lights, bg = TC.random_lights(K, D, R, 21 + K)
    rgb = torch.empty(K, R, 3, device=DEV)
    lin = torch.empty(K, R, 3, device=DEV)
    args = (T.to(DEV), None if exps is None else exps.to(DEV), acc.to(DEV), lights.to(DEV), bg.to(DEV))
    hip.transfer_relight(*args, rgb, lin)
    ref = TC.relit_linear(dense, acc, lights, bg)
    mag = TC.relit_magnitude(dense, lights, bg)
    q = 0.0 if storage == "fp32" else HALF
    err = (lin.cpu().double() - ref).abs()
    print(f"relight {storage} D={D} K={K}: worst error / magnitude {(err / mag).max().item():.3e} (bound {D * EPS + q:.3e})")
    assert (err <= (D * EPS + q) * mag).all()
    # the tone curve of the same linear values
    assert (rgb.cpu().double() - TC.linear_to_srgb(lin.cpu().double())).abs().max().item() <= 2e-6
    rgb2 = torch.empty_like(rgb)
    hip.transfer_relight(*args, rgb2, None)
    assert torch.equal(rgb2, rgb)


def test_relight_at_full_frame_size_crosses_two_to_the_31():
    R, D = 2_073_600, 512
    torch.manual_seed(4)
    T = torch.rand(R, D, 3, dtype=torch.float16, device=DEV)
    exps = torch.randint(0, 12, (R,), dtype=torch.int32, device=DEV)
    acc = torch.rand(R, device=DEV)
    lights = torch.rand(1, D, 3, device=DEV) * 2.0
    bg = torch.rand(1, R, 3, device=DEV)
    rgb = torch.empty(1, R, 3, device=DEV)
    lin = torch.empty(1, R, 3, device=DEV)
    hip.transfer_relight(T, exps, acc, lights, bg, rgb, lin)
    cross = (1 << 31) // (D * 3)  # the row that holds element 2^31
    assert cross * D * 3 < (1 << 31) < (cross + 1) * D * 3 < R * D * 3
    rows = torch.cat([torch.arange(0, 9), torch.arange(cross - 4, cross + 5), torch.arange(R - 9, R)]).to(DEV)
    dense = torch.ldexp(T[rows].double(), -exps[rows].double()[:, None, None])
    ref = torch.einsum("rdc,dc->rc", dense, lights[0].double()) + bg[0, rows].double() * (1.0 - acc[rows].double())[:, None]
    mag = torch.einsum("rdc,dc->rc", dense, lights[0].double()) + bg[0, rows].double()
    err = (lin[0, rows].double() - ref).abs()
    print(f"full-size relight: worst error / magnitude {(err / mag).max().item():.3e} (bound {D * EPS + HALF:.3e})")
    assert (err <= (D * EPS + HALF) * mag).all()
    assert (rgb[0, rows].double() - TC.linear_to_srgb(lin[0, rows].double())).abs().max().item() <= 2e-6


@pytest.mark.parametrize("storage", ["fp32", "fp16"])
@pytest.mark.parametrize("D", [6, 8])
def test_relight_of_nine_lights_over_short_rows(D, storage):
    """a pass of 8 lights and a pass of one behind it, at the smallest rows of each kernel: D = 6 takes the any-D kernel in both storages,
    D = 8 the 16-byte one (two loads of a fp32 row, one of a fp16 row); the restatement and the bars of the test above"""
    test_relight_matches_the_restatement(D, 9, storage)
