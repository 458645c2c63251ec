"""Radiance transfer on the CPU: the float64 restatement (transfer_cpu.py) against the oracle's renderer, the package's scaled-fp16
packing, save / load, and the command line's --transfer option."""
import numpy as np
import pytest
import torch

import transfer_cpu as TC
from oracle import neusky_oracle as O
from neusky_amd.relight import transfer as X


@pytest.mark.parametrize("D", [42, 512])
@pytest.mark.parametrize("with_vis", [True, False])
def test_restatement_matches_the_oracle_renderer(D, with_vis):
    R, S = 12, 17
    albedo, normals, weights, dirs, vis = (None if t is None else t.double() for t in TC.random_inputs(R, S, D, 11 + D, with_vis))
    lights, bg = (t.double() for t in TC.random_lights(2, D, R, 5, sun=True))
    assert lights.max() == 3.0e4
    cos = torch.einsum("rsi,di->rsd", normals, dirs).clamp(0, 1)
    assert ((cos > 0).sum(-1) == 0).any(), "no sample faces no direction"
    T, acc = TC.transfer(albedo, normals, weights, dirs, vis)
    assert acc[0] == 0.0 and acc[1] == 1.0
    got = TC.relit(T, acc, lights, bg)
    for k in range(2):
        ref = O.lambertian_render(albedo, normals, dirs, lights[k][None], torch.zeros(R, dtype=torch.long), vis, bg[k], weights,
                                  training=False)
        assert (got[k] - ref).abs().max().item() <= 1e-12
    # the linear values too (the sun saturates sRGB): the oracle's composite before its tone curve
    dot = cos / torch.where((cos > 0).sum(-1, keepdim=True) > 0, (cos > 0).double().sum(-1, keepdim=True), torch.ones(R, S, 1).double())
    if vis is not None:
        dot = dot * vis[:, None, :]
    comp = (weights[..., None] * albedo * torch.einsum("rsj,jc->rsc", dot, lights[0])).sum(-2) + bg[0] * (1 - weights.sum(-1, keepdim=True))
    lin = TC.relit_linear(T, acc, lights, bg)[0]
    assert ((lin - comp).abs() / comp.abs().clamp_min(1.0)).max().item() <= 1e-12


def _rows():
    g = torch.Generator().manual_seed(3)
    T = torch.rand(6, 40, 3, generator=g, dtype=torch.float64) ** 3
    T[0] *= 1e-3
    T[1] = 0.0
    T[2] *= 1e-9 / T[2].max()
    T[3] *= 37.0
    T[4, 1:] *= 1e-7  # one large entry over a tiny row
    return T


def test_pack_round_trip_is_within_half_precision_of_the_row_maximum():
    T = _rows()
    half, e = X.pack_fp16(T)
    assert half.dtype == torch.float16 and e.dtype == torch.int32 and e.shape == (6,)
    back = X.unpack_fp16(half, e, torch.float64)
    mx = T.reshape(6, -1).abs().amax(1)
    err = (back - T).abs().reshape(6, -1).amax(1)
    assert (err <= 2.0 ** -11 * mx).all(), (err / mx.clamp_min(1e-300)).tolist()
    scaled_max = half.double().reshape(6, -1).abs().amax(1)
    live = mx > 0
    assert ((scaled_max[live] >= 0.5) & (scaled_max[live] <= 1.0)).all()
    # the package's packing is the restatement's
    h2, e2 = TC.pack_fp16(T.numpy())
    assert np.array_equal(h2.view(np.uint16), half.numpy().view(np.uint16)) and np.array_equal(e2, e.numpy())
    assert np.array_equal(TC.unpack_fp16(h2, e2), back.numpy())


def test_pack_keeps_a_zero_row_and_a_tiny_row():
    T = _rows()
    half, e = X.pack_fp16(T)
    assert e[1] == 0 and (half[1] == 0).all()
    assert (X.unpack_fp16(half, e, torch.float64)[1] == 0).all()
    back = X.unpack_fp16(half, e, torch.float64)[2]
    assert back.max().item() == pytest.approx(1e-9, rel=2.0 ** -11)
    assert ((back - T[2]).abs() <= 2.0 ** -11 * 1e-9 * (1 + 1e-12)).all()
    # unscaled fp16 would have lost the row
    assert (T[2].to(torch.float16) == 0).all()


@pytest.mark.parametrize("storage", ["fp32", "fp16"])
def test_save_load_round_trip(tmp_path, storage):
    g = torch.Generator().manual_seed(9)
    H, W, D = 3, 4, 8
    R = H * W
    T = torch.rand(R, D, 3, generator=g)
    exps = None
    if storage == "fp16":
        T, exps = X.pack_fp16(T)
    outputs = {k: torch.rand(H, W, 3 if k in ("albedo", "normal") else 1, generator=g) for k in X.FRAME_KEYS}
    a = X.RadianceTransfer(T, exps, torch.rand(R, generator=g), torch.randn(D, 3, generator=g), torch.randn(R, 3, generator=g), (H, W),
                           outputs, camera_index=2)
    a.save(tmp_path / "frame.pt")
    b = X.RadianceTransfer.load(tmp_path / "frame.pt", "cpu")
    assert b.storage == storage and b.shape == (H, W) and b.camera_index == 2
    assert torch.equal(a.T, b.T) and torch.equal(a.acc, b.acc) and torch.equal(a.dirs, b.dirs)
    assert torch.equal(a.ray_directions, b.ray_directions)
    assert (a.exponents is None and b.exponents is None) or torch.equal(a.exponents, b.exponents)
    assert a.outputs.keys() == b.outputs.keys() and all(torch.equal(a.outputs[k], b.outputs[k]) for k in a.outputs)
    assert torch.equal(a.dense(), b.dense())


def test_constructor_rejects_mismatched_parts():
    T = torch.zeros(6, 4, 3)
    with pytest.raises(ValueError):
        X.RadianceTransfer(T.half(), None, torch.zeros(6), torch.zeros(4, 3), torch.zeros(6, 3), (2, 3), {})
    with pytest.raises(ValueError):
        X.RadianceTransfer(T, None, torch.zeros(6), torch.zeros(4, 3), torch.zeros(6, 3), (2, 2), {})


def test_command_line_parses_transfer():
    from neusky_amd.relight.__main__ import build_parser
    base = ["--checkpoint", "c", "--camera-path", "p", "--output-dir", "o", "--latent-index", "0"]
    ap = build_parser()
    assert ap.parse_args(base).transfer == "off"
    assert ap.parse_args(base + ["--transfer", "fp16"]).transfer == "fp16"
    assert ap.parse_args(base + ["--transfer", "fp32", "--turntable", "4"]).transfer == "fp32"
    with pytest.raises(SystemExit):
        ap.parse_args(base + ["--transfer", "bf16"])
