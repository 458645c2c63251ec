"""The spherical-harmonic light basis on the CPU: the float64 restatement (transfer_sh_cpu.py) against closed forms and a quadrature, the
package's sh_basis / light_basis against the restatement, the identity a projected transfer rests on, and light_residual."""
import math

import numpy as np
import pytest
import torch

import transfer_sh_cpu as SC
from neusky_amd.model_components.illumination import antipodal_sphere
from neusky_amd.relight import SHRadianceTransfer, RadianceTransfer, light_basis, project_lights, sh_basis
from neusky_amd.relight import transfer as X


def _random_directions(n, seed):
    d = np.random.default_rng(seed).normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def test_restated_harmonics_equal_the_closed_forms_up_to_l_2():
    d = _random_directions(200, 0)
    d[0], d[1], d[2] = (0.0, 0.0, 1.0), (0.0, 0.0, -1.0), (1.0, 0.0, 0.0)  # the poles, where the azimuth is arbitrary
    x, y, z = d.T
    pi = math.pi
    closed = [0.5 / math.sqrt(pi) * np.ones_like(x),
              math.sqrt(3 / (4 * pi)) * y, math.sqrt(3 / (4 * pi)) * z, math.sqrt(3 / (4 * pi)) * x,
              0.5 * math.sqrt(15 / pi) * x * y, 0.5 * math.sqrt(15 / pi) * y * z, 0.25 * math.sqrt(5 / pi) * (3 * z * z - 1),
              0.5 * math.sqrt(15 / pi) * x * z, 0.5 * math.sqrt(15 / (4 * pi)) * (x * x - y * y)]
    Y = SC.real_sh(d, 2)
    assert Y.shape == (200, 9)
    for j, ref in enumerate(closed):
        assert np.abs(Y[:, j] - ref).max() <= 1e-14, j


def test_restated_harmonics_are_orthonormal_under_a_quadrature_exact_for_degree_16():
    # products of two harmonics of order <= 8 are polynomials of degree <= 16: 9 Gauss-Legendre nodes in z are exact to degree 17,
    # 17 equally spaced azimuths to every frequency <= 16
    zs, wz = np.polynomial.legendre.leggauss(9)
    phis = 2.0 * math.pi * np.arange(17) / 17
    zz, pp = np.meshgrid(zs, phis, indexing="ij")
    r = np.sqrt(1.0 - zz * zz)
    d = np.stack([r * np.cos(pp), r * np.sin(pp), zz], -1).reshape(-1, 3)
    w = np.repeat(wz, 17) * (2.0 * math.pi / 17)
    Y = SC.real_sh(d, 8)
    gram = Y.T @ (Y * w[:, None])
    assert np.abs(gram - np.eye(81)).max() <= 1e-12


def test_the_package_harmonics_equal_the_restatement():
    dirs = antipodal_sphere(512)
    Y = sh_basis(dirs, 8)
    assert Y.dtype == torch.float64 and Y.shape == (512, 81)
    assert np.abs(Y.numpy() - SC.real_sh(dirs.double().numpy(), 8)).max() <= 1e-12
    assert torch.equal(sh_basis(dirs, 3), Y[:, :16])  # column j = l (l + 1) + m: a lower order is a prefix


def test_light_basis_is_orthonormal_and_the_directions_resolve_order_8():
    dirs = antipodal_sphere(512)
    Q = light_basis(dirs, 8)
    assert Q.dtype == torch.float32 and Q.shape == (512, 81) and Q.is_contiguous()
    assert (Q.double().T @ Q.double() - torch.eye(81, dtype=torch.float64)).abs().max().item() <= 1e-6
    sv = np.linalg.svd(SC.real_sh(dirs.double().numpy(), 8), compute_uv=False)
    print(f"condition number of the harmonics up to order 8 on antipodal_sphere(512): {sv[0] / sv[-1]:.4f}")
    assert sv[0] / sv[-1] <= 1.2
    # the restatement's basis, and the same span as the harmonics
    ref = SC.light_basis(dirs.double().numpy(), 8)
    assert np.abs(Q.double().numpy() - ref).max() <= 1e-6
    Y = SC.real_sh(dirs.double().numpy(), 8)
    assert np.abs(ref @ (ref.T @ Y) - Y).max() <= 1e-12


def test_light_basis_refuses_what_the_directions_cannot_hold():
    with pytest.raises(ValueError, match="coefficients"):
        light_basis(antipodal_sphere(16), 4)  # J = 25 > D = 16
    with pytest.raises(ValueError, match="resolve"):
        light_basis(antipodal_sphere(16), 3)  # J = 16 = D, singular
    with pytest.raises(ValueError):
        light_basis(antipodal_sphere(512), 9)
    with pytest.raises(ValueError):
        light_basis(antipodal_sphere(512), -1)
    assert light_basis(antipodal_sphere(16), 0).shape == (16, 1)


@pytest.mark.parametrize("order", [0, 3, 8])
def test_a_band_limited_light_relights_exactly_from_the_coefficients(order):
    rng = np.random.default_rng(10 + order)
    dirs = antipodal_sphere(512).double().numpy()
    R, D, J = 9, 512, (order + 1) ** 2
    T = rng.random((R, D, 3)) ** 3
    acc = rng.random(R)
    bg = rng.random((2, R, 3))
    L = np.einsum("dj,kjc->kdc", SC.real_sh(dirs, order), rng.normal(size=(2, J, 3)))
    Q = SC.light_basis(dirs, order)
    C = SC.project(T, Q)
    l = np.einsum("dj,kdc->kjc", Q, L)  # noqa: E741
    got = SC.relit_linear(C, acc, l, bg)
    ref = np.einsum("rdc,kdc->krc", T, L) + bg * (1.0 - acc)[None, :, None]
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"order {order}: coefficient relight against dense relight, band-limited light: {err:.3e}")
    assert err <= 1e-11
    for k in range(2):
        assert SC.light_residual(Q, L[k]) <= 1e-6
    # the package's projection of the same lights, with its fp32 basis
    l32, residual = project_lights(light_basis(torch.from_numpy(dirs), order), torch.from_numpy(L))
    assert l32.dtype == torch.float32 and residual.shape == (2,) and (residual <= 1e-6).all()
    assert np.abs(l32.double().numpy() - l).max() <= 1e-5 * np.abs(l).max()


def test_light_residual_is_the_share_of_the_light_outside_the_basis():
    rng = np.random.default_rng(5)
    dirs = antipodal_sphere(512)
    Q32 = light_basis(dirs, 5)
    Q = Q32.double().numpy()
    inside = Q @ rng.normal(size=(36, 3))
    outside = rng.normal(size=(512, 3))
    outside -= Q @ np.linalg.solve(Q.T @ Q, Q.T @ outside)  # orthogonal to the (fp32) basis
    for share in (0.0, 0.05, 0.6):
        L = inside / np.linalg.norm(inside) * math.sqrt(1.0 - share ** 2) + outside / np.linalg.norm(outside) * share
        _, residual = project_lights(Q32, torch.from_numpy(L)[None])
        assert abs(residual.item() - share) <= 1e-6, (share, residual.item())
        assert abs(SC.light_residual(Q, L) - share) <= 1e-6
    _, zero = project_lights(Q32, torch.zeros(1, 512, 3))
    assert zero.item() == 0.0  # no light: nothing left out


def _frame(storage, g):
    H, W, D, order = 3, 4, 64, 2
    R, J = H * W, 9
    C = torch.rand(R, J, 3, generator=g)
    exps = None
    if storage == "fp16":
        C, exps = X.pack_fp16(C)
    outputs = {k: torch.rand(H, W, 3 if k in ("albedo", "normal") else 1, generator=g) for k in X.FRAME_KEYS}
    dirs = antipodal_sphere(D)
    return SHRadianceTransfer(C, exps, torch.rand(R, generator=g), light_basis(dirs, order), dirs, torch.randn(R, 3, generator=g), (H, W),
                              outputs, camera_index=2, order=order)


@pytest.mark.parametrize("storage", ["fp32", "fp16"])
def test_save_load_round_trip_and_each_loader_refuses_the_other_format(tmp_path, storage):
    g = torch.Generator().manual_seed(9)
    a = _frame(storage, g)
    assert a.storage == storage and a.order == 2 and a.nbytes == 12 * 9 * 3 * (4 if storage == "fp32" else 2)
    a.save(tmp_path / "sh.pt")
    b = SHRadianceTransfer.load(tmp_path / "sh.pt", "cpu")
    assert b.storage == storage and b.shape == (3, 4) and b.camera_index == 2 and b.order == 2
    for name in ("C", "acc", "Q", "dirs", "ray_directions"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert (a.exponents is None and b.exponents is None) or torch.equal(a.exponents, b.exponents)
    assert a.outputs.keys() == b.outputs.keys() and all(torch.equal(a.outputs[k], b.outputs[k]) for k in a.outputs)
    with pytest.raises(ValueError):
        RadianceTransfer.load(tmp_path / "sh.pt", "cpu")
    dense = RadianceTransfer(torch.rand(12, 64, 3, generator=g), None, a.acc, a.dirs, a.ray_directions, (3, 4), a.outputs)
    dense.save(tmp_path / "dense.pt")
    with pytest.raises(ValueError):
        SHRadianceTransfer.load(tmp_path / "dense.pt", "cpu")


SHARED_KEYS = ["format", "exponents", "acc", "dirs", "ray_directions", "shape", "camera_index", "outputs"]
FILES = {  # class: (file name, "format", keys of the saved dictionary, fields to compare after a load)
    RadianceTransfer: ("dense.pt", 1, SHARED_KEYS + ["T"], ["T", "exponents", "acc", "dirs", "ray_directions", "shape", "camera_index"]),
    SHRadianceTransfer: ("sh.pt", 2, SHARED_KEYS + ["C", "Q", "order"],
                         ["C", "exponents", "acc", "Q", "dirs", "ray_directions", "shape", "camera_index", "order"]),
}


@pytest.mark.parametrize("storage", ["fp32", "fp16"])
def test_the_two_file_formats_keep_their_keys(tmp_path, storage):
    """what a saved file holds is written out here, not read off the classes: format 1 and 2, their key sets, every field back after a
    load, and each loader's message for the other's file"""
    g = torch.Generator().manual_seed(3)
    sh = _frame(storage, g)
    T = torch.rand(12, 64, 3, generator=g)
    T, exps = X.pack_fp16(T) if storage == "fp16" else (T, None)
    dense = RadianceTransfer(T, exps, sh.acc, sh.dirs, sh.ray_directions, (3, 4), sh.outputs, camera_index=2)
    for frame in (dense, sh):
        name, fmt, keys, fields = FILES[type(frame)]
        frame.save(tmp_path / name)
        state = torch.load(tmp_path / name, map_location="cpu", weights_only=True)
        assert state["format"] == fmt and sorted(state) == sorted(keys)
        assert state["shape"] == [3, 4] and state["camera_index"] == 2 and sorted(state["outputs"]) == sorted(X.FRAME_KEYS)
        assert (state["exponents"] is None) == (storage == "fp32")
        back = type(frame).load(tmp_path / name, "cpu")
        assert type(back) is type(frame) and back.storage == storage
        for f in fields:
            a, b = getattr(frame, f), getattr(back, f)
            assert (a is None and b is None) or (torch.equal(a, b) if torch.is_tensor(a) else a == b), f
        assert all(torch.equal(frame.outputs[k], back.outputs[k]) for k in X.FRAME_KEYS)
    with pytest.raises(ValueError, match="dense.pt: not a saved SHRadianceTransfer"):
        SHRadianceTransfer.load(tmp_path / "dense.pt", "cpu")
    with pytest.raises(ValueError, match="sh.pt: not a saved RadianceTransfer"):
        RadianceTransfer.load(tmp_path / "sh.pt", "cpu")


def test_constructor_rejects_mismatched_parts():
    g = torch.Generator().manual_seed(1)
    a = _frame("fp32", g)
    with pytest.raises(ValueError):
        SHRadianceTransfer(a.C.half(), None, a.acc, a.Q, a.dirs, a.ray_directions, a.shape, {})
    with pytest.raises(ValueError):
        SHRadianceTransfer(a.C, None, a.acc, a.Q[:, :4], a.dirs, a.ray_directions, a.shape, {})


def test_command_line_parses_sh_order():
    from neusky_amd.relight.__main__ import build_parser, main
    base = ["--checkpoint", "c", "--camera-path", "p", "--output-dir", "o", "--latent-index", "0"]
    ap = build_parser()
    assert ap.parse_args(base).sh_order is None
    assert ap.parse_args(base + ["--transfer", "fp16", "--sh-order", "5"]).sh_order == 5
    for bad in (["--sh-order", "3"], ["--transfer", "fp32", "--sh-order", "9"], ["--transfer", "fp32", "--sh-order", "-1"]):
        with pytest.raises(SystemExit) as e:
            main(base + bad)
        assert e.value.code == 2
