"""The environment-map kernels (csrc/envmap.hip) against the float64 restatement (tests/envmap_cpu.py): labels, cell averages and the
lookup, with and without a rotation, in both conventions; a 4096 x 8192 map; bitwise repeatability; a small bright sun between the
light directions."""
import math

import numpy as np
import pytest
import torch

import envmap_cpu as E
from neusky_amd.relight import EnvironmentMap, envmap_labels, envmap_lookup, project_envmap, z_rotation

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TIE = 1e-6  # labels are compared where the best and the second-best dot product are further apart than this


def _unit(n, seed):
    d = torch.randn(n, 3, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    return (d / d.norm(dim=1, keepdim=True)).float()


def _random_rotation(seed):
    q, r = torch.linalg.qr(torch.randn(3, 3, generator=torch.Generator().manual_seed(seed), dtype=torch.float64))
    q = q * torch.sign(torch.diagonal(r))[None]
    if torch.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q.float()


def _map(H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(H, W, 3, generator=g) ** 4 * 50.0


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-30)))


@pytest.mark.parametrize("rotated", [False, True])
@pytest.mark.parametrize("conv", ["neusky", "blender"])
@pytest.mark.parametrize("H,W,D", [(4, 8, 200), (16, 32, 42), (64, 128, 24), (256, 512, 512)])
def test_kernels_match_restatement(H, W, D, conv, rotated):
    m = _map(H, W, H + D)
    dirs = _unit(D, W)
    rot = _random_rotation(D) if rotated else None
    R64 = None if rot is None else rot.double().numpy()
    env = EnvironmentMap(m, conv)
    lab = envmap_labels(env, dirs.to(DEV), rot).cpu().numpy().reshape(-1).astype(np.int64)
    ref, gap = E.labels_of(E.texel_directions(H, W, conv).reshape(-1, 3), dirs.double().numpy(), R64)
    far = gap > TIE
    assert far.mean() > 0.99 and np.array_equal(lab[far], ref[far])
    cols, cw = project_envmap(env, dirs.to(DEV), rot)
    # a float64 reduction over the GPU's own labels (the restatement's labels could move a near-tie texel to the other cell)
    rc, rw = E.project(m.double().numpy(), conv, dirs.double().numpy(), R64, labels=lab)
    assert _rel(cols.cpu().double().numpy(), rc) < 1e-5
    full = rw > 0
    assert np.array_equal(cw.cpu().numpy() > 0, full)
    assert _rel(cw.cpu().double().numpy()[full], rw[full]) < 1e-5
    if (H, W) == (4, 8):
        assert (~full).sum() > 100  # the empty-cell fallback is exercised: a map too coarse for D


def test_lookup_matches_restatement():
    H, W = 48, 96
    m = _map(H, W, 2)
    for conv in ("neusky", "blender"):
        env = EnvironmentMap(m, conv, exposure=1.5)
        cen = torch.from_numpy(E.texel_directions(H, W, conv).reshape(-1, 3)).float()
        u0 = 0.0  # the seam, where the columns wrap
        phi = 2 * math.pi * u0 if conv == "neusky" else math.pi - 2 * math.pi * u0
        th = torch.linspace(0.05, math.pi - 0.05, 50, dtype=torch.float64)
        seam = torch.stack([torch.sin(th) * math.cos(phi), torch.sin(th) * math.sin(phi), torch.cos(th)], 1).float()
        poles = torch.tensor([[0.0, 0.0, 1.0], [0.0, 0.0, -1.0], [0.0, 0.0, 2.5]])
        v = torch.cat([cen, seam, poles, _unit(5000, 3) * 1.7])
        got = envmap_lookup(env, v.to(DEV)).cpu().double().numpy()
        ref = E.lookup(m.double().numpy(), conv, v.double().numpy(), exposure=1.5)
        assert np.abs(got - ref).max() <= 1e-5 * np.abs(ref).max() and _rel(got, ref) < 1e-5
        cen_ref = 1.5 * m.reshape(-1, 3).double().numpy()  # texel centres (fp32 directions: within 1e-6 of a texel of the centre)
        assert np.allclose(got[:H * W], cen_ref, rtol=1e-5, atol=1e-5 * cen_ref.max())
        rot = _random_rotation(9)
        got = envmap_lookup(env, v[-5000:].to(DEV), rot).cpu().double().numpy()
        ref = E.lookup(m.double().numpy(), conv, v[-5000:].double().numpy(), rot.double().numpy(), exposure=1.5)
        assert _rel(got, ref) < 1e-5


def test_large_map_labels_colours_energy_and_repeatability():
    H, W, D = 4096, 8192, 512
    g = torch.Generator(device=DEV).manual_seed(0)
    data = torch.rand(H, W, 3, device=DEV, generator=g) ** 4 * 100.0
    env = EnvironmentMap(data, "blender")
    dirs = _unit(D, 5).to(DEV)
    lab = envmap_labels(env, dirs).cpu().numpy().reshape(-1).astype(np.int64)
    pick = np.random.default_rng(0).choice(H * W, 100_000, replace=False)
    i, j = pick // W, pick % W
    th, ph = E.texel_angles(H, W, "blender")
    t = np.stack([np.sin(th[i]) * np.cos(ph[j]), np.sin(th[i]) * np.sin(ph[j]), np.cos(th[i])], 1)
    ref, gap = E.labels_of(t, dirs.cpu().double().numpy())
    far = gap > TIE
    assert far.mean() > 0.99 and np.array_equal(lab[pick][far], ref[far])
    cols, cw = project_envmap(env, dirs)
    cols2, cw2 = project_envmap(env, dirs)
    assert torch.equal(cols, cols2) and torch.equal(cw, cw2)  # bitwise repeatable
    m = data.cpu().numpy().reshape(-1, 3)
    w = np.repeat(E.solid_angles(H, W), W)
    wsum = np.bincount(lab, weights=w, minlength=D)
    ref_c = np.stack([np.bincount(lab, weights=w * m[:, c], minlength=D) for c in range(3)], 1) / wsum[:, None]
    assert (wsum > 0).all()
    assert _rel(cols.cpu().double().numpy(), ref_c) < 1e-5
    assert _rel(cw.cpu().double().numpy(), wsum) < 1e-5
    energy = (w[:, None] * m).sum(0)
    assert _rel((cw.cpu().double().numpy()[:, None] * cols.cpu().double().numpy()).sum(0), energy) < 1e-5
    v = _unit(100_000, 6).to(DEV)
    a, b = envmap_lookup(env, v, z_rotation(0.3)), envmap_lookup(env, v, z_rotation(0.3))
    assert torch.equal(a, b)


def test_sun_between_the_directions_keeps_its_energy():
    """a 3 x 3 texel disc of 1e4 that no light direction points at: point samples of the map see nothing, the projection puts all of
    its energy into the one or two cells that hold it"""
    H, W, D, conv = 256, 512, 64, "blender"
    dirs = _unit(D, 8)
    rng = np.random.default_rng(1)
    while True:
        i0, j0 = int(rng.integers(40, H - 40)), int(rng.integers(2, W - 2))
        m = np.zeros((H, W, 3), np.float32)
        m[i0 - 1:i0 + 2, j0 - 1:j0 + 2] = 1e4
        if not E.lookup(m, conv, dirs.double().numpy()).any():
            break
    env = EnvironmentMap(torch.from_numpy(m), conv)
    assert envmap_lookup(env, dirs.to(DEV)).abs().max().item() == 0.0  # what point sampling would give
    cols, cw = project_envmap(env, dirs.to(DEV))
    cols, cw = cols.cpu().double().numpy(), cw.cpu().double().numpy()
    energy = 9 * 1e4 * E.solid_angles(H, W)[i0 - 1:i0 + 2].mean()
    lab = envmap_labels(env, dirs.to(DEV)).cpu().numpy()
    cells = np.unique(lab[i0 - 1:i0 + 2, j0 - 1:j0 + 2])
    assert 1 <= len(cells) <= 2
    got = (cw[:, None] * cols).sum(0)
    assert np.allclose(got, energy, rtol=1e-5)
    assert np.allclose((cw[cells, None] * cols[cells]).sum(0), energy, rtol=1e-5)
    others = np.setdiff1d(np.arange(D), cells)
    assert not cols[others].any()
