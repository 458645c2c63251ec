"""The marching-cubes kernels (csrc/mesh.hip through neusky_amd.exporter.marching_cubes) against the numpy restatement of the
same definitions (tests/marching_cubes_cpu.py), and the properties a mesh of a signed distance field must have."""
import numpy as np
import pytest
import torch

import marching_cubes_cpu as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _grid(shape, lo=-1.0, hi=1.0):
    axes = [torch.linspace(lo, hi, n, dtype=torch.float64) for n in shape]
    return torch.meshgrid(*axes, indexing="ij")


def sphere(n, r=0.5):
    X, Y, Z = _grid((n, n, n))
    return (torch.sqrt(X**2 + Y**2 + Z**2) - r).float()


def torus(n, R=0.5, r=0.2):
    X, Y, Z = _grid((n, n, n))
    return (torch.sqrt((torch.sqrt(X**2 + Y**2) - R) ** 2 + Z**2) - r).float()


def box(n, h=(0.6, 0.4, 0.5)):
    X, Y, Z = _grid((n, n, n))
    q = torch.stack([X.abs() - h[0], Y.abs() - h[1], Z.abs() - h[2]], -1)
    return (q.clamp(min=0).norm(dim=-1) + q.max(-1).values.clamp(max=0)).float()


def random_grid(n, seed):
    return torch.randn(n, n, n, generator=torch.Generator().manual_seed(seed))


def mc(vol, level=0.0, lo=(-1.0, -1.0, -1.0), hi=(1.0, 1.0, 1.0)):
    from neusky_amd.exporter import marching_cubes
    v, f = marching_cubes(vol.to(DEV), level, lo, hi)
    torch.cuda.synchronize()
    assert v.device.type == "cuda" and v.dtype == torch.float32 and f.dtype == torch.int32
    return v.cpu().numpy().astype(np.float64), f.cpu().numpy().astype(np.int64)


CASES = {"sphere": lambda: sphere(48), "torus": lambda: torus(40), "box": lambda: box(33),
         "random0": lambda: random_grid(64, 0), "random1": lambda: random_grid(64, 1)}


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_matches_restatement(name):
    vol = CASES[name]()
    v, f = mc(vol, 0.0)
    rv, rf = M.marching_cubes_cpu(vol.numpy(), 0.0)
    assert v.shape == rv.shape and f.shape == rf.shape
    assert np.abs(v - rv).max() <= 1e-6
    assert np.array_equal(f, rf)


def test_random_grid_covers_every_case():
    inside = (random_grid(64, 0) < 0).numpy()
    n = 63
    cube = np.zeros((n, n, n), np.int64)
    for c in range(8):
        cube |= inside[c & 1:n + (c & 1), (c >> 1) & 1:n + ((c >> 1) & 1), (c >> 2) & 1:n + ((c >> 2) & 1)].astype(np.int64) << c
    assert len(np.unique(cube)) == 256


def _open_edges_on_box(v, f, lo, hi):
    edges, counts = M.edge_face_counts(f)
    assert counts.max() <= 2
    open_ = edges[counts == 1]
    lo, hi = np.asarray(lo), np.asarray(hi)
    on = lambda p: (np.abs(p - lo) < 1e-6) | (np.abs(p - hi) < 1e-6)  # noqa: E731
    pa, pb = v[open_[:, 0]], v[open_[:, 1]]
    return bool((on(pa) & on(pb) & (np.abs(pa - pb) < 1e-6)).any(1).all()), int(open_.shape[0])


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_grid_interior_edges_have_two_faces(seed):
    v, f = mc(random_grid(64, seed))
    edges, counts = M.edge_face_counts(f)
    assert counts.max() == 2
    ok, n_open = _open_edges_on_box(v, f, (-1, -1, -1), (1, 1, 1))
    assert ok and n_open > 0
    assert M.directed_edges_unique(f)


def test_sphere_closed_euler_area_volume():
    v, f = mc(sphere(128))
    _, counts = M.edge_face_counts(f)
    assert (counts == 2).all() and M.directed_edges_unique(f)
    assert M.euler_characteristic(len(v), f) == 2
    area, vol = M.area_and_volume(v, f)
    assert abs(area / (4 * np.pi * 0.25) - 1) < 0.01
    assert vol > 0 and abs(vol / (4 / 3 * np.pi * 0.125) - 1) < 0.01


def test_torus_euler_zero():
    v, f = mc(torus(96))
    _, counts = M.edge_face_counts(f)
    assert (counts == 2).all()
    assert M.euler_characteristic(len(v), f) == 0


def test_vertex_count_is_crossing_edge_count():
    vol = random_grid(48, 5)
    ins = vol < 0
    want = int((ins[1:] != ins[:-1]).sum() + (ins[:, 1:] != ins[:, :-1]).sum() + (ins[:, :, 1:] != ins[:, :, :-1]).sum())
    v, _ = mc(vol)
    assert len(v) == want


def test_empty_volume():
    for vol in (torch.ones(9, 9, 9), -torch.ones(5, 6, 7)):
        v, f = mc(vol)
        assert v.shape == (0, 3) and f.shape == (0, 3)


def test_surface_leaving_the_box_is_open_only_on_the_box_faces():
    lo, hi = (-0.3, -0.4, -0.2), (0.9, 0.6, 0.8)
    X, Y, Z = [torch.linspace(l, h, 41, dtype=torch.float64) for l, h in zip(lo, hi)]
    X, Y, Z = torch.meshgrid(X, Y, Z, indexing="ij")
    vol = (torch.sqrt(X**2 + Y**2 + Z**2) - 0.5).float()
    v, f = mc(vol, 0.0, lo, hi)
    ok, n_open = _open_edges_on_box(v, f, lo, hi)
    assert ok and n_open > 0
    rv, rf = M.marching_cubes_cpu(vol.numpy(), 0.0, lo, hi)
    assert np.abs(v - rv).max() <= 1e-6 and np.array_equal(f, rf)


def test_values_exactly_at_the_level():
    """a quantised field: many corners equal the level (outside by definition), so vertices coincide with grid points"""
    vol = (sphere(40) * 8).round() / 8
    assert (vol == 0).sum() > 100
    v, f = mc(vol, 0.0)
    assert np.isfinite(v).all()
    _, counts = M.edge_face_counts(f)
    assert (counts == 2).all()
    rv, rf = M.marching_cubes_cpu(vol.numpy(), 0.0)
    assert np.abs(v - rv).max() <= 1e-6 and np.array_equal(f, rf)
    v, f = mc(vol, 0.25)  # a non-zero level
    rv, rf = M.marching_cubes_cpu(vol.numpy(), 0.25)
    assert np.abs(v - rv).max() <= 1e-6 and np.array_equal(f, rf)


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_non_finite_volume_raises(bad):
    from neusky_amd.exporter import marching_cubes
    vol = sphere(20).to(DEV)
    vol[3, 17, 11] = bad
    with pytest.raises(ValueError):
        marching_cubes(vol)


def test_bad_shapes_raise():
    from neusky_amd.exporter import marching_cubes
    for shape in [(1, 5, 5), (5, 5), (4, 4, 4, 4)]:
        with pytest.raises(ValueError):
            marching_cubes(torch.zeros(shape, device=DEV))


def test_non_cubic_volume():
    shape, lo, hi = (23, 37, 17), (-1.0, -2.0, -0.5), (1.0, 2.0, 0.5)
    X, Y, Z = [torch.linspace(l, h, n, dtype=torch.float64) for l, h, n in zip(lo, hi, shape)]
    X, Y, Z = torch.meshgrid(X, Y, Z, indexing="ij")
    vol = (torch.sqrt((X / 0.8) ** 2 + (Y / 1.5) ** 2 + (Z / 0.4) ** 2) - 1.0).float()
    v, f = mc(vol, 0.0, lo, hi)
    rv, rf = M.marching_cubes_cpu(vol.numpy(), 0.0, lo, hi)
    assert len(f) > 100 and np.abs(v - rv).max() <= 1e-6 and np.array_equal(f, rf)
    _, counts = M.edge_face_counts(f)
    assert (counts == 2).all() and M.euler_characteristic(len(v), f) == 2


def test_repeatable_bitwise():
    from neusky_amd.exporter import marching_cubes
    vol = random_grid(96, 7).to(DEV)
    a = marching_cubes(vol)
    b = marching_cubes(vol)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_peak_extra_memory_at_most_8_bytes_per_point():
    from neusky_amd.exporter import marching_cubes
    vol = sphere(200).to(DEV)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    v, f = marching_cubes(vol)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    out = v.numel() * 4 + f.numel() * 4
    assert peak - out <= 8 * vol.numel(), (peak, out, vol.numel())


def test_64bit_indexing_plane():
    """sdf = x - 0.25 in [3, 1000, 720000] (2.16e9 points, past 2^31): one vertex per (j, k) on the x edges of i = 0, two faces per
    yz cell of i = 0"""
    from neusky_amd.exporter import marching_cubes
    nx, ny, nz = 3, 1000, 720_000
    assert nx * ny * nz > 2**31
    free, _ = torch.cuda.mem_get_info()
    assert free > 64 * 2**30, f"needs ~50 GB of free device memory, {free / 2**30:.1f} GB free"
    vol = torch.empty(nx, ny, nz, device=DEV)
    for i in range(nx):
        vol[i].fill_(i - 0.25)
    v, f = marching_cubes(vol, 0.0, (0.0, 0.0, 0.0), (float(nx - 1), float(ny - 1), float(nz - 1)))
    torch.cuda.synchronize()
    assert v.shape == (ny * nz, 3) and f.shape == (2 * (ny - 1) * (nz - 1), 3)
    for vid in (0, 1, nz, ny * nz // 2 + 3, ny * nz - 2, ny * nz - 1):  # vertex j nz + k sits at (0.25, j, k)
        j, k = divmod(vid, nz)
        assert v[vid].tolist() == [0.25, float(j), float(k)], vid
    assert bool((v[:, 0] == 0.25).all())
    tail = f[-2:].cpu().numpy()  # the last cell (0, ny - 2, nz - 2)
    assert sorted(set(tail.reshape(-1).tolist())) == [(ny - 2) * nz + nz - 2, (ny - 2) * nz + nz - 1, ny * nz - 2, ny * nz - 1]
    assert int(f.min()) == 0 and int(f.max()) == ny * nz - 1
    head = f[:2].cpu().numpy()  # the first cell
    assert sorted(set(head.reshape(-1).tolist())) == [0, 1, nz, nz + 1]
    del vol, v, f
    torch.cuda.empty_cache()


def test_face_total_beyond_int32_raises():
    """[2, 1100, 1e6]: 2.2e9 faces, more than int32 counts -- a ValueError before any output is allocated"""
    from neusky_amd.exporter import marching_cubes
    vol = torch.empty(2, 1100, 1_000_000, device=DEV)
    vol[0].fill_(-0.25)
    vol[1].fill_(0.75)
    with pytest.raises(ValueError, match="int32"):
        marching_cubes(vol)
    del vol
    torch.cuda.empty_cache()
