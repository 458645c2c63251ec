"""Mesh simplification, the parts that need no GPU: the numpy restatement of the clustering definitions (tests/mesh_simplify_cpu.py)
on marching-cubes meshes of analytic surfaces and random volumes, and the host logic of neusky_amd.exporter.simplify (argument
checks, the command line's flags, the bisection on a face budget)."""
import numpy as np
import pytest
import torch

import marching_cubes_cpu as M
import mesh_simplify_cpu as S


def _grid(n, lo=-1.0, hi=1.0):
    x = np.linspace(lo, hi, n)
    return np.meshgrid(x, x, x, indexing="ij")


def _sphere(n, r=0.5):
    X, Y, Z = _grid(n)
    return (np.sqrt(X**2 + Y**2 + Z**2) - r).astype(np.float32)


def _torus(n, R=0.5, r=0.2):
    X, Y, Z = _grid(n)
    return (np.sqrt((np.sqrt(X**2 + Y**2) - R) ** 2 + Z**2) - r).astype(np.float32)


def _box(n, h=(0.6, 0.4, 0.5)):
    X, Y, Z = _grid(n)
    q = np.stack([np.abs(X) - h[0], np.abs(Y) - h[1], np.abs(Z) - h[2]], -1)
    return (np.linalg.norm(np.maximum(q, 0), axis=-1) + np.minimum(q.max(-1), 0)).astype(np.float32)


def _random(n, seed):
    return torch.randn(n, n, n, generator=torch.Generator().manual_seed(seed)).numpy()


VOLUMES = {"sphere": lambda: _sphere(48), "torus": lambda: _torus(40), "box": lambda: _box(33), "random0": lambda: _random(64, 0)}
SPACINGS = (2.0, 3.5, 8.0)  # cell edges in grid spacings: not only multiples, so that cell walls do not coincide with grid planes
OFFSET = np.array([0.37, 0.61, 0.13])  # of the grid origin below the mesh's box, in grid spacings: not a grid point
_MESHES = {}


def mesh_of(name):
    if name not in _MESHES:
        vol = VOLUMES[name]()
        v, f = M.marching_cubes_cpu(vol, 0.0)
        _MESHES[name] = (v.astype(np.float32), f, 2.0 / (vol.shape[0] - 1))
    return _MESHES[name]


def grid_of(v, spacing, k):
    return v.astype(np.float64).min(0) - OFFSET * spacing, k * spacing


@pytest.mark.parametrize("k", SPACINGS)
@pytest.mark.parametrize("name", list(VOLUMES))
def test_restatement_output_is_well_formed(name, k):
    v, f, spacing = mesh_of(name)
    lo, h = grid_of(v, spacing, k)
    out = S.simplify_cpu(v, f, lo, h)
    nv, nf = out["vertices"], out["faces"]
    C = len(nv)
    assert 0 < C < len(v) and 0 < len(nf) < len(f)
    assert nf.min() >= 0 and nf.max() < C
    assert (nf[:, 0] != nf[:, 1]).all() and (nf[:, 1] != nf[:, 2]).all() and (nf[:, 0] != nf[:, 2]).all()
    assert (nf[:, 0] < nf[:, 1]).all() and (nf[:, 0] < nf[:, 2]).all()  # rotated: the smallest index leads
    assert len(np.unique(nf, axis=0)) == len(nf)
    assert (np.diff(out["keys"]) > 0).all()
    assert S.inside_cells(nv, out["cells"], lo, h)
    assert len(nf) <= out["counted"] == S.cluster_count(v, f, lo, h)
    # the inputs of the GPU position test: few cells sit on a discontinuity of the placement rule
    assert out["borderline"].mean() <= 0.01, out["borderline"].mean()


@pytest.mark.parametrize("k", SPACINGS)
def test_restatement_sphere_orientation_and_placement(k):
    v, f, spacing = mesh_of("sphere")
    lo, h = grid_of(v, spacing, k)
    out = S.simplify_cpu(v, f, lo, h)
    _, vol = M.area_and_volume(out["vertices"], out["faces"])
    assert vol > 0  # orientation kept
    err_q = np.abs(np.linalg.norm(out["vertices"], axis=1) - 0.5).max()
    err_mean = np.abs(np.linalg.norm(out["xbar"], axis=1) - 0.5).max()
    assert err_q <= err_mean  # the quadric minimiser is at least as close to the sphere as the cell mean


def test_restatement_attributes_and_degenerate_faces():
    v, f, spacing = mesh_of("box")
    lo, h = grid_of(v, spacing, 3.5)
    rng = np.random.default_rng(0)
    normals = rng.standard_normal(v.shape).astype(np.float32)
    colours = rng.integers(0, 256, v.shape).astype(np.uint8)
    f2 = np.concatenate([f, f[:5, [0, 0, 1]], f[:7]], 0)  # zero-area faces add nothing; repeated faces are dropped
    a, b = S.simplify_cpu(v, f, lo, h, normals, colours), S.simplify_cpu(v, f2, lo, h)
    assert np.array_equal(a["faces"], b["faces"])
    assert np.allclose(np.linalg.norm(a["normals"], axis=1), 1.0)
    assert a["colours"].min() >= 0 and a["colours"].max() <= 255


# ---- host logic of neusky_amd.exporter.simplify

def test_simplify_mesh_is_exported_and_checks_its_arguments():
    from neusky_amd.exporter import Mesh, cluster_face_count, simplify_mesh
    host = Mesh(torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32))
    with pytest.raises(ValueError, match="exactly one"):
        simplify_mesh(host)
    with pytest.raises(ValueError, match="exactly one"):
        simplify_mesh(host, cell_size=0.1, target_num_faces=10)
    for bad in (0.0, -1.0, float("nan"), float("inf"), "0.1"):
        with pytest.raises(ValueError, match="cell_size"):
            simplify_mesh(host, cell_size=bad)
    for bad in (-1, 2.5, True):
        with pytest.raises(ValueError, match="target_num_faces"):
            simplify_mesh(host, target_num_faces=bad)
    with pytest.raises(ValueError, match="origin"):
        simplify_mesh(host, cell_size=0.1, origin=(0.0, 1.0))
    with pytest.raises(ValueError, match="CUDA"):  # the kernels run on the device only: no host path
        simplify_mesh(host, cell_size=0.1)
    with pytest.raises(ValueError, match="CUDA"):
        cluster_face_count(host, 0.1)


def test_cli_flags_exist_exclude_each_other_and_default_off():
    from neusky_amd.exporter.__main__ import build_parser
    base = ["--checkpoint", "c.ckpt", "--output", "m.ply"]
    args = build_parser().parse_args(base)
    assert args.target_num_faces is None and args.simplify_cell_size is None
    assert build_parser().parse_args(base + ["--target-num-faces", "50000"]).target_num_faces == 50000
    assert build_parser().parse_args(base + ["--simplify-cell-size", "0.02"]).simplify_cell_size == 0.02
    with pytest.raises(SystemExit):
        build_parser().parse_args(base + ["--target-num-faces", "50000", "--simplify-cell-size", "0.02"])


def _counting(fn):
    calls = []

    def count(n):
        calls.append(n)
        return fn(n)
    return count, calls


@pytest.mark.parametrize("target", [0, 7, 1000, 123456, 4 * 2048**2 - 1])
def test_bisection_monotonic_count(target):
    from neusky_amd.exporter.simplify import bisect_cells
    fn = lambda n: 4 * n * n  # noqa: E731  (a closed surface crosses ~ n^2 cells)
    count, calls = _counting(fn)
    n, counted, n_calls = bisect_cells(count, target)
    assert n_calls == len(calls) <= 13
    if n >= 2:
        assert counted == fn(n) <= target < fn(n + 1)
    else:
        assert n == 1 and counted == 0 and fn(2) > target


def test_bisection_ends_of_the_range():
    from neusky_amd.exporter.simplify import bisect_cells
    count, calls = _counting(lambda n: n)
    assert bisect_cells(count, 5000) == (2048, 2048, 1) and calls == [2048]
    count, calls = _counting(lambda n: 10 * n)
    assert bisect_cells(count, 19) == (1, 0, 2) and calls == [2048, 2]


@pytest.mark.parametrize("seed", range(8))
def test_bisection_keeps_its_invariant_for_a_non_monotonic_count(seed):
    from neusky_amd.exporter.simplify import bisect_cells
    rng = np.random.default_rng(seed)
    table = (np.arange(2049) ** 2 * 3 + rng.integers(-40000, 40000, 2049)).clip(0)  # rising on the whole, jagged locally
    target = int(table[2]) + int(rng.integers(0, int(table[2048] - table[2])))
    assert table[2] <= target < table[2048]
    count, calls = _counting(lambda n: int(table[n]))
    n, counted, n_calls = bisect_cells(count, target)
    assert n_calls == len(calls) <= 13 and len(set(calls)) == len(calls)
    assert 2 <= n < 2048 and counted == table[n] <= target < table[n + 1]
