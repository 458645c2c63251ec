"""The mesh-simplification kernels (csrc/simplify.hip through neusky_amd.exporter.simplify_mesh) against the numpy restatement of
the same definitions (tests/mesh_simplify_cpu.py): topology bit for bit, positions away from the placement rule's discontinuities,
the cell sums before the solve, repeatability, the face budget, attributes, and the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_simplify_cpu as S
from util_step import randomise, small_pipeline_config

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LO, HI = (-0.9, -0.8, -1.0), (0.7, 0.9, 0.6)


def _grid(n):
    axes = [torch.linspace(-1.0, 1.0, n, dtype=torch.float64) for _ in range(3)]
    return torch.meshgrid(*axes, indexing="ij")


def sphere(n, r=0.5):
    X, Y, Z = _grid(n)
    return (torch.sqrt(X**2 + Y**2 + Z**2) - r).float()


def torus(n, R=0.5, r=0.2):
    X, Y, Z = _grid(n)
    return (torch.sqrt((torch.sqrt(X**2 + Y**2) - R) ** 2 + Z**2) - r).float()


def box(n, h=(0.6, 0.4, 0.5)):
    X, Y, Z = _grid(n)
    q = torch.stack([X.abs() - h[0], Y.abs() - h[1], Z.abs() - h[2]], -1)
    return (q.clamp(min=0).norm(dim=-1) + q.max(-1).values.clamp(max=0)).float()


def random_grid(n, seed):
    return torch.randn(n, n, n, generator=torch.Generator().manual_seed(seed))


VOLUMES = {"sphere": lambda: sphere(48), "torus": lambda: torus(40), "box": lambda: box(33),
           "random0": lambda: random_grid(64, 0), "random1": lambda: random_grid(64, 1)}
SPACINGS = (2.0, 3.5, 8.0)  # cell edges in grid spacings
OFFSET = np.array([0.37, 0.61, 0.13])  # of the grid origin below the mesh's box, in grid spacings: not a grid point
_MESHES, _ORACLE = {}, {}


def mesh_of(name):
    """(Mesh on the device, the very fp32 vertices and faces on the host, grid spacing)"""
    from neusky_amd.exporter import Mesh, marching_cubes
    if name not in _MESHES:
        vol = VOLUMES[name]()
        v, f = marching_cubes(vol.to(DEV), 0.0)
        _MESHES[name] = (Mesh(v, f), v.cpu().numpy(), f.cpu().numpy().astype(np.int64), 2.0 / (vol.shape[0] - 1))
    return _MESHES[name]


def grid_of(v, spacing, k):
    lo = v.astype(np.float64).min(0) - OFFSET * spacing
    return tuple(float(x) for x in lo), float(k * spacing)


def oracle_of(name, k):
    if (name, k) not in _ORACLE:
        _, v, f, spacing = mesh_of(name)
        lo, h = grid_of(v, spacing, k)
        _ORACLE[(name, k)] = S.simplify_cpu(v, f, lo, h)
    return _ORACLE[(name, k)]


@pytest.mark.parametrize("k", SPACINGS)
@pytest.mark.parametrize("name", list(VOLUMES))
def test_topology_exact_and_positions(name, k):
    from neusky_amd.exporter import cluster_face_count, simplify_mesh
    mesh, v, f, spacing = mesh_of(name)
    lo, h = grid_of(v, spacing, k)
    want = oracle_of(name, k)
    info = {}
    got = simplify_mesh(mesh, cell_size=h, origin=lo, info=info)
    torch.cuda.synchronize()
    assert got.vertices.dtype == torch.float32 and got.faces.dtype == torch.int32 and got.vertices.is_cuda
    gv, gf = got.vertices.cpu().numpy(), got.faces.cpu().numpy()
    assert gv.shape[0] == want["vertices"].shape[0]
    assert np.array_equal(gf, want["faces"])
    assert cluster_face_count(mesh, h, lo) == want["counted"] == info["counted_faces"] >= gf.shape[0]
    ulp = float(np.spacing(np.float32(np.abs(v).max())))
    assert S.inside_cells(gv, want["cells"], lo, h, slack=ulp)  # borderline or not (the slack: the one rounding to fp32)
    border = want["borderline"]
    print(f"{name} k={k}: V {len(v)} F {len(f)} -> V {len(gv)} F {len(gf)}; borderline {border.sum()} of {len(border)}")
    assert border.mean() <= 0.01
    err = np.abs(gv.astype(np.float64) - want["vertices"])[~border].max()
    bar = 1e-6 * h + ulp
    print(f"  max position error {err:.3e} (bar {bar:.3e})")
    assert err <= bar


@pytest.mark.parametrize("group", [8, 64])
@pytest.mark.parametrize("k", SPACINGS)
@pytest.mark.parametrize("name", ["sphere", "box", "random0"])
def test_cell_sums_before_the_solve(name, k, group):
    from neusky_amd.exporter.simplify import cluster_pass
    mesh, v, f, spacing = mesh_of(name)
    lo, h = grid_of(v, spacing, k)
    want = oracle_of(name, k)
    *_, sums = cluster_pass(mesh.vertices, mesh.faces, None, None, lo, h, group=group, want_sums=True)
    sums = sums.cpu().numpy()
    assert sums.shape == (len(want["keys"]), 20)
    excess = np.abs(sums[:, :10] - want["quadrics"]) - 1e-12 * want["quadric_abs"]
    print(f"{name} k={k} group={group}: worst quadric error over its bar {excess.max():.3e}")
    assert (excess <= 0).all()
    counts = np.bincount(want["rank"])
    assert np.array_equal(sums[:, 19], counts.astype(np.float64))
    xbar = sums[:, 10:13] / counts[:, None] + np.asarray(lo)
    assert np.abs(xbar - want["xbar"]).max() <= 1e-12


def test_two_runs_are_bit_identical():
    from neusky_amd.exporter import simplify_mesh
    mesh, v, f, spacing = mesh_of("random0")  # the largest test mesh
    g = torch.Generator().manual_seed(3)
    mesh = type(mesh)(mesh.vertices, mesh.faces, torch.nn.functional.normalize(torch.randn(v.shape, generator=g), dim=-1).to(DEV),
                      torch.randint(0, 256, v.shape, generator=g, dtype=torch.uint8).to(DEV))
    for k in SPACINGS:
        lo, h = grid_of(v, spacing, k)
        a = simplify_mesh(mesh, cell_size=h, origin=lo)
        b = simplify_mesh(mesh, cell_size=h, origin=lo)
        assert torch.equal(a.vertices, b.vertices) and torch.equal(a.faces, b.faces)
        assert torch.equal(a.normals, b.normals) and torch.equal(a.colours, b.colours)
    a = simplify_mesh(mesh, target_num_faces=len(f) // 10)
    b = simplify_mesh(mesh, target_num_faces=len(f) // 10)
    assert torch.equal(a.vertices, b.vertices) and torch.equal(a.faces, b.faces)


@pytest.mark.parametrize("fraction", [10, 100])
@pytest.mark.parametrize("name", ["sphere", "torus", "random0"])
def test_target_num_faces(name, fraction):
    from neusky_amd.exporter import cluster_face_count, simplify_mesh
    mesh, v, f, _ = mesh_of(name)
    target = len(f) // fraction
    info = {}
    got = simplify_mesh(mesh, target_num_faces=target, info=info)
    F2 = got.faces.shape[0]
    print(f"{name} 1/{fraction}: target {target} -> F {F2}, counted {info['counted_faces']}, n {info['cells']}, calls {info['count_calls']}")
    assert F2 <= info["counted_faces"] <= target
    assert info["count_calls"] <= 13
    n = info["cells"]
    lo = v.astype(np.float64).min(0)
    extent = float((v.astype(np.float64).max(0) - lo).max())
    assert info["origin"] == tuple(lo) and info["cell_size"] == (extent / n if n >= 2 else 2.0 * extent)
    if n >= 2:
        assert S.cluster_count(v, f, lo, extent / n) == info["counted_faces"] == cluster_face_count(mesh, extent / n)
    if n < 2048:  # tight: one more cell along the longest axis breaks the budget
        assert cluster_face_count(mesh, extent / (n + 1)) > target
        assert S.cluster_count(v, f, lo, extent / (n + 1)) > target
    want = S.simplify_cpu(v, f, lo, info["cell_size"])
    assert np.array_equal(got.faces.cpu().numpy(), want["faces"]) and got.vertices.shape[0] == len(want["vertices"])


def test_budget_at_or_above_the_face_count_returns_the_input():
    from neusky_amd.exporter import simplify_mesh
    mesh, _, f, _ = mesh_of("box")
    assert simplify_mesh(mesh, target_num_faces=len(f)) is mesh
    assert simplify_mesh(mesh, target_num_faces=len(f) + 5) is mesh
    assert simplify_mesh(mesh, target_num_faces=len(f) - 1).faces.shape[0] < len(f)


def test_attributes_without_a_field():
    from neusky_amd.exporter import Mesh, simplify_mesh
    mesh, v, f, spacing = mesh_of("torus")
    g = torch.Generator().manual_seed(5)
    normals = torch.nn.functional.normalize(torch.randn(v.shape, generator=g), dim=-1)
    colours = torch.randint(0, 256, v.shape, generator=g, dtype=torch.uint8)
    lo, h = grid_of(v, spacing, 3.5)
    got = simplify_mesh(Mesh(mesh.vertices, mesh.faces, normals.to(DEV), colours.to(DEV)), cell_size=h, origin=lo)
    want = S.simplify_cpu(v, f, lo, h, normals.numpy(), colours.numpy())
    gn, gc = got.normals.cpu().numpy().astype(np.float64), got.colours.cpu().numpy().astype(np.float64)
    assert got.colours.dtype == torch.uint8 and gn.shape == want["normals"].shape
    assert np.abs(np.linalg.norm(gn, axis=1) - 1.0).max() <= 1e-6
    assert np.abs(gn - want["normals"]).max() <= 1e-6
    assert np.abs(gc - np.rint(want["colours"])).max() <= 1 and np.abs(gc - want["colours"]).max() <= 0.5 + 1e-9
    only_normals = simplify_mesh(Mesh(mesh.vertices, mesh.faces, normals.to(DEV)), cell_size=h, origin=lo)
    assert only_normals.colours is None and torch.equal(only_normals.normals, got.normals)


def test_empty_mesh_and_range_checks():
    from neusky_amd.exporter import Mesh, cluster_face_count, simplify_mesh
    empty = Mesh(torch.zeros(0, 3, device=DEV), torch.zeros(0, 3, dtype=torch.int32, device=DEV))
    out = simplify_mesh(empty, cell_size=0.1)
    assert out.vertices.shape == (0, 3) and out.faces.shape == (0, 3)
    assert cluster_face_count(empty, 0.1) == 0
    pts = Mesh(torch.rand(50, 3, device=DEV), torch.zeros(0, 3, dtype=torch.int32, device=DEV))  # vertices without faces
    out = simplify_mesh(pts, cell_size=0.25)
    assert 0 < out.vertices.shape[0] <= 50 and out.faces.shape == (0, 3)
    mesh, _, _, _ = mesh_of("box")
    bad = Mesh(mesh.vertices, mesh.faces.clone())
    bad.faces[3, 1] = mesh.vertices.shape[0]
    with pytest.raises(ValueError, match="face indices"):
        simplify_mesh(bad, cell_size=0.1)
    with pytest.raises(ValueError, match="cells along an axis"):
        simplify_mesh(mesh, cell_size=1e-7)
    with pytest.raises(ValueError, match="cells along an axis"):
        cluster_face_count(mesh, 1e-7)


def test_host_tensors_raise_at_the_abi():
    from neusky_amd import hip
    with pytest.raises(hip.NeuSkyHipError):
        hip.mesh_cell_keys(torch.zeros(4, 3), (0.0, 0.0, 0.0), 0.1, torch.zeros(4, dtype=torch.int64))
    with pytest.raises(hip.NeuSkyHipError):
        hip.mesh_cluster_count(torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32), (0.0, 0.0, 0.0), 0.1, torch.zeros(1, dtype=torch.int64))


# ---- with a field: attributes from the field, and the command line

@pytest.fixture(scope="module")
def pipe():
    torch.manual_seed(0)
    p = small_pipeline_config().setup(device=DEV)
    randomise(p)
    return p


@pytest.fixture(scope="module")
def level(pipe):
    """an iso level the randomised field crosses inside the box (its zero set may lie outside)"""
    from neusky_amd.exporter import sdf_grid
    return float(sdf_grid(pipe.model.field, 17, LO, HI).median())


def test_attributes_from_the_field(pipe, level):
    from neusky_amd.exporter import extract_mesh, simplify_mesh
    from neusky_amd.exporter.mesh import vertex_attributes
    field = pipe.model.field
    mesh = extract_mesh(field, 40, LO, HI, isosurface_threshold=level)
    got = simplify_mesh(mesh, cell_size=0.11, field=field)
    assert 0 < got.faces.shape[0] < mesh.faces.shape[0]
    normals, colours = vertex_attributes(field, got.vertices)
    assert torch.equal(got.normals, normals) and torch.equal(got.colours, colours)


def _read_ply(path):
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    header = data[:end].decode("ascii").splitlines()
    nv = int(next(l for l in header if l.startswith("element vertex")).split()[2])
    nf = int(next(l for l in header if l.startswith("element face")).split()[2])
    vd = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                   ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    fd = np.dtype([("n", "u1"), ("i", "<i4", (3,))])
    assert len(data) == end + vd.itemsize * nv + fd.itemsize * nf
    vert = np.frombuffer(data, vd, nv, end)
    face = np.frombuffer(data, fd, nf, end + vd.itemsize * nv)
    assert (face["n"] == 3).all()
    return vert, face["i"]


def _cli(ckpt, out, level, *extra):
    cmd = [sys.executable, "-m", "neusky_amd.exporter", "--checkpoint", ckpt, "--output", str(out), "--resolution", "40",
           "--bounding-box-min", *map(str, LO), "--bounding-box-max", *map(str, HI), "--isosurface-threshold", repr(level), *extra]
    r = subprocess.run(["timeout", "-k", "10", "300"] + cmd, cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def test_cli_simplifies_and_is_unchanged_without_the_flag(pipe, level, tmp_path):
    from neusky_amd.exporter import extract_mesh, simplify_mesh, write_ply
    from neusky_amd.exporter.mesh import vertex_attributes
    from neusky_amd.utils.checkpoints import save_checkpoint
    ckpt = save_checkpoint(tmp_path, 7, pipe)
    field = pipe.model.field
    full = extract_mesh(field, 40, LO, HI, isosurface_threshold=level)
    target = full.faces.shape[0] // 8
    stdout = _cli(ckpt, tmp_path / "small.ply", level, "--target-num-faces", str(target))
    assert "->" in stdout and "simplify" in stdout and f"F {full.faces.shape[0]}" in stdout
    vert, faces = _read_ply(tmp_path / "small.ply")
    assert 0 < len(faces) <= target and faces.min() >= 0 and faces.max() < len(vert)
    want = simplify_mesh(extract_mesh(field, 40, LO, HI, isosurface_threshold=level, attributes=False), target_num_faces=target)
    assert np.array_equal(faces, want.faces.cpu().numpy())
    assert np.array_equal(np.stack([vert["x"], vert["y"], vert["z"]], 1), want.vertices.cpu().numpy())
    normals, colours = vertex_attributes(field, want.vertices)
    assert np.array_equal(np.stack([vert["nx"], vert["ny"], vert["nz"]], 1), normals.cpu().numpy())
    assert np.array_equal(np.stack([vert["red"], vert["green"], vert["blue"]], 1), colours.cpu().numpy())
    # without the flags: the file the code path before simplification writes, byte for byte
    _cli(ckpt, tmp_path / "plain.ply", level)
    write_ply(tmp_path / "direct.ply", full)
    assert (tmp_path / "plain.ply").read_bytes() == (tmp_path / "direct.ply").read_bytes()
