"""The mesh-component kernels (csrc/components.hip through neusky_amd.exporter.label_components / remove_floaters) against the numpy
restatement of the same definitions (tests/mesh_components_cpu.py).  Everything compared is an integer or a copied bit pattern: no
tolerance anywhere.  Every mesh has at least 8192 faces (32 workgroups of 256: all eight XCDs take part in the link pass)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_components_cpu as CC
from util_step import randomise, small_pipeline_config

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LO, HI = (-0.9, -0.8, -1.0), (0.7, 0.9, 0.6)
N = 8192


def random_grid(n, seed):
    return torch.randn(n, n, n, generator=torch.Generator().manual_seed(seed))


def _renumber(faces, how, V, seed=0):
    number = {"identity": np.arange(V), "reversed": np.arange(V)[::-1], "random": np.random.default_rng(seed).permutation(V)}[how]
    return number[faces]


def strip(how):
    i = np.arange(N)
    return N + 2, _renumber(np.stack([i, i + 1, i + 2], 1), how, N + 2)


def fan(hub):
    """N faces that share one vertex and nothing else: the hub is the only path between any two of them"""
    i = np.arange(N)
    V = 2 * N + 1
    if hub == "smallest":
        return V, np.stack([np.zeros(N, np.int64), 2 * i + 1, 2 * i + 2], 1)
    return V, np.stack([np.full(N, V - 1), 2 * i, 2 * i + 1], 1)


def crumbs():
    """3000 single triangles, one sheet of 6000 faces and 100 vertices without a face, numbered at random, faces shuffled"""
    t = np.arange(3000)
    singles = np.stack([3 * t, 3 * t + 1, 3 * t + 2], 1)
    nx, ny = 50, 60
    ix, iy = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    a = (ix * (ny + 1) + iy).ravel() + 9000
    sheet = np.concatenate([np.stack([a, a + ny + 1, a + 1], 1), np.stack([a + 1, a + ny + 1, a + ny + 2], 1)])
    V = 9000 + (nx + 1) * (ny + 1) + 100
    faces = np.concatenate([singles, sheet])
    rng = np.random.default_rng(4)
    return V, _renumber(faces[rng.permutation(len(faces))], "random", V, seed=5)


SPHERES = (((-0.5, -0.5, -0.5), 0.4), ((0.5, 0.5, 0.5), 0.35), ((0.5, -0.5, 0.3), 0.3), ((-0.5, 0.5, 0.4), 0.25), ((0.1, 0.0, -0.6), 0.2))


def spheres_volume(n=48):
    x = torch.linspace(-1.0, 1.0, n, dtype=torch.float64)
    X, Y, Z = torch.meshgrid(x, x, x, indexing="ij")
    d = [torch.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2) - r for c, r in SPHERES]
    return torch.stack(d).min(0).values.float()


SYNTHETIC = {"strip-identity": lambda: strip("identity"), "strip-reversed": lambda: strip("reversed"), "strip-random": lambda: strip("random"),
             "fan-hub-smallest": lambda: fan("smallest"), "fan-hub-largest": lambda: fan("largest"), "crumbs": crumbs}
VOLUMES = {"spheres": spheres_volume, "random0": lambda: random_grid(64, 0)}
CASES = list(SYNTHETIC) + list(VOLUMES)
_MESHES, _ORACLE = {}, {}


def mesh_of(name):
    """(Mesh on the device with random normals and colours, its arrays on the host: vertices, faces (int64), normals, colours)"""
    from neusky_amd.exporter import Mesh, marching_cubes
    if name not in _MESHES:
        g = torch.Generator().manual_seed(len(name))
        if name in SYNTHETIC:
            V, faces = SYNTHETIC[name]()
            v, f = torch.randn(V, 3, generator=g).to(DEV), torch.from_numpy(np.ascontiguousarray(faces)).to(torch.int32).to(DEV)
        else:
            v, f = marching_cubes(VOLUMES[name]().to(DEV), 0.0)
        normals = torch.nn.functional.normalize(torch.randn(v.shape, generator=g), dim=-1).to(DEV)
        colours = torch.randint(0, 256, v.shape, generator=g, dtype=torch.uint8).to(DEV)
        assert f.shape[0] >= N, (name, f.shape)
        _MESHES[name] = (Mesh(v, f, normals, colours), v.cpu().numpy(), f.cpu().numpy().astype(np.int64), normals.cpu().numpy(),
                         colours.cpu().numpy())
    return _MESHES[name]


def oracle_of(name):
    if name not in _ORACLE:
        _, v, f, _, _ = mesh_of(name)
        _ORACLE[name] = CC.label_components_cpu(len(v), f)
    return _ORACLE[name]


def assert_components(got, want):
    assert got.labels.dtype == torch.int32 and got.face_labels.dtype == torch.int32 and got.roots.dtype == torch.int32
    assert got.face_counts.dtype == torch.int64 and got.labels.is_cuda
    assert got.num_components == len(want["roots"])
    assert np.array_equal(got.roots.cpu().numpy(), want["roots"])
    assert np.array_equal(got.face_counts.cpu().numpy(), want["face_counts"])
    assert np.array_equal(got.labels.cpu().numpy(), want["labels"])
    assert np.array_equal(got.face_labels.cpu().numpy(), want["face_labels"])


def assert_mesh(got, want):
    assert got.vertices.dtype == torch.float32 and got.faces.dtype == torch.int32 and got.faces.shape[1:] == (3,)
    assert np.array_equal(got.faces.cpu().numpy(), want["faces"])  # input order, orientation, re-indexed corners
    assert np.array_equal(got.vertices.cpu().numpy().view(np.uint32), want["vertices"].view(np.uint32))  # bit for bit
    assert np.array_equal(got.normals.cpu().numpy().view(np.uint32), want["normals"].view(np.uint32))
    assert np.array_equal(got.colours.cpu().numpy(), want["colours"])


EXPECTED_COMPONENTS = {"strip-identity": 1, "strip-reversed": 1, "strip-random": 1, "fan-hub-smallest": 1, "fan-hub-largest": 1,
                       "crumbs": 3001, "spheres": 5}


@pytest.mark.parametrize("name", CASES)
def test_labels_roots_and_counts_are_exact(name):
    from neusky_amd.exporter import label_components
    mesh, v, f, _, _ = mesh_of(name)
    want = oracle_of(name)
    got = label_components(mesh)
    print(f"{name}: V {len(v)} F {len(f)} components {got.num_components} largest {int(want['face_counts'][0])}")
    assert_components(got, want)
    if name in EXPECTED_COMPONENTS:
        assert got.num_components == EXPECTED_COMPONENTS[name]
    else:
        assert got.num_components > 1000  # a random volume: thousands of crumbs
    again = label_components(mesh)  # two runs: bit for bit
    for field in ("labels", "face_labels", "roots", "face_counts"):
        assert torch.equal(getattr(got, field), getattr(again, field))


@pytest.mark.parametrize("name", CASES)
def test_labels_do_not_depend_on_the_face_order(name):
    from neusky_amd.exporter import Mesh, label_components
    mesh, v, f, _, _ = mesh_of(name)
    want = oracle_of(name)
    perm = torch.randperm(len(f), generator=torch.Generator().manual_seed(7))
    got = label_components(Mesh(mesh.vertices, mesh.faces[perm.to(DEV)][:, [2, 0, 1]].contiguous()))
    assert np.array_equal(got.labels.cpu().numpy(), want["labels"]) and np.array_equal(got.roots.cpu().numpy(), want["roots"])
    assert np.array_equal(got.face_counts.cpu().numpy(), want["face_counts"])
    assert np.array_equal(got.face_labels.cpu().numpy(), want["face_labels"][perm.numpy()])


def test_loose_vertices_get_minus_one_and_are_dropped():
    from neusky_amd.exporter import label_components, remove_floaters
    mesh, v, f, n, c = mesh_of("crumbs")
    loose = np.setdiff1d(np.arange(len(v)), f.ravel())
    assert len(loose) == 100
    labels = label_components(mesh).labels.cpu().numpy()
    assert (labels[loose] == -1).all() and (np.delete(labels, loose) >= 0).all()
    got = remove_floaters(mesh, min_faces=1_000_000)  # nothing stays
    assert got.vertices.shape == (0, 3) and got.faces.shape == (0, 3) and got.normals.shape == (0, 3) and got.colours.shape == (0, 3)
    info = {}
    got = remove_floaters(mesh, keep_largest=1, info=info)  # the sheet alone: crumbs and loose vertices go
    assert info == dict(components=3001, kept_components=1, faces_before=9000, faces_after=6000, largest=6000)
    assert got.vertices.shape[0] == 51 * 61
    assert_mesh(got, CC.remove_floaters_cpu(v, f, keep_largest=1, normals=n, colours=c))
    assert_mesh(remove_floaters(mesh, keep_largest=1), CC.remove_floaters_cpu(v, f, keep_largest=1, normals=n, colours=c))


def test_spheres_keep_exactly_what_the_restatement_keeps():
    from neusky_amd.exporter import remove_floaters
    mesh, v, f, n, c = mesh_of("spheres")
    counts = oracle_of("spheres")["face_counts"]
    assert len(counts) == 5 and (np.diff(counts) < 0).all()
    third = int(counts[2])
    for kwargs, kept in ((dict(keep_largest=2), 2), (dict(min_faces=third), 3), (dict(min_faces=third + 1), 2),
                         (dict(keep_largest=4, min_faces=third), 3), (dict(keep_largest=1, min_faces=third), 1)):
        info = {}
        got = remove_floaters(mesh, info=info, **kwargs)
        want = CC.remove_floaters_cpu(v, f, normals=n, colours=c, **kwargs)
        assert want["kept_components"] == kept == info["kept_components"] and info["components"] == 5
        assert info["faces_before"] == len(f) and info["faces_after"] == len(want["faces"]) == int(counts[:kept].sum())
        assert info["largest"] == int(counts[0])
        assert_mesh(got, want)
        again = remove_floaters(mesh, **kwargs)
        assert torch.equal(got.vertices, again.vertices) and torch.equal(got.faces, again.faces)
        assert torch.equal(got.normals, again.normals) and torch.equal(got.colours, again.colours)
    # every face stays: the mesh itself comes back
    assert remove_floaters(mesh, keep_largest=5) is mesh and remove_floaters(mesh, keep_largest=9) is mesh
    assert remove_floaters(mesh, min_faces=int(counts[4])) is mesh and remove_floaters(mesh, min_faces=1, keep_largest=5) is mesh


@pytest.mark.parametrize("name", ["crumbs", "random0"])
def test_filtered_mesh_without_attributes(name):
    from neusky_amd.exporter import Mesh, remove_floaters
    mesh, v, f, _, _ = mesh_of(name)
    bare = Mesh(mesh.vertices, mesh.faces)
    for kwargs in (dict(keep_largest=3), dict(min_faces=2)):
        got = remove_floaters(bare, **kwargs)
        want = CC.remove_floaters_cpu(v, f, **kwargs)
        assert got.normals is None and got.colours is None
        assert np.array_equal(got.faces.cpu().numpy(), want["faces"])
        assert np.array_equal(got.vertices.cpu().numpy().view(np.uint32), want["vertices"].view(np.uint32))


def test_simplification_of_the_filtered_mesh():
    from neusky_amd.exporter import Mesh, remove_floaters, simplify_mesh
    mesh, v, f, n, c = mesh_of("spheres")
    want = CC.remove_floaters_cpu(v, f, keep_largest=3, normals=n, colours=c)
    restated = Mesh(torch.from_numpy(want["vertices"]).to(DEV), torch.from_numpy(want["faces"]).to(DEV),
                    torch.from_numpy(want["normals"]).to(DEV), torch.from_numpy(want["colours"]).to(DEV))
    a = simplify_mesh(remove_floaters(mesh, keep_largest=3), cell_size=0.11, origin=(-1.0, -1.0, -1.0))
    b = simplify_mesh(restated, cell_size=0.11, origin=(-1.0, -1.0, -1.0))
    assert 0 < a.faces.shape[0] < len(want["faces"])
    assert torch.equal(a.vertices, b.vertices) and torch.equal(a.faces, b.faces)
    assert torch.equal(a.normals, b.normals) and torch.equal(a.colours, b.colours)


def test_empty_meshes_and_range_checks():
    from neusky_amd import hip
    from neusky_amd.exporter import Mesh, label_components, remove_floaters
    empty = Mesh(torch.zeros(0, 3, device=DEV), torch.zeros(0, 3, dtype=torch.int32, device=DEV))
    comps = label_components(empty)
    assert comps.num_components == 0 and comps.labels.shape == (0,) and comps.face_labels.shape == (0,) and comps.roots.shape == (0,)
    out = remove_floaters(empty, keep_largest=1)
    assert out.vertices.shape == (0, 3) and out.faces.shape == (0, 3) and out.faces.dtype == torch.int32
    pts = Mesh(torch.rand(50, 3, device=DEV), torch.zeros(0, 3, dtype=torch.int32, device=DEV),
               colours=torch.zeros(50, 3, dtype=torch.uint8, device=DEV))  # vertices without faces
    comps = label_components(pts)
    assert comps.num_components == 0 and (comps.labels == -1).all() and comps.labels.shape == (50,) and comps.labels.dtype == torch.int32
    info = {}
    out = remove_floaters(pts, min_faces=1, info=info)
    assert out.vertices.shape == (0, 3) and out.faces.shape == (0, 3) and out.colours.shape == (0, 3) and out.normals is None
    assert info == dict(components=0, kept_components=0, faces_before=0, faces_after=0, largest=0)
    mesh, _, _, _, _ = mesh_of("spheres")
    launches = []
    original = hip.cc_link
    hip.cc_link = lambda *a: launches.append(a) or original(*a)
    try:
        for bad_index in (mesh.vertices.shape[0], -1):
            bad = Mesh(mesh.vertices, mesh.faces.clone())
            bad.faces[3, 1] = bad_index
            with pytest.raises(ValueError, match="face indices"):
                label_components(bad)
            with pytest.raises(ValueError, match="face indices"):
                remove_floaters(bad, keep_largest=1)
        nan = Mesh(mesh.vertices.clone(), mesh.faces)
        nan.vertices[5, 0] = float("nan")
        with pytest.raises(ValueError, match="non-finite"):
            remove_floaters(nan, keep_largest=1)
        assert not launches  # refused before anything was launched
        label_components(mesh)
        assert len(launches) == 1
    finally:
        hip.cc_link = original


def test_host_tensors_raise():
    from neusky_amd import hip
    from neusky_amd.exporter import Mesh, label_components, remove_floaters
    host = Mesh(torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32))
    with pytest.raises(ValueError, match="CUDA"):
        label_components(host)
    with pytest.raises(ValueError, match="CUDA"):
        remove_floaters(host, min_faces=2)
    with pytest.raises(hip.NeuSkyHipError):
        hip.cc_link(torch.zeros(2, 3, dtype=torch.int32), torch.arange(4, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(hip.NeuSkyHipError):
        hip.cc_select(torch.zeros(2, 3, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), torch.ones(1, dtype=torch.uint8),
                      torch.zeros(2, dtype=torch.uint8), torch.zeros(4, dtype=torch.uint8))


def test_a_broken_invariant_sets_the_status_word_and_ends():
    """parent[x] > x on entry (not the identity): the link pass refuses the value before it follows it, and says so"""
    from neusky_amd import hip
    from neusky_amd.exporter.components import _status_error
    mesh, _, _, _, _ = mesh_of("strip-identity")
    V = mesh.vertices.shape[0]
    parent = (torch.arange(V, dtype=torch.int32, device=DEV) + 1).clamp(max=V - 1)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    hip.cc_link(mesh.faces, parent, status)
    assert int(status.item()) == hip.CC_STATUS_LINK
    with pytest.raises(RuntimeError, match="iteration cap"):
        _status_error(int(status.item()), "label_components")


# ---- the command line, on a saved randomised checkpoint

@pytest.fixture(scope="module")
def pipe():
    torch.manual_seed(0)
    p = small_pipeline_config().setup(device=DEV)
    randomise(p)
    return p


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


def test_cli_drops_floaters_and_is_unchanged_without_the_flags(pipe, tmp_path):
    from neusky_amd.exporter import extract_mesh, label_components, remove_floaters, sdf_grid, write_ply
    from neusky_amd.exporter.mesh import vertex_attributes
    from neusky_amd.utils.checkpoints import save_checkpoint
    ckpt = save_checkpoint(tmp_path, 7, pipe)
    field = pipe.model.field
    level = float(sdf_grid(field, 17, LO, HI).median())  # an iso level the randomised field crosses inside the box
    bare = extract_mesh(field, 40, LO, HI, isosurface_threshold=level, attributes=False)
    comps = label_components(bare)
    stdout = _cli(ckpt, tmp_path / "main.ply", level, "--keep-largest-components", "1")
    print(stdout.strip())
    assert f"components {comps.num_components} -> 1" in stdout and f"F {bare.faces.shape[0]}" in stdout
    assert re.search(r"components \d+\.\d+s", stdout)  # the stage's timing
    vert, faces = _read_ply(tmp_path / "main.ply")
    want = remove_floaters(bare, keep_largest=1)
    assert len(faces) == int(comps.face_counts[0]) and np.array_equal(faces, want.faces.cpu().numpy())
    assert np.array_equal(np.stack([vert["x"], vert["y"], vert["z"]], 1), want.vertices.cpu().numpy())
    normals, colours = vertex_attributes(field, want.vertices)
    assert np.array_equal(np.stack([vert["nx"], vert["ny"], vert["nz"]], 1), normals.cpu().numpy())
    assert np.array_equal(np.stack([vert["red"], vert["green"], vert["blue"]], 1), colours.cpu().numpy())
    # without the flags: the file the code path without the component step writes, byte for byte
    _cli(ckpt, tmp_path / "plain.ply", level)
    write_ply(tmp_path / "direct.ply", extract_mesh(field, 40, LO, HI, isosurface_threshold=level))
    assert (tmp_path / "plain.ply").read_bytes() == (tmp_path / "direct.ply").read_bytes()
