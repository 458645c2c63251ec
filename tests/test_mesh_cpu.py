"""Mesh export, the parts that need no GPU: the numpy restatement of the marching-cubes definitions (tests/marching_cubes_cpu.py)
on analytic surfaces and on every single-cube case, the PLY writer, and the checkpoint mapping onto a bare SDF field."""
import numpy as np
import pytest
import torch

import marching_cubes_cpu as M


def _grid(n, lo=-1.0, hi=1.0):
    x = np.linspace(lo, hi, n)
    return np.meshgrid(x, x, x, indexing="ij")


def _sphere(n, r=0.5):
    X, Y, Z = _grid(n)
    return (np.sqrt(X**2 + Y**2 + Z**2) - r).astype(np.float32)


def _torus(n, R=0.5, r=0.2):
    X, Y, Z = _grid(n)
    return (np.sqrt((np.sqrt(X**2 + Y**2) - R) ** 2 + Z**2) - r).astype(np.float32)


def test_restatement_sphere_closed_and_accurate():
    v, f = M.marching_cubes_cpu(_sphere(96))
    _, counts = M.edge_face_counts(f)
    assert (counts == 2).all()
    assert M.directed_edges_unique(f)
    assert M.euler_characteristic(len(v), f) == 2
    area, vol = M.area_and_volume(v, f)
    assert abs(area / (np.pi) - 1) < 0.01
    assert abs(vol / (4 / 3 * np.pi * 0.125) - 1) < 0.01 and vol > 0
    assert np.abs(np.linalg.norm(v, axis=1) - 0.5).max() < 2.0 / 95 * 0.1


def test_restatement_torus_genus_one():
    v, f = M.marching_cubes_cpu(_torus(80))
    _, counts = M.edge_face_counts(f)
    assert (counts == 2).all() and M.directed_edges_unique(f)
    assert M.euler_characteristic(len(v), f) == 0
    _, vol = M.area_and_volume(v, f)
    assert abs(vol / (2 * np.pi**2 * 0.5 * 0.04) - 1) < 0.02


def test_every_single_cube_case_uses_exactly_its_crossing_edges():
    for case in range(256):
        used = sorted({e for tri in M.TABLE[case] for e in tri})
        assert used == M.crossing_edges(case), case
        for tri in M.TABLE[case]:
            assert len(set(tri)) == 3, (case, tri)
        # within one cube a mesh edge is either on the patch's boundary (one face) or a diagonal inside it (two)
        _, counts = M.edge_face_counts(np.array(M.TABLE[case]).reshape(-1, 3)) if M.TABLE[case] else (None, np.array([], int))
        assert ((counts == 1) | (counts == 2)).all(), case


def test_every_single_cube_case_orientation():
    """a 2x2x2 volume of case c: every face's normal has a positive component from the inside corners towards the outside ones"""
    for case in range(1, 255):
        vol = np.array([1.0 if not (case >> c) & 1 else -1.0 for c in range(8)], np.float32)
        grid = np.zeros((2, 2, 2), np.float32)
        for c in range(8):
            grid[c & 1, (c >> 1) & 1, (c >> 2) & 1] = vol[c]
        v, f = M.marching_cubes_cpu(grid, 0.0, (0, 0, 0), (1, 1, 1))
        assert len(v) == len(M.crossing_edges(case)) and len(f) == len(M.TABLE[case])
        assert M.directed_edges_unique(f), case
        centre_in = np.mean([[c & 1, (c >> 1) & 1, (c >> 2) & 1] for c in range(8) if (case >> c) & 1], 0)
        a, b, c_ = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
        n = np.cross(b - a, c_ - a).sum(0)  # the vector area of the patch
        centre_out = np.mean([[c & 1, (c >> 1) & 1, (c >> 2) & 1] for c in range(8) if not (case >> c) & 1], 0)
        if np.linalg.norm(centre_out - centre_in) > 1e-9 and np.linalg.norm(n) > 1e-9:
            assert n @ (centre_out - centre_in) > 0, case


def test_restatement_random_grid_is_crack_free():
    """random values hit all 256 cases many times; every edge off the box faces has exactly two faces, oriented oppositely"""
    n = 24
    vol = np.random.default_rng(3).standard_normal((n, n, n)).astype(np.float32)
    v, f = M.marching_cubes_cpu(vol, 0.0, (0, 0, 0), (n - 1, n - 1, n - 1))
    edges, counts = M.edge_face_counts(f)
    assert counts.max() == 2 and M.directed_edges_unique(f)
    open_ = edges[counts == 1]
    on_box = lambda p: ((np.abs(p) < 1e-9) | (np.abs(p - (n - 1)) < 1e-9))  # noqa: E731
    for end in (0, 1):
        p = v[open_[:, end]]
        assert on_box(p).any(1).all()
    # both ends on the SAME box face
    pa, pb = v[open_[:, 0]], v[open_[:, 1]]
    assert (on_box(pa) & on_box(pb) & (np.abs(pa - pb) < 1e-9)).any(1).all()


def _read_ply(path):
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    header = data[:end].decode("ascii").splitlines()
    assert header[0] == "ply" and header[1] == "format binary_little_endian 1.0"
    props, counts, cur = {"vertex": [], "face": []}, {}, None
    for line in header[2:-1]:
        w = line.split()
        if w[0] == "element":
            cur = w[1]
            counts[cur] = int(w[2])
        elif w[0] == "property" and w[1] != "list":
            props[cur].append((w[2], {"float": "<f4", "uchar": "u1"}[w[1]]))
        elif w[0] == "property":
            assert w[1:] == ["list", "uchar", "int", "vertex_indices"]
    vd = np.dtype(props["vertex"])
    vert = np.frombuffer(data, vd, counts["vertex"], end)
    fd = np.dtype([("n", "u1"), ("idx", "<i4", (3,))])
    face = np.frombuffer(data, fd, counts["face"], end + vd.itemsize * counts["vertex"])
    assert len(data) == end + vd.itemsize * counts["vertex"] + fd.itemsize * counts["face"]
    assert (face["n"] == 3).all()
    return header, vert, face["idx"]


@pytest.mark.parametrize("attributes", [True, False])
def test_write_ply_round_trip(tmp_path, attributes):
    from neusky_amd.exporter import Mesh, write_ply
    g = torch.Generator().manual_seed(0)
    mesh = Mesh(torch.randn(7, 3, generator=g), torch.randint(0, 7, (5, 3), generator=g, dtype=torch.int32))
    if attributes:
        mesh.normals = torch.nn.functional.normalize(torch.randn(7, 3, generator=g), dim=-1)
        mesh.colours = torch.randint(0, 256, (7, 3), generator=g, dtype=torch.uint8)
    path = tmp_path / "m.ply"
    write_ply(path, mesh)
    header, vert, faces = _read_ply(path)
    want = ["element vertex 7", "property float x", "property float y", "property float z"]
    if attributes:
        want += ["property float nx", "property float ny", "property float nz",
                 "property uchar red", "property uchar green", "property uchar blue"]
    want += ["element face 5", "property list uchar int vertex_indices", "end_header"]
    assert header[2:] == want
    assert np.array_equal(np.stack([vert["x"], vert["y"], vert["z"]], 1), mesh.vertices.numpy())
    assert np.array_equal(faces, mesh.faces.numpy())
    if attributes:
        assert np.array_equal(np.stack([vert["nx"], vert["ny"], vert["nz"]], 1), mesh.normals.numpy())
        assert np.array_equal(np.stack([vert["red"], vert["green"], vert["blue"]], 1), mesh.colours.numpy())


def test_write_ply_empty_mesh(tmp_path):
    from neusky_amd.exporter import Mesh, write_ply
    write_ply(tmp_path / "e.ply", Mesh(torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32)))
    header, vert, faces = _read_ply(tmp_path / "e.ply")
    assert len(vert) == 0 and len(faces) == 0 and "element vertex 0" in header


def test_load_field_state_reference_keys_on_host():
    from neusky_amd.exporter import load_field_state
    from neusky_amd.fields.sdf_albedo_field import SDFAlbedoFieldConfig
    cfg = SDFAlbedoFieldConfig(log2_hashmap_size=12, max_res=64)
    field = cfg.setup(aabb=torch.tensor([[-1.0, -1, -1], [1, 1, 1]]), num_images=3)
    g = torch.Generator().manual_seed(1)
    state = {"_model.field.encoding.params": torch.randn(field.encoding.params.numel(), generator=g).half(),
             "_model.field.deviation_network.variance": torch.tensor([0.7]),
             "_model.field.aabb": torch.tensor([[-2.0, -2, -2], [2, 2, 2]]),
             "_model.proposal_networks.0.encoding.params": torch.zeros(4)}  # (not the field's: ignored)
    want = {}
    for kind in ("glin", "clin"):
        for l in range(3):
            lin = getattr(field, f"{kind}{l}")
            v = torch.randn(lin.weight_v.shape, generator=g)
            gg = torch.rand(lin.weight_g.shape, generator=g) + 0.5
            b = torch.randn(lin.bias.shape, generator=g)
            if (kind, l) in (("glin", 0), ("glin", 2), ("clin", 1)):  # old-style torch weight_norm
                state[f"_model.field.{kind}{l}.weight_g"], state[f"_model.field.{kind}{l}.weight_v"] = gg, v
            else:  # torch.nn.utils.parametrizations.weight_norm
                state[f"_model.field.{kind}{l}.parametrizations.weight.original0"] = gg
                state[f"_model.field.{kind}{l}.parametrizations.weight.original1"] = v
            state[f"_model.field.{kind}{l}.bias"] = b
            want[(kind, l)] = (gg, v, b)
    loaded, unmapped = load_field_state(field, {"pipeline": state})
    assert unmapped == []
    assert len(loaded) == len(state) - 1
    assert torch.equal(field.encoding.params, state["_model.field.encoding.params"].float())
    assert torch.equal(field.aabb, state["_model.field.aabb"])
    assert field.deviation_network.variance.item() == pytest.approx(0.7)
    for (kind, l), (gg, v, b) in want.items():
        lin = getattr(field, f"{kind}{l}")
        assert torch.equal(lin.weight_g, gg) and torch.equal(lin.weight_v, v) and torch.equal(lin.bias, b)
    with pytest.raises(ValueError):
        load_field_state(field, {"_model.field.glin0.bias": torch.zeros(3)})
    _, unmapped = load_field_state(field, {"_model.field.not_a_parameter": torch.zeros(1)})
    assert unmapped == ["_model.field.not_a_parameter"]


def test_marching_cubes_rejects_host_tensors():
    from neusky_amd.exporter import marching_cubes
    with pytest.raises(ValueError):
        marching_cubes(torch.zeros(4, 4, 4))
