"""Texture baking (neusky_amd.exporter.texture, csrc/texture.hip): the texel-points kernel against the float64 restatement
(tests/texture_cpu.py), the store kernel's encodings through a `shade` callable, a bake from a randomised field against the float64
oracle, chunking, the vertex-colour identity, argument errors, and the command line from a saved checkpoint."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import texture_cpu as T
from oracle import neusky_oracle as O
from util_step import oracle_params, randomise, small_pipeline_config

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LO, HI = (-0.9, -0.8, -1.0), (0.7, 0.9, 0.6)


def _mesh(v, f):
    from neusky_amd.exporter import Mesh
    return Mesh(torch.as_tensor(v, dtype=torch.float32).reshape(-1, 3).to(DEV), torch.as_tensor(f, dtype=torch.int32).reshape(-1, 3).to(DEV))


@pytest.fixture(scope="module")
def meshes():
    """an analytic sphere at 12^3 (a few hundred faces), the same without its last face (odd F), one face, two faces, none"""
    from neusky_amd.exporter import marching_cubes
    ax = torch.linspace(-1, 1, 12)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    v, f = marching_cubes(((x * x + y * y + z * z).sqrt() - 0.6).to(DEV))
    assert 100 <= f.shape[0] <= 2000
    f = f[:f.shape[0] - f.shape[0] % 2]  # even; the next one is odd
    hand_v = [[0.1, 0.2, 0.3], [1.5, -0.25, 0.75], [-0.5, 2.0, 1.0], [3.0, 3.0, -3.0]]
    return {"sphere": _mesh(v, f), "sphere_odd": _mesh(v, f[:-1]), "one": _mesh(hand_v, [[0, 1, 2]]),
            "two": _mesh(hand_v, [[0, 1, 2], [2, 1, 3]]), "none": _mesh(hand_v, np.zeros((0, 3)))}


@pytest.mark.parametrize("P", (1, 4))
@pytest.mark.parametrize("name", ("sphere", "sphere_odd", "one", "two"))
def test_texel_points_match_restatement(meshes, name, P):
    """owners and offsets exactly; positions within 8 * 2^-23 * max |vertex coordinate| of the float64 value.  Roundings of the
    kernel per axis, in units of u = 2^-24 relative to a term bounded by max |coordinate| (the weights are >= 0 and sum to 1): one
    division per weight (their errors add up to at most u over the convex combination), one product and two fused multiply-adds
    (u each): 4 u = 2 * 2^-23, a quarter of the bar."""
    from neusky_amd.exporter import atlas_layout, texel_points
    mesh = meshes[name]
    F = mesh.faces.shape[0]
    W, S, Q = atlas_layout(F, P)
    v, f = mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy()
    owner, offset, points = T.texel_points(v, f, P)
    n_sq = (F + 1) // 2
    got = texel_points(mesh, P)
    assert got[0].dtype == torch.int32 and got[1].dtype == torch.int64 and got[2].dtype == torch.float32
    assert got[0].shape == (n_sq * Q * Q,) and got[2].shape == (n_sq * Q * Q, 3)
    assert np.array_equal(got[0].cpu().numpy(), owner) and np.array_equal(got[1].cpu().numpy(), offset)
    assert np.array_equal(T.owner_map(F, P).reshape(-1)[offset], owner) and len(np.unique(offset)) == len(offset)
    err = np.abs(got[2].cpu().numpy().astype(np.float64) - points).max()
    bar = 8 * 2.0 ** -23 * np.abs(v).max()
    print(f"{name} P {P}: F {F} W {W} position err {err:.3e} bar {bar:.3e}")
    assert err <= bar
    # split ranges (a ragged one included) concatenate to the whole; squares past the last face are unowned
    cuts = sorted({0, 1 % (n_sq + 1), n_sq // 3, n_sq - 1, n_sq})
    parts = [texel_points(mesh, P, squares=(a, b)) for a, b in zip(cuts[:-1], cuts[1:])]
    for k in range(3):
        assert torch.equal(torch.cat([p[k] for p in parts]), got[k])
    if S * S > n_sq:
        tail = texel_points(mesh, P, squares=(n_sq, S * S))
        assert (tail[0] == -1).all() and (tail[2] == 0).all()
        assert np.array_equal(np.sort(np.concatenate([offset, tail[1].cpu().numpy()])), np.arange(W * W))


def _shade(x):
    """a fixed function of position: colours below the linear segment's knee, above 1 and negative; gradients of any length"""
    rgb = torch.stack([x[:, 0] * x[:, 0] * 2.0, torch.sin(5.0 * x[:, 1]) * 1.2, 0.004 * x[:, 2].abs()], -1)
    grad = torch.stack([2.0 * x[:, 0] - 0.1, x[:, 1] * x[:, 2] * 30.0, torch.sin(x[:, 2]) + 1e-3], -1)
    return rgb, grad


def _encode_colour(rgb):
    from neusky_amd.utils.utils import linear_to_sRGB
    return (linear_to_sRGB(rgb) * 255.0).round().clamp(0, 255).to(torch.uint8)


def _encode_normal(grad):
    """the header's normal encoding in IEEE fp32, one rounding per operation (on the host)"""
    g = grad.cpu()
    length = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1] + g[:, 2] * g[:, 2]).sqrt().clamp_min(1e-12)
    return (((g / length[:, None]) * 0.5 + 0.5) * 255.0).round().clamp(0, 255).to(torch.uint8)


def _scatter(W, owner, offset, values):
    img = torch.zeros(W * W, 3, dtype=torch.uint8)
    keep = owner.cpu() >= 0
    img[offset.cpu()[keep]] = values.cpu()[keep]
    return img.view(W, W, 3)


@pytest.mark.parametrize("name,P", (("sphere", 4), ("sphere_odd", 2), ("one", 1), ("two", 7)))
def test_bake_from_a_shade_callable(meshes, name, P):
    """every owned texel is exactly the encoding of the callable at the kernel's own texel point, every other texel 0"""
    from neusky_amd.exporter import atlas_layout, bake_texture, face_uvs, texel_points
    mesh = meshes[name]
    F = mesh.faces.shape[0]
    W, _, Q = atlas_layout(F, P)
    atlas = bake_texture(mesh, shade=_shade, px_per_uv_triangle=P, normal_map=True, chunk=5 * Q * Q)
    assert atlas.image.shape == (W, W, 3) and atlas.image.dtype == torch.uint8 and atlas.normal_image.shape == (W, W, 3)
    assert atlas.px_per_uv_triangle == P and torch.equal(atlas.uvs.cpu(), face_uvs(F, P))
    owner, offset, points = texel_points(mesh, P)
    rgb, grad = _shade(points)
    want = _scatter(W, owner, offset, _encode_colour(rgb))
    want_n = _scatter(W, owner, offset, _encode_normal(grad))
    bad, bad_n = (atlas.image.cpu() != want).sum().item(), (atlas.normal_image.cpu() != want_n).sum().item()
    print(f"{name} P {P}: {int((owner >= 0).sum())} owned texels, colour mismatches {bad}, normal mismatches {bad_n}")
    assert bad == 0 and bad_n == 0
    owned = torch.from_numpy(T.owner_map(F, P) >= 0)
    assert (atlas.image.cpu()[~owned] == 0).all() and (atlas.normal_image.cpu()[~owned] == 0).all()
    assert want[owned].float().std() > 20  # the image is not flat
    assert bake_texture(mesh, shade=_shade, px_per_uv_triangle=P).normal_image is None


def test_bake_of_an_empty_mesh(meshes):
    from neusky_amd.exporter import bake_texture, texel_points
    atlas = bake_texture(meshes["none"], shade=_shade, normal_map=True)
    assert atlas.image.shape == (0, 0, 3) and atlas.normal_image.shape == (0, 0, 3) and atlas.uvs.shape == (0, 3, 2)
    assert [t.shape[0] for t in texel_points(meshes["none"])] == [0, 0, 0]


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


@pytest.fixture(scope="module")
def field_mesh(pipe, level):
    from neusky_amd.exporter import extract_mesh
    mesh = extract_mesh(pipe.model.field, 16, LO, HI, isosurface_threshold=level)
    assert mesh.faces.shape[0] > 100
    return mesh


def _oracle_grad_albedo(pipe, x, dtype):
    p = oracle_params(pipe, dtype)
    x = x.to(dtype).requires_grad_(True)
    h = O.geo_network(x, p, O.HashGridCfg(smoothstep=True))
    grad = torch.autograd.grad(h[:, 0].sum(), x)[0]
    return grad.detach(), O.colour_network(x, h[:, 1:], p).detach()


def test_bake_from_field_matches_oracle(pipe, field_mesh):
    """colours within 0.5 + 1e-3 levels of the float64 oracle's albedo at the kernel's own texel points (the bar of the vertex
    colours: positions are not part of the comparison); normal texels within the vertex normals' bar (1e-5 of the largest
    component, or three times what the float32 oracle misses by), scaled to levels, plus half a level of rounding"""
    from neusky_amd.exporter import atlas_layout, bake_texture, texel_points
    P = 2
    atlas = bake_texture(field_mesh, pipe.model.field, px_per_uv_triangle=P, normal_map=True)
    W, _, _ = atlas_layout(field_mesh.faces.shape[0], P)
    owner, offset, points = texel_points(field_mesh, P)
    keep = (owner >= 0).cpu()
    x = points.cpu()[keep]
    g64, a64 = _oracle_grad_albedo(pipe, x, torch.float64)
    g32, _ = _oracle_grad_albedo(pipe, x, torch.float32)
    got = atlas.image.view(-1, 3)[offset[owner >= 0]].cpu().double()
    diff = (got - torch.from_numpy(T.srgb_levels(a64.numpy()))).abs().max().item()
    n64 = torch.nn.functional.normalize(g64, dim=-1)
    n32 = torch.nn.functional.normalize(g32.double(), dim=-1)
    bar = max(1e-5 * n64.abs().max().item(), 3.0 * (n32 - n64).abs().max().item()) * 0.5 * 255.0 + 0.5
    got_n = atlas.normal_image.view(-1, 3)[offset[owner >= 0]].cpu().double()
    diff_n = (got_n - (n64 * 0.5 + 0.5) * 255.0).abs().max().item()
    print(f"{x.shape[0]} texels of a {W} x {W} atlas: colour {diff:.4f} levels (bar 0.501), normal {diff_n:.4f} levels (bar {bar:.4f})")
    assert diff <= 0.5 + 1e-3, f"colours: {diff:.3f} levels from the oracle's albedo"
    assert diff_n <= bar, f"normal map: {diff_n:.4f} levels from the oracle's unit gradient, bar {bar:.4f}"
    unowned = torch.ones(W * W, dtype=torch.bool)
    unowned[offset[owner >= 0].cpu()] = False
    assert (atlas.image.view(-1, 3).cpu()[unowned] == 0).all() and (atlas.normal_image.view(-1, 3).cpu()[unowned] == 0).all()


def test_chunking_and_repeatability(pipe, field_mesh):
    from neusky_amd.exporter import atlas_layout, bake_texture
    f = pipe.model.field
    W, S, Q = atlas_layout(field_mesh.faces.shape[0], 4)
    assert S > 3
    whole = bake_texture(field_mesh, f, normal_map=True, chunk=1 << 30)  # one chunk, larger than the texture
    again = bake_texture(field_mesh, f, normal_map=True, chunk=1 << 30)
    part_row = bake_texture(field_mesh, f, normal_map=True, chunk=(S - 1) * Q * Q - 1)  # less than a row of squares, last chunk ragged
    for other in (again, part_row):
        assert torch.equal(other.image, whole.image) and torch.equal(other.normal_image, whole.normal_image)
    one_square = bake_texture(field_mesh, shade=_shade, chunk=1)  # rounds up to one square per call
    assert torch.equal(one_square.image, bake_texture(field_mesh, shade=_shade).image)


def test_texel_at_a_vertex_has_the_vertex_colour(pipe, field_mesh):
    """the texel at corner v0 of a lower face samples that vertex (barycentrics (1, 0, 0)); its position is re-derived in fp32, so
    the colours may differ by one level"""
    from neusky_amd.exporter import atlas_layout, bake_texture
    P = 3
    atlas = bake_texture(field_mesh, pipe.model.field, px_per_uv_triangle=P)
    faces = field_mesh.faces
    W, S, Q = atlas_layout(faces.shape[0], P)
    s = torch.arange((faces.shape[0] + 1) // 2, device=DEV)
    texel = atlas.image[(s // S) * Q, (s % S) * Q]
    vertex = field_mesh.colours[faces[0::2, 0].long()]
    diff = (texel.int() - vertex.int()).abs().max().item()
    print(f"{s.numel()} lower faces: texel at v0 vs vertex colour, max {diff} levels")
    assert diff <= 1


def test_argument_errors(meshes, pipe):
    from neusky_amd.exporter import Mesh, bake_texture, texel_points
    mesh = meshes["two"]
    host = Mesh(mesh.vertices.cpu(), mesh.faces.cpu())
    with pytest.raises(ValueError, match="CUDA"):
        bake_texture(host, pipe.model.field)
    with pytest.raises(ValueError, match="exactly one"):
        bake_texture(mesh, pipe.model.field, shade=_shade)
    with pytest.raises(ValueError, match="exactly one"):
        bake_texture(mesh)
    with pytest.raises(ValueError):
        bake_texture(Mesh(mesh.vertices.double(), mesh.faces), shade=_shade)
    with pytest.raises(ValueError):
        bake_texture(Mesh(mesh.vertices, mesh.faces.long()), shade=_shade)
    with pytest.raises(ValueError):
        bake_texture(mesh, shade=_shade, px_per_uv_triangle=0)
    with pytest.raises(ValueError):
        bake_texture(mesh, shade=_shade, chunk=0)
    with pytest.raises(ValueError, match="rgb"):
        bake_texture(mesh, shade=lambda x: (x.double(), x))
    with pytest.raises(ValueError):
        texel_points(mesh, 4, squares=(0, 2))  # the atlas of two faces has one square


def _parse_obj(path):
    v, faces, n_vt, n_vn = [], [], 0, 0
    for line in open(path).read().splitlines():
        tok = line.split()
        if tok[:1] == ["v"]:
            v.append([float(t) for t in tok[1:]])
        elif tok[:1] == ["f"]:
            faces.append([[int(x) for x in t.split("/")] for t in tok[1:]])
        n_vt += tok[:1] == ["vt"]
        n_vn += tok[:1] == ["vn"]
    return np.array(v, np.float64).astype(np.float32), np.array(faces, np.int64), n_vt, n_vn


def test_cli_from_saved_checkpoint(pipe, level, tmp_path):
    from PIL import Image
    from neusky_amd.exporter import atlas_layout, bake_texture, extract_mesh, simplify_mesh, write_ply
    from neusky_amd.exporter.mesh import vertex_attributes
    from neusky_amd.utils.checkpoints import save_checkpoint
    ckpt = save_checkpoint(tmp_path, 7, pipe)
    field, N = pipe.model.field, 300

    def run(output, *extra):
        cmd = [sys.executable, "-m", "neusky_amd.exporter", "--checkpoint", ckpt, "--output", str(output), "--resolution", "24",
               "--bounding-box-min", *map(str, LO), "--bounding-box-max", *map(str, HI), "--isosurface-threshold", repr(level),
               "--target-num-faces", str(N), *extra]
        return subprocess.run(["timeout", "-k", "10", "300"] + cmd, cwd=ROOT, capture_output=True, text=True)

    r = run(tmp_path / "mesh.obj", "--px-per-uv-triangle", "2")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "texture " in r.stdout and "simplify" in r.stdout
    assert sorted(p for p in os.listdir(tmp_path) if p.startswith("mesh.")) == ["mesh.mtl", "mesh.obj", "mesh.png"]
    mesh = simplify_mesh(extract_mesh(field, 24, LO, HI, isosurface_threshold=level, attributes=False), target_num_faces=N)
    mesh.normals, mesh.colours = vertex_attributes(field, mesh.vertices)
    F = mesh.faces.shape[0]
    assert 0 < F <= N
    v, faces, n_vt, n_vn = _parse_obj(tmp_path / "mesh.obj")
    assert np.array_equal(v, mesh.vertices.cpu().numpy()) and np.array_equal(faces[..., 0] - 1, mesh.faces.cpu().numpy())
    assert n_vt == 3 * F and n_vn == v.shape[0] and np.array_equal(faces[..., 1], np.arange(1, 3 * F + 1).reshape(F, 3))
    png = np.asarray(Image.open(tmp_path / "mesh.png"))
    W, _, _ = atlas_layout(F, 2)
    assert png.shape == (W, W, 3) and f"texture {W} x {W}" in r.stdout
    assert np.array_equal(png, bake_texture(mesh, field, px_per_uv_triangle=2).image.cpu().numpy())
    assert "map_Kd mesh.png" in open(tmp_path / "mesh.mtl").read()
    # the same command with a .ply output and no texture flag: the bytes write_ply gives from Python
    r = run(tmp_path / "mesh.ply")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "texture" not in r.stdout
    write_ply(tmp_path / "want.ply", mesh)
    assert open(tmp_path / "mesh.ply", "rb").read() == open(tmp_path / "want.ply", "rb").read()
    # a texture flag with a .ply output is an argparse error
    r = run(tmp_path / "bad.ply", "--texture-normal-map")
    assert r.returncode != 0 and "--texture-normal-map" in r.stderr and not os.path.exists(tmp_path / "bad.ply")
