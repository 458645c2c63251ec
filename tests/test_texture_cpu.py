"""The texture atlas without a GPU: the layout's no-bleed property on the float64 restatement (tests/texture_cpu.py), face_uvs and
atlas_layout against it, the OBJ / MTL / PNG writer on a host mesh, and the argument errors."""
import os

import numpy as np
import pytest
import torch

import texture_cpu as T

PS, FS = (1, 2, 4, 7), (1, 2, 5, 8)


@pytest.mark.parametrize("P", PS)
def test_bilinear_lookup_never_reads_a_foreign_texel(P):
    """for every point of a face's UV triangle (random ones, the corners, the edge midpoints) every tap with a non-zero weight is a
    texel of the image that this face owns.  A condition on the layout: no exception is allowed.  The points are formed in texel
    coordinates from the corner v0 and the two legs, (1 - s - t) v0 + s v1 + t v2 with s, t >= 0 and s + t <= 1, which cannot leave
    the triangle's bounding box by rounding."""
    rng = np.random.default_rng(P)
    for F in FS:
        W, S, Q = T.layout(F, P)
        owners = T.owner_map(F, P)
        corners = T.corner_texels(F, P).astype(np.float64)
        st = rng.random((4000, 2))
        fold = st.sum(1) > 1.0
        st[fold] = 1.0 - st[fold]
        st = np.concatenate([st, [[0, 0], [1, 0], [0, 1], [0.5, 0], [0, 0.5], [0.5, 0.5]]])
        foreign = 0
        for f in range(F):
            c0, e1, e2 = corners[f, 0], corners[f, 1] - corners[f, 0], corners[f, 2] - corners[f, 0]
            for s, t in st:
                x, y = c0 + s * e1 + t * e2
                for i, j, w in T.bilinear_taps(x, y):
                    foreign += not (0 <= i < W and 0 <= j < W and owners[j, i] == f)
        assert foreign == 0, f"P {P} F {F}: {foreign} taps outside the face's own texels"


@pytest.mark.parametrize("P", PS)
def test_face_uvs_layout_and_ownership(P):
    from neusky_amd.exporter import atlas_layout, face_uvs
    for F in FS:
        W, S, Q = T.layout(F, P)
        assert atlas_layout(F, P) == (W, S, Q) and W == S * Q and Q == P + 3 and (S - 1) ** 2 < (F + 1) // 2 <= S * S
        uv = face_uvs(F, P)
        assert uv.shape == (F, 3, 2) and uv.dtype == torch.float32 and uv.device.type == "cpu"
        want = T.uvs(F, P)
        assert np.array_equal(uv.numpy(), want.astype(np.float32))
        assert (want > 0).all() and (want < 1).all() and (uv > 0).all() and (uv < 1).all()
        # a UV maps back to its corner's texel centre
        back = np.stack([want[..., 0] * W - 0.5, (1.0 - want[..., 1]) * W - 0.5], -1)
        assert np.abs(back - T.corner_texels(F, P)).max() < 1e-9
        owners = T.owner_map(F, P)
        for s in range(S * S):
            sq = owners[(s // S) * Q:(s // S + 1) * Q, (s % S) * Q:(s % S + 1) * Q]
            n_lower, n_upper = (P + 3) * (P + 4) // 2, (P + 3) * (P + 2) // 2
            assert n_lower + n_upper == Q * Q
            assert (sq == 2 * s).sum() == (n_lower if 2 * s < F else 0)
            assert (sq == 2 * s + 1).sum() == (n_upper if 2 * s + 1 < F else 0)
            assert (sq == -1).sum() == Q * Q - (sq == 2 * s).sum() - (sq == 2 * s + 1).sum()
        if F % 2:
            last = (F - 1) // 2
            sq = owners[(last // S) * Q:(last // S + 1) * Q, (last % S) * Q:(last % S + 1) * Q]
            assert (sq == -1).sum() == (P + 3) * (P + 2) // 2 and (sq == F - 1).sum() == (P + 3) * (P + 4) // 2
    assert atlas_layout(0, P) == (0, 0, P + 3) and face_uvs(0, P).shape == (0, 3, 2)


def test_gutter_texels_sample_their_own_triangle():
    """the clamped barycentrics are a convex combination; inside the triangle they are the plain ones"""
    for P in PS:
        for upper in (False, True):
            for j in range(P + 3):
                for i in range(P + 3):
                    if (i + j >= P + 3) != upper:
                        continue
                    b = T.barycentrics(P, upper, i, j)
                    assert (b >= 0).all() and abs(b.sum() - 1.0) < 1e-15
                    b1, b2 = ((P + 2 - i) / P, (P + 2 - j) / P) if upper else (i / P, j / P)
                    if min(b1, b2, 1 - b1 - b2) >= 0:
                        assert np.allclose(b, [1 - b1 - b2, b1, b2], atol=1e-15)


def _parse_obj(path):
    v, vn, vt, faces, other = [], [], [], [], []
    for line in open(path).read().splitlines():
        tok = line.split()
        if not tok or tok[0] == "#":
            continue
        if tok[0] == "v":
            v.append([np.float32(float(t)) for t in tok[1:]])
        elif tok[0] == "vn":
            vn.append([np.float32(float(t)) for t in tok[1:]])
        elif tok[0] == "vt":
            vt.append([np.float32(float(t)) for t in tok[1:]])
        elif tok[0] == "f":
            faces.append([[int(x) if x else 0 for x in t.split("/")] for t in tok[1:]])
        else:
            other.append(tok)
    return (np.array(v, np.float32).reshape(-1, 3), np.array(vn, np.float32).reshape(-1, 3), np.array(vt, np.float32).reshape(-1, 2),
            np.array(faces, np.int64), other)


def _host_mesh(normals):
    from neusky_amd.exporter import Mesh
    g = torch.Generator().manual_seed(0)
    v = torch.randn(9, 3, generator=g) * torch.tensor([1e-3, 1.0, 1e4])  # values of very different size: nine digits must carry them all
    f = torch.tensor([[0, 1, 2], [2, 1, 3], [4, 5, 6], [6, 5, 7], [0, 8, 4]], dtype=torch.int32)
    n = torch.nn.functional.normalize(torch.randn(9, 3, generator=g), dim=-1) if normals else None
    return Mesh(v, f, n)


@pytest.mark.parametrize("normals", (True, False))
def test_write_obj_round_trip(tmp_path, normals):
    from PIL import Image
    from neusky_amd.exporter import TextureAtlas, atlas_layout, face_uvs, write_obj
    mesh = _host_mesh(normals)
    F, P = mesh.faces.shape[0], 2
    W, _, _ = atlas_layout(F, P)
    g = torch.Generator().manual_seed(1)
    image = torch.randint(0, 256, (W, W, 3), dtype=torch.uint8, generator=g)
    normal_image = torch.randint(0, 256, (W, W, 3), dtype=torch.uint8, generator=g) if normals else None
    path = tmp_path / "out.obj"
    write_obj(path, mesh, TextureAtlas(image, normal_image, face_uvs(F, P), P))
    v, vn, vt, faces, other = _parse_obj(path)
    assert np.array_equal(v.view(np.uint32), mesh.vertices.numpy().view(np.uint32))  # bit-equal after float32(...)
    assert faces.shape == (F, 3, 3 if normals else 2)
    assert np.array_equal(faces[..., 0] - 1, mesh.faces.numpy())
    assert vt.shape == (3 * F, 2) and np.array_equal(vt.reshape(F, 3, 2), face_uvs(F, P).numpy())
    assert np.array_equal(faces[..., 1], np.arange(1, 3 * F + 1).reshape(F, 3))
    if normals:
        assert np.array_equal(vn.view(np.uint32), mesh.normals.numpy().view(np.uint32))
        assert np.array_equal(faces[..., 2], faces[..., 0])
    else:
        assert vn.shape[0] == 0
    assert ["mtllib", "out.mtl"] in other and ["usemtl", "material_0"] in other
    text = open(path).read()
    assert text.index("mtllib") < text.index("\nv ") < text.index("\nvt ") < text.index("usemtl") < text.index("\nf ")
    mtl = open(tmp_path / "out.mtl").read()
    assert "newmtl material_0" in mtl.splitlines() and "map_Kd out.png" in mtl.splitlines()
    assert np.array_equal(np.asarray(Image.open(tmp_path / "out.png")), image.numpy())
    if normals:
        assert np.array_equal(np.asarray(Image.open(tmp_path / "out_normal.png")), normal_image.numpy())
        assert any(l.startswith("#") and "out_normal.png" in l for l in mtl.splitlines())
    else:
        assert not os.path.exists(tmp_path / "out_normal.png") and "normal" not in mtl


def test_write_obj_without_an_atlas_is_a_plain_obj(tmp_path):
    from neusky_amd.exporter import write_obj
    for normals in (True, False):
        mesh = _host_mesh(normals)
        path = tmp_path / f"plain{int(normals)}.obj"
        write_obj(path, mesh, None)
        v, vn, vt, faces, other = _parse_obj(path)
        assert np.array_equal(v.view(np.uint32), mesh.vertices.numpy().view(np.uint32)) and vt.shape[0] == 0 and other == []
        assert np.array_equal(faces[..., 0] - 1, mesh.faces.numpy()) and vn.shape[0] == (9 if normals else 0)
        if normals:
            assert (faces[..., 1] == 0).all() and np.array_equal(faces[..., 2], faces[..., 0])  # a//n
        assert all(p.endswith(".obj") for p in os.listdir(tmp_path))  # no .mtl, no .png


def test_layout_errors():
    from neusky_amd.exporter import atlas_layout, face_uvs
    assert atlas_layout(2 * 2340 ** 2, 4)[0] == 16380  # the largest 7-texel-square atlas that fits
    with pytest.raises(ValueError) as e:
        atlas_layout(2 * 2340 ** 2 + 1, 4)
    msg = str(e.value)
    assert str(2 * 2340 ** 2 + 1) in msg and "P = 4" in msg and "--target-num-faces" in msg
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError):
            atlas_layout(10, bad)
        with pytest.raises(ValueError):
            face_uvs(10, bad)
    with pytest.raises(ValueError):
        atlas_layout(-1, 4)


def test_bake_argument_errors_without_gpu():
    """host tensors, both of field and shade, neither, px_per_uv_triangle = 0: ValueError before anything is launched"""
    from neusky_amd.exporter import bake_texture, texel_points
    mesh = _host_mesh(False)
    shade = lambda x: (x, x)
    with pytest.raises(ValueError, match="CUDA"):
        bake_texture(mesh, shade=shade)
    with pytest.raises(ValueError, match="CUDA"):
        texel_points(mesh)
    with pytest.raises(ValueError, match="exactly one"):
        bake_texture(mesh)
    with pytest.raises(ValueError, match="exactly one"):
        bake_texture(mesh, object(), shade=shade)
    with pytest.raises(ValueError, match="px_per_uv_triangle"):
        bake_texture(mesh, shade=shade, px_per_uv_triangle=0)
