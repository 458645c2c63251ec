"""Environment maps without a GPU: the readers (.hdr flat / RLE, .pfm, .npy, sRGB .png), the float64 restatement of the definitions
(tests/envmap_cpu.py) and its invariants, z_rotation against a column roll, and the camera-path rays."""
import json
import math
import sys

import numpy as np
import pytest
import torch

import envmap_cpu as E
from neusky_amd.relight import camera_rays, load_camera_path, read_envmap, srgb_to_linear, z_rotation
from neusky_amd.utils.utils import linear_to_sRGB


def _random_map(H, W, seed=0):
    return np.random.default_rng(seed).uniform(0.0, 5.0, (H, W, 3)) ** 3  # a heavy-tailed HDR range


def _unit(n, seed):
    d = np.random.default_rng(seed).normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


@pytest.mark.parametrize("rle", [False, True])
def test_hdr_round_trip(tmp_path, rle):
    H, W = 5, 300
    rgbe = E.float_to_rgbe(_random_map(H, W))
    rgbe[1, 20:290] = rgbe[1, 20]  # runs longer than 128 (split by the writer) in every component
    rgbe[2, :] = 0
    path = tmp_path / "m.hdr"
    E.write_hdr(path, rgbe, rle=rle)
    got = read_envmap(path)
    assert got.dtype == np.float32 and got.shape == (H, W, 3)
    assert np.array_equal(got, E.rgbe_to_float(rgbe))
    assert np.array_equal(got[2], np.zeros((W, 3), np.float32))


def test_hdr_rejects_other_orientations(tmp_path):
    rgbe = E.float_to_rgbe(_random_map(3, 4))
    path = tmp_path / "m.hdr"
    E.write_hdr(path, rgbe, rle=False, orientation="+Y 3 +X 4")
    with pytest.raises(ValueError, match="orientation"):
        read_envmap(path)


def test_pfm_npy_png_round_trips(tmp_path):
    from PIL import Image
    m = _random_map(6, 10).astype(np.float32)
    for le in (True, False):
        E.write_pfm(tmp_path / "m.pfm", m, little_endian=le)
        assert np.array_equal(read_envmap(tmp_path / "m.pfm"), m)
    np.save(tmp_path / "m.npy", m)
    assert np.array_equal(read_envmap(tmp_path / "m.npy"), m)
    np.save(tmp_path / "a.npy", np.concatenate([m, np.ones_like(m[..., :1])], -1))
    assert np.array_equal(read_envmap(tmp_path / "a.npy"), m)
    lin = np.random.default_rng(1).uniform(0.0, 1.0, (6, 10, 3))
    q = np.round(linear_to_sRGB(torch.from_numpy(lin)).numpy() * 255).astype(np.uint8)
    Image.fromarray(q).save(tmp_path / "m.png")
    got = read_envmap(tmp_path / "m.png")
    assert np.allclose(got, srgb_to_linear(q / 255.0), rtol=1e-6, atol=1e-7)  # exact up to 8-bit quantisation
    # the linearisation is the exact inverse of utils.linear_to_sRGB
    s = np.linspace(0.0, 1.0, 1001)
    assert np.allclose(linear_to_sRGB(torch.from_numpy(srgb_to_linear(s))).numpy(), s, atol=1e-12)


def test_exr_without_pyexr_names_the_readable_formats(tmp_path, monkeypatch):
    monkeypatch.setitem(sys.modules, "pyexr", None)
    (tmp_path / "m.exr").write_bytes(b"\x76\x2f\x31\x01")
    with pytest.raises(ValueError, match=r"\.hdr.*\.pfm.*\.npy"):
        read_envmap(tmp_path / "m.exr")


def test_solid_angles_and_texel_mapping():
    for H, W in ((1, 1), (7, 13), (512, 1024)):
        assert abs(E.solid_angles(H, W).sum() * W - 4 * math.pi) < 1e-12
    for conv in E.CONVENTIONS:
        H, W = 9, 16
        d = E.texel_directions(H, W, conv)
        assert np.allclose(np.linalg.norm(d, axis=-1), 1.0)
        x, y = E.direction_to_texel(d.reshape(-1, 3), H, W, conv)
        jj, ii = np.meshgrid(np.arange(W), np.arange(H))
        assert np.allclose(np.mod(x - jj.reshape(-1) + W / 2, W) - W / 2, 0.0, atol=1e-9)  # columns wrap
        assert np.allclose(y, ii.reshape(-1), atol=1e-9)
    # texel (0, 0) of a 2 x 4 map: theta = pi / 4; phi = pi / 4 (neusky) or 3 pi / 4 (blender)
    h = math.sqrt(0.5)
    assert np.allclose(E.texel_directions(2, 4, "neusky")[0, 0], [0.5, 0.5, h])
    assert np.allclose(E.texel_directions(2, 4, "blender")[0, 0], [-0.5, 0.5, h])


def test_restatement_invariants():
    H, W, conv = 32, 64, "blender"
    dirs = _unit(40, 3)
    c, _ = E.project(np.full((H, W, 3), 2.5), conv, dirs)
    assert np.allclose(c, 2.5, rtol=1e-14)
    m = _random_map(H, W)
    for conv in E.CONVENTIONS:
        cols, cw = E.project(m, conv, dirs, z_rotation(0.4).double().numpy(), exposure=1.0)
        total = (np.repeat(E.solid_angles(H, W), W)[:, None] * m.reshape(-1, 3)).sum(0)
        assert np.allclose((cw[:, None] * cols).sum(0), total, rtol=1e-12)
        assert abs(cw.sum() - 4 * math.pi) < 1e-12


@pytest.mark.parametrize("conv,sign", [("neusky", -1), ("blender", +1)])
def test_z_rotation_is_the_documented_column_roll(conv, sign):
    H, W, m_cols = 16, 32, 5
    m = _random_map(H, W, 7)
    R = z_rotation(2 * math.pi * m_cols / W).double().numpy()
    dirs = _unit(30, 11)
    a = E.project(m, conv, dirs, R)
    b = E.project(np.roll(m, sign * m_cols, axis=1), conv, dirs)
    assert np.allclose(a[0], b[0], rtol=1e-12) and np.allclose(a[1], b[1], rtol=1e-12)
    v = _unit(200, 12)
    # z_rotation is fp32: the angle is 2 pi m / W to ~1e-7, which moves the bilinear weights by as much
    assert np.allclose(E.lookup(m, conv, v, R), E.lookup(np.roll(m, sign * m_cols, axis=1), conv, v), rtol=1e-5)


def test_empty_cells_take_the_lookup():
    H, W = 4, 8
    m = _random_map(H, W, 5)
    dirs = _unit(200, 6)
    cols, cw = E.project(m, "neusky", dirs)
    empty = cw == 0
    assert empty.sum() >= 150
    assert np.allclose(cols[empty], E.lookup(m, "neusky", dirs[empty]))
    lab = E.labels_of(E.texel_directions(H, W, "neusky").reshape(-1, 3), dirs)[0]
    k = lab[0]
    sel = lab == k
    w = np.repeat(E.solid_angles(H, W), W)[sel]
    assert np.allclose(cols[k], (w[:, None] * m.reshape(-1, 3)[sel]).sum(0) / w.sum())


def test_lookup_texel_centres_and_seam():
    H, W = 6, 12
    m = _random_map(H, W, 8)
    for conv in E.CONVENTIONS:
        d = E.texel_directions(H, W, conv).reshape(-1, 3)
        assert np.allclose(E.lookup(m, conv, d), m.reshape(-1, 3), rtol=1e-9)
        # halfway between the last and the first column: the mean of the two (the wrap)
        theta, _ = E.texel_angles(H, W, conv)
        u = 1.0  # the seam u = 0 = 1
        phi = 2 * math.pi * u if conv == "neusky" else math.pi - 2 * math.pi * u
        v = np.array([[math.sin(theta[2]) * math.cos(phi), math.sin(theta[2]) * math.sin(phi), math.cos(theta[2])]])
        assert np.allclose(E.lookup(m, conv, v)[0], 0.5 * (m[2, 0] + m[2, W - 1]), rtol=1e-9)


def test_camera_path_and_pinhole_rays(tmp_path):
    c2w = np.array([[0.0, 0.0, 1.0, 0.3], [1.0, 0.0, 0.0, -0.2], [0.0, 1.0, 0.0, 0.1], [0, 0, 0, 1]])
    cp = {"render_width": 4, "render_height": 3, "camera_type": "perspective", "seconds": 1.0,
          "camera_path": [{"camera_to_world": c2w.reshape(-1).tolist(), "fov": 60.0, "aspect": 4 / 3}]}
    path = tmp_path / "camera_path.json"
    path.write_text(json.dumps(cp))
    cams = load_camera_path(path)
    assert len(cams) == 1 and (cams.width, cams.height) == (4, 3)
    f = 0.5 * 3 / math.tan(math.radians(30.0))
    assert abs(cams.focal(0) - f) < 1e-9
    rb = camera_rays(cams, 0, device="cpu")
    assert rb.origins.shape == (3, 4, 3)
    y, x = 2, 1
    d_cam = np.array([(x + 0.5 - 2.0) / f, -(y + 0.5 - 1.5) / f, -1.0])
    d = c2w[:3, :3] @ d_cam
    assert np.allclose(rb.directions[y, x].numpy(), d / np.linalg.norm(d), atol=1e-6)
    assert abs(rb.metadata["directions_norm"][y, x, 0].item() - np.linalg.norm(d)) < 1e-6
    assert np.allclose(rb.origins[y, x].numpy(), c2w[:3, 3], atol=1e-7)
    bad = dict(cp, camera_type="fisheye")
    path.write_text(json.dumps(bad))
    with pytest.raises(ValueError, match="fisheye"):
        load_camera_path(path)
