"""The antialiasing rules without a GPU: the R2 offsets, the sub-pixel ray construction against the float64 pinhole on the four cameras of
the header's table, relight.Antialias' validation, and the edge rule's restatement (antialias_cpu.py) on hand-made G-buffers."""
import math

import numpy as np
import pytest
import torch

import antialias_cpu as A
from neusky_amd.relight import Antialias, r2_offsets

CAMERAS = ((9, 13, 55.0), (16, 24, 55.0), (5, 7, 120.0), (1080, 1920, 50.0))  # H, W, fov


def test_r2_offsets():
    for S in (2, 4, 16, 64):
        o = r2_offsets(S)
        assert o.dtype == torch.float32 and tuple(o.shape) == (S - 1, 2)
        assert bool((o >= -0.5).all()) and bool((o < 0.5).all())
        assert len({tuple(v) for v in o.tolist()}) == S - 1  # pairwise distinct
        assert np.array_equal(o.numpy(), A.r2_offsets(S).astype(np.float32))
    first = r2_offsets(4).double().numpy()
    assert np.abs(first - np.array([[-0.245, -0.430], [-0.490, 0.140], [0.265, -0.290]])).max() <= 1e-3
    assert Antialias(samples=4).sample_offsets().tolist() == r2_offsets(4).tolist()


def camera_directions(H, W, fov, c2w):
    """relight.camera_rays' arithmetic in float32 numpy: (directions [H, W, 3], norm [H, W, 1])"""
    f = np.float32(0.5 * H / math.tan(math.radians(float(np.float32(fov))) / 2.0))
    y, x = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    cam = np.stack([(x + np.float32(0.5) - np.float32(0.5 * W)) / f, -(y + np.float32(0.5) - np.float32(0.5 * H)) / f, -np.ones_like(x)], -1)
    d = (cam @ c2w[:, :3].astype(np.float32).T).astype(np.float32)
    n = np.linalg.norm(d, axis=-1, keepdims=True).astype(np.float32)
    return (d / n).astype(np.float32), n


@pytest.mark.parametrize("H,W,fov", CAMERAS)
def test_float32_rays_are_the_float64_pinholes(H, W, fov):
    c2w = A.look_at().astype(np.float32).astype(np.float64)  # (the camera's own float32 pose)
    d, n = camera_directions(H, W, fov, c2w)
    offsets = A.r2_offsets(16)
    P = H * W
    pixels = np.arange(P) if P <= 4096 else np.unique(np.concatenate([
        np.arange(W), np.arange(P - W, P), np.arange(0, P, W), np.arange(W - 1, P, W), np.random.default_rng(0).integers(0, P, 4096)]))
    got, got_n = A.subpixel_rays(d, n, pixels, offsets.astype(np.float32))
    want, want_n = A.pinhole_subpixel(H, W, fov, c2w, pixels, offsets.astype(np.float32))
    worst = np.abs(got.astype(np.float64) - want).max()
    print(f"{H} x {W}, fov {fov}: worst difference of a direction component {worst:.2e}, of the norm {np.abs(got_n - want_n).max():.2e}")
    assert worst <= 1e-6
    assert np.abs(got_n.astype(np.float64) / want_n - 1.0).max() <= 1e-6
    # and the float64 run of the rule on the float64 pinhole is the pinhole: the construction is exact
    yy, xx = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    d64, n64 = A.pinhole(H, W, fov, c2w, xx, yy)
    exact, _ = A.subpixel_rays(d64, n64[..., None], pixels, offsets, dtype=np.float64)
    assert np.abs(exact - A.pinhole_subpixel(H, W, fov, c2w, pixels, offsets)[0]).max() <= 1e-13


def test_antialias_validation():
    a = Antialias()
    assert (a.samples, a.colour, a.depth, a.normal_deg, a.accumulation, a.covered, a.every_pixel, a.offsets, a.batch_pixels) == \
        (4, 0.1, 0.02, 15.0, 0.1, 0.5, False, None, 1 << 18)
    assert Antialias(samples=2).samples == 2 and Antialias(samples=64).samples == 64
    for bad in (1, 65, 0, -3, 2.5, True):
        with pytest.raises(ValueError, match="samples"):
            Antialias(samples=bad)
    for name in ("colour", "depth", "normal_deg", "accumulation", "covered"):
        for bad in (-1e-3, float("nan"), float("inf"), "x"):
            with pytest.raises(ValueError, match=name):
                Antialias(**{name: bad})
        assert getattr(Antialias(**{name: 0}), name) == 0.0
    with pytest.raises(ValueError, match="normal_deg"):
        Antialias(normal_deg=90.0)
    assert Antialias(normal_deg=89.9).normal_deg == 89.9
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="batch_pixels"):
            Antialias(batch_pixels=bad)
    # the caller's offsets: [S - 1, 2], each end of [-0.5, 0.5] accepted, anything outside refused
    ends = torch.tensor([[-0.5, 0.5], [0.5, -0.5], [0.0, 0.0]])
    assert torch.equal(Antialias(samples=4, offsets=ends).sample_offsets(), ends)
    for bad in (torch.tensor([[0.0, 0.5000001]] * 3), torch.tensor([[-0.51, 0.0]] * 3), torch.tensor([[float("nan"), 0.0]] * 3)):
        with pytest.raises(ValueError, match="offsets"):
            Antialias(samples=4, offsets=bad)
    for shape in ((2, 2), (3, 3), (3,)):
        with pytest.raises(ValueError, match="offsets"):
            Antialias(samples=4, offsets=torch.zeros(shape))
    with pytest.raises(Exception):
        a.samples = 8  # frozen


def flat_scene(H=5, W=7):
    """a G-buffer on which nothing differs: covered, depth 2, normal +z, one grey image"""
    return dict(depth=np.full((H, W), 2.0, np.float32), normal=np.tile(np.float32([0, 0, 1]), (H, W, 1)), acc=np.ones((H, W), np.float32),
                lin=np.full((1, H, W, 3), 0.5, np.float32))


def cross(H, W, y, x):
    """the pixel and its neighbours inside the image"""
    m = np.zeros((H, W), np.uint8)
    for yy, xx in ((y, x), (y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
        if 0 <= yy < H and 0 <= xx < W:
            m[yy, xx] = 1
    return m


@pytest.mark.parametrize("criterion", ("accumulation", "depth", "normal", "colour"))
def test_each_criterion_marks_exactly_its_pixels(criterion):
    H, W = 5, 7
    s = flat_scene(H, W)
    assert not A.edge_mask(**s).any()
    at = {"accumulation": (2, 3), "depth": (0, 0), "normal": (4, 6), "colour": (1, 5)}[criterion]
    if criterion == "accumulation":
        s["acc"][at] = 0.875  # differs by 0.125 > 0.1, both covered, depth and normal alike
    elif criterion == "depth":
        s["depth"][at] = 2.0625  # |d_p - d_q| = 0.0625 > 0.02 * 2
    elif criterion == "normal":
        s["normal"][at] = (0.0, 0.5, 0.75)  # 33.7 degrees from +z, not unit length: the test does not need it
    else:
        s["lin"][0][at] = (0.5, 0.625, 0.5)  # Y differs by 0.0894 > 0.1 * 0.589
    got = A.edge_mask(**s)
    assert np.array_equal(got, cross(H, W, *at)), got
    assert np.array_equal(A.edge_mask(**s, criteria=(criterion,)), got)
    for other in ("accumulation", "depth", "normal", "colour"):
        if other != criterion:
            assert not A.edge_mask(**s, criteria=(other,)).any(), other
    # below its threshold the same change marks nothing
    loose = {"accumulation": dict(accumulation=0.25), "depth": dict(depth_t=0.05), "normal": dict(normal_deg=45.0), "colour": dict(colour=0.25)}
    assert not A.edge_mask(**s, **loose[criterion]).any()


def test_uncovered_pairs_and_zero_normals():
    H, W = 5, 7
    s = flat_scene(H, W)
    s["acc"][:] = 0.25  # nothing is covered: depth and normal must not fire
    s["depth"][2, 3] = 9.0
    s["normal"][1, 1] = (1.0, 0.0, 0.0)
    assert not A.edge_mask(**s).any()
    s["acc"][:] = 1.0
    assert A.edge_mask(**s).sum() == 10
    s = flat_scene(H, W)
    s["normal"][2, 2] = 0.0  # a zero normal switches the normal test off for its pairs
    assert not A.edge_mask(**s).any()
    s["normal"][2, 2] = (0.0, 1e-5, 0.0)  # long enough, and at a right angle
    assert np.array_equal(A.edge_mask(**s), cross(H, W, 2, 2))


def test_the_rule_is_symmetric():
    """both pixels of a differing pair are marked: the mask of the mirrored (and of the transposed) frame is the mirrored mask, and a marked
    pixel has a marked neighbour"""
    H, W = 17, 13
    s, kinds = A.synthetic_gbuffer(H, W, 2, seed=0)
    m = A.edge_mask(**s)
    assert 0 < m.sum() < H * W and len(np.unique(kinds)) == 8
    # a pair of two uncovered kinds differs in depth and normal and is not marked for it: inside such a pair's blocks only their other
    # neighbours mark
    assert not A.edge_mask(**s, criteria=("depth", "normal"))[(kinds == 5) | (kinds == 6)].any()
    flip = dict(depth=s["depth"][:, ::-1], normal=s["normal"][:, ::-1], acc=s["acc"][:, ::-1], lin=s["lin"][:, :, ::-1])
    assert np.array_equal(A.edge_mask(**flip), m[:, ::-1])
    turn = dict(depth=s["depth"].T, normal=s["normal"].transpose(1, 0, 2), acc=s["acc"].T, lin=s["lin"].transpose(0, 2, 1, 3))
    assert np.array_equal(A.edge_mask(**turn), m.T)
    pad = np.pad(m, 1)
    near = pad[:-2, 1:-1] | pad[2:, 1:-1] | pad[1:-1, :-2] | pad[1:-1, 2:]
    assert np.all(near[m == 1] == 1)


def test_resolve_restatement():
    frame = np.arange(2 * 5 * 3, dtype=np.float64).reshape(2, 5, 3)
    X = np.ones((2, 2, 3, 3))
    out = A.resolve(frame, X, [4, 1])
    assert np.array_equal(out[:, [0, 2, 3]], frame[:, [0, 2, 3]])
    assert np.allclose(out[:, [4, 1]], (frame[:, [4, 1]] + 3.0) / 4.0)
