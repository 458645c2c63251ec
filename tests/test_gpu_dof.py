"""The three depth-of-field kernels (csrc/dof.hip) alone, against their numpy restatement (dof_cpu.py): the circle of confusion and the mark
exactly, the lens rays against the float64 run of the rule, within four times what the float32 run of the same rule in the same order
loses on the same inputs."""
import numpy as np
import pytest
import torch

import antialias_cpu as A
import dof_cpu as L
from neusky_amd import hip
from neusky_amd.cameras.rays import RayBundle
from neusky_amd.relight import (CameraPath, DepthOfField, camera_rays, circle_of_confusion, lens_block, lens_frame, lens_rays, lens_table,
                                mark_pixels)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32


def lens_of(afpx, izf, a=0.0):
    block = torch.zeros(hip.DOF_LENS_FLOATS)
    block[9], block[10], block[11] = a, izf, afpx
    return block.to(DEV)


# ------------------------------------------------------------------------------------------ circle of confusion
def gbuffer(H, W, seed):
    rng = np.random.default_rng(seed)
    depth = (rng.random((H, W)) * 4 + 0.05).astype(F)
    acc = rng.random((H, W)).astype(F)
    kind = rng.integers(0, 10, (H, W))
    depth[kind == 0] = 0.0
    depth[kind == 1] = -depth[kind == 1]
    depth[kind == 2] = np.nan
    acc[kind == 3] = 0.5  # at `covered`: not above it
    acc[kind == 4] = np.nan
    depth[kind == 5] = np.inf
    return depth, acc


@pytest.mark.parametrize("izf", (0.0, 1.0 / 0.7))
@pytest.mark.parametrize("H,W", ((7, 11), (37, 70)))
def test_circle_of_confusion_bits(H, W, izf):
    depth, acc = gbuffer(H, W, H)
    izf = float(F(izf))
    lens = lens_of(11.3, izf)
    c = circle_of_confusion(torch.from_numpy(depth).to(DEV)[..., None], torch.from_numpy(acc).to(DEV)[..., None], lens)
    want = L.coc(depth, acc, F(11.3), F(izf))
    assert c.dtype == torch.float32 and tuple(c.shape) == (H, W)
    assert np.array_equal(c.cpu().numpy().view(np.uint32), want.view(np.uint32))  # the same bits, NaNs included
    assert np.isnan(want).any()
    assert float(lens[10]) == izf  # untouched without a focus pixel


def test_circle_of_confusion_reads_its_focus_on_the_device():
    H, W = 7, 11
    depth, acc = gbuffer(H, W, 3)
    d, a = torch.from_numpy(depth).to(DEV), torch.from_numpy(acc).to(DEV)
    seen = set()
    for p in range(H * W):
        lens = lens_of(5.0, 123.0)
        c = circle_of_confusion(d, a, lens, focus_pixel=p)
        izf = L.focus_of(depth, acc, p)
        seen.add(bool(izf > 0))
        assert lens[10].cpu().numpy().view(np.uint32) == np.asarray(izf, F).view(np.uint32), p
        assert np.array_equal(c.cpu().numpy().view(np.uint32), L.coc(depth, acc, F(5.0), izf).view(np.uint32)), p
    assert seen == {False, True}
    lens = lens_of(5.0, 123.0)
    circle_of_confusion(d, a, lens, focus_pixel=0, covered=2.0)  # covered above every accumulation: focus at infinity
    assert float(lens[10]) == 0.0
    with pytest.raises(ValueError, match="focus_pixel"):
        circle_of_confusion(d, a, lens, focus_pixel=H * W)


# ------------------------------------------------------------------------------------------ mark
SIZES = ((5, 9), (37, 70), (65, 130))  # smaller than every window but reach 1's; a tile and a bit; two tiles by three, by one pixel
REACHES = (1, 3, 16, 64)
_marks = {}


def reference_mark(c, threshold, reach, key):
    if key not in _marks:
        _marks[key] = L.mark(c, threshold, reach)
    return _marks[key]


def device_mark(c, threshold, reach):
    m = mark_pixels(torch.from_numpy(c).to(DEV), threshold, reach)
    assert m.dtype == torch.uint8 and tuple(m.shape) == c.shape
    return m.cpu().numpy()


@pytest.mark.parametrize("reach", REACHES)
@pytest.mark.parametrize("H,W", SIZES)
def test_mark_of_random_fields(H, W, reach):
    rng = np.random.default_rng(H * 100 + reach)
    # few blurred pixels, of every radius up to beyond the reach, so that the mask is neither empty nor full; NaN, inf and negative too
    c = ((rng.random((H, W)) < 2.0 / (reach + 2) ** 2) * rng.random((H, W)) * 1.5 * reach).astype(F)
    c[rng.random((H, W)) < 0.02] = np.nan
    c[rng.random((H, W)) < 0.02] = -1.0
    c[H // 2, W // 3] = np.inf
    for threshold in (0.5, 0.0 if reach == 3 else 1.25):
        want = reference_mark(c, threshold, reach, (H, W, reach, threshold))
        got = device_mark(c, threshold, reach)
        print(f"{H} x {W}, reach {reach}, threshold {threshold}: {want.mean():.3f} of the pixels marked")
        assert np.array_equal(got, want)
        assert want.any()
    assert np.array_equal(device_mark(c, 0.5, reach), reference_mark(c, 0.5, reach, (H, W, reach, 0.5)))  # repeatable


@pytest.mark.parametrize("reach", REACHES)
@pytest.mark.parametrize("H,W", SIZES)
def test_mark_of_single_pixels(H, W, reach):
    """one blurred pixel at each corner of the image and at the corners of the 64 x 64 tiles: its mask is the square of its radius, cut by
    the image (the restatement says so too: test_dof_cpu.py)"""
    spots = {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 2)}
    spots |= {(y, x) for y in (63, 64) for x in (63, 64, 127, 128) if y < H and x < W}
    yy, xx = np.mgrid[0:H, 0:W]
    for y, x in sorted(spots):
        for radius in (reach - 0.5, reach + 7.0, 0.5):
            c = np.zeros((H, W), F)
            c[y, x] = radius
            r = min(reach, int(np.floor(F(radius) + F(0.5))))
            want = (np.maximum(abs(yy - y), abs(xx - x)) <= r).astype(np.uint8)
            assert np.array_equal(device_mark(c, 0.5, reach), want), (y, x, radius)
    assert not device_mark(np.zeros((H, W), F), 0.5, reach).any()
    assert not device_mark(np.full((H, W), np.nan, F), 0.0, reach).any()
    assert device_mark(np.zeros((H, W), F), 0.0, reach).all()  # threshold 0: every pixel marks itself


def test_mark_errors():
    c = torch.zeros(4, 5, device=DEV)
    for reach in (0, 65):
        with pytest.raises(ValueError, match="reach"):
            mark_pixels(c, 0.5, reach)
    with pytest.raises(ValueError):
        mark_pixels(c.view(-1), 0.5, 4)
    assert tuple(mark_pixels(torch.zeros(0, 5, device=DEV), 0.5, 4).shape) == (0, 5)


# ------------------------------------------------------------------------------------------ lens rays
def pinhole_bundle(H, W, fov):
    c2w = torch.from_numpy(A.look_at()).float()
    path = CameraPath(W, H, c2w[None], torch.tensor([fov], dtype=torch.float32))
    return camera_rays(path, 0, DEV, camera_index=2)


def host(rb):
    return (rb.origins.cpu().numpy(), rb.directions.cpu().numpy(), rb.metadata["directions_norm"].cpu().numpy())


def border_pixels(H, W):
    P = H * W
    return np.unique(np.concatenate([[0, W - 1, P - W, P - 1], np.arange(P - W, P), np.arange(W - 1, P, W), np.arange(0, P, 5)]))


# what four times the float32 run's worst deviation from the float64 run comes to, per case and output (origins, directions, norm); the
# test computes each before the kernel runs and prints it with the kernel's own worst (on one MI355X: 3.1e-08, 1.5e-07, 2.9e-07):
#   9 x 13, fov 55, rotate:      bars 1.22e-07, 4.91e-07, 8.82e-07
#   9 x 13, fov 55, no rotate:   bars 1.17e-07, 4.40e-07, 9.26e-07
#   64 x 64, fov 3, rotate:      bars 1.24e-07, 5.26e-07, 8.97e-07
#   64 x 64, fov 3, no rotate:   bars 1.20e-07, 5.49e-07, 8.38e-07
@pytest.mark.parametrize("rotate", (True, False))
@pytest.mark.parametrize("H,W,fov,a,z_f", ((9, 13, 55.0, 0.03, 0.6), (64, 64, 3.0, 0.02, 0.45)))
def test_lens_rays_against_float64(H, W, fov, a, z_f, rotate):
    rb = pinhole_bundle(H, W, fov)
    o, d, n = host(rb)
    S = 16
    dof = DepthOfField(a, focus_distance=z_f, samples=S, rotate=rotate)
    pixels = border_pixels(H, W)  # the four corners, the last row and column, and pixels inside
    # the lens block: the device's float64 against numpy's, then its float32 values into both runs of the restatement
    block = lens_block(lens_frame(rb), a, 1.0 / z_f)
    ref = L.lens_block(d, n, a, 1.0 / z_f)
    assert block.dtype == torch.float32 and tuple(block.shape) == (12,)
    assert (np.abs(block.double().cpu().numpy() - ref) <= 2.0 ** -23 * np.maximum(1.0, np.abs(ref))).all()
    lens = block.cpu().numpy()
    table = lens_table(S).numpy()
    hi = L.lens_rays(o, d, n, pixels, table, lens, rotate=rotate)
    lo = L.lens_rays(o, d, n, pixels, table, lens, rotate=rotate, dtype=F)
    bars = [4.0 * float(np.abs(x.astype(np.float64) - y).max()) for x, y in zip(lo, hi)]
    assert all(b > 0 for b in bars)
    out = lens_rays(rb, torch.from_numpy(pixels), dof)
    N = len(pixels) * (S - 1)
    assert tuple(out.origins.shape) == (N, 3) and tuple(out.directions.shape) == (N, 3) and tuple(out.metadata["directions_norm"].shape) == (N, 1)
    got = (out.origins.cpu().numpy(), out.directions.cpu().numpy(), out.metadata["directions_norm"].cpu().numpy()[:, 0])
    for name, g, want, bar in zip(("origins", "directions", "directions_norm"), got, hi, bars):
        worst = float(np.abs(g.astype(np.float64) - want).max())
        print(f"{H} x {W}, fov {fov:g}, rotate {rotate}: {name} worst difference from float64 {worst:.2e}, bar {bar:.2e}")
        assert worst <= bar, (name, worst, bar)
    # every lens ray of a pixel passes through its point of the plane in focus, to float32
    w = ref[6:9]
    da, na = A.subpixel_rays(d.astype(np.float64), n.astype(np.float64), pixels, table[:, :2].astype(np.float64), dtype=np.float64)
    Dp = da * na[:, None]
    focus = np.repeat(o.reshape(-1, 3)[pixels].astype(np.float64), S - 1, 0) + Dp * (z_f / (Dp @ w))[:, None]
    to = focus - got[0]
    off = to - (to * got[1]).sum(1, keepdims=True) * got[1].astype(np.float64)
    assert np.linalg.norm(off, axis=1).max() <= 2e-6
    # what is copied from the pixel
    rows = torch.from_numpy(np.repeat(pixels, S - 1)).to(DEV)
    assert torch.equal(out.pixel_area, rb.pixel_area.view(-1, 1)[rows]) and torch.equal(out.camera_indices, rb.camera_indices.view(-1, 1)[rows])
    assert int(out.camera_indices[0]) == 2
    # a given focus (a frame's dof_focus) in place of the value's
    again = lens_rays(rb, torch.from_numpy(pixels), DepthOfField(a, samples=S, rotate=rotate), focus=block[10:11])
    assert torch.equal(again.directions, out.directions) and torch.equal(again.origins, out.origins)


def test_lens_rays_edge_cases():
    H, W = 9, 13
    rb = pinhole_bundle(H, W, 55.0)
    o, d, n = host(rb)
    dof = DepthOfField(0.03, focus_distance=0.6, samples=4)
    empty = lens_rays(rb, torch.zeros(0, dtype=torch.long), dof)
    assert tuple(empty.directions.shape) == (0, 3) and tuple(empty.origins.shape) == (0, 3)
    lens = lens_block(lens_frame(rb), 0.03, 1.0 / 0.6).cpu().numpy()
    for p in (0, H * W - 1, 5 * W + 12, 8 * W + 3):  # a one-pixel list: a corner, the last pixel, the last column, the last row
        out = lens_rays(rb, torch.tensor([p]), dof)
        want = L.lens_rays(o, d, n, [p], lens_table(4).numpy(), lens)
        assert np.abs(out.directions.cpu().numpy() - want[1]).max() <= 1e-6 and np.abs(out.origins.cpu().numpy() - want[0]).max() <= 1e-6
    # a lens of radius 0: the antialiasing pass's sub-pixel rays, the rows of the table as its offsets
    zero = lens_rays(rb, torch.arange(H * W), DepthOfField(0.0, focus_distance=0.6, samples=4))
    d32, n32 = A.subpixel_rays(d, n, np.arange(H * W), lens_table(4).numpy()[:, :2])
    assert torch.equal(zero.origins, rb.origins.view(-1, 3).repeat_interleave(3, 0))
    assert np.abs(zero.directions.cpu().numpy() - d32).max() <= 2.0 ** -22
    assert np.abs(zero.metadata["directions_norm"].cpu().numpy()[:, 0] / n32 - 1.0).max() <= 1e-6


def test_lens_rays_errors():
    rb = pinhole_bundle(4, 5, 55.0)
    dof = DepthOfField(0.03, focus_distance=0.6, samples=4)
    with pytest.raises(ValueError, match="pixels"):
        lens_rays(rb, torch.tensor([0, 20]), dof)
    with pytest.raises(ValueError, match="pixels"):
        lens_rays(rb, torch.tensor([-1]), dof)
    flat = RayBundle(rb.origins.view(-1, 3), rb.directions.view(-1, 3))
    with pytest.raises(ValueError, match=r"\[H, W\]"):
        lens_rays(flat, torch.tensor([0]), dof)
    with pytest.raises(ValueError, match="focus"):
        lens_rays(rb, torch.tensor([0]), DepthOfField(0.03, samples=4))
    with pytest.raises(ValueError, match="DepthOfField"):
        lens_rays(rb, torch.tensor([0]), 4)
    bent = RayBundle(rb.origins, rb.directions.clone(), metadata=dict(rb.metadata))
    bent.directions[0, 0, 0] += 0.05
    with pytest.raises(ValueError, match="pinhole"):
        lens_rays(bent, torch.tensor([0]), dof)
    with pytest.raises(ValueError, match="pinhole"):
        lens_frame(bent)
