"""The three antialiasing kernels (csrc/antialias.hip) alone, against their numpy restatement (antialias_cpu.py): the edge mask exactly,
the sub-pixel rays against the float64 pinhole to 1e-6 (the number format's bar: include/neusky_hip.h), the resolve against float64 to
one float32 rounding."""
import numpy as np
import pytest
import torch

import antialias_cpu as A
from neusky_amd import hip
from neusky_amd.cameras.rays import RayBundle
from neusky_amd.relight import Antialias, CameraPath, camera_rays, r2_offsets, subpixel_rays
from neusky_amd.relight.antialias import resolve

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = ((1, 1), (1, 7), (7, 1), (5, 7), (33, 17), (64, 65))  # none a multiple of a block of 256 pixels; the last two span several


def device_mask(s, aa=Antialias()):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    return aa.edge_mask(t(s["depth"])[..., None], t(s["normal"]), t(s["acc"])[..., None], t(s["lin"]) if s["lin"].shape[0] else None).cpu().numpy()


@pytest.mark.parametrize("K", (1, 3))
@pytest.mark.parametrize("H,W", SIZES)
def test_edge_mask_is_the_restatements(H, W, K):
    s, kinds = A.synthetic_gbuffer(H, W, K, seed=H * 100 + W + K)
    want = A.edge_mask(**s)
    got = device_mask(s)
    assert got.dtype == np.uint8 and got.shape == (H, W) and set(np.unique(got)) <= {0, 1}
    assert np.array_equal(got, want)
    if H * W > 1000:  # every kind of block occurs: something is marked, something is not
        assert len(np.unique(kinds)) == 8 and 0 < want.sum() < H * W
    # other thresholds, by value: the same restatement
    aa = Antialias(colour=0.25, depth=0.05, normal_deg=45.0, accumulation=0.25, covered=0.2)
    assert np.array_equal(device_mask(s, aa), A.edge_mask(**s, colour=0.25, depth_t=0.05, normal_deg=45.0, accumulation=0.25, covered=0.2))
    assert device_mask(s, Antialias(every_pixel=True)).all()


@pytest.mark.parametrize("criterion", ("accumulation", "depth", "normal", "colour"))
def test_a_pixel_marked_by_one_criterion_alone(criterion):
    H, W, K = 5, 7, 3
    s = dict(depth=np.full((H, W), 2.0, np.float32), normal=np.tile(np.float32([0, 0, 1]), (H, W, 1)), acc=np.ones((H, W), np.float32),
             lin=np.full((K, H, W, 3), 0.5, np.float32))
    assert not device_mask(s).any()
    at = {"accumulation": (2, 3), "depth": (0, 0), "normal": (4, 6), "colour": (1, 5)}[criterion]
    if criterion == "accumulation":
        s["acc"][at] = 0.875
    elif criterion == "depth":
        s["depth"][at] = 2.0625
    elif criterion == "normal":
        s["normal"][at] = (0.0, 0.5, 0.75)
    else:
        s["lin"][1][at] = (0.5, 0.625, 0.5)  # the middle image alone
    got = device_mask(s)
    assert got[at] == 1 and np.array_equal(got, A.edge_mask(**s, criteria=(criterion,))) and np.array_equal(got, A.edge_mask(**s))
    # an uncovered pair: depth and normal must not fire; a zero normal switches its pairs' normal test off
    s["acc"][:] = 0.25
    s["depth"][3, 1], s["normal"][3, 5] = 9.0, (1.0, 0.0, 0.0)
    hidden = device_mask(s)
    assert np.array_equal(hidden, A.edge_mask(**s)) and hidden[3, 1] == 0 and hidden[3, 5] == 0
    s["acc"][:] = 1.0
    s["lin"][:] = 0.5
    s["depth"][:] = 2.0
    s["normal"][:] = (0.0, 0.0, 1.0)
    s["normal"][2, 2] = 0.0
    assert not device_mask(s).any()


# ------------------------------------------------------------------------------------------ rays
def pinhole_bundle(H, W, fov):
    c2w = torch.from_numpy(A.look_at()).float()
    path = CameraPath(W, H, c2w[None], torch.tensor([fov], dtype=torch.float32))
    return camera_rays(path, 0, DEV, camera_index=2), c2w.double().numpy(), float(path.fov[0])


def border_pixels(H, W):
    P = H * W
    return np.unique(np.concatenate([[0, W - 1, P - W, P - 1], np.arange(P - W, P), np.arange(W - 1, P, W), np.arange(0, P, 5)]))


@pytest.mark.parametrize("S1", (1, 3, 15))
@pytest.mark.parametrize("H,W,fov", ((9, 13, 55.0), (5, 7, 120.0)))
def test_subpixel_rays_are_the_float64_pinholes(H, W, fov, S1):
    rb, c2w, fov = pinhole_bundle(H, W, fov)
    pixels = border_pixels(H, W)  # the four corners, the last row and column, and pixels inside
    offsets = r2_offsets(S1 + 1)
    out = subpixel_rays(rb, torch.from_numpy(pixels), offsets)
    N = len(pixels) * S1
    assert tuple(out.origins.shape) == (N, 3) and tuple(out.directions.shape) == (N, 3) and tuple(out.metadata["directions_norm"].shape) == (N, 1)
    want, want_n = A.pinhole_subpixel(H, W, fov, c2w, pixels, offsets.numpy())
    got, got_n = out.directions.double().cpu().numpy(), out.metadata["directions_norm"].double().cpu().numpy()[:, 0]
    worst = np.abs(got - want).max()
    print(f"{H} x {W}, fov {fov:g}, {S1} offsets: worst difference of a direction component {worst:.2e}")
    assert worst <= 1e-6
    assert np.abs(got_n / want_n - 1.0).max() <= 1e-6
    # and the float32 restatement, the same order of operations
    d32, n32 = A.subpixel_rays(rb.directions.cpu().numpy(), rb.metadata["directions_norm"].cpu().numpy(), pixels, offsets.numpy())
    assert np.abs(out.directions.cpu().numpy() - d32).max() <= 2.0 ** -22 and np.abs(got_n / n32 - 1.0).max() <= 2.0 ** -22
    # what is copied from the pixel
    rows = torch.from_numpy(np.repeat(pixels, S1)).to(DEV)
    assert torch.equal(out.origins, rb.origins.view(-1, 3)[rows])
    assert torch.equal(out.pixel_area, rb.pixel_area.view(-1, 1)[rows]) and torch.equal(out.camera_indices, rb.camera_indices.view(-1, 1)[rows])
    assert int(out.camera_indices[0]) == 2


@pytest.mark.parametrize("H,W", ((1, 1), (1, 6), (6, 1)))
def test_subpixel_rays_of_a_frame_without_an_axis(H, W):
    """where an axis has one pixel its difference is zero: the samples coincide along it"""
    rb, c2w, fov = pinhole_bundle(max(H, 2), max(W, 2), 55.0)
    cut = lambda t: t[:H, :W].contiguous()  # noqa: E731
    rb = RayBundle(cut(rb.origins), cut(rb.directions), cut(rb.pixel_area), cut(rb.camera_indices),
                   metadata={"directions_norm": cut(rb.metadata["directions_norm"])})
    pixels = np.arange(H * W)
    offsets = r2_offsets(4)
    out = subpixel_rays(rb, torch.from_numpy(pixels), offsets)
    kept = offsets.numpy().astype(np.float64) * np.array([W > 1, H > 1], dtype=np.float64)  # (the missing axis' offset does nothing)
    want, _ = A.pinhole_subpixel(max(H, 2), max(W, 2), fov, c2w, (pixels // W) * max(W, 2) + pixels % W, kept)
    assert np.abs(out.directions.double().cpu().numpy() - want).max() <= 1e-6
    if H == 1 and W == 1:
        assert torch.equal(out.directions, out.directions[:1].expand(3, 3))  # one ray, three times
    # a bundle without directions_norm: norm 1
    bare = RayBundle(rb.origins, rb.directions)
    again = subpixel_rays(bare, torch.from_numpy(pixels), offsets)
    d32, n32 = A.subpixel_rays(rb.directions.cpu().numpy(), None, pixels, offsets.numpy())
    assert np.abs(again.directions.cpu().numpy() - d32).max() <= 2.0 ** -22 and again.pixel_area is None and again.camera_indices is None


def test_subpixel_rays_errors():
    rb, _, _ = pinhole_bundle(4, 5, 55.0)
    with pytest.raises(ValueError, match="pixels"):
        subpixel_rays(rb, torch.tensor([0, 20]), r2_offsets(4))
    with pytest.raises(ValueError, match="pixels"):
        subpixel_rays(rb, torch.tensor([-1]), r2_offsets(4))
    flat = RayBundle(rb.origins.view(-1, 3), rb.directions.view(-1, 3))
    with pytest.raises(ValueError, match=r"\[H, W\]"):
        subpixel_rays(flat, torch.tensor([0]), r2_offsets(4))
    empty = subpixel_rays(rb, torch.zeros(0, dtype=torch.long), r2_offsets(4))
    assert tuple(empty.directions.shape) == (0, 3)


# ------------------------------------------------------------------------------------------ resolve
@pytest.mark.parametrize("E", ("none", "one", "all"))
@pytest.mark.parametrize("layout", ("K leads in memory", "ray-major in memory"))
@pytest.mark.parametrize("K", (1, 3))
@pytest.mark.parametrize("C", (1, 3))
def test_resolve_against_float64(C, K, layout, E):
    P, S1 = 301, 3  # (E K C = 2709 at the most: several blocks)
    g = torch.Generator().manual_seed(C * 10 + K)
    frame = (torch.rand(K, P, C, generator=g) * 4.0).to(DEV)
    if layout == "ray-major in memory":  # a frame of K suns as its chunks assemble it: [P, K, C], K leading in the shape alone
        frame = frame.permute(1, 0, 2).contiguous().permute(1, 0, 2)
        assert frame.is_contiguous() == (K == 1)
    frame[0, 5] = 1e-3  # below the sRGB curve's knee after the average
    pixels = {"none": torch.zeros(0, dtype=torch.long), "one": torch.tensor([P - 1]), "all": torch.randperm(P, generator=g)}[E].to(DEV)
    n = pixels.shape[0]
    # the samples as the second pass's chunks arrive: ray-major [E S1, K, C]; K leads only through the strides
    arrived = (torch.rand(n * S1, K, C, generator=g) * 4.0).to(DEV)
    if n:
        arrived[(pixels == 5).nonzero().view(-1) * S1] = 2e-3
    X = arrived.view(n, S1, K, C)
    before, rgb = frame.clone(), torch.full_like(frame, -1.0)
    resolve(frame, X, pixels, rgb)
    want = A.resolve(before.cpu().numpy(), X.permute(2, 0, 1, 3).cpu().numpy(), pixels.cpu().numpy())
    got = frame.double().cpu().numpy()
    err = np.abs(got - want)
    print(f"C {C} K {K} E {n}: worst difference {err.max():.2e}")
    assert np.all(err <= np.maximum(2.0 ** -22 * np.abs(want), 1e-7))
    listed = torch.zeros(P, dtype=torch.bool, device=DEV)
    listed[pixels] = True
    assert torch.equal(frame[:, ~listed].view(torch.int32), before[:, ~listed].view(torch.int32))  # unlisted pixels keep their bits
    assert bool((rgb[:, ~listed] == -1.0).all())
    if n:
        assert not torch.equal(frame[:, listed], before[:, listed])
        assert np.abs(rgb[:, listed].double().cpu().numpy() - A.srgb(frame[:, listed].cpu().numpy())).max() <= 1e-6
    # without rgb: the same frame
    again = before.clone()
    resolve(again, X, pixels)
    assert torch.equal(again, frame)


def test_resolve_refuses_a_frame_it_cannot_address():
    frame, X = torch.zeros(2, 9, 3, device=DEV), torch.zeros(4, 3, 2, 3, device=DEV)
    with pytest.raises(ValueError):
        hip.aa_resolve(frame.permute(1, 0, 2), X.permute(2, 0, 1, 3), torch.arange(4, device=DEV))  # a frame that is not K-leading contiguous
    with pytest.raises(ValueError):
        hip.aa_resolve(frame, X.permute(2, 0, 1, 3)[..., :2], torch.arange(4, device=DEV))
