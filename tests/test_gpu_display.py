"""The display transform's kernels (csrc/display.hip) against the numpy restatement of their definitions (display_cpu.py): the histogram
integer for integer, the exposure to two float32 ulps, the bloom and the mapped image against float64 on the same float32 inputs."""
import numpy as np
import pytest
import torch

import display_cpu as D
from neusky_amd import hip
from neusky_amd.relight import DisplayTransform
from neusky_amd.relight.display import bloom_weights

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
LIN_BAR = 1e-5  # the project's bar on a linear image, relative to its largest entry
RGB_BAR = 1e-4  # and on rendered radiance, absolute
EDGES = [2.0 ** -24, float(np.nextafter(F32(2.0 ** -24), F32(0))), 1.0, 1.0 + 1.0 / 64.0, float(np.nextafter(F32(2), F32(0))),
         float(np.nextafter(F32(2.0 ** 24), F32(0))), 2.0 ** 24, 0.0, -1.0, -1e-3, 1e-40, float("inf"), float("nan"), 2.0 ** 25, 3e38]
# pixel counts: 1, around a wave, beyond a workgroup, beyond one pass of the scalar grid (256 workgroups of 256), and a multiple of 4
# beyond one pass of the 4-pixel grid
COUNTS = (1, 63, 64, 65, 257, 70001, 262148 + 8)


def _pixels(P, K, seed):
    """[K, 1, P, 3] float32: grey pixels at the edge luminances first (as many as fit; image k starts at edge k), random ones after"""
    rng = np.random.default_rng(seed)
    lin = (np.exp(rng.uniform(-8.0, 8.0, size=(K, 1, P, 3))) * rng.uniform(0.1, 4.0)).astype(F32)
    for k in range(K):
        e = np.roll(np.array(EDGES, dtype=F32), -k)[:P]
        lin[k, 0, :len(e)] = e[:, None]
    return lin


def _hist_cpu(lin, mask=None, thr=None):
    return np.stack([D.histogram(lin[k], None if mask is None else mask[k], thr) for k in range(lin.shape[0])])


@pytest.fixture(scope="module")
def references():
    """the restatement's histograms, computed once per (P, K) and left unchanged"""
    out = {}
    for P in COUNTS:
        for K in (1, 3):
            lin = _pixels(P, K, P + K)
            mask = np.random.default_rng(P).uniform(size=(K, 1, P)).astype(F32)
            out[P, K] = (lin, mask, _hist_cpu(lin), _hist_cpu(lin, mask, 0.5))
    return out


def test_grey_edges_keep_their_luminance():
    """a grey pixel's luminance is its value only up to the rounding of the three weights: the edges are metered as the restatement's
    float32 luminance says, which is what the kernel is compared against"""
    Y = D.luminance(np.array(EDGES, dtype=F32)[:, None].repeat(3, axis=1))
    assert D.bins_of(Y)[2] in (1535, 1536) and D.bins_of(Y)[7:13].tolist() == [-1] * 6


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("P", COUNTS)
def test_histogram_is_integer_equal(references, P, K):
    lin, mask, want, want_masked = references[P, K]
    t = DisplayTransform(meter_mask_threshold=0.5)
    dl, dm = torch.from_numpy(lin).to(DEV), torch.from_numpy(mask).to(DEV)
    got = DisplayTransform().luminance_histogram(dl)
    assert got.dtype == torch.int64 and got.shape == (K, 3072)
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(t.luminance_histogram(dl, dm).cpu().numpy(), want_masked)
    assert np.array_equal(DisplayTransform().luminance_histogram(dl, dm).cpu().numpy(), want)  # no threshold: the mask is not read
    assert torch.equal(DisplayTransform().luminance_histogram(dl), got)  # two runs, the same bits
    shared = torch.zeros(1, 3072, dtype=torch.int64, device=DEV)
    assert np.array_equal(DisplayTransform().luminance_histogram(dl, out=shared).cpu().numpy(), want.sum(axis=0, keepdims=True))


def test_histogram_of_exact_edges():
    """luminances exactly at the edges, one pixel per launch: the bins of the header's list, straight from the kernel"""
    # with r = g = 0 the luminance is the one product 0.0722f b: take b = e / 0.0722f, nudged until the product is the edge itself
    e = np.array(EDGES[:7], dtype=F32)
    b = (e / F32(0.0722)).astype(F32)
    lin = np.zeros((1, 1, len(e), 3), dtype=F32)
    lin[0, 0, :, 2] = b
    Y = D.luminance(lin[0, 0])
    for i in range(len(e)):  # nudge b by ulps until the float32 product is the edge itself
        for step in range(-4, 5):
            cand = b[i]
            for _ in range(abs(step)):
                cand = np.nextafter(cand, F32(np.inf) if step > 0 else F32(0))
            if F32(F32(0.0722) * cand) == e[i]:
                lin[0, 0, i, 2] = cand
                break
    Y = D.luminance(lin[0, 0])
    exact = Y == e
    assert exact.sum() >= 5, (Y, e)
    want = [0, -1, 1536, 1537, 1599, 3071, 3071]
    for i in np.nonzero(exact)[0]:
        got = DisplayTransform().luminance_histogram(torch.from_numpy(lin[:, :, i:i + 1]).to(DEV))[0].cpu().numpy()
        assert got.sum() == (0 if want[i] < 0 else 1) and (want[i] < 0 or got[want[i]] == 1), (i, np.nonzero(got))


def test_accumulating_two_calls_is_the_histogram_of_the_concatenation(references):
    a, _, ha, _ = references[257, 3]
    b, _, hb, _ = references[70001, 3]
    t = DisplayTransform()
    out = t.luminance_histogram(torch.from_numpy(a).to(DEV))
    same = t.luminance_histogram(torch.from_numpy(b).to(DEV), out=out)
    assert same is out
    both = _hist_cpu(np.concatenate([a, b], axis=2))
    assert np.array_equal(out.cpu().numpy(), both) and np.array_equal(both, ha + hb)


@pytest.mark.parametrize("keywords", [{}, {"key": 0.3, "ev": 1.5, "percentiles": (0.2, 0.6)}, {"percentiles": (0.0, 1.0)}])
def test_exposure_matches_the_restatement(references, keywords):
    t = DisplayTransform(exposure="frame", **keywords)
    for P in (1, 65, 70001):
        _, _, want, _ = references[P, 3]
        hist = torch.from_numpy(want).to(DEV)
        E = t.exposure_from_histogram(hist)
        assert E.dtype == torch.float32 and E.shape == (3,)
        ref = np.array([D.exposure(h, t.key, t.ev, t.percentiles) for h in want])
        rel = np.abs(E.cpu().numpy().astype(np.float64) / ref - 1.0).max()
        print(f"P {P} {keywords}: E {E.tolist()}, rel {rel:.2e}")
        assert rel <= 2.0 ** -22
    empty = torch.zeros(2, 3072, dtype=torch.int64, device=DEV)
    assert t.exposure_from_histogram(empty).tolist() == [1.0, 1.0]  # nothing metered
    one = empty.clone()
    one[0, 1536] = 1  # one pixel, percentiles (0.05, 0.95): a = 0, b = 1
    one[1, 100] = 19  # a = 0, b = 19 - 0
    E = t.exposure_from_histogram(one).cpu().numpy().astype(np.float64)
    ref = np.array([D.exposure(h, t.key, t.ev, t.percentiles) for h in one.cpu().numpy()])
    assert np.abs(E / ref - 1.0).max() <= 2.0 ** -22


def test_scaling_by_a_power_of_two_is_exact_on_the_device():
    # luminances within 2^-8 .. 2^8: room for 2^3 and 2^-5 inside the histogram's 48 octaves
    lin = np.exp(np.random.default_rng(8).uniform(-4.0, 4.0, size=(1, 1, 70001, 3))).astype(F32)
    t = DisplayTransform(curve="aces", exposure="frame")
    for k in (3, -5):
        a = torch.from_numpy(lin).to(DEV)
        b = torch.from_numpy(lin * F32(2.0 ** k)).to(DEV)
        ha, hb = t.luminance_histogram(a), t.luminance_histogram(b)
        assert torch.equal(hb, torch.roll(ha, 64 * k, dims=1))
        Ea, Eb = t.exposure_from_histogram(ha), t.exposure_from_histogram(hb)
        assert torch.equal(Eb, Ea * 2.0 ** -k), (Ea, Eb)
        # and so the picture does not change: E lin is the same float
        assert torch.equal(t.apply(a)["rgb8"], t.apply(b)["rgb8"])


# ------------------------------------------------------------------------------------------ bloom
SHAPES = ((1, 1), (1, 300), (300, 1), (5, 7), (33, 257), (70, 130))


@pytest.mark.parametrize("sigma", [0.5, 4.0, 32.0])
@pytest.mark.parametrize("shape", SHAPES)
def test_blur_matches_float64(shape, sigma):
    H, W = shape
    rng = np.random.default_rng(H * 1000 + W)
    lin = np.zeros((2, H, W, 3), dtype=F32)  # image 0 bright, image 1 all zero: its bloom must be exactly 0
    lin[0] = (np.exp(rng.uniform(-3.0, 6.0, size=(H, W, 3)))).astype(F32)
    lin[0].reshape(-1)[::7] = 0.0
    lin[0].reshape(-1)[3::11] = np.nan  # a NaN is no source
    E, thr = F32(0.7), F32(1.25)
    t = DisplayTransform(bloom_sigma=sigma, bloom_threshold=float(thr))
    w = bloom_weights(sigma)
    assert w.numel() == 2 * int(np.ceil(3 * sigma)) + 1 and np.array_equal(w.numpy(), D.gaussian_weights(sigma).astype(F32))
    dl = torch.from_numpy(lin).to(DEV)
    B, scratch = torch.full_like(dl, float("nan")), torch.full_like(dl, float("nan"))
    hip.display_blur(dl, torch.tensor([float(E), float(E)], dtype=torch.float32, device=DEV), t.params(DEV), w.to(DEV), scratch, B)
    src = D.bloom_source(lin[0], E, thr)
    want = D.blur(src.astype(np.float64), w.numpy().astype(np.float64))
    got = B.cpu().numpy()
    err = np.abs(got[0] - want).max()
    print(f"{shape} sigma {sigma}: worst {err:.2e} of a source up to {src.max():.3g} (bar {LIN_BAR * src.max():.2e})")
    assert np.isfinite(got).all() and err <= LIN_BAR * float(src.max())
    assert not got[1].any(), "image 1 is black: nothing of image 0 may reach it"
    B1 = torch.empty_like(dl)
    hip.display_blur(dl, torch.tensor([float(E)], dtype=torch.float32, device=DEV), t.params(DEV), w.to(DEV), scratch, B1)  # one exposure for both, and a second run
    assert torch.equal(B1, B)


# ------------------------------------------------------------------------------------------ map
SPECIAL = [0.0, -0.0, -1.0, -1e-8, float("nan"), 1e-8, 0.0031, 0.0031308, 0.0032, 0.5, 1.0, 1.5, 1e4, float("inf"), 3e38]


def _map_input(P, seed):
    """[1, 1, P, 3]: the special values first (across the channels), then random ones; for every curve some values land on both sides
    of 0.0031308 after the curve (near 0 every curve is close to a multiple of x: the ladder below covers them)"""
    rng = np.random.default_rng(seed)
    lin = (np.exp(rng.uniform(-9.0, 5.0, size=(P * 3,)))).astype(F32)
    vals = np.array(SPECIAL + list(0.0031308 * np.array([0.1, 0.2, 0.4, 0.6, 0.9, 1.1, 1.7, 2.5, 5.0, 10.0])), dtype=F32)
    n = min(len(vals), P * 3)
    lin[:n] = vals[:n]
    return lin.reshape(1, 1, P, 3)


@pytest.mark.parametrize("curve", D.CURVES)
@pytest.mark.parametrize("P", [1, 63, 64, 65, 257])
def test_map_matches_float64(P, curve):
    lin = _map_input(P, P)
    if P == 257:
        with np.errstate(over="ignore"):  # (3e38 becomes inf)
            lin = np.concatenate([lin, _map_input(P, 1)[..., ::-1, :] * F32(3.0)])  # K = 2, each image under its own exposure
    K = lin.shape[0]
    t = DisplayTransform(curve=curve, exposure="frame", white=3.0)
    res = t.apply(torch.from_numpy(lin).to(DEV))
    E = res["exposure"].cpu().numpy()
    assert E.shape == (K,) and res["rgb"].shape == lin.shape and res["rgb8"].shape == lin.shape and res["rgb8"].dtype == torch.uint8
    want = D.display_map(lin, E.reshape(K, 1, 1, 1), curve, white=3.0)
    got = res["rgb"].cpu().numpy()
    assert np.isfinite(got).all() and got.min() >= 0.0 and got.max() <= 1.0
    err = np.abs(got - want).max()
    y = D.curve(np.maximum(np.nan_to_num(E.reshape(K, 1, 1, 1).astype(np.float64) * lin, nan=0.0, posinf=2.0 ** 60), 0), curve, 3.0)
    print(f"P {P} {curve}: E {E.tolist()}, worst {err:.2e}; after the curve {int((y <= 0.0031308).sum())} values at or below 0.0031308, "
          f"{int((y > 0.0031308).sum())} above")
    if P >= 63:
        assert (y[y > 0] <= 0.0031308).any() and (y > 0.0031308).any()
    assert err <= RGB_BAR
    # the bytes are the rounding of the kernel's own float image, ties to even
    assert torch.equal(res["rgb8"], torch.round(res["rgb"] * 255).to(torch.uint8))
    # a set exposure, with the float image left out of nothing: the same kernel, E from the caller
    again = t.apply(torch.from_numpy(lin).to(DEV), exposure=res["exposure"])
    assert torch.equal(again["rgb"], res["rgb"]) and torch.equal(again["rgb8"], res["rgb8"])


@pytest.mark.parametrize("curve", D.CURVES)
def test_map_with_bloom_matches_float64(curve):
    H, W = 33, 52  # P % 4 == 0: the 4-pixel path with a bloom
    rng = np.random.default_rng(11)
    lin = np.exp(rng.uniform(-6.0, 4.0, size=(2, H, W, 3))).astype(F32)
    lin[0, 5, 5] = [np.nan, -2.0, 900.0]
    t = DisplayTransform(curve=curve, exposure=0.8, bloom_sigma=2.0, bloom_threshold=1.5, bloom_strength=0.35)
    dl = torch.from_numpy(lin).to(DEV)
    res = t.apply(dl)
    assert res["exposure"].tolist() == [float(F32(0.8))]
    w = bloom_weights(2.0)
    B = torch.empty_like(dl)
    hip.display_blur(dl, res["exposure"], t.params(DEV), w.to(DEV), torch.empty_like(dl), B)
    want = D.display_map(lin, F32(0.8), curve, bloom=B.cpu().numpy(), strength=0.35)
    err = np.abs(res["rgb"].cpu().numpy() - want).max()
    print(f"{curve} with bloom: worst {err:.2e}")
    assert err <= RGB_BAR
    assert torch.equal(res["rgb8"], torch.round(res["rgb"] * 255).to(torch.uint8))
    plain = DisplayTransform(curve=curve, exposure=0.8).apply(dl)
    assert not torch.equal(plain["rgb"], res["rgb"])  # the bloom arrived
    off = DisplayTransform(curve=curve, exposure=0.8, bloom_sigma=2.0, bloom_strength=0.0).apply(dl)
    assert torch.equal(off["rgb"], plain["rgb"])


@pytest.mark.parametrize("P", [1, 63, 64, 65, 257])
def test_default_transform_has_the_bits_of_the_relight_kernels_rgb(P):
    """clamp, E = 1, no bloom: rgb is srgb_fwd of the input to the bit, against nsky_transfer_relight's rgb for the same linear image"""
    g = torch.Generator().manual_seed(P)
    Dn = 8
    T = torch.rand(P, Dn, 3, generator=g).to(DEV)
    lights = (torch.rand(1, Dn, 3, generator=g) * 3.0).to(DEV)
    bg = (torch.randn(1, P, 3, generator=g) * 2.0).to(DEV)  # negative values too
    vals = torch.tensor(SPECIAL[:min(len(SPECIAL), 3 * P)])
    bg.view(-1)[:len(vals)] = vals.to(DEV)
    acc = torch.zeros(P, device=DEV)  # lin = T.L + bg: the special values pass through where T's row is zero
    T[:(len(vals) + 2) // 3] = 0.0
    rgb, lin = torch.empty(1, P, 3, device=DEV), torch.empty(1, P, 3, device=DEV)
    hip.transfer_relight(T, None, acc, lights, bg, rgb, lin)
    assert bool(torch.isnan(lin).any()) == (P * 3 > 4)
    res = DisplayTransform().apply(lin.view(1, 1, P, 3))
    assert torch.equal(res["rgb"].view(1, P, 3).view(torch.int32), rgb.view(torch.int32))
    assert res["exposure"].tolist() == [1.0]
    assert torch.equal(res["rgb8"].view(1, P, 3), torch.round(rgb * 255).to(torch.uint8))


def test_argument_errors():
    t = DisplayTransform()
    lin = torch.zeros(2, 4, 4, 3, device=DEV)
    with pytest.raises(ValueError):
        t.luminance_histogram(lin, out=torch.zeros(3, 3072, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError):
        t.luminance_histogram(lin, out=torch.zeros(2, 3072, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        t.apply(lin, exposure=torch.ones(3, device=DEV))
    with pytest.raises(ValueError):
        t.apply(torch.zeros(4, 4, device=DEV))
    with pytest.raises(ValueError):
        hip.display_blur(lin, torch.ones(1, device=DEV), t.params(DEV), torch.ones(4, device=DEV), torch.empty_like(lin), torch.empty_like(lin))
    flat = t.apply(torch.rand(10, 3, device=DEV))  # [N, 3]: a row of pixels
    assert flat["rgb"].shape == (10, 3) and flat["rgb8"].shape == (10, 3)
