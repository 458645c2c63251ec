"""relight.DepthOfField on the host: the value's and the command line's validation, the sample table, and the numpy restatement (dof_cpu.py)
against the geometry it claims: on a float64 pinhole bundle every lens ray of a pixel passes through the pixel's point on the plane in
focus, `depth` along a lens ray stays the z-depth, a point at depth z lands a f_px (1 / z - 1 / z_f) (u, v) pixels from its pinhole image,
a lens of radius 0 gives the antialiasing pass's sub-pixel rays, and focus at infinity gives parallel rays; and the mark against a plain
double loop over all pairs of pixels."""
import math

import numpy as np
import pytest
import torch

import antialias_cpu as A
import dof_cpu as L
from neusky_amd.relight import DepthOfField, lens_table
from neusky_amd.relight.__main__ import build_parser, parse_depth_of_field

F = np.float32


def test_depth_of_field_validation():
    d = DepthOfField(0.01)
    assert (d.aperture, d.focus_distance, d.focus_pixel, d.samples, d.threshold, d.reach, d.covered, d.every_pixel, d.rotate, d.table,
            d.batch_pixels) == (0.01, None, None, 16, 0.5, 16, 0.5, False, True, None, 1 << 18)
    assert DepthOfField(0).aperture == 0.0 and isinstance(DepthOfField(1).aperture, float)
    assert d.focus_index(9, 13) == 4 * 13 + 6 and DepthOfField(0.01, focus_pixel=(12, 8)).focus_index(9, 13) == 9 * 13 - 1
    assert DepthOfField(0.01, focus_distance=2).focus_index(9, 13) == -1
    with pytest.raises(dataclasses_error()):
        d.aperture = 1.0
    bad = [dict(aperture=-1.0), dict(aperture=math.inf), dict(aperture=math.nan), dict(aperture="wide"), dict(aperture=None),
           dict(aperture=0.01, focus_distance=0.0), dict(aperture=0.01, focus_distance=-1.0), dict(aperture=0.01, focus_distance=math.inf),
           dict(aperture=0.01, focus_distance=1.0, focus_pixel=(1, 1)), dict(aperture=0.01, focus_pixel=(1,)),
           dict(aperture=0.01, focus_pixel=(-1, 0)), dict(aperture=0.01, focus_pixel=(0.5, 1)), dict(aperture=0.01, focus_pixel=3),
           dict(aperture=0.01, samples=1), dict(aperture=0.01, samples=65), dict(aperture=0.01, samples=4.0), dict(aperture=0.01, samples=True),
           dict(aperture=0.01, reach=0), dict(aperture=0.01, reach=65), dict(aperture=0.01, reach=2.5),
           dict(aperture=0.01, threshold=-0.5), dict(aperture=0.01, threshold=math.nan), dict(aperture=0.01, covered=-1.0),
           dict(aperture=0.01, batch_pixels=0),
           dict(aperture=0.01, samples=3, table=torch.zeros(3, 4)), dict(aperture=0.01, samples=3, table=torch.zeros(2, 2)),
           dict(aperture=0.01, samples=2, table=[[0.6, 0.0, 0.0, 0.0]]), dict(aperture=0.01, samples=2, table=[[0.0, -0.51, 0.0, 0.0]]),
           dict(aperture=0.01, samples=2, table=[[0.0, 0.0, 0.8, 0.8]]), dict(aperture=0.01, samples=2, table=[[0.0, 0.0, math.nan, 0.0]])]
    for kw in bad:
        with pytest.raises(ValueError):
            DepthOfField(**kw)
    with pytest.raises(ValueError, match="outside the frame"):
        DepthOfField(0.01, focus_pixel=(13, 0)).focus_index(9, 13)
    own = DepthOfField(0.01, samples=3, table=[[0.5, -0.5, 1.0, 0.0], [0.0, 0.25, -0.6, 0.8]])
    assert own.table.dtype == torch.float32 and torch.equal(own.sample_table(), own.table)
    assert torch.equal(DepthOfField(0.01, samples=5).sample_table(), lens_table(5))


def dataclasses_error():
    import dataclasses
    return dataclasses.FrozenInstanceError


BASE = ["--checkpoint", "c", "--camera-path", "p", "--output-dir", "o", "--latent-index", "0"]


def _parse(*flags):
    ap = build_parser()
    return parse_depth_of_field(ap, ap.parse_args(BASE + list(flags)))


def test_command_line_parser(capsys):
    assert _parse() is None
    d = _parse("--dof-aperture", "0.02")
    assert isinstance(d, DepthOfField) and (d.aperture, d.focus_distance, d.focus_pixel, d.samples, d.reach, d.every_pixel) == \
        (0.02, None, None, 16, 16, False)
    d = _parse("--dof-aperture", "0.02", "--dof-focus-distance", "1.5", "--dof-samples", "8", "--dof-threshold", "1", "--dof-reach", "32",
               "--dof-all", "--dof-map")
    assert (d.focus_distance, d.samples, d.threshold, d.reach, d.every_pixel) == (1.5, 8, 1.0, 32, True)
    assert _parse("--dof-aperture", "0", "--dof-focus-pixel", "3", "4").focus_pixel == (3, 4)
    refused = [(("--dof-focus-distance", "1"), "--dof-focus-distance needs --dof-aperture"),
               (("--dof-focus-pixel", "1", "2"), "--dof-focus-pixel needs --dof-aperture"),
               (("--dof-samples", "4"), "--dof-samples needs --dof-aperture"), (("--dof-threshold", "1"), "--dof-threshold needs --dof-aperture"),
               (("--dof-reach", "4"), "--dof-reach needs --dof-aperture"), (("--dof-all",), "--dof-all needs --dof-aperture"),
               (("--dof-map",), "--dof-map needs --dof-aperture"),
               (("--dof-aperture", "0.1", "--dof-focus-distance", "1", "--dof-focus-pixel", "1", "2"), "exclude each other"),
               (("--dof-aperture", "0.1", "--transfer", "fp32"), "--transfer"), (("--dof-all", "--transfer", "fp16"), "--transfer"),
               (("--dof-aperture", "-1"), "aperture"), (("--dof-aperture", "0.1", "--dof-samples", "1"), "samples"),
               (("--dof-aperture", "0.1", "--dof-reach", "65"), "reach"), (("--dof-aperture", "0.1", "--dof-focus-distance", "0"), "focus_distance")]
    for flags, message in refused:
        with pytest.raises(SystemExit) as e:
            _parse(*flags)
        assert e.value.code not in (0, None) and message in capsys.readouterr().err, flags


def test_lens_table():
    g = 1.2
    for _ in range(200):
        g = (g + 1.0) ** 0.2
    assert abs(g - L.R4_G) < 1e-15 and abs(g ** 5 - g - 1.0) < 1e-14
    for S in (2, 4, 16, 64):
        t = lens_table(S)
        assert t.dtype == torch.float32 and tuple(t.shape) == (S - 1, 4)
        ref = L.lens_table(S)
        assert np.array_equal(t.numpy(), ref.astype(F))  # float64 values, rounded once
        assert np.abs(ref[:, :2]).max() <= 0.5 and (ref[:, 2] ** 2 + ref[:, 3] ** 2).max() <= 1.0
        t64 = t.double().numpy()
        assert np.abs(t64[:, :2]).max() <= 0.5 and (t64[:, 2] ** 2 + t64[:, 3] ** 2).max() <= 1.0
    ref = L.lens_table(16)
    # s = 1: t = frac(0.5 + (1 / g, 1 / g^2, 1 / g^3, 1 / g^4)); pinned
    # (1 / g = 0.856674883854..., so dx_1 = frac(1.356674...) - 0.5; (a, b) = (-0.742587, -0.922805): |a| < |b|, r = b,
    # phi = pi / 2 - (pi / 4)(a / b) = 0.938780, (u, v) = b (cos phi, sin phi))
    want = np.array([[-0.143325116145, -0.266108143373, -0.545166761352, -0.744555683937],
                     [-0.286650232291, 0.467783713254, 0.500612998501, 0.12013886289],
                     [-0.149876742182, 0.008377849407, 0.852285922646, 0.123599981908]])
    assert np.abs(ref[[0, 1, 14]] - want).max() < 5e-12, ref[[0, 1, 14]]
    # the 15 lens points spread over the disc: every quadrant is visited, and the mean lies near the centre
    assert all(((np.sign(ref[:, 2]) == a) & (np.sign(ref[:, 3]) == b)).any() for a in (-1, 1) for b in (-1, 1))
    assert np.linalg.norm(ref[:, 2:].mean(0)) < 0.15
    # the concentric map: the square's axes and diagonals
    sq = lambda a, b: ((a, (math.pi / 4) * (b / a)) if abs(a) > abs(b) else (b, math.pi / 2 - (math.pi / 4) * (a / b)))  # noqa: E731
    r, phi = sq(1.0, 1.0)
    assert abs(r * math.cos(phi) - math.sqrt(0.5)) < 1e-15 and abs(r * math.sin(phi) - math.sqrt(0.5)) < 1e-15


def test_hash_restatement():
    # lowbias32: 0 is a fixed point of any xorshift-multiply hash; the others pinned from the statement in the header, by hand
    def by_hand(x):
        x ^= x >> 16
        x = (x * 0x7FEB352D) & 0xFFFFFFFF
        x ^= x >> 15
        x = (x * 0x846CA68B) & 0xFFFFFFFF
        return x ^ (x >> 16)
    xs = [0, 1, 2, 116, 1920 * 1080 - 1, 2 ** 32 - 1]
    assert L.hash32(np.array(xs)).tolist() == [by_hand(x) for x in xs] and by_hand(0) == 0
    h = L.hash32(np.arange(1 << 16)) >> 8
    assert h.max() < 1 << 24 and abs(float(h.mean()) / (1 << 24) - 0.5) < 0.01  # the top 24 bits, spread over the circle


# ------------------------------------------------------------------------------------------ the lens rays on a float64 pinhole
H, W, FOV = 9, 13, 55.0


def pinhole_bundle(h=H, w=W, fov=FOV):
    c2w = A.look_at()
    x, y = np.meshgrid(np.arange(w) + 0.5, np.arange(h) + 0.5)
    d, n = A.pinhole(h, w, fov, c2w, x, y)
    o = np.broadcast_to(c2w[:, 3], (h, w, 3)).copy()
    return o, d, n[..., None], c2w


def test_lens_frame_of_a_pinhole():
    o, d, n, c2w = pinhole_bundle()
    r, s, w, f_px, bend = L.lens_frame(d, n)
    f = 0.5 * H / math.tan(math.radians(FOV) / 2.0)
    assert np.abs(r - c2w[:, 0]).max() < 1e-12 and np.abs(s + c2w[:, 1]).max() < 1e-12  # +x right, +y down the image: -up
    assert np.abs(w + c2w[:, 2]).max() < 1e-12 and abs(f_px / f - 1.0) < 1e-12 and bend < 1e-12  # the camera looks down -z
    D = d * n
    assert np.abs(D @ w - 1.0).max() < 1e-12  # D . w^ = 1: depth = p2p_dist / directions_norm is the z-depth
    d2 = d.copy()
    d2[0, 0] = d2[0, 0] + np.array([0.01, 0.0, 0.0])
    assert L.lens_frame(d2, n)[4] > 1e-3


@pytest.mark.parametrize("rotate", (False, True))
@pytest.mark.parametrize("z_f", (0.4, 2.5))
def test_lens_rays_meet_on_the_plane_in_focus(rotate, z_f):
    o, d, n, _ = pinhole_bundle()
    a = 0.03
    lens = L.lens_block(d, n, a, 1.0 / z_f)
    r, s, w, f_px = lens[0:3], lens[3:6], lens[6:9], lens[11] / a
    table = L.lens_table(16)
    pixels = np.arange(H * W)
    o2, d2, n2 = L.lens_rays(o, d, n, pixels, table, lens, rotate=rotate)
    S1 = table.shape[0]
    assert o2.shape == (H * W * S1, 3) and d2.shape == o2.shape and n2.shape == (H * W * S1,)
    assert np.abs(np.linalg.norm(d2, axis=1) - 1.0).max() < 1e-14
    # D' of every (pixel, row): the antialiasing rule, and the focus point o + D' z_f / k
    da, na = A.subpixel_rays(d, n, pixels, table[:, :2], dtype=np.float64)
    Dp = da * na[:, None]
    k = Dp @ w
    assert np.abs(k - 1.0).max() < 1e-12
    focus = np.repeat(o.reshape(-1, 3), S1, 0) + Dp * (z_f / k)[:, None]
    to = focus - o2
    off = to - (to * d2).sum(1, keepdims=True) * d2
    assert np.linalg.norm(off, axis=1).max() < 1e-12
    # the origins lie on the lens: in the plane through o across w^, within the radius; every pixel's lens points differ under `rotate`
    l = o2 - np.repeat(o.reshape(-1, 3), S1, 0)
    assert np.abs(l @ w).max() < 1e-15 and np.linalg.norm(l, axis=1).max() <= a * (1 + 1e-12)
    same = np.abs(l.reshape(H * W, S1, 3) - l.reshape(H * W, S1, 3)[:1]).max()
    assert (same > 1e-3 * a) if rotate else (same == 0.0)
    # depth along a lens ray is the z-depth
    for z in (0.1, 0.7, 3.0):
        X = o2 + d2 * (n2 * z)[:, None]
        assert np.abs((X - np.repeat(o.reshape(-1, 3), S1, 0)) @ w - z).max() < 1e-12
    if not rotate:
        # a point at depth z seen through the lens point (u, v) lands a f_px (1 / z - 1 / z_f) (u, v) pixels from its pinhole image
        for z in (0.2, 1.0, 6.0):
            X = o2 + d2 * (n2 * z)[:, None] - np.repeat(o.reshape(-1, 3), S1, 0)
            seen = np.stack([X @ r, X @ s], 1) / (X @ w)[:, None] * f_px
            pinhole = np.stack([Dp @ r, Dp @ s], 1) / k[:, None] * f_px
            want = a * f_px * (1.0 / z - 1.0 / z_f) * np.tile(table[:, 2:], (H * W, 1))
            assert np.abs(seen - pinhole - want).max() < 1e-10
            # ... which is the circle of confusion: the largest shift over the unit disc is c
            c = a * f_px * abs(1.0 / z - 1.0 / z_f)
            assert np.linalg.norm(seen - pinhole, axis=1).max() <= c * (1 + 1e-9)


def test_aperture_zero_gives_the_subpixel_rays():
    o, d, n, _ = pinhole_bundle()
    table = L.lens_table(8)
    pixels = np.array([0, 5, W - 1, W, H * W - 1])
    o2, d2, n2 = L.lens_rays(o, d, n, pixels, table, L.lens_block(d, n, 0.0, 1.0 / 0.7))
    da, na = A.subpixel_rays(d, n, pixels, table[:, :2], dtype=np.float64)
    assert np.array_equal(o2, np.repeat(o.reshape(-1, 3)[pixels], 7, 0))
    assert np.abs(d2 - da).max() < 1e-14 and np.abs(n2 - na).max() < 1e-12


def test_focus_at_infinity_gives_parallel_rays():
    o, d, n, _ = pinhole_bundle()
    table = L.lens_table(8)
    table[:, :2] = 0.0  # every sample through the pixel centre
    pixels = np.arange(H * W)
    o2, d2, n2 = L.lens_rays(o, d, n, pixels, table, L.lens_block(d, n, 0.05, 0.0))
    assert np.abs(d2.reshape(H * W, 7, 3) - d.reshape(H * W, 1, 3)).max() < 1e-15
    assert np.abs(n2.reshape(H * W, 7) - n.reshape(H * W, 1)).max() < 1e-12
    assert np.linalg.norm(o2 - np.repeat(o.reshape(-1, 3), 7, 0), axis=1).max() > 0.01


def test_float32_lens_rays_are_near_the_float64_ones():
    o, d, n, _ = pinhole_bundle()
    o, d, n = (x.astype(F) for x in (o, d, n))
    lens = L.lens_block(d, n, 0.03, 1.0 / 0.6).astype(F)
    table = L.lens_table(16).astype(F)
    hi = L.lens_rays(o, d, n, np.arange(H * W), table, lens)
    lo = L.lens_rays(o, d, n, np.arange(H * W), table, lens, dtype=F)
    assert all(x.dtype == F for x in lo)
    for a, b in zip(hi, lo):
        assert np.abs(a - b).max() < 5e-6


# ------------------------------------------------------------------------------------------ circle of confusion and mark
def test_circle_of_confusion_restatement():
    depth = np.array([[2.0, 0.5, 0.0, -1.0], [np.nan, 4.0, np.nan, 1.0]], F)
    acc = np.array([[1.0, 1.0, 1.0, 1.0], [1.0, 0.25, 0.25, 0.5]], F)
    c = L.coc(depth, acc, afpx=8.0, izf=0.5)
    # covered at depth 2: in focus; at 0.5: 8 |2 - 0.5|; depth 0 and < 0: at infinity, 8 * 0.5; a covered NaN stays a NaN; uncovered
    # pixels (accumulation 0.5 is not above `covered`) lie at infinity whatever their depth
    assert c.dtype == F and np.array_equal(c, np.array([[0.0, 12.0, 4.0, 4.0], [np.nan, 4.0, 4.0, 4.0]], F), equal_nan=True)
    assert np.array_equal(L.coc(depth, acc, 8.0, 0.0)[0], F([4.0, 16.0, 0.0, 0.0]))  # focus at infinity
    assert L.focus_of(depth, acc, 1) == F(2.0) and L.focus_of(depth, acc, 2) == 0 and L.focus_of(depth, acc, 4) == 0
    assert L.focus_of(depth, acc, 5) == 0 and L.focus_of(depth, acc, 0, covered=1.0) == 0
    assert L.focus_of(F([3.0]), F([1.0]), 0) == F(1.0) / F(3.0)
    assert not L.mark(np.full((3, 3), np.nan, F), 0.0, 4).any()  # a NaN marks nothing


def blurred_fields():
    rng = np.random.default_rng(7)
    yield "nothing", (6, 7), np.zeros((6, 7), F), 0.5, 4
    yield "threshold", (5, 5), np.full((5, 5), 0.49999997, F), 0.5, 4
    for H_, W_ in ((5, 9), (1, 1), (2, 17)):  # smaller than the window
        for reach in (1, 3, 16):
            c = (rng.random((H_, W_)) < 0.15) * rng.random((H_, W_)) * 2 * reach
            yield f"random {H_}x{W_} reach {reach}", (H_, W_), c.astype(F), 0.5, reach
    for y, x in ((0, 0), (0, 8), (4, 0), (4, 8), (2, 4)):  # one blurred pixel: each corner, and the middle
        for radius in (0.4, 0.5, 1.49, 1.5, 2.5, 40.0):
            c = np.zeros((5, 9), F)
            c[y, x] = radius
            yield f"single ({y}, {x}) c {radius}", (5, 9), c, 0.5, 3
    c = rng.random((12, 14)).astype(F) * 3
    c[rng.random((12, 14)) < 0.3] = np.nan
    c[rng.random((12, 14)) < 0.3] = 0.0
    yield "NaN and uncovered", (12, 14), c, 1.0, 5
    yield "infinite", (7, 7), np.where(np.eye(7) > 0, np.inf, 0).astype(F), 0.5, 2


FIELDS = list(blurred_fields())
FIELD_NAMES = [field[0] for field in FIELDS]


@pytest.mark.parametrize("name,shape,c,threshold,reach", FIELDS, ids=FIELD_NAMES)
def test_mark_is_the_double_loop(name, shape, c, threshold, reach):
    got, want = L.mark(c, threshold, reach), L.mark_pairs(c, threshold, reach)
    assert got.dtype == np.uint8 and got.shape == shape and np.array_equal(got, want)
    if name.startswith("single"):
        (y, x), = np.argwhere(c > 0)
        r = min(reach, int(math.floor(float(F(c[y, x]) + F(0.5))))) if c[y, x] >= threshold else -1
        yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
        assert np.array_equal(got.astype(bool), np.maximum(abs(yy - y), abs(xx - x)) <= r)  # the square of its radius, cut by the image
    if name == "nothing" or name == "threshold":
        assert not got.any()
