"""The display transform's definitions (include/neusky_hip.h, "A display transform") on their numpy restatement (display_cpu.py), the
values relight.DisplayTransform refuses, and the command line's display flags.  No GPU."""
import numpy as np
import pytest

import display_cpu as D

F32 = np.float32


def _image(seed=0, n=4000, scale=1.0):
    rng = np.random.default_rng(seed)
    return (np.exp(rng.uniform(-8.0, 8.0, size=(n, 3))) * scale).astype(F32)


def test_bin_edges():
    edges = np.array([2.0 ** -24, np.nextafter(F32(2.0 ** -24), F32(0)), 1.0, 1.0 + 1.0 / 64.0, np.nextafter(F32(2), F32(0)),
                      np.nextafter(F32(2.0 ** 24), F32(0)), 2.0 ** 24], dtype=F32)
    assert D.bins_of(edges).tolist() == [0, -1, 1536, 1537, 1599, 3071, 3071]
    # the unclamped rule puts 2^24 in bin 3072: the clamp is what keeps it
    assert (int(F32(2.0 ** 24).view(np.uint32)) >> 17) - 6592 == 3072
    odd = np.array([0.0, -0.0, -1.0, 1e-40, np.inf, -np.inf, np.nan, 3e38], dtype=F32)
    assert D.bins_of(odd).tolist() == [-1, -1, -1, -1, -1, -1, -1, 3071]
    # 64 bins per octave: every bin of [1, 2) is met once by its lower edge
    lower = (1.0 + np.arange(64) / 64.0).astype(F32)
    assert D.bins_of(lower).tolist() == list(range(1536, 1600))


def test_luminance_rounds_every_operation_once():
    rgb = _image(1, 1000)
    r, g, b = (rgb[:, c].astype(np.float64) for c in range(3))
    want = (F32(F32(F32(0.2126) * rgb[:, 0]) + F32(F32(0.7152) * rgb[:, 1])) + F32(F32(0.0722) * rgb[:, 2])).astype(F32)
    assert np.array_equal(D.luminance(rgb), want)
    exact = 0.2126 * r + 0.7152 * g + 0.0722 * b
    assert np.abs(D.luminance(rgb) / exact - 1.0).max() < 4 * 2.0 ** -24


def test_histogram_total_is_the_metered_count():
    lin = _image(2)
    lin[:7] = [[0, 0, 0], [-1, -1, -1], [np.nan, 1, 1], [np.inf, 0, 0], [1e-30, 1e-30, 1e-30], [1, 1, 1], [3e38, 3e38, 3e38]]
    Y = D.luminance(lin)
    with np.errstate(invalid="ignore"):
        metered = np.isfinite(Y) & (Y >= F32(2.0 ** -24))
    h = D.histogram(lin)
    assert h.dtype == np.int64 and h.shape == (3072,) and h.sum() == metered.sum() == len(lin) - 5
    mask = np.random.default_rng(3).uniform(size=len(lin)).astype(F32)
    hm = D.histogram(lin, mask, 0.5)
    assert hm.sum() == (metered & (mask > F32(0.5))).sum() and (hm <= h).all()
    assert np.array_equal(D.histogram(lin, mask, None), h)  # no threshold: the mask is not read


def test_scaling_by_a_power_of_two_rolls_the_histogram():
    lin = _image(4, scale=0.37)
    h, h8 = D.histogram(lin), D.histogram(lin * F32(8))
    assert h[-192:].sum() == 0  # (nothing reaches the clamped end)
    assert np.array_equal(h8, np.roll(h, 192))
    for kw in ({}, {"key": 0.3, "ev": 1.5, "percentiles": (0.2, 0.6)}):
        E, E8 = D.exposure(h, **kw), D.exposure(h8, **kw)
        assert F32(E8) == F32(E) / F32(8)  # E is stored in float32
        assert E8 == pytest.approx(E / 8.0, rel=1e-14)


def test_percentiles_zero_one_meter_everything():
    lin = _image(5, 500)
    h = D.histogram(lin)
    centres = (np.arange(3072) + 0.5) / 64.0 - 24.0
    m = float((h * centres).sum() / h.sum())
    assert D.exposure(h, 0.18, 0.0, (0.0, 1.0)) == pytest.approx(float(F32(0.18)) * 2.0 ** -m, rel=1e-12)
    # a bin's centre is exponent + mantissa fraction, the piecewise-linear log2: at most 0.0861 below log2, and half a bin off
    gap = float(np.log2(D.luminance(lin).astype(np.float64)).mean()) - m
    assert -1.0 / 128.0 <= gap <= 0.0861 + 1.0 / 128.0
    # a narrower window moves the exposure only through the pixels it keeps
    one = np.zeros(3072, dtype=np.int64)
    one[1536] = 1000
    assert D.exposure(one, 1.0, 0.0, (0.05, 0.95)) == D.exposure(one, 1.0, 0.0, (0.0, 1.0)) == 2.0 ** -(1536.5 / 64.0 - 24.0)


def test_nothing_metered_gives_unit_exposure():
    assert D.exposure(np.zeros(3072, dtype=np.int64)) == 1.0
    assert D.exposure(D.histogram(np.zeros((10, 3), dtype=F32))) == 1.0
    assert D.exposure(D.histogram(np.full((10, 3), np.nan, dtype=F32))) == 1.0


def test_curves():
    x = np.concatenate([[0.0], np.logspace(-8, 4, 6001)])
    for name in D.CURVES:
        y = D.curve(x, name)
        assert (np.diff(y) >= 0.0).all(), name  # monotone on [0, 1e4]
        assert float(D.curve(0.0, name)) == 0.0, name
    assert np.array_equal(D.curve(x, "clamp"), x)
    assert float(D.curve(0.0, "aces")) == 0.03 * 0.0 / 0.14 == 0.0
    assert float(D.curve(4.0, "reinhard", white=4.0)) == pytest.approx(1.0, abs=1e-15)  # the white point maps to 1
    assert float(D.curve(11.2 / 2.0, "hable")) == pytest.approx(1.0, abs=1e-15)  # and Hable's W, after the exposure bias
    assert float(D.curve(1e4, "aces")) == pytest.approx(2.51 / 2.43, rel=1e-4)
    # the kernel's form of Hable's operator, with the constant terms cancelled on paper, is the same function
    v = 2.0 * x
    same = v * (0.042 * v + 0.005) / (0.3 * (v * (0.15 * v + 0.5) + 0.06))
    assert np.abs(same - D.hable_partial(v)).max() < 1e-15
    assert np.array_equal(D.srgb(np.array([-1.0, 0.0, np.nan, 2.0])), np.array([0.0, 0.0, np.nan, 1.0]), equal_nan=True)


def test_an_interior_impulse_blurs_to_the_kernel():
    for sigma in (0.5, 4.0, 7.3):
        w = D.gaussian_weights(sigma)
        r = (len(w) - 1) // 2
        assert r == int(np.ceil(3 * sigma)) and abs(w.sum() - 1.0) < 1e-12 and np.array_equal(w, w[::-1])
        n = 2 * r + 5
        src = np.zeros((n, n, 3))
        src[n // 2, n // 2] = [1.0, 2.0, 0.0]
        out = D.blur(src, w)
        assert abs(out[..., 0].sum() - 1.0) < 1e-12 and abs(out[..., 1].sum() - 2.0) < 1e-12 and not out[..., 2].any()
        assert np.allclose(out, out[::-1], atol=1e-18) and np.allclose(out, out[:, ::-1], atol=1e-18)
        assert np.allclose(out, out.transpose(1, 0, 2), atol=1e-18)
        assert np.allclose(out[..., 0], np.outer(w, w)[r - n // 2:r + n // 2 + 1, r - n // 2:r + n // 2 + 1]
                           if n <= 2 * r + 1 else np.pad(np.outer(w, w), 2), atol=1e-18)
    # near an edge the weight that falls outside the frame is lost (the source there is zero)
    w = D.gaussian_weights(1.0)
    out = D.blur(np.ones((1, 4, 1)), w)
    assert out[0, 0, 0] == pytest.approx(w[3] * w[3:].sum()) and out.shape == (1, 4, 1)


def test_display_map_restatement():
    lin = np.array([[0.0, -1.0, np.nan], [1e-8, 0.0031308, 1.0], [1e4, np.inf, 0.5]], dtype=F32)
    rgb = D.display_map(lin, 1.0, "clamp")
    assert rgb[0].tolist() == [0.0, 0.0, 0.0] and rgb[2, 0] == 1.0 and rgb[2, 1] == 1.0
    assert rgb[1, 2] == pytest.approx(1.0, abs=1e-15) and rgb[1, 0] == pytest.approx(12.92 * float(F32(1e-8)))
    assert np.array_equal(D.display_map(lin * F32(0.5), 2.0, "aces"), D.display_map(lin, 1.0, "aces"))
    src = D.bloom_source(lin, 2.0, 1.0)
    assert src[0].tolist() == [0.0, 0.0, 0.0] and src[1].tolist() == [0.0, 0.0, 1.0] and src[2, 2] == 0.0


# ------------------------------------------------------------------------------------------ relight.DisplayTransform
def test_display_transform_values():
    from neusky_amd.relight import DisplayTransform
    from neusky_amd.relight.display import bloom_weights
    d = DisplayTransform()
    assert (d.curve, d.exposure, d.key, d.ev, d.percentiles, d.white) == ("clamp", 1.0, 0.18, 0.0, (0.05, 0.95), 4.0)
    assert (d.bloom_sigma, d.bloom_threshold, d.bloom_strength, d.meter_mask_threshold) == (0.0, 1.0, 0.1, None)
    assert not d.metered and DisplayTransform(exposure="frame").metered and DisplayTransform(exposure="sequence").metered
    assert DisplayTransform(curve="aces", ev=1) == DisplayTransform(curve="aces", ev=1.0) and hash(d) == hash(DisplayTransform())
    with pytest.raises(Exception):
        d.curve = "aces"  # frozen
    assert d.params("cpu").tolist() == [float(F32(v)) for v in (0.18, 0.0, 0.05, 0.95, 4.0, 1.0, 0.1, 0.0)]
    for sigma in (0.5, 4.0, 32.0):
        w = bloom_weights(sigma)
        assert w.dtype.is_floating_point and w.numel() == 2 * int(np.ceil(3 * sigma)) + 1
        assert np.array_equal(w.numpy(), D.gaussian_weights(sigma).astype(F32))


@pytest.mark.parametrize("keywords", [
    {"curve": "filmic"}, {"curve": None}, {"exposure": "auto"}, {"exposure": -1.0}, {"exposure": float("nan")}, {"exposure": None},
    {"key": 0.0}, {"key": -0.18}, {"key": float("inf")}, {"ev": float("nan")}, {"ev": "one"}, {"percentiles": (0.5, 0.5)},
    {"percentiles": (0.9, 0.1)}, {"percentiles": (-0.1, 0.9)}, {"percentiles": (0.1, 1.1)}, {"percentiles": (0.1,)},
    {"percentiles": 0.5}, {"white": 0.0}, {"white": -4.0}, {"bloom_sigma": -1.0}, {"bloom_sigma": 32.5},
    {"bloom_sigma": float("nan")}, {"bloom_threshold": -0.1}, {"bloom_strength": -0.1}, {"meter_mask_threshold": float("nan")},
    {"meter_mask_threshold": "half"}])
def test_display_transform_refuses(keywords):
    from neusky_amd.relight import DisplayTransform
    with pytest.raises(ValueError):
        DisplayTransform(**keywords)


# ------------------------------------------------------------------------------------------ the command line
BASE = ["--checkpoint", "c.ckpt", "--camera-path", "p.json", "--output-dir", "out", "--latent-index", "0"]


def _display(argv):
    from neusky_amd.relight.__main__ import build_parser, parse_display
    ap = build_parser()
    return parse_display(ap, ap.parse_args(BASE + argv))


def test_parser_defaults_are_off():
    from neusky_amd.relight.__main__ import build_parser
    args = build_parser().parse_args(BASE)
    for name in ("tonemap", "auto_exposure", "exposure_key", "exposure_ev", "meter_percentiles", "white_point", "bloom_sigma",
                 "bloom_threshold", "bloom_strength"):
        assert getattr(args, name) is None, name
    assert args.save_linear is False
    assert _display([]) is None


def test_parser_builds_the_transform():
    from neusky_amd.relight import DisplayTransform
    assert _display(["--tonemap", "aces"]) == DisplayTransform(curve="aces")
    assert _display(["--tonemap", "aces", "--auto-exposure", "off"]) == DisplayTransform(curve="aces")
    assert _display(["--save-linear"]) == DisplayTransform()
    got = _display(["--tonemap", "reinhard", "--auto-exposure", "sequence", "--exposure-key", "0.25", "--exposure-ev", "-1",
                    "--meter-percentiles", "0.1", "0.9", "--white-point", "8", "--bloom-sigma", "3", "--bloom-threshold", "2",
                    "--bloom-strength", "0.5", "--save-linear"])
    assert got == DisplayTransform("reinhard", "sequence", 0.25, -1.0, (0.1, 0.9), 8.0, 3.0, 2.0, 0.5)
    assert _display(["--tonemap", "hable", "--auto-exposure", "frame"]).exposure == "frame"


@pytest.mark.parametrize("argv, message", [
    (["--auto-exposure", "frame"], "--auto-exposure needs --tonemap"),
    (["--exposure-key", "0.2"], "--exposure-key needs --tonemap"),
    (["--exposure-ev", "1"], "--exposure-ev needs --tonemap"),
    (["--meter-percentiles", "0.1", "0.9"], "--meter-percentiles needs --tonemap"),
    (["--white-point", "4"], "--white-point needs --tonemap"),
    (["--bloom-sigma", "2"], "--bloom-sigma needs --tonemap"),
    (["--bloom-threshold", "2"], "--bloom-threshold needs --tonemap"),
    (["--bloom-strength", "2"], "--bloom-strength needs --tonemap"),
    (["--tonemap", "aces", "--exposure-key", "0.2"], "--exposure-key shapes the metered exposure"),
    (["--tonemap", "aces", "--auto-exposure", "off", "--exposure-ev", "1"], "--exposure-ev shapes the metered exposure"),
    (["--tonemap", "aces", "--meter-percentiles", "0.1", "0.9"], "--meter-percentiles shapes the metered exposure"),
    (["--tonemap", "aces", "--white-point", "4"], "--white-point is the white point of --tonemap reinhard"),
    (["--tonemap", "aces", "--bloom-threshold", "2"], "--bloom-threshold needs --bloom-sigma"),
    (["--tonemap", "aces", "--bloom-strength", "2"], "--bloom-strength needs --bloom-sigma"),
    (["--tonemap", "aces", "--bloom-sigma", "40"], "bloom_sigma is at most 32"),
    (["--tonemap", "aces", "--auto-exposure", "frame", "--exposure-key", "0"], "key must be finite and > 0"),
    (["--tonemap", "aces", "--auto-exposure", "frame", "--meter-percentiles", "0.9", "0.1"], "percentiles: two numbers"),
    (["--tonemap", "reinhard", "--white-point", "0"], "white must be finite and > 0"),
    (["--tonemap", "filmic"], "invalid choice"),
    (["--auto-exposure", "always"], "invalid choice"),
])
def test_parser_errors(argv, message, capsys):
    with pytest.raises(SystemExit) as e:
        _display(argv)
    assert e.value.code == 2
    assert message in capsys.readouterr().err
