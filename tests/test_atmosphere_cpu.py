"""The height-fog rule (include/neusky_hip.h) on its float64 restatement, atmosphere_cpu.py: its limits and invariants; and the value
relight.Atmosphere, its place in FrameLighting and the command line's flags.  No GPU."""
import dataclasses

import numpy as np
import pytest

import atmosphere_cpu as AC
from neusky_amd.relight import Atmosphere, FrameLighting, PointLight, SunLight
from neusky_amd.relight.__main__ import build_parser, parse_atmosphere

R = 40
SUN = SunLight(130.0, 35.0, (2.0, 1.7, 1.2))


def _rays(seed=0, Kb=2):
    g = np.random.default_rng(seed)
    d = g.normal(size=(R, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return dict(origins=g.uniform(-0.5, 0.5, (R, 3)), directions=d, depth=g.uniform(0.0, 2.5, R), accumulation=g.uniform(-0.1, 1.1, R),
                lin=g.uniform(0.0, 2.0, (Kb, R, 3)), background=g.uniform(0.0, 1.0, (Kb, R, 3)), abar=g.uniform(0.1, 0.6, (Kb, 3)))


def _suns(Kb, seed=1):
    g = np.random.default_rng(seed)
    s = g.normal(size=(Kb, 3))
    s[:, 2] = np.abs(s[:, 2]) + 0.1
    return s / np.linalg.norm(s, axis=1, keepdims=True), g.uniform(0.5, 2.0, (Kb, 3))


def test_no_density_returns_the_frame():
    rays = _rays()
    s, C = _suns(2)
    for H in (None, 0.3):
        out = AC.apply(**rays, sun_dirs=s, sun_colours=C, vis=None, params=AC.block(0.0, H, anisotropy=0.8), M=5)
        scale = np.maximum(np.abs(rays["lin"]), np.abs(rays["background"]))
        assert np.abs(out["lin"] - rays["lin"]).max() <= 1e-15 * scale.max()
        assert np.array_equal(out["transmittance"], np.ones((R, 3))) and np.abs(out["inscatter"]).max() == 0.0


def test_a_tall_medium_is_the_homogeneous_one():
    rays = _rays(2)
    s, C = _suns(2)
    tall = AC.block((0.5, 1.0, 2.0), 1e12, base_height=0.25, albedo=0.9, anisotropy=0.5)
    flat = AC.block((0.5, 1.0, 2.0), None, base_height=0.25, albedo=0.9, anisotropy=0.5)
    a, b = (AC.apply(**rays, sun_dirs=s, sun_colours=C, vis=None, params=p, M=3) for p in (tall, flat))
    for k in ("lin", "inscatter", "transmittance"):
        assert np.abs(a[k] - b[k]).max() <= 1e-9, k


def test_phi_is_continuous_across_its_series():
    for u in (1e-4, -1e-4):
        inner, outer = np.nextafter(u, 0.0), np.nextafter(u, 2 * u)
        assert abs(AC.phi(np.float64(inner)) - AC.phi_series(inner)) == 0.0 and abs(AC.phi(np.float64(outer)) - AC.phi_closed(outer)) == 0.0
        assert abs(AC.phi_series(u) - AC.phi_closed(u)) <= 1e-12
        assert abs(AC.phi(np.float64(inner)) - AC.phi(np.float64(outer))) <= 1e-12
    assert AC.phi(np.float64(0.0)) == 1.0 and abs(AC.phi(np.float64(2.0)) - (1 - np.exp(-2.0)) / 2.0) < 1e-16


@pytest.mark.parametrize("M", (1, 5, 64))
def test_unshadowed_inscatter_telescopes(M):
    rays = _rays(3)
    s, C = _suns(2)
    params = AC.block((0.5, 1.0, 2.0), 0.3, albedo=(0.9, 0.8, 0.7), anisotropy=0.6, far=2.0)
    rays["accumulation"] = np.ones(R)  # inscatter is then S(t_s)
    out = AC.apply(**rays, sun_dirs=s, sun_colours=C, vis=np.ones((M, 2, R)), params=params, M=M)
    md = AC.Medium(params, rays["origins"], rays["directions"])
    mu = np.einsum("ri,ki->kr", md.d, s)
    J = md.albedo * (rays["abar"][:, None, :] + 2 * np.pi * md.phase(mu)[:, :, None] * C[:, None, :])
    want = J * (1.0 - md.T(np.clip(rays["depth"], 0.0, 2.0)))[None]
    assert np.abs(out["inscatter"] - want).max() <= 1e-14 * max(1.0, J.max())


def test_a_uniform_world_is_unchanged_by_any_fog():
    rays = _rays(4, Kb=1)
    abar = np.array([[0.4, 0.6, 0.9]])
    for H in (None, 0.3):
        for M in (0, 4):
            params = AC.block((0.5, 1.0, 2.0), H, albedo=0.9)
            J = params[3:6] * abar[0]  # the source, with the albedo the block holds; lin = A J + (1 - A) J, B = J
            rays.update(abar=abar, lin=np.broadcast_to(J, (1, R, 3)).copy(), background=np.broadcast_to(J, (R, 3)).copy())
            out = AC.apply(**rays, sun_dirs=None, sun_colours=None, vis=None, params=params, M=M)
            assert np.abs(out["lin"] - J).max() <= 1e-14


def test_transmittance_falls_with_distance():
    rays = _rays(5)
    for H in (None, 0.3, 0.05):
        md = AC.Medium(AC.block((0.5, 1.0, 2.0), H), rays["origins"], rays["directions"])
        ts = np.linspace(0.0, 2.0, 41)
        T = np.stack([md.T(t) for t in ts])
        assert (np.diff(T, axis=0) <= 0.0).all() and (T[0] == 1.0).all() and (T >= 0.0).all()
        assert (np.diff(T, axis=0) < 0.0).any()


def test_a_clear_background_is_left_alone():
    rays = _rays(6)
    s, C = _suns(2)
    rays["accumulation"] = np.zeros(R)
    rays["lin"] = rays["background"].copy()  # nothing accumulates: the frame shows the background
    out = AC.apply(**rays, sun_dirs=s, sun_colours=C, vis=None, params=AC.block(1.5, 0.3, background=False), M=0)
    assert np.array_equal(out["lin"], rays["background"]) and np.abs(out["inscatter"]).max() == 0.0
    fogged = AC.apply(**rays, sun_dirs=s, sun_colours=C, vis=None, params=AC.block(1.5, 0.3, background=True), M=0)
    assert np.abs(fogged["lin"] - rays["background"]).max() > 1e-2


def test_a_set_sun_adds_nothing():
    rays = _rays(7)
    s, C = _suns(2)
    s[1, 2] = -s[1, 2]
    params = AC.block(1.5, None, anisotropy=0.8)
    with_sun = AC.apply(**rays, sun_dirs=s, sun_colours=C, vis=None, params=params, M=0)
    dark = AC.apply(**rays, sun_dirs=s, sun_colours=C * np.array([[1.0], [0.0]]), vis=None, params=params, M=0)
    assert np.array_equal(with_sun["lin"][1], dark["lin"][1]) and np.array_equal(with_sun["lin"][0], dark["lin"][0])


# ---------------------------------------------------------------------------------------------- the value
def test_the_value_normalises_and_checks():
    a = Atmosphere(1.5)
    assert a.density == (1.5, 1.5, 1.5) and a.albedo == (1.0, 1.0, 1.0) and a.scale_height is None and a.far == 2.0
    assert a.shaft_samples == 0 and a.background is True and a.anisotropy == 0.0 and a.base_height == 0.0
    b = Atmosphere((0.5, 1, 2), scale_height=0.3, base_height=-0.1, albedo=(0.9, 0.8, 0.7), anisotropy=-0.5, far=3, shaft_samples=64, background=False)
    assert b.density == (0.5, 1.0, 2.0) and b.block().tolist() == np.float32([0.5, 1, 2, 0.9, 0.8, 0.7, 0.3, -0.1, -0.5, 3, 0, 0]).tolist()
    assert a.block()[6] == 0.0 and a.block()[10] == 1.0 and a.block().shape == (12,)
    assert b.extra_shadow_rows(3) == 192 and a.extra_shadow_rows(3) == 0
    assert dataclasses.replace(a, density=2.0).density == (2.0, 2.0, 2.0)
    with pytest.raises(dataclasses.FrozenInstanceError):
        a.far = 1.0
    for bad in (dict(density=-1.0), dict(density=(1.0, 2.0)), dict(density=float("inf")), dict(density="thick"), dict(density=(1.0, -1.0, 1.0)),
                dict(density=1.0, scale_height=0.0), dict(density=1.0, scale_height=-1.0), dict(density=1.0, scale_height=float("nan")),
                dict(density=1.0, albedo=1.5), dict(density=1.0, albedo=(0.5, 0.5, -0.1)), dict(density=1.0, anisotropy=0.995),
                dict(density=1.0, anisotropy=-1.0), dict(density=1.0, far=0.0), dict(density=1.0, far=float("inf")),
                dict(density=1.0, scale_height=0.03, far=2.0), dict(density=1.0, shaft_samples=65), dict(density=1.0, shaft_samples=-1),
                dict(density=1.0, shaft_samples=2.0), dict(density=1.0, shaft_samples=True), dict(density=1.0, background=1),
                dict(density=1.0, base_height=float("nan"))):
        with pytest.raises(ValueError):
            Atmosphere(**bad)
    Atmosphere(1.0, scale_height=2.0 / 60.0, far=2.0)  # far / H = 60 is allowed


def test_frame_lighting_takes_an_atmosphere():
    fog = Atmosphere(1.5, shaft_samples=4)
    plain, none = FrameLighting.of(), FrameLighting.of(atmosphere=None)
    assert type(none) is FrameLighting and none.atmosphere is None
    for f in dataclasses.fields(FrameLighting):
        assert getattr(none, f.name) is getattr(plain, f.name) or getattr(none, f.name) == getattr(plain, f.name), f.name
    assert [f.name for f in dataclasses.fields(none)] == [f.name for f in dataclasses.fields(plain)]
    sunny = FrameLighting.of(sun=SUN, atmosphere=fog)
    assert isinstance(sunny, FrameLighting) and sunny.atmosphere is fog and sunny.lights is None
    assert dataclasses.replace(sunny, rotation=None).atmosphere is fog
    lamp = PointLight((0.3, 0.6, 0.2), (1.0, 0.8, 0.6))
    lit = FrameLighting.of(sun=SUN, lights=lamp, atmosphere=fog)
    assert lit.atmosphere is fog and lit.lights == (lamp,) and lit.light_trace is not None
    assert type(FrameLighting.of(lights=lamp)).__name__ == "LitFrameLighting"
    assert FrameLighting.of(atmosphere=Atmosphere(1.5)).atmosphere.shaft_samples == 0  # (no shafts: no sun is needed)
    with pytest.raises(ValueError, match="sun"):
        FrameLighting.of(atmosphere=fog)  # shafts without a sun
    with pytest.raises(ValueError, match="bake"):
        FrameLighting.of(bake="fp32", atmosphere=Atmosphere(1.5))
    with pytest.raises(ValueError, match="Atmosphere"):
        FrameLighting.of(atmosphere={"density": 1.5})


# ---------------------------------------------------------------------------------------------- the command line
BASE = ["--checkpoint", "c.ckpt", "--camera-path", "p.json", "--output-dir", "o", "--latent-index", "0"]


def _parse(*flags):
    ap = build_parser()
    return parse_atmosphere(ap, ap.parse_args(BASE + list(flags)))


def test_the_parser_takes_the_fog_flags(capsys):
    assert _parse() is None
    assert _parse("--fog-density", "1.5") == Atmosphere(1.5)
    got = _parse("--fog-density", "0.5", "1", "2", "--fog-scale-height", "0.3", "--fog-base-height", "-0.1", "--fog-albedo", "0.9", "--fog-anisotropy",
                 "0.8", "--fog-far", "3", "--fog-shafts", "16", "--fog-clear-background", "--fog-map", "--sun-azimuth", "10", "--sun-elevation", "20")
    assert got == Atmosphere((0.5, 1.0, 2.0), 0.3, -0.1, 0.9, 0.8, 3.0, 16, False)
    assert _parse("--fog-density", "1", "--fog-albedo", "0.9", "0.8", "0.7").albedo == (0.9, 0.8, 0.7)
    for flags, words in ((("--fog-scale-height", "0.3"), ("--fog-scale-height needs --fog-density",)),
                         (("--fog-map",), ("--fog-map needs --fog-density",)),
                         (("--fog-clear-background",), ("--fog-clear-background needs --fog-density",)),
                         (("--fog-shafts", "4"), ("--fog-shafts needs --fog-density",)),
                         (("--fog-density", "1.5", "--transfer", "fp16"), ("--fog-density", "--transfer fp16")),
                         (("--fog-far", "3", "--transfer", "fp32"), ("--fog-far", "--transfer fp32")),
                         (("--fog-density", "1", "2"), ("one number or R G B",)),
                         (("--fog-density", "1", "--fog-shafts", "4"), ("--fog-shafts", "needs a sun")),
                         (("--fog-density", "1", "--fog-shafts", "65", "--sun-azimuth", "1", "--sun-elevation", "2"), ("0..64",)),
                         (("--fog-density", "-1"), ("density",)),
                         (("--fog-density", "1", "--fog-scale-height", "0.01"), ("far / scale_height",))):
        with pytest.raises(SystemExit) as refused:
            _parse(*flags)
        message = capsys.readouterr().err
        assert refused.value.code not in (0, None) and all(w in message for w in words), (flags, message[-300:])
