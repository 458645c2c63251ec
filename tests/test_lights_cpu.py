"""The rules of point and spot lights (include/neusky_hip.h), pinned by analytic facts on their float64 restatement (lights_cpu.py): the
inverse-square law on a plane, the cone, the floor, a sample at the lamp; the bounded march on the analytic plane-and-sphere scene, where
an unbounded march sees the geometry behind a lamp; and the host values: PointLight, the device block, the JSON file, FrameLighting's
rules.  No device."""
import dataclasses
import json

import numpy as np
import pytest

import lights_cpu as LC
import sphere_trace_cpu as ST

# ---------------------------------------------------------------------------------------------- transfer


def _one_sample(x, light, normal=(0.0, 0.0, 1.0)):
    x = np.asarray(x, np.float64).reshape(1, 1, 3)
    n = np.asarray(normal, np.float64).reshape(1, 1, 3)
    t, scale = LC.transfer(x, np.ones((1, 1, 3)), n, np.ones((1, 1)), light[None])
    return t[0, 0], scale[0, 0]


@pytest.mark.parametrize("d", (0.0, 0.3, 1.0))
def test_a_plane_under_a_lamp_follows_the_inverse_square_law(d):
    h = 0.5
    t, _ = _one_sample((d, 0.0, 0.0), LC.light_row((0.0, 0.0, h)))
    want = h / (h * h + d * d) ** 1.5
    assert np.all(np.abs(t - want) <= 1e-14 * want), (t, want)


def test_the_cone():
    inner, outer = 20.0, 40.0
    ci, co = np.cos(np.radians(inner)), np.cos(np.radians(outer))
    got = LC.spot(np.array([ci, co, 0.5 * (ci + co), 1.0, -1.0]), ci, co)
    assert got[[0, 1, 3, 4]].tolist() == [1.0, 0.0, 1.0, 0.0] and abs(got[2] - 0.5) <= 1e-14  # (the midpoint of two cosines is rounded)
    # through the transfer: a lamp at height 1 pointing down, samples on the plane at the cone's angles
    light = LC.light_row((0.0, 0.0, 1.0), axis=(0.0, 0.0, -3.0), inner_deg=inner, outer_deg=outer)
    free = LC.light_row((0.0, 0.0, 1.0))
    for deg, want in ((0.0, 1.0), (19.9, 1.0), (40.1, 0.0), (80.0, 0.0)):
        x = (np.tan(np.radians(deg)), 0.0, 0.0)
        assert np.allclose(_one_sample(x, light)[0], want * _one_sample(x, free)[0], rtol=1e-13, atol=0.0), deg
    mid = np.degrees(np.arccos(0.5 * (ci + co)))
    x = (np.tan(np.radians(mid)), 0.0, 0.0)
    assert np.allclose(_one_sample(x, light)[0], 0.5 * _one_sample(x, free)[0], rtol=1e-12)
    # the omnidirectional light: 1 in every direction, c = -1 included, and no division (0 / 0 would be NaN)
    with np.errstate(all="raise"):
        assert LC.spot(np.array([-1.0, -0.3, 0.0, 1.0]), -1.0, -1.0).tolist() == [1.0] * 4
    assert _one_sample((0.0, 0.0, 2.0), free, normal=(0.0, 0.0, -1.0))[0].tolist() == [1.0] * 3  # straight along the stored axis's c = -1


def test_the_floor_of_the_inverse_square_law():
    light = LC.light_row((0.0, 0.0, 0.05), min_distance=0.1)
    t, _ = _one_sample((0.0, 0.0, 0.0), light)
    assert np.allclose(t, 1.0 / 0.1 ** 2, rtol=1e-14)
    t, _ = _one_sample((0.0, 0.0, -0.15), light)  # 0.2 away: beyond the floor
    assert np.allclose(t, 1.0 / 0.2 ** 2, rtol=1e-14)


def test_a_sample_at_the_lamp_adds_nothing():
    p = (0.25, -0.5, 0.125)
    with np.errstate(all="raise"):
        t, scale = _one_sample(p, LC.light_row(p))
    assert t.tolist() == [0.0] * 3 and scale.tolist() == [0.0] * 3
    x = np.array([[p, (0.0, 0.0, 0.0)]])  # one ray, two samples: the other one still counts
    t, _ = LC.transfer(x, np.ones((1, 2, 3)), np.tile(np.array([0.6, 0.0, 0.8]), (1, 2, 1)), np.ones((1, 2)), LC.light_row(p)[None])
    assert np.isfinite(t).all() and (t > 0.0).all()


# ---------------------------------------------------------------------------------------------- the bounded march
LAMPS = {"above": (0.1, -0.05, 0.9), "under": (0.1, -0.05, 0.08), "low side": (-0.45, 0.3, 0.15), "outside the collider": (0.9, 0.9, 0.9)}
RHOS = (0.0, 0.02, 0.08)
HEIGHTS = (1e-2, 0.0, -5e-3)
_REF = {}


def _march(name, rho, z, dtype=np.float64):
    key = (name, rho, z, dtype)
    if key not in _REF:
        light = LC.light_row(LAMPS[name], rho=rho, clearance=rho)[None]
        _REF[key] = LC.march_to(ST.scene_sdf, ST.scene_starts(32, z), light, dtype=dtype)
    return _REF[key]


@pytest.mark.parametrize("z", HEIGHTS[:2])
def test_geometry_behind_a_lamp_does_not_shadow_it(z):
    """the lamp hangs under the sphere: every start point on the plane sees it, and the sun's march along the same rays runs on into
    the sphere (18 and 21 of the 1024 rays at the two start heights)"""
    m, status, t, s = _march("under", 0.0, z)
    assert (status == LC.ESCAPED).all() and (m == 1.0).all()
    _, unbounded, _ = ST.march(ST.scene_sdf, ST.scene_starts(32, z), s[0])
    hits = int((unbounded == ST.HIT).sum())
    print(f"z {z}: the unbounded march reports HIT on {hits} rays that see the lamp")
    assert hits >= 1


@pytest.mark.parametrize("name", LAMPS)
def test_a_point_source_gives_a_hard_shadow(name):
    for z in HEIGHTS:
        m, status, _, _ = _march(name, 0.0, z)
        assert set(np.unique(m)) <= {0.0, 1.0}
        assert np.array_equal(m == 0.0, status == LC.HIT)


def test_a_spherical_source_gives_a_penumbra():
    m, status, _, _ = _march("above", 0.08, 0.0)
    assert ((m > 0.0) & (m < 1.0)).sum() >= 10 and (status == LC.HIT).sum() >= 10 and (m == 1.0).sum() >= 10


@pytest.mark.parametrize("rho", RHOS)
@pytest.mark.parametrize("name", LAMPS)
def test_float32_keeps_the_verdicts(name, rho):
    for z in HEIGHTS:
        m64, s64, _, _ = _march(name, rho, z)
        m32, s32, _, _ = _march(name, rho, z, np.float32)
        differ = s64 != s32
        err = np.abs(m32.astype(np.float64) - m64)[~differ].max()
        print(f"{name}, rho {rho}, z {z}: {int(differ.sum())} of {differ.size} statuses differ, visibility by {err:.2e}")
        assert differ.sum() == 0 and err <= 1e-5


def test_a_lamp_outside_the_collider_is_reached_by_leaving_the_scene():
    m, status, t, _ = _march("outside the collider", 0.0, 1e-2)
    lit = status == LC.ESCAPED
    assert lit.sum() >= 100 and (t[lit] < np.linalg.norm(np.array(LAMPS["outside the collider"])) + 0.7).all()
    x, s, t_end, tan_half, st = LC.begin(LC.light_row((0.0, 0.0, 0.5), rho=0.1, clearance=0.1)[None], 1.0,
                                         starts=np.array([[0.0, 0.0, 0.5], [0.0, 0.0, 0.45], [0.0, 0.0, 0.0], [0.9, 0.9, 0.0]]))
    assert s[0].tolist() == [0.0, 0.0, 1.0] and t_end[0] == 0.0 and tan_half[0] == 0.0  # len == 0
    assert st.tolist() == [LC.ESCAPED, LC.ESCAPED, LC.ALIVE, LC.ESCAPED]  # at the lamp; inside its clearance; marching; beyond the radius
    assert np.isclose(t_end[2], 0.4) and np.isclose(tan_half[2], 0.2)


# ---------------------------------------------------------------------------------------------- the composite
def test_the_lamps_add_into_one_frame_under_the_accumulation_rule():
    g = np.random.default_rng(3)
    R, L = 5, 2
    base, t, vis = g.random((3, R, 3)), g.random((L, R, 3)), g.random((L, R))
    acc = np.array([0.0, 0.2, 0.5, 0.9, 1.0])
    lights = np.stack([LC.light_row((0, 0, 1), intensity=(1.0, 2.0, 3.0)), LC.light_row((0, 1, 0), intensity=(0.5, 0.0, 0.25))])
    rgb, lin, E, V = LC.composite(base, t, vis, acc, 0.2, lights)
    assert np.array_equal(V[:, :2], np.zeros((L, 2))) and np.array_equal(V[:, 2:], vis[:, 2:])
    want = sum(lights[l, LC.I][None] * V[l][:, None] * t[l] for l in range(L))
    assert np.allclose(E, want, rtol=1e-15) and np.allclose(lin, base + E[None], rtol=1e-15) and np.array_equal(lin[:, :2], base[:, :2])
    assert np.array_equal(LC.composite(base, t, None, acc, 0.2, lights)[3][:, 2:], np.ones((L, 3)))
    assert rgb.min() >= 0.0 and rgb.max() <= 1.0


# ---------------------------------------------------------------------------------------------- host values
def test_point_light_is_a_validated_value():
    from neusky_amd.relight import PointLight
    a = PointLight([0, 0.5, 1], (1, 2, 3))
    assert a.position == (0.0, 0.5, 1.0) and a.intensity == (1.0, 2.0, 3.0) and a.radius == 0.0 and a.direction is None
    assert a.clearance == 0.02 and a.min_distance == 0.01  # the defaults, design choices
    b = PointLight((0, 0, 1), (1, 1, 1), radius=0.05)
    assert b.clearance == 0.05 and b.min_distance == 0.05
    assert PointLight((0, 0, 1), (1, 1, 1), radius=0.05, clearance=0.0, min_distance=1e-3).clearance == 0.0
    s = PointLight((0, 0, 1), (1, 1, 1), direction=(0, 0, -2), inner_deg=10, outer_deg=30)
    assert s.direction == (0.0, 0.0, -1.0) and (s.inner_deg, s.outer_deg) == (10.0, 30.0)
    assert a == PointLight((0, 0.5, 1), (1, 2, 3)) and hash(a) == hash(PointLight((0, 0.5, 1), (1, 2, 3)))
    with pytest.raises(dataclasses.FrozenInstanceError):
        a.radius = 1.0
    for wrong in (dict(position=(0, 0)), dict(intensity=(1, 1, float("nan"))), dict(radius=-1.0), dict(clearance=-0.1), dict(min_distance=0.0),
                  dict(inner_deg=10.0), dict(outer_deg=30.0), dict(direction=(0, 0, 0)), dict(direction=(0, 0, 1), inner_deg=40, outer_deg=30),
                  dict(direction=(0, 0, 1), outer_deg=181), dict(direction=(0, 0, 1), inner_deg=-1, outer_deg=30)):
        with pytest.raises(ValueError):
            PointLight(**{"position": (0, 0, 1), "intensity": (1, 1, 1), **wrong})


def test_the_block_has_the_documented_columns():
    import torch
    from neusky_amd.relight import PointLight, as_lights, lights_block
    a = PointLight((0.1, 0.2, 0.3), (1, 2, 3), radius=0.05)
    s = PointLight((-1, 0, 2), (4, 5, 6), direction=(0, 3, -4), inner_deg=10, outer_deg=30, clearance=0.5, min_distance=0.25)
    block = lights_block([a, s])
    assert block.shape == (2, 16) and block.dtype == torch.float32
    want = np.stack([LC.light_row((0.1, 0.2, 0.3), (1, 2, 3), 0.05),
                     LC.light_row((-1, 0, 2), (4, 5, 6), 0.0, 0.5, 0.25, (0, 3, -4), 10, 30)]).astype(np.float32)
    assert np.array_equal(block.numpy(), want)
    assert block[0, 6] == -1.0 and block[0, 7] == -1.0 and block[:, 11].tolist() == [0.0, 0.0] and block[:, 15].tolist() == [0.0, 0.0]
    assert torch.equal(lights_block(a), block[:1])
    assert as_lights(None) == () and as_lights([]) == () and as_lights(a) == (a,)
    with pytest.raises(TypeError):
        as_lights([a, "lamp"])
    with pytest.raises(ValueError, match="at most 64"):
        as_lights([a] * 65)
    assert len(as_lights([a] * 64)) == 64


def test_a_lights_file_round_trips(tmp_path):
    from neusky_amd.relight import PointLight, load_lights, save_lights
    lights = (PointLight((0.1, 0.2, 0.3), (1, 2, 3), radius=0.05),
              PointLight((-1, 0, 2), (4, 5, 6), direction=(0, 3, -4), inner_deg=10, outer_deg=30, clearance=0.5, min_distance=0.25))
    path = tmp_path / "lights.json"
    save_lights(path, lights)
    assert load_lights(path) == lights
    path.write_text(json.dumps([{"position": [0, 0, 1], "intensity": [1, 1, 1]}]))
    assert load_lights(path) == (PointLight((0, 0, 1), (1, 1, 1)),)
    for wrong in ({"position": [0, 0, 1]}, [{"position": [0, 0, 1]}], [{"position": [0, 0, 1], "intensity": [1, 1, 1], "colour": 3}]):
        path.write_text(json.dumps(wrong))
        with pytest.raises(ValueError):
            load_lights(path)


def test_frame_lighting_takes_lights():
    from neusky_amd.relight import LIGHT_TRACE_DEFAULTS, SHADOW_DEFAULTS, DaylightSky, FrameLighting, PointLight, SunLight
    lamp, sun = PointLight((0, 0, 1), (1, 1, 1)), SunLight(130.0, 35.0)
    assert LIGHT_TRACE_DEFAULTS == {k: v for k, v in SHADOW_DEFAULTS.items() if k != "angular_diameter_deg"}
    plain = FrameLighting.of()
    for same in (FrameLighting.of(lights=None), FrameLighting.of(lights=()), FrameLighting.of(lights=[], light_shadows=False)):
        assert type(same) is FrameLighting
        for f in dataclasses.fields(plain):
            x, y = getattr(plain, f.name), getattr(same, f.name)
            assert x is y or x == y, f.name
        assert same.lights is None and same.light_trace is None
    one, listed = FrameLighting.of(lights=lamp), FrameLighting.of(lights=[lamp, lamp])
    assert isinstance(one, FrameLighting) and one.lights == (lamp,) and listed.lights == (lamp, lamp) and one.light_shadows is True
    assert one.light_trace == {**LIGHT_TRACE_DEFAULTS, "radius": 1.0}
    assert FrameLighting.of(lights=lamp, light_trace={"steps": 16, "bias": 0}).light_trace == {**LIGHT_TRACE_DEFAULTS, "steps": 16, "bias": 0.0}
    assert FrameLighting.of(lights=lamp, light_shadows=False).light_trace is None
    assert dataclasses.replace(one, lights=(lamp, lamp)).lights == (lamp, lamp)
    # they go with every sky and sun
    for keywords in (dict(envmap=object()), dict(rotation=np.eye(3)), dict(sun=sun), dict(sun=[sun, sun]), dict(sun=sun, daylight=DaylightSky()),
                     dict(sun=sun, sun_shadows="sdf"), dict(sun=sun, sun_shadows="ddf", shadow_threshold=0.3)):
        got = FrameLighting.of(lights=lamp, **keywords)
        ref = FrameLighting.of(**keywords)
        assert got.lights == (lamp,)
        for f in dataclasses.fields(ref):
            x, y = getattr(ref, f.name), getattr(got, f.name)
            assert x is y or x == y, f.name
    for wrong in (dict(light_trace={}), dict(light_trace={"steps": 8}, lights=()), dict(lights=lamp, light_shadows=False, light_trace={}),
                  dict(lights=lamp, bake="fp32"), dict(lights=[lamp] * 65), dict(lights=lamp, light_trace={"angular_diameter_deg": 1.0}),
                  dict(lights=lamp, light_trace={"steps": 0})):
        with pytest.raises(ValueError):
            FrameLighting.of(**wrong)
    with pytest.raises(TypeError):
        FrameLighting.of(lights=["lamp"])
