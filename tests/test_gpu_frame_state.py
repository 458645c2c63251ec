"""The frame render's state (models/frame.py: model.frames): a failure inside a frame leaves none active, the chunk-graph key is a function
of the frame's parts only, a FrameLighting handed to the owner renders the frame of its keywords, a chunk carries the keys its lighting
declares, a training forward ignores an active frame, and the runner cache evicts as documented.  The fixture is the one
of the frame tests: 13 x 16 rays of one camera at chunk 64, three whole chunks and a padded one."""
import pytest
import torch

from util_frames import frame_scene
from neusky_amd.models import neusky_model
from neusky_amd.models.frame import chunk_keys
from neusky_amd.relight import Atmosphere, DaylightSky, DisplayTransform, EnvironmentMap, FrameLighting, PointLight, bake_transfer, z_rotation
from neusky_amd.relight.sun import SunLight

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W, CHUNK = 13, 16, 64
SUN = SunLight(130.0, 35.0, (2.0, 1.7, 1.2))


@pytest.fixture(scope="module")
def scene():
    pipe, rb = frame_scene(H, W, DEV)
    m = pipe.model
    render = lambda chunk=CHUNK, **kw: m.get_outputs_for_camera_ray_bundle(rb, camera_index=1, chunk=chunk, **kw)  # noqa: E731
    return pipe, rb, render


def _fail_on_second_call(m):
    real, calls = m.forward, []

    def forward(*args, **kwargs):
        calls.append(1)
        if len(calls) == 2:
            raise RuntimeError("second chunk")  # a host exception: nothing is launched for this chunk
        return real(*args, **kwargs)
    return forward


@pytest.mark.parametrize("what", ["sun frame", "bake"])
def test_a_failure_inside_a_frame_leaves_no_frame_behind(scene, monkeypatch, what):
    pipe, rb, render = scene
    m = pipe.model
    before = {k: v.clone() for k, v in render(use_graph=True).items()}
    with monkeypatch.context() as mp:
        mp.setattr(m, "forward", _fail_on_second_call(m))
        with pytest.raises(RuntimeError, match="second chunk"):
            if what == "bake":
                bake_transfer(m, rb, storage="fp32", chunk=CHUNK, use_graph=False, camera_index=1)
            else:
                render(use_graph=False, sun=SUN)
    assert m.frames.active is None
    after = render(use_graph=True)
    assert after.keys() == before.keys()
    for k, v in before.items():
        assert torch.equal(after[k], v), k


def test_the_key_is_a_function_of_the_frames_parts_only(scene):
    pipe, _, _ = scene
    m, f = pipe.model, pipe.model.frames

    def key(*args, **kw):
        m.begin_frame(*args, **kw)
        try:
            return f.active.key, f.active.shading, f.active.rotation
        finally:
            m.end_frame()

    with torch.no_grad():
        sun_key, shading, _ = key(1, None, None, SUN)
        assert shading == "sun" and "sun" in sun_key
        sky_key, shading, _ = key(1)  # the sun of the frame before is gone
        assert shading == "sky" and sky_key == (1, None) and sun_key[0] == sky_key

        r1 = z_rotation(0.37).to(DEV)
        r2 = r1.clone()
        k1, _, pinned1 = key(1, r1)
        k2, _, pinned2 = key(1, r2)
        assert k1 == k2 and k1 != sky_key and pinned1 is r1 and pinned2 is r1

        env = EnvironmentMap((torch.rand(32, 64, 3, generator=torch.Generator().manual_seed(7)) ** 2 * 3.0).numpy(), "blender", exposure=0.8)
        e0, shading, _ = key(1, None, env)
        assert shading == "sky" and e0 != sky_key
        assert key(1, z_rotation(0.9).to(DEV), env)[0] == e0
        env.exposure = 0.5
        assert key(1, z_rotation(-2.2).to(DEV), env)[0] == e0

        other = SunLight(250.0, 15.0, (3.0, 2.0, 0.5))
        assert key(1, sun=other)[0] == sun_key and key(1, sun=[other])[0] == sun_key
        assert key(1, sun=SUN, shadow_threshold=0.3, accumulation_mask_threshold=0.5)[0] == sun_key
        assert key(1, sun=SUN, shadow_sigmoid_scale=m.sigmoid_scale)[0] == sun_key
        assert key(1, sun=[SUN, other])[0] == (sky_key, "sun", 2, float(m.sigmoid_scale))
        assert key(1, sun=SUN, shadow_sigmoid_scale=2.0 * m.sigmoid_scale)[0] == (sky_key, "sun", 1, 2.0 * m.sigmoid_scale)
        assert key(1, None, env, SUN)[0] == (e0, "sun", 1, float(m.sigmoid_scale))
    assert f.active is None


@pytest.mark.parametrize("keywords", [{}, {"sun": SUN}, {"sun": SUN, "sun_shadows": "sdf", "shadow_trace": {"steps": 16}}],
                         ids=["plain", "sun", "sdf shadows"])
def test_a_frame_lighting_renders_the_frame_of_its_keywords(scene, keywords):
    pipe, rb, render = scene
    m = pipe.model
    ref = {k: v.clone() for k, v in render(use_graph=True, **keywords).items()}
    runners = dict(m.frames.runners)
    out = m.frames.render(rb, FrameLighting.of(**keywords), camera_index=1, chunk=CHUNK, use_graph=True)
    assert m.frames.runners.keys() == runners.keys() and all(m.frames.runners[k] is r for k, r in runners.items())
    assert m.frames.active is None
    assert out.keys() == ref.keys()
    for k, v in ref.items():
        assert out[k].dtype == v.dtype and out[k].shape == v.shape and torch.equal(out[k], v), k


OTHER = SunLight(250.0, 15.0, (3.0, 2.0, 0.5))
SKY = DaylightSky(turbidity=3.0, exposure=0.1)
LAMP = PointLight((0.3, -0.2, 0.6), (2.0, 1.8, 1.5), radius=0.03)
SDF = {"sun_shadows": "sdf", "shadow_trace": {"steps": 4}}
FOG = {M: Atmosphere(1.5, scale_height=0.3, shaft_samples=M) for M in (0, 2)}
# the frame's keywords; `linear` is set by a display transform, as FrameRenderer.render sets it
LIGHTINGS = {
    "sky": {},
    "sky, linear": {"display": DisplayTransform()},
    "one sun": {"sun": SUN},
    "two suns, sdf shadows": {"sun": [SUN, OTHER], **SDF},
    "daylight sweep": {"daylight": SKY, "sun": SKY.sun_path(100.0, 8.0, 190.0, 62.0, 3)},
    "lamp over the sky": {"lights": LAMP, "light_trace": {"steps": 4}},
    "lamp without shadows over the sky": {"lights": LAMP, "light_shadows": False},
    "lamp over a sun": {"sun": SUN, "lights": LAMP, "light_trace": {"steps": 4}},
    "lamp without shadows over two suns": {"sun": [SUN, OTHER], "lights": [LAMP], "light_shadows": False},
    "fog": {"atmosphere": FOG[0]},
    "fog under a sun": {"sun": SUN, "atmosphere": FOG[0]},
    "shafts under two suns": {"sun": [SUN, OTHER], "atmosphere": FOG[2]},
    "shafts under sdf shadows": {"sun": [SUN, OTHER], **SDF, "atmosphere": FOG[2]},
    "bake": {"bake": "fp32"},
    "bake, fp16": {"bake": "fp16"},
}


@pytest.mark.parametrize("name", LIGHTINGS)
def test_a_chunk_carries_the_keys_its_lighting_declares(scene, monkeypatch, name):
    pipe, rb, render = scene
    kw = dict(LIGHTINGS[name])
    display = kw.pop("display", None)
    keys, sun_keys = chunk_keys(FrameLighting.of(**kw), linear=display is not None)
    real, seen = neusky_model.shade, []

    def shade(*args):
        out = real(*args)
        seen.append(sorted(out))
        return out
    monkeypatch.setattr(neusky_model, "shade", shade)
    if "bake" in kw:  # (a bake has no frame to assemble: its rows go to the transfer)
        bake_transfer(pipe.model, rb, storage=kw["bake"], chunk=CHUNK, use_graph=False, camera_index=1)
        assert len(seen) == 4 and all(s == sorted(keys) for s in seen) and sun_keys == ()
        return
    out = render(use_graph=False, display=display, **kw)
    assert len(seen) == 4 and all(s == sorted(keys) for s in seen), (seen[0], keys)  # three whole chunks and a padded one
    assert len(set(keys)) == len(keys) and set(keys) <= set(out) and set(sun_keys) <= set(keys)
    suns = kw.get("sun")
    assert bool(sun_keys) == (suns is not None) and (suns is None or {"rgb", "lin", "shadow_map", "shadow_difference"} <= set(sun_keys))
    lead = (len(suns),) if isinstance(suns, list) else ()  # (a single SunLight drops its K = 1)
    for k in keys:
        assert out[k].shape[:-1] == ((*lead, H, W) if k in sun_keys else (H, W)), (k, out[k].shape)


def test_training_ignores_an_active_frame(scene):
    pipe, rb, _ = scene
    m = pipe.model
    chunk = lambda: rb.slice(0, CHUNK).static_clone()  # noqa: E731  (the collider writes nears / fars into the bundle it is given)
    m.train()
    try:
        m.begin_step()
        plain = m.forward(chunk())
        with torch.no_grad():
            m.begin_frame(1, sun=SUN)
        assert m.frames.active is not None and m.frames.active.shading == "sun"
        m.begin_step()
        out = m.forward(chunk())
        assert "rgb" in out and "lin" not in out and "shadow_map" not in out
        assert out["rgb"].shape == (CHUNK, 3)
        assert out.keys() == plain.keys()
    finally:
        m.eval()
        pipe.eval()
        m.end_frame()
    assert m.frames.active is None


def test_eviction(scene):
    pipe, _, render = scene
    m = pipe.model
    m.frames.runners.clear()
    first = {k: v.clone() for k, v in render(16, use_graph=True).items()}
    for chunk in (32, 48, 64):
        render(chunk, use_graph=True)
    runners = dict(m.frames.runners)
    assert sorted(k[0] for k in runners) == [16, 32, 48, 64] and all(k[1] for k in runners)
    for chunk in (16, 32, 48, 64):  # all four serve a repeat
        render(chunk, use_graph=True)
    assert m.frames.runners.keys() == runners.keys() and all(m.frames.runners[k] is r for k, r in runners.items())
    render(80, use_graph=True)  # a fifth: the four are dropped
    assert [k[0] for k in m.frames.runners] == [80]
    again = render(16, use_graph=True)
    assert len(m.frames.runners) == 2
    for k, v in first.items():
        assert torch.equal(again[k], v), k
