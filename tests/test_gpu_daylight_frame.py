"""Frames lit by a clear-sky daylight model (get_outputs_for_camera_ray_bundle(..., daylight=, sun=)): a K = 3 frame against the float64
restatement of its definition on the chunk's own field outputs (daylight_cpu.py for the skies, transfer_cpu.py and sun_cpu.py for the
rest), K suns against K single-sun frames, graph against eager, replay across sun positions and turbidities, a sweep through the
horizon, the paths without `daylight` before and after; and the `python -m neusky_amd.relight --daylight` command line from a saved
checkpoint.  The scene is test_gpu_sun_frame.py's."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import daylight_cpu as DC
import sun_cpu as SC
import transfer_cpu as TC
from util_frames import frame_scene
from util_step import randomise
from neusky_amd.relight import DaylightSky, EnvironmentMap
from neusky_amd.relight.sun import SunLight

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, CHUNK = 13, 16, 64  # 208 rays: three whole chunks and a padded one
LIN_BAR = 1e-5  # the bar of test_gpu_relight_frame.py and test_gpu_sun_frame.py on a linear image
SKY = DaylightSky(turbidity=3.0, exposure=0.1)
THREE = SKY.sun_path(100.0, 8.0, 190.0, 62.0, 3)
SUN_KEYS = ("rgb", "lin", "shadow_map", "shadow_difference")


@pytest.fixture(scope="module")
def scene():
    pipe, rb = frame_scene(H, W, DEV)
    m = pipe.model
    render = lambda **kw: m.get_outputs_for_camera_ray_bundle(rb, camera_index=1, chunk=CHUNK, **kw)  # noqa: E731
    env = EnvironmentMap((torch.rand(32, 64, 3, generator=torch.Generator().manual_seed(7)) ** 2 * 3.0).numpy(), "blender", exposure=0.8)
    plain = {"latent": {}, "envmap": {"envmap": env}, "envmap and sun": {"envmap": env, "sun": SunLight(130.0, 35.0, (2.0, 1.7, 1.2))}}
    before = {name: {k: v.clone() for k, v in render(use_graph=True, **kw).items()} for name, kw in plain.items()}  # BEFORE any daylight
    three = render(use_graph=True, daylight=SKY, sun=THREE)
    return pipe, rb, render, plain, before, three


def _f64(t):
    return t.detach().cpu().double().numpy()


def _bar(lin):
    return LIN_BAR * max(1.0, float(np.abs(lin).max()))


def test_outputs_are_those_of_a_sun_frame(scene):
    _, _, render, _, before, three = scene
    assert set(three) == set(before["envmap and sun"])
    assert three["rgb"].shape == (3, H, W, 3) and three["lin"].shape == (3, H, W, 3) and three["shadow_map"].shape == (3, H, W, 1)
    for k in ("albedo", "accumulation", "depth", "p2p_dist", "normal"):  # the keys without a sun keep their meaning
        assert torch.equal(three[k], before["latent"][k]), k
    assert all(torch.isfinite(three[k]).all() for k in SUN_KEYS)
    assert not torch.equal(three["lin"][0], three["lin"][2]) and three["lin"].max().item() > 1e-2
    one = render(use_graph=True, daylight=SKY, sun=THREE[1])  # a single SunLight drops the leading K
    assert one["rgb"].shape == (H, W, 3) and torch.equal(one["rgb"], three["rgb"][1])


def test_frame_matches_its_definition(scene):
    pipe, rb, render, _, _, three = scene
    m = pipe.model
    eager = render(use_graph=False, daylight=SKY, sun=THREE)
    flat = rb.slice(0, 1 << 62)
    s32 = np.array([s.direction for s in THREE], np.float64).astype(np.float32).astype(np.float64)
    C = np.array([s.colour for s in THREE], np.float32).astype(np.float64)
    T32, E32, G32 = (np.float64(np.float32(SKY.turbidity)), np.float64(np.float32(SKY.exposure)), np.asarray(SKY.ground, np.float32).astype(np.float64))
    lin_sky, t = [], []
    with torch.no_grad():
        m.begin_frame(1, None, None, THREE, daylight=SKY)
        try:
            m.begin_step()
            for a in range(0, H * W, CHUNK):
                c = flat.slice(a, min(a + CHUNK, H * W))
                c = type(c)(c.origins.contiguous(), c.directions.contiguous(), c.pixel_area.contiguous(), c.camera_indices.contiguous(),
                            metadata={k: v.contiguous() for k, v in c.metadata.items()})
                so = m.sample_and_forward_field(m.collider(c))
                fo = so["field_outputs"]
                albedo = [v for k, v in fo.items() if str(k).lower().endswith("albedo")][0]
                normals = [v for k, v in fo.items() if str(k).lower().endswith("normals")][0]
                w = so["weights"][..., 0]
                dirs = so["illumination_directions"]
                vis = so["visibility_dict"]["visibility"] if m.config.use_visibility else None
                Tr, acc = TC.transfer(albedo.cpu(), normals.cpu(), w.cpu(), dirs.cpu(), None if vis is None else vis.cpu())
                lights = DC.radiance(T32, s32, _f64(dirs), E32, G32)
                bg = DC.radiance(T32, s32, _f64(c.directions), E32, G32)
                lin_sky.append(TC.relit_linear(Tr, acc, torch.from_numpy(lights), torch.from_numpy(bg)).numpy())
                t.append(SC.transfer(_f64(albedo), _f64(normals), _f64(w), s32)[0])
        finally:
            m.end_frame()
    lin_sky, t = np.concatenate(lin_sky, axis=1), np.concatenate(t, axis=1)  # [3, N, 3]
    for got in (eager, three):
        V = _f64(got["shadow_map"]).reshape(3, -1, 1)
        ref = lin_sky + C[:, None, :] * V * t
        err = np.abs(_f64(got["lin"]).reshape(3, -1, 3) - ref).max()
        print(f"lin vs its definition: max err {err:.3e}, bar {_bar(ref):.3e}, max {ref.max():.3f}, sun term max {(ref - lin_sky).max():.3f}")
        assert err <= _bar(ref)
        np.testing.assert_allclose(_f64(got["rgb"]).reshape(-1, 3), SC.linear_to_srgb(_f64(got["lin"]).reshape(-1, 3)), rtol=1e-4, atol=1e-6)
    assert (lin_sky.max(axis=(1, 2)) > 1e-2).all()  # every sky lit something
    assert (C[:, None, :] * _f64(three["shadow_map"]).reshape(3, -1, 1) * t).max() > 1e-2  # and so did a sun


def test_nine_suns_are_nine_single_frames(scene):
    _, _, render, _, _, _ = scene
    suns = [SKY.sun(40.0 * i, 8.0 * i - 6.0) for i in range(9)]  # (the first has set)
    many = render(use_graph=True, daylight=SKY, sun=suns)
    assert many["rgb"].shape == (9, H, W, 3) and many["shadow_map"].shape == (9, H, W, 1) and many["albedo"].shape == (H, W, 3)
    bar = _bar(_f64(many["lin"]))
    for i, s in enumerate(suns):
        one = render(use_graph=True, daylight=SKY, sun=s)
        err = np.abs(_f64(many["lin"][i]) - _f64(one["lin"])).max()
        print(f"sun {i}: K = 9 against single, lin max err {err:.3e} (bar {bar:.3e})")
        assert err <= bar
        assert (many["shadow_map"][i] - one["shadow_map"]).abs().max().item() <= 2e-6
    assert not torch.equal(many["rgb"][3], many["rgb"][5])


def test_graph_and_eager_agree(scene):
    _, _, render, _, _, three = scene
    eager = render(use_graph=False, daylight=SKY, sun=THREE)
    for k in SUN_KEYS + ("albedo", "accumulation", "depth"):
        assert torch.equal(three[k], eager[k]), k


def test_a_new_sweep_and_turbidity_replay_the_captured_chunk(scene):
    pipe, _, render, _, _, three = scene
    m = pipe.model
    render(use_graph=True, daylight=SKY, sun=THREE)
    runners = dict(m.frames.runners)
    hazy = DaylightSky(turbidity=7.5, exposure=0.05, ground=(0.1, 0.2, 0.3))
    other = hazy.sun_path(300.0, 70.0, 250.0, 3.0, 3)
    got = render(use_graph=True, daylight=hazy, sun=other)
    assert len(m.frames.runners) == len(runners) and all(m.frames.runners[k] is r for k, r in runners.items())
    assert not torch.equal(got["rgb"], three["rgb"])
    eager = render(use_graph=False, daylight=hazy, sun=other)
    for k in SUN_KEYS:
        assert torch.equal(got[k], eager[k]), k
    # no latent is read: another camera index replays the same chunk and changes nothing
    _, rb, _, _, _, _ = scene
    again = m.get_outputs_for_camera_ray_bundle(rb, camera_index=2, chunk=CHUNK, use_graph=True, daylight=hazy, sun=other)
    assert len(m.frames.runners) == len(runners) and all(m.frames.runners[k] is r for k, r in runners.items())
    for k in SUN_KEYS:
        assert torch.equal(again[k], got[k]), k


def test_sweep_through_the_horizon(scene):
    _, _, render, _, _, _ = scene
    path = SKY.sun_path(90.0, 5.0, 100.0, -5.0, 5)
    out = render(use_graph=True, daylight=SKY, sun=path)
    assert all(torch.isfinite(out[k]).all() for k in SUN_KEYS)
    empty = (out["accumulation"] == 0.0)[..., 0]
    print(f"{int(empty.sum())} of {H * W} rays meet nothing")
    down = [i for i, s in enumerate(path) if s.elevation_deg <= 0.0]
    assert len(down) == 3
    for i in down:
        assert (out["rgb"][i][empty] == 0.0).all(), i
        assert (out["lin"][i] == 0.0).all(), i  # no sky, no sun: nothing lights the scene either
        assert out["shadow_map"][i].abs().max().item() == 0.0 and out["shadow_difference"][i].abs().max().item() == 0.0
    assert out["lin"][0].max().item() > 0.0 and out["lin"][1].max().item() > 0.0


def test_daylight_needs_a_sun_and_excludes_the_other_skies(scene):
    pipe, _, render, plain, _, _ = scene
    with pytest.raises(ValueError, match="sun"):
        render(daylight=SKY)
    with pytest.raises(ValueError, match="envmap"):
        render(daylight=SKY, sun=THREE, envmap=plain["envmap"]["envmap"])
    with pytest.raises(ValueError, match="rotation"):
        render(daylight=SKY, sun=THREE, rotation=torch.eye(3, device=DEV))
    assert pipe.model.frames.active is None


def test_paths_without_daylight_are_untouched(scene):
    _, _, render, plain, before, _ = scene
    render(use_graph=True, daylight=SKY, sun=THREE)
    for name, kw in plain.items():
        after = render(use_graph=True, **kw)
        assert set(after) == set(before[name])
        for k, v in before[name].items():
            assert torch.equal(after[k], v), (name, k)


def test_cli_sweeps_a_daylight_sun_over_a_checkpoint(tmp_path):
    from PIL import Image

    from neusky_amd.configs.neusky_config import synthetic_pipeline_config
    from neusky_amd.data.synthetic_datamanager import SyntheticDataManagerConfig
    from neusky_amd.relight import camera_rays, load_camera_path
    from neusky_amd.relight.__main__ import build_pipeline
    from neusky_amd.utils.checkpoints import load_reference_pipeline_state, save_checkpoint
    torch.manual_seed(1)
    cfg = synthetic_pipeline_config()
    cfg.datamanager = SyntheticDataManagerConfig(num_train_images=3, num_eval_images=2)
    pipe = cfg.setup(device=DEV)
    randomise(pipe)
    ckpt = save_checkpoint(tmp_path, 3, pipe)
    Hc, Wc = 16, 24

    def pose(a):
        c, s = math.cos(a), math.sin(a)
        eye = np.array([0.6 * c, 0.6 * s, 0.05])
        fwd = -eye / np.linalg.norm(eye)
        right = np.cross(fwd, [0.0, 0.0, 1.0])
        right /= np.linalg.norm(right)
        up = np.cross(right, fwd)
        m = np.eye(4)
        m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = right, up, -fwd, eye
        return {"camera_to_world": m.reshape(-1).tolist(), "fov": 55.0}

    path_file = tmp_path / "camera_path.json"
    path_file.write_text(json.dumps({"render_width": Wc, "render_height": Hc, "camera_type": "perspective", "camera_path": [pose(0.3)]}))
    out = tmp_path / "frames"
    cmd = [sys.executable, "-m", "neusky_amd.relight", "--checkpoint", ckpt, "--camera-path", str(path_file), "--output-dir", str(out),
           "--daylight", "--turbidity", "4", "--sun-path", "120", "10", "240", "40", "--sun-steps", "3", "--shadow-map"]
    r = subprocess.run(["timeout", "-k", "10", "400"] + cmd, cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "3 frames" in r.stdout and "daylight: turbidity 4" in r.stdout
    assert sorted(os.listdir(out)) == sorted([f"frame_0000_{f:03d}.png" for f in range(3)] + [f"shadow_0000_{f:03d}.png" for f in range(3)])
    frames = [np.asarray(Image.open(str(out / f"frame_0000_{f:03d}.png"))) for f in range(3)]
    shadows = [np.asarray(Image.open(str(out / f"shadow_0000_{f:03d}.png"))) for f in range(3)]
    assert all(f.shape == (Hc, Wc, 3) and f.dtype == np.uint8 for f in frames)
    assert all(s.shape == (Hc, Wc) and s.dtype == np.uint8 for s in shadows)
    assert not np.array_equal(frames[0], frames[1]) and not np.array_equal(frames[1], frames[2])
    # frame 0 against the Python API on the same checkpoint, after the 8-bit rounding
    state = torch.load(ckpt, map_location="cpu", weights_only=False)["pipeline"]
    again = build_pipeline(state, DEV)
    load_reference_pipeline_state(again, state)
    again.eval()
    sky = DaylightSky(turbidity=4.0)
    api = again.model.get_outputs_for_camera_ray_bundle(camera_rays(load_camera_path(str(path_file)), 0, DEV), camera_index=0, chunk=4096,
                                                        daylight=sky, sun=sky.sun_path(120.0, 10.0, 240.0, 40.0, 3))
    want = np.round(api["rgb"][0].clamp(0.0, 1.0).cpu().numpy() * 255.0).astype(np.uint8)
    assert np.array_equal(frames[0], want)
