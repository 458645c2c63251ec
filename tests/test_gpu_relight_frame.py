"""Frames lit by an environment map (get_outputs_for_camera_ray_bundle(..., envmap=)): against a composition of the oracle's functions
with the CPU projection and lookup, chunking and graphs, a rotation without a recapture, the latent path unchanged; and the
`python -m neusky_amd.relight` command line from a saved checkpoint."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import envmap_cpu as E
from oracle import neusky_oracle as O
from util_frames import frame_scene
from util_step import oracle_params, oracle_step_cfg, randomise
from neusky_amd.relight import EnvironmentMap, z_rotation

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def scene():
    H, W = 9, 13
    pipe, rb = frame_scene(H, W, DEV)
    m = pipe.model
    # the latent-lit frame BEFORE any environment-map call
    before = m.get_outputs_for_camera_ray_bundle(rb, camera_index=1, chunk=32, use_graph=True)
    envmap = (torch.rand(32, 64, 3, generator=torch.Generator().manual_seed(7)) ** 2 * 3.0).numpy()
    return pipe, rb, envmap, {k: v.clone() for k, v in before.items()}


def _oracle(pipe, rb, envmap, conv, rotation=None, exposure=1.0):
    p = {k: v.detach() for k, v in oracle_params(pipe).items()}
    cfg = oracle_step_cfg(pipe)
    origins, directions = rb.origins.reshape(-1, 3).cpu().double(), rb.directions.reshape(-1, 3).cpu().double()
    R = origins.shape[0]
    light = pipe.model.illumination_sampler.directions.double()
    nears, fars = O.sphere_collider(origins, directions, cfg.radius)
    samp = O.proposal_sample(origins, directions, nears, fars, p, cfg.prop_grids, cfg.num_prop, cfg.num_final, None, 1.0)
    fo = O.field_pass(p, cfg, origins, directions, samp["ebins"])
    weights = fo["weights"]
    rot = None if rotation is None else rotation.double().numpy()
    cols = torch.from_numpy(E.project(envmap, conv, light.numpy(), rot, exposure)[0])[None]
    bg = torch.from_numpy(E.lookup(envmap, conv, directions.numpy(), rot, exposure))
    p2p = O.render_depth(weights, samp["ebins"])
    ddf_fn = lambda sp, dd: {"expected_termination_dist": O.ddf_query(sp, dd, p, cfg.ddf_grid, cfg.radius)}  # noqa: E731
    vis = O.compute_visibility(origins, directions, p2p, light, p["visibility_threshold"], cfg.sigmoid_scale, cfg.radius, ddf_fn, True, True)
    return O.lambertian_render(fo["albedo"], fo["normals"], light, cols, torch.zeros(R, dtype=torch.long), vis["visibility"], bg, weights,
                               training=False)


def _rel(got, ref):
    return ((got["rgb"].reshape(-1, 3).cpu().double() - ref).abs().max() / ref.abs().max()).item()


@pytest.mark.parametrize("conv", ["blender", "neusky"])
def test_envmap_frame_matches_oracle_and_chunking(scene, conv):
    pipe, rb, envmap, _ = scene
    env = EnvironmentMap(envmap, conv, exposure=0.8)
    full = pipe.model.get_outputs_for_camera_ray_bundle(rb, camera_index=1, chunk=32, use_graph=True, envmap=env)
    assert _rel(full, _oracle(pipe, rb, envmap, conv, exposure=0.8)) < 1e-4
    other = pipe.model.get_outputs_for_camera_ray_bundle(rb, camera_index=1, chunk=50, use_graph=False, envmap=env)
    assert (other["rgb"] - full["rgb"]).abs().max().item() < 2e-6


def test_rotation_replays_the_captured_graph(scene):
    pipe, rb, envmap, _ = scene
    m = pipe.model
    env = EnvironmentMap(envmap, "blender")
    r1, r2 = z_rotation(0.9), z_rotation(-2.2) @ torch.tensor([[1.0, 0.0, 0.0], [0.0, math.cos(0.3), -math.sin(0.3)],
                                                               [0.0, math.sin(0.3), math.cos(0.3)]])
    got = m.get_outputs_for_camera_ray_bundle(rb, camera_index=1, chunk=64, rotation=r1.to(DEV), use_graph=True, envmap=env)
    assert _rel(got, _oracle(pipe, rb, envmap, "blender", r1)) < 1e-4
    runners = dict(m.frames.runners)
    graphs = {k: r.graph for k, r in runners.items()}
    got = m.get_outputs_for_camera_ray_bundle(rb, camera_index=1, chunk=64, rotation=r2.to(DEV), use_graph=True, envmap=env)
    assert _rel(got, _oracle(pipe, rb, envmap, "blender", r2)) < 1e-4
    assert m.frames.runners.keys() == runners.keys()  # no new capture: the same runner and graph served the second rotation
    assert all(m.frames.runners[k] is r and r.graph is graphs[k] for k, r in runners.items())


def test_latent_path_unchanged_after_envmap_frames(scene):
    pipe, rb, _, before = scene
    after = pipe.model.get_outputs_for_camera_ray_bundle(rb, camera_index=1, chunk=32, use_graph=True)
    for k, v in before.items():
        assert torch.equal(after[k], v), k


def test_cli_renders_a_checkpoint_under_an_hdr(tmp_path):
    from PIL import Image

    from neusky_amd.configs.neusky_config import synthetic_pipeline_config
    from neusky_amd.data.synthetic_datamanager import SyntheticDataManagerConfig
    from neusky_amd.relight import camera_rays, load_camera_path, srgb_to_linear
    from neusky_amd.utils.checkpoints import save_checkpoint
    torch.manual_seed(1)
    cfg = synthetic_pipeline_config()
    cfg.datamanager = SyntheticDataManagerConfig(num_train_images=3, num_eval_images=2)
    pipe = cfg.setup(device=DEV)
    randomise(pipe)
    ckpt = save_checkpoint(tmp_path, 3, pipe)
    pipe.eval()
    H, W = 16, 24
    rgbe = E.float_to_rgbe(np.random.default_rng(2).uniform(0.0, 2.0, (32, 64, 3)) ** 2)
    E.write_hdr(tmp_path / "sky.hdr", rgbe, rle=True)

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

    (tmp_path / "camera_path.json").write_text(json.dumps({"render_width": W, "render_height": H, "camera_type": "perspective",
                                                           "camera_path": [pose(0.3), pose(2.0)]}))
    out = tmp_path / "frames"
    cmd = [sys.executable, "-m", "neusky_amd.relight", "--checkpoint", ckpt, "--camera-path", str(tmp_path / "camera_path.json"),
           "--output-dir", str(out), "--envmap", str(tmp_path / "sky.hdr"), "--turntable", "2", "--save-hdr", "--exposure", "0.7"]
    r = subprocess.run(["timeout", "-k", "10", "400"] + cmd, cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "4 frames" in r.stdout
    env = EnvironmentMap.from_file(tmp_path / "sky.hdr", exposure=0.7)
    cams = load_camera_path(tmp_path / "camera_path.json")
    for c in range(2):
        rb = camera_rays(cams, c, DEV)
        for f in range(2):
            rot = None if f == 0 else z_rotation(math.pi).to(DEV)
            rgb = pipe.model.get_outputs_for_camera_ray_bundle(rb, camera_index=0, chunk=4096, rotation=rot, envmap=env)["rgb"]
            rgb = rgb.clamp(0.0, 1.0).cpu().numpy()
            stem = out / f"frame_{c:04d}_{f:03d}"
            png = np.asarray(Image.open(str(stem) + ".png"), dtype=np.float64) / 255.0
            assert png.shape == (H, W, 3) and np.abs(png - rgb).max() <= 1.0 / 255 + 1e-6
            assert np.abs(np.load(str(stem) + ".npy") - srgb_to_linear(rgb)).max() < 1e-5
