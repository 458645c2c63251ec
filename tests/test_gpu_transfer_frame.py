"""A frame baked once into its radiance transfer (relight.bake_transfer) and relit: against the frame render for the same light on the
same model and the float64 oracle compositions of the frame tests; chunking, graphs, the mode flag, save / load and the command line."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import test_gpu_relight_frame as EnvFrame
import test_gpu_render_frame as LatentFrame
from oracle import neusky_oracle as O
from util_frames import frame_scene
from util_step import oracle_params, oracle_step_cfg, randomise
from neusky_amd.relight import EnvironmentMap, RadianceTransfer, bake_transfer, z_rotation

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -24
SEED = 2  # chosen on the CPU oracle: 38 of the frame's 117 pixels accumulate more than 0.5, 79 less


@pytest.fixture(scope="module")
def scene():
    H, W = 9, 13
    pipe, rb = frame_scene(H, W, DEV, seed=SEED)
    envmap = (torch.rand(32, 64, 3, generator=torch.Generator().manual_seed(7)) ** 2 * 3.0).numpy()
    return pipe, rb, envmap


def _sizes(pipe):
    return pipe.model.config.num_neus_samples_per_ray, pipe.model.illumination_sampler.directions.shape[0]


def _lights(envmap):
    rot = z_rotation(0.9)
    tilt = z_rotation(-2.2) @ torch.tensor([[1.0, 0.0, 0.0], [0.0, math.cos(0.3), -math.sin(0.3)], [0.0, math.sin(0.3), math.cos(0.3)]])
    return [("latent", None, None, 1.0), ("latent rotated", None, rot, 1.0), ("envmap", envmap, None, 1.0), ("envmap rotated", envmap, tilt, 0.8)]


def _oracle(pipe, rb, env, rot, exposure):
    if env is None:
        return LatentFrame._oracle(pipe, rb, rot)["rgb"]
    return EnvFrame._oracle(pipe, rb, env, "blender", rot, exposure)


def test_the_frame_exercises_both_terms(scene):
    pipe, rb, _ = scene
    p = {k: v.detach() for k, v in oracle_params(pipe).items()}
    cfg = oracle_step_cfg(pipe)
    origins, directions = rb.origins.reshape(-1, 3).cpu().double(), rb.directions.reshape(-1, 3).cpu().double()
    nears, fars = O.sphere_collider(origins, directions, cfg.radius)
    samp = O.proposal_sample(origins, directions, nears, fars, p, cfg.prop_grids, cfg.num_prop, cfg.num_final, None, 1.0)
    acc = O.field_pass(p, cfg, origins, directions, samp["ebins"])["weights"].sum(-1)
    assert (acc > 0.5).any() and (acc < 0.5).any(), (float(acc.min()), float(acc.max()))


@pytest.mark.parametrize("storage", ["fp32", "fp16"])
def test_relit_frames_match_the_frame_render_and_the_oracle(scene, storage):
    pipe, rb, envmap = scene
    m = pipe.model
    S, D = _sizes(pipe)
    bound = 0.44 * (S + D) * EPS + 1e-6 + (0.44 * 2.0 ** -11 if storage == "fp16" else 0.0)
    baked = bake_transfer(m, rb, storage=storage, chunk=32, camera_index=1)
    assert baked.storage == storage and baked.shape == (9, 13) and baked.T.shape == (117, D, 3)
    for name, env, rot, exposure in _lights(envmap):
        em = None if env is None else EnvironmentMap(env, "blender", exposure=exposure)
        r = None if rot is None else rot.to(DEV)
        ref = m.get_outputs_for_camera_ray_bundle(rb, camera_index=1, chunk=32, rotation=r, use_graph=True, envmap=em)
        got = baked.relight(m, envmap=em, camera_index=1, rotations=r)
        assert got.keys() >= ref.keys()
        diff = (got["rgb"] - ref["rgb"]).abs().max().item()
        orc = _oracle(pipe, rb, env, rot, exposure)
        rel = ((got["rgb"].reshape(-1, 3).cpu().double() - orc).abs().max() / orc.abs().max()).item()
        print(f"{storage} {name}: max |rgb - frame render| {diff:.3e} (bound {bound:.3e}); vs oracle rel {rel:.3e}")
        assert got["rgb"].shape == ref["rgb"].shape and diff <= bound, (name, diff, bound)
        assert rel < 1e-4, (name, rel)
        for k in ("albedo", "accumulation", "depth", "p2p_dist", "normal"):
            assert torch.equal(got[k], ref[k]), (name, k)


def test_several_rotations_come_back_with_a_leading_axis(scene):
    pipe, rb, envmap = scene
    m = pipe.model
    em = EnvironmentMap(envmap, "blender")
    baked = bake_transfer(m, rb, storage="fp32", chunk=64, camera_index=1)
    rots = [None] + [z_rotation(2.0 * math.pi * f / 11).to(DEV) for f in range(1, 11)]  # 11 lights: a pass of 8 and a pass of 3
    many = baked.relight(m, envmap=em, rotations=rots)["rgb"]
    assert many.shape == (11, 9, 13, 3)
    for f in (0, 3, 7, 8, 10):
        one = baked.relight(m, envmap=em, rotations=rots[f])["rgb"]
        assert torch.equal(many[f], one), f
    gained = baked.relight(m, envmap=em, rotations=rots[3], exposure=0.5, return_linear=True)
    plain = baked.relight(m, envmap=em, rotations=rots[3], return_linear=True)
    assert (gained["linear"] - 0.5 * plain["linear"]).abs().max().item() <= 1e-6 * plain["linear"].abs().max().item()


def test_chunking_and_graphs(scene):
    pipe, rb, _ = scene
    m = pipe.model
    for storage in ("fp32", "fp16"):
        a = bake_transfer(m, rb, storage=storage, chunk=32, camera_index=1)
        b = bake_transfer(m, rb, storage=storage, chunk=64, camera_index=1)
        assert torch.equal(a.T, b.T) and torch.equal(a.acc, b.acc)
        assert a.exponents is None or torch.equal(a.exponents, b.exponents)
    eager = bake_transfer(m, rb, storage="fp32", chunk=50, use_graph=False, camera_index=1)
    graph = bake_transfer(m, rb, storage="fp32", chunk=32, use_graph=True, camera_index=1)
    x, y = graph.relight(m, camera_index=1)["rgb"], eager.relight(m, camera_index=1)["rgb"]
    assert (x - y).abs().max().item() < 2e-6


def test_a_bake_leaves_the_frame_render_untouched(scene):
    pipe, rb, _ = scene
    m = pipe.model
    before = m.get_outputs_for_camera_ray_bundle(rb, camera_index=1, chunk=32, use_graph=True)
    before = {k: v.clone() for k, v in before.items()}
    runners = dict(m.frames.runners)
    bake_transfer(m, rb, storage="fp16", chunk=32, camera_index=1)
    assert m.frames.active is None
    assert m.frames.runners.keys() == runners.keys() and all(m.frames.runners[k] is r for k, r in runners.items())
    after = m.get_outputs_for_camera_ray_bundle(rb, camera_index=1, chunk=32, use_graph=True)
    assert after.keys() == before.keys()
    for k, v in before.items():
        assert torch.equal(after[k], v), k


@pytest.mark.parametrize("storage", ["fp32", "fp16"])
def test_save_load_relight(scene, tmp_path, storage):
    pipe, rb, envmap = scene
    m = pipe.model
    em = EnvironmentMap(envmap, "blender", exposure=0.8)
    baked = bake_transfer(m, rb, storage=storage, chunk=64, camera_index=1)
    baked.save(tmp_path / "frame.pt")
    loaded = RadianceTransfer.load(tmp_path / "frame.pt", DEV)
    assert loaded is not baked and loaded.storage == storage
    rot = z_rotation(1.3).to(DEV)
    for kw in (dict(envmap=em, rotations=rot), dict(camera_index=1)):
        a, b = baked.relight(m, **kw), loaded.relight(m, **kw)
        assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


def test_bake_needs_fixed_illumination_directions(scene):
    pipe, rb, _ = scene
    m = pipe.model
    m.config.fix_test_illumination_directions = False
    try:
        with pytest.raises(ValueError, match="fix_test_illumination_directions"):
            bake_transfer(m, rb, storage="fp32", chunk=32, camera_index=1)
    finally:
        m.config.fix_test_illumination_directions = True


def test_bake_without_visibility(scene):
    pipe, rb, _ = scene
    m = pipe.model
    S, D = _sizes(pipe)
    m.config.use_visibility = False
    try:
        ref = m.get_outputs_for_camera_ray_bundle(rb, camera_index=1, chunk=50, use_graph=False)
        got = bake_transfer(m, rb, storage="fp32", chunk=50, use_graph=False, camera_index=1).relight(m, camera_index=1)
    finally:
        m.config.use_visibility = True
    assert (got["rgb"] - ref["rgb"]).abs().max().item() <= 0.44 * (S + D) * EPS + 1e-6


def test_cli_turntable_from_a_transfer(tmp_path):
    from PIL import Image

    from neusky_amd.configs.neusky_config import synthetic_pipeline_config
    from neusky_amd.data.synthetic_datamanager import SyntheticDataManagerConfig
    from neusky_amd.utils.checkpoints import save_checkpoint
    torch.manual_seed(1)
    cfg = synthetic_pipeline_config()
    cfg.datamanager = SyntheticDataManagerConfig(num_train_images=3, num_eval_images=2)
    pipe = cfg.setup(device=DEV)
    randomise(pipe)
    ckpt = save_checkpoint(tmp_path, 3, pipe)
    H, W = 16, 24

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
    names = {}
    for mode in ("off", "fp32"):
        out = tmp_path / f"frames_{mode}"
        cmd = [sys.executable, "-m", "neusky_amd.relight", "--checkpoint", ckpt, "--camera-path", str(tmp_path / "camera_path.json"),
               "--output-dir", str(out), "--latent-index", "1", "--turntable", "4", "--save-hdr", "--transfer", mode]
        r = subprocess.run(["timeout", "-k", "10", "400"] + cmd, cwd=ROOT, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "8 frames" in r.stdout and (("bake" in r.stdout and "relight" in r.stdout) == (mode != "off"))
        names[mode] = sorted(os.listdir(out))
    assert names["off"] == names["fp32"] and len(names["off"]) == 16
    for n in names["off"]:
        if n.endswith(".png"):
            a = np.asarray(Image.open(tmp_path / "frames_off" / n), dtype=np.int64)
            b = np.asarray(Image.open(tmp_path / "frames_fp32" / n), dtype=np.int64)
            assert a.shape == (H, W, 3) and np.abs(a - b).max() <= 1, n
