"""Relighting render pass (BASELINE config 5 at test size): chunked, HIP-graph-replayed full-frame forward against the
CPU oracle, chunk-size independence, and z-rotation of the illumination."""
import math

import pytest
import torch

from oracle import neusky_oracle as O
from util_frames import frame_scene
from util_step import oracle_params, oracle_step_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def scene():
    H, W = 9, 13
    pipe, rb = frame_scene(H, W, DEV)
    return pipe, rb, (H, W)


def _oracle(pipe, rb, rotation=None):
    p = oracle_params(pipe)
    m = pipe.model
    light = m.illumination_sampler.directions.double()
    return O.neusky_render({k: v.detach() for k, v in p.items()} | {"field.table": p["field.table"]}, oracle_step_cfg(pipe),
                           rb.origins.reshape(-1, 3).cpu().double(), rb.directions.reshape(-1, 3).cpu().double(),
                           m.eval_illumination_latents[1].detach().cpu().double(), m.eval_scale[1].detach().cpu().double(), light,
                           None if rotation is None else rotation.double())


def test_frame_matches_oracle_and_chunking(scene):
    pipe, rb, (H, W) = scene
    ref = _oracle(pipe, rb)
    full = pipe.model.get_outputs_for_camera_ray_bundle(rb, camera_index=1, chunk=32, use_graph=True)
    assert full["rgb"].shape == (H, W, 3)
    got = full["rgb"].reshape(-1, 3).cpu().double()
    rel = ((got - ref["rgb"]).abs().max() / ref["rgb"].abs().max()).item()
    assert rel < 1e-4, rel  # north-star tolerance on rendered radiance
    assert (full["p2p_dist"].reshape(-1, 1).cpu().double() - ref["p2p_dist"]).abs().max().item() < 1e-4
    assert (full["normal"].reshape(-1, 3).cpu().double() - ref["normal"]).abs().max().item() < 2e-4
    # any chunking (and no graph) gives the same image
    other = pipe.model.get_outputs_for_camera_ray_bundle(rb, camera_index=1, chunk=50, use_graph=False)
    assert (other["rgb"] - full["rgb"]).abs().max().item() < 2e-6


def test_frame_with_z_rotation(scene):
    pipe, rb, _ = scene
    a = 0.9
    rot = torch.tensor([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]])
    ref = _oracle(pipe, rb, rot)
    got = pipe.model.get_outputs_for_camera_ray_bundle(rb, camera_index=1, chunk=64, rotation=rot.to(DEV), use_graph=True)
    rel = ((got["rgb"].reshape(-1, 3).cpu().double() - ref["rgb"]).abs().max() / ref["rgb"].abs().max()).item()
    assert rel < 1e-4, rel
