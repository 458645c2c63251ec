"""Frames lit by a directional sun (get_outputs_for_camera_ray_bundle(..., sun=)): the sun term against the float64 restatement of its
definition (sun_cpu.py) on the chunk's own field outputs, the shadow map against the DDF query it is defined by, K suns against K
single-sun frames, graph replay across sun positions, a sweep through the horizon, a sun on an environment-map frame; and the
`python -m neusky_amd.relight --sun-path` command line from a saved checkpoint."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import sun_cpu as SC
from util_frames import frame_scene
from util_step import randomise
from neusky_amd.relight import EnvironmentMap
from neusky_amd.relight.sun import SunLight, sun_path

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, CHUNK = 13, 16, 64  # 208 rays: three whole chunks and a padded one
SUN = SunLight(130.0, 35.0, (2.0, 1.7, 1.2))
DARK = SunLight(130.0, 35.0, (0.0, 0.0, 0.0))
LIN_BAR = 1e-5  # the bar of test_gpu_relight_frame.py on its linear image


@pytest.fixture(scope="module")
def scene():
    pipe, rb = frame_scene(H, W, DEV)
    m = pipe.model
    render = lambda **kw: m.get_outputs_for_camera_ray_bundle(rb, camera_index=1, chunk=CHUNK, **kw)  # noqa: E731
    before = {k: v.clone() for k, v in render(use_graph=True).items()}  # the frame BEFORE any sun
    lit = render(use_graph=True, sun=SUN)
    dark = render(use_graph=True, sun=DARK)
    return pipe, rb, render, before, lit, dark


def _f64(t):
    return t.detach().cpu().double().numpy()


def test_zero_colour_sun_is_the_frame_without_one(scene):
    _, _, render, before, _, dark = scene
    for k, v in before.items():
        assert torch.equal(dark[k], v), k
    assert set(dark) == set(before) | {"lin", "shadow_map", "shadow_difference"}
    assert dark["shadow_map"].shape == (H, W, 1) and dark["shadow_difference"].shape == (H, W, 1) and dark["lin"].shape == (H, W, 3)
    after = render(use_graph=True)  # and the path without a sun is what it was
    for k, v in before.items():
        assert torch.equal(after[k], v), k


def test_sun_term_matches_its_definition(scene):
    pipe, rb, render, _, lit, dark = scene
    m = pipe.model
    eager, eager_dark = render(use_graph=False, sun=SUN), render(use_graph=False, sun=DARK)
    flat = rb.slice(0, 1 << 62)
    s32 = np.array(SUN.direction, np.float64).astype(np.float32)
    t = []
    with torch.no_grad():
        m.begin_frame(1, None, None, SUN)
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
                t.append(SC.transfer(_f64(albedo), _f64(normals), _f64(so["weights"][..., 0]), s32[None])[0][0])
        finally:
            m.end_frame()
    t = np.concatenate(t)  # [N, 3]
    for got, sky in ((eager, eager_dark), (lit, dark)):
        V = _f64(got["shadow_map"]).reshape(-1, 1)
        ref = _f64(sky["lin"]).reshape(-1, 3) + np.array(SUN.colour, np.float32).astype(np.float64)[None] * V * t
        err = np.abs(_f64(got["lin"]).reshape(-1, 3) - ref).max()
        print(f"lin vs lin_sky + C V t: max err {err:.3e}, max {ref.max():.3f}, sun term max {(ref - _f64(sky['lin']).reshape(-1, 3)).max():.3f}")
        assert err < LIN_BAR
        np.testing.assert_allclose(_f64(got["rgb"]).reshape(-1, 3), SC.linear_to_srgb(_f64(got["lin"]).reshape(-1, 3)), rtol=1e-4, atol=1e-6)
    assert (_f64(lit["lin"]) - _f64(dark["lin"])).max() > 1e-2  # the sun lit something
    assert (lit["rgb"] - eager["rgb"]).abs().max().item() < 2e-6


def test_shadow_map_is_the_ddf_query_of_the_sun_direction(scene):
    """the reference query runs all 208 rays at once, the frame 64 at a time: the DDF distances of the two agree to fp32 chain
    rounding (1e-5 on distances of order 1), and the sigmoid turns a distance error e into at most scale / 4 * e."""
    pipe, rb, _, before, lit, _ = scene
    m = pipe.model
    flat = rb.slice(0, 1 << 62)
    sun_dirs = torch.tensor([SUN.direction], dtype=torch.float64).to(torch.float32).to(DEV)
    with torch.no_grad():
        m.begin_step()
        ref = m.compute_visibility_compact(flat.origins.contiguous(), flat.directions.contiguous(), before["p2p_dist"].reshape(-1, 1), sun_dirs,
                                           m.visibility_threshold, m.sigmoid_scale, compute_shadow_map=True,
                                           sel=torch.zeros(1, dtype=torch.int32, device=DEV))
    mask = (before["accumulation"].reshape(-1) > 0.0).double().cpu().numpy()
    assert mask.any()
    d_err = np.abs(_f64(lit["shadow_difference"]).reshape(-1) - _f64(ref["difference"]).reshape(-1) * mask).max()
    v_err = np.abs(_f64(lit["shadow_map"]).reshape(-1) - _f64(ref["visibility"]).reshape(-1) * mask).max()
    print(f"shadow_difference err {d_err:.3e}, shadow_map err {v_err:.3e}")
    assert d_err < 1e-5 and v_err < m.sigmoid_scale / 4.0 * 1e-5
    sm = lit["shadow_map"]
    assert sm.min().item() >= 0.0 and sm.max().item() <= 1.0


def test_overrides_reach_the_shadow(scene):
    pipe, _, render, _, lit, _ = scene
    m = pipe.model
    n = len(m.frames.runners)
    d = _f64(lit["shadow_difference"])
    thr = float(np.median(d))  # a threshold inside the frame's own range of differences
    got = render(use_graph=True, sun=SUN, shadow_threshold=thr)
    assert len(m.frames.runners) == n  # a threshold replays the chunk graph
    ref = 1.0 - 1.0 / (1.0 + np.exp(-m.sigmoid_scale * (d - thr)))
    on = _f64(lit["accumulation"]) > 0.0
    assert np.abs(_f64(got["shadow_map"]) - ref * on).max() < 1e-5
    masked = render(use_graph=True, sun=SUN, accumulation_mask_threshold=2.0)  # no ray accumulates more than 1
    assert len(m.frames.runners) == n
    assert masked["shadow_map"].abs().max().item() == 0.0 and masked["shadow_difference"].abs().max().item() == 0.0
    assert torch.equal(masked["rgb"], render(use_graph=True)["rgb"])


def test_nine_suns_are_nine_single_frames(scene):
    _, _, render, _, _, _ = scene
    suns = [SunLight(40.0 * i, 8.0 * i - 6.0, (1.0 + 0.1 * i, 1.0, 2.0 - 0.2 * i)) for i in range(9)]  # (the first has set)
    many = render(use_graph=True, sun=suns)
    assert many["rgb"].shape == (9, H, W, 3) and many["shadow_map"].shape == (9, H, W, 1) and many["shadow_difference"].shape == (9, H, W, 1)
    assert many["albedo"].shape == (H, W, 3)
    for i, s in enumerate(suns):
        one = render(use_graph=True, sun=s)
        for k in ("rgb", "lin", "shadow_map", "shadow_difference"):
            assert torch.equal(many[k][i], one[k]), (i, k)
    assert not torch.equal(many["rgb"][3], many["rgb"][5])


def test_a_new_sun_replays_the_captured_chunk(scene):
    pipe, _, render, _, _, _ = scene
    m = pipe.model
    a, b = SunLight(20.0, 60.0, (1.0, 1.0, 1.0)), SunLight(250.0, 15.0, (3.0, 2.0, 0.5))
    got_a = render(use_graph=True, sun=a)
    runners = dict(m.frames.runners)
    got_b = render(use_graph=True, sun=b)
    assert len(m.frames.runners) == len(runners) and all(m.frames.runners[k] is r for k, r in runners.items())
    assert not torch.equal(got_a["rgb"], got_b["rgb"])
    for got, s in ((got_a, a), (got_b, b)):
        eager = render(use_graph=False, sun=s)
        for k in ("rgb", "lin", "shadow_map"):
            assert (got[k] - eager[k]).abs().max().item() < 2e-6, k


def test_sweep_through_the_horizon(scene):
    _, _, render, before, _, _ = scene
    path = sun_path(90.0, 5.0, 100.0, -5.0, 5, colour=(2.0, 2.0, 2.0))
    out = render(use_graph=True, sun=path)
    assert all(torch.isfinite(out[k]).all() for k in ("rgb", "lin", "shadow_map", "shadow_difference"))
    for i, s in enumerate(path):
        if s.elevation_deg <= 0.0:
            assert torch.equal(out["rgb"][i], before["rgb"]), i
            assert out["shadow_map"][i].abs().max().item() == 0.0 and out["shadow_difference"][i].abs().max().item() == 0.0
    assert not torch.equal(out["rgb"][0], before["rgb"])


def test_sun_on_an_envmap_frame(scene):
    _, _, render, _, lit, dark = scene
    env = EnvironmentMap((torch.rand(32, 64, 3, generator=torch.Generator().manual_seed(7)) ** 2 * 3.0).numpy(), "blender", exposure=0.8)
    plain = render(use_graph=True, envmap=env)
    e_dark, e_lit = render(use_graph=True, envmap=env, sun=DARK), render(use_graph=True, envmap=env, sun=SUN)
    assert torch.equal(e_dark["rgb"], plain["rgb"])
    assert not torch.equal(e_dark["lin"], dark["lin"])  # another sky
    term = _f64(lit["lin"]) - _f64(dark["lin"])
    assert np.abs(_f64(e_lit["lin"]) - (_f64(e_dark["lin"]) + term)).max() < LIN_BAR
    assert torch.equal(e_lit["shadow_map"], lit["shadow_map"])


def test_cli_sweeps_a_sun_over_a_checkpoint(tmp_path):
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

    (tmp_path / "camera_path.json").write_text(json.dumps({"render_width": Wc, "render_height": Hc, "camera_type": "perspective",
                                                           "camera_path": [pose(0.3)]}))
    out = tmp_path / "frames"
    cmd = [sys.executable, "-m", "neusky_amd.relight", "--checkpoint", ckpt, "--camera-path", str(tmp_path / "camera_path.json"),
           "--output-dir", str(out), "--latent-index", "0", "--sun-path", "120", "10", "240", "10", "--sun-steps", "3", "--shadow-map"]
    r = subprocess.run(["timeout", "-k", "10", "400"] + cmd, cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "3 frames" in r.stdout
    frames = [np.asarray(Image.open(str(out / f"frame_0000_{f:03d}.png"))) for f in range(3)]
    shadows = [np.asarray(Image.open(str(out / f"shadow_0000_{f:03d}.png"))) for f in range(3)]
    assert sorted(os.listdir(out)) == sorted([f"frame_0000_{f:03d}.png" for f in range(3)] + [f"shadow_0000_{f:03d}.png" for f in range(3)])
    assert all(f.shape == (Hc, Wc, 3) and f.dtype == np.uint8 for f in frames)
    assert all(s.shape == (Hc, Wc) and s.dtype == np.uint8 for s in shadows)
    assert not np.array_equal(frames[0], frames[1]) and not np.array_equal(frames[1], frames[2]) and not np.array_equal(frames[0], frames[2])
