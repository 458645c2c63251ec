"""python -m neusky_amd.relight on three paths through its run (relight/sequence.py) that no other test takes: frames that wait for their
camera's exposure together with their lamps' share, over two cameras; a sun path of one step under a moving lamp, with the lamps' picture
of a run without a display transform (the default transform's: HIP kernels, so tests/test_relight_sequence_cpu.py leaves it to this
test); the mask a sun sweep's frames share."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from util_step import randomise
from neusky_amd.relight import DisplayTransform, PointLight, camera_rays, load_camera_path, sun_path, z_rotation

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pose(a):
    c, s = math.cos(a), math.sin(a)
    eye = np.array([0.6 * c, 0.6 * s, 0.05])
    fwd = -eye / np.linalg.norm(eye)
    right = np.cross(fwd, [0.0, 0.0, 1.0])
    right /= np.linalg.norm(right)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = right, np.cross(right, fwd), -fwd, eye
    return {"camera_to_world": m.reshape(-1).tolist(), "fov": 55.0}


def test_cli_deferred_lamps_a_lamp_under_a_one_step_sun_path_and_a_sweeps_mask(tmp_path):
    from PIL import Image

    from neusky_amd.configs.neusky_config import synthetic_pipeline_config
    from neusky_amd.data.synthetic_datamanager import SyntheticDataManagerConfig
    from neusky_amd.relight.__main__ import build_pipeline
    from neusky_amd.utils.checkpoints import load_reference_pipeline_state, save_checkpoint
    torch.manual_seed(1)
    cfg = synthetic_pipeline_config()
    cfg.datamanager = SyntheticDataManagerConfig(num_train_images=3, num_eval_images=2)
    pipe = cfg.setup(device=DEV)
    randomise(pipe)
    ckpt = save_checkpoint(tmp_path, 3, pipe)
    Hc, Wc = 16, 24
    shape = {"render_width": Wc, "render_height": Hc, "camera_type": "perspective"}
    two_file, one_file = tmp_path / "two_cameras.json", tmp_path / "one_camera.json"
    two_file.write_text(json.dumps({**shape, "camera_path": [_pose(0.3), _pose(1.4)]}))
    one_file.write_text(json.dumps({**shape, "camera_path": [_pose(0.3)]}))
    base = ["--checkpoint", str(ckpt), "--latent-index", "1"]
    lamp = ["--light", "0.3", "-0.2", "0.4", "1.5", "1.2", "0.9", "--light-shadow-steps", "16"]
    ends = ((0.3, -0.2, 0.4), (-0.3, 0.3, 0.2))
    runs = [base + ["--camera-path", str(two_file), "--output-dir", str(tmp_path / "metered"), "--turntable", "2", "--tonemap", "aces",
                    "--auto-exposure", "sequence", "--save-linear", "--light-map"] + lamp,
            base + ["--camera-path", str(one_file), "--output-dir", str(tmp_path / "lamp"), "--sun-path", "120", "30", "240", "30",
                    "--sun-steps", "1", "--light-path", *map(str, ends[0] + ends[1]), "--light-steps", "2", "--light-map"] + lamp,
            base + ["--camera-path", str(one_file), "--output-dir", str(tmp_path / "sweep"), "--sun-path", "120", "10", "240", "40",
                    "--sun-steps", "2", "--antialias", "4", "--aa-mask"]]
    script = "import sys, json\nfrom neusky_amd.relight.__main__ import main\nfor argv in json.loads(sys.argv[1]):\n    assert main(argv) == 0\n"
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-c", script, json.dumps(runs)], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    # the same frames from Python
    state = torch.load(ckpt, map_location="cpu", weights_only=False)["pipeline"]
    again = build_pipeline(state, DEV)
    load_reference_pipeline_state(again, state)
    again.eval()
    model = again.model
    with torch.no_grad():
        model.eval_illumination_latents[0].copy_(model.train_illumination_latents[1])
        model.eval_scale[0].copy_(model.train_scale[1])
    png = lambda *p: np.asarray(Image.open(os.path.join(tmp_path, *p)))  # noqa: E731
    intensity = (1.5, 1.2, 0.9)

    # frames that wait for their camera's exposure, and their lamps' share with them
    stems = [f"_{c:04d}_{f:03d}" for c in range(2) for f in range(2)]
    assert sorted(os.listdir(tmp_path / "metered")) == sorted(
        [f"frame{s}{e}" for s in stems for e in (".png", ".lin.npy", ".lights.npy")] + [f"lights{s}.png" for s in stems])
    display = DisplayTransform(curve="aces", exposure="sequence")
    cams = load_camera_path(str(two_file))
    exposures, images = [], []
    for c in range(2):
        rb = camera_rays(cams, c, DEV)
        outs = [model.get_outputs_for_camera_ray_bundle(rb, camera_index=0, chunk=4096, rotation=None if f == 0 else z_rotation(math.pi).to(DEV),
                                                        lights=PointLight(ends[0], intensity), light_trace={"steps": 16}) for f in range(2)]
        hist = None
        for f, out in enumerate(outs):
            assert np.array_equal(np.load(tmp_path / "metered" / f"frame_{c:04d}_{f:03d}.lin.npy"), out["lin"].cpu().numpy()), (c, f)
            assert np.array_equal(np.load(tmp_path / "metered" / f"frame_{c:04d}_{f:03d}.lights.npy"), out["light_lin"].cpu().numpy()), (c, f)
            hist = display.luminance_histogram(out["lin"], out["accumulation"], out=hist)
        E = display.exposure_from_histogram(hist)
        for f, out in enumerate(outs):
            for name, x in (("frame", out["lin"]), ("lights", out["light_lin"])):
                want = display.apply(x, exposure=E)["rgb8"].cpu().numpy()
                assert np.array_equal(png("metered", f"{name}_{c:04d}_{f:03d}.png"), want), (name, c, f)
        exposures.append(float(E))
        images.append(torch.stack([out["lin"] for out in outs]))
    assert png("metered", "lights_0000_000.png").max() > 0
    if not torch.equal(images[0], images[1]):
        assert exposures[0] != exposures[1], exposures
    closing = [line for line in r.stdout.splitlines() if line.startswith("display:")]
    assert len(closing) == 1 and "tonemap aces" in closing[0] and "metered per camera" in closing[0], r.stdout
    words = closing[0].split()
    for word, want in (("smallest", min(exposures)), ("largest", max(exposures))):
        assert abs(float(words[words.index(word) + 1]) / want - 1.0) < 1e-3  # (four digits are printed)

    # a sun path of one step is one sun: the moving lamp's frames are rendered one by one under it
    assert sorted(os.listdir(tmp_path / "lamp")) == ["frame_0000_000.png", "frame_0000_001.png", "lights_0000_000.png", "lights_0000_001.png"]
    rb = camera_rays(load_camera_path(str(one_file)), 0, DEV)
    sun = sun_path(120.0, 30.0, 240.0, 30.0, 1)[0]
    for f, at in enumerate(ends):
        out = model.get_outputs_for_camera_ray_bundle(rb, camera_index=0, chunk=4096, sun=sun, lights=PointLight(at, intensity),
                                                      light_trace={"steps": 16})
        want = np.round(out["rgb"].clamp(0.0, 1.0).cpu().numpy() * 255.0).astype(np.uint8)
        assert want.shape == (Hc, Wc, 3) and np.array_equal(png("lamp", f"frame_0000_{f:03d}.png"), want), f
        # no display transform: the lamps' picture is the default transform's, the sRGB curve and 8 bits
        want = DisplayTransform().apply(out["light_lin"])["rgb8"].cpu().numpy()
        assert want.max() > 0 and np.array_equal(png("lamp", f"lights_0000_{f:03d}.png"), want), f
    for name in ("frame", "lights"):
        assert not np.array_equal(png("lamp", f"{name}_0000_000.png"), png("lamp", f"{name}_0000_001.png")), name

    # a sweep's frames come from one render: they share its mask
    assert sorted(os.listdir(tmp_path / "sweep")) == sorted([f"{k}_0000_{f:03d}.png" for k in ("aa", "frame") for f in range(2)])
    assert (tmp_path / "sweep" / "aa_0000_000.png").read_bytes() == (tmp_path / "sweep" / "aa_0000_001.png").read_bytes()
    assert set(np.unique(png("sweep", "aa_0000_000.png")).tolist()) <= {0, 255}
