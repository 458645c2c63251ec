"""python -m neusky_amd.relight with the prop flags: what they exclude is refused while the arguments are read; --prop-sphere and --props
write the frame the Python call renders, --prop-mask the props' share of each pixel, --prop-path the frames of a moving prop; the closing
line counts the props and the share of pixels they cover; without prop flags the frame is the plain frame's bytes."""
import gc
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import antialias_cpu as A
from util_step import randomise
from neusky_amd.relight import Prop, camera_rays, load_camera_path, load_props

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cli_with_the_prop_flags(tmp_path, capsys):
    from PIL import Image

    from neusky_amd.configs.neusky_config import synthetic_pipeline_config
    from neusky_amd.data.synthetic_datamanager import SyntheticDataManagerConfig
    from neusky_amd.relight.__main__ import build_pipeline, main
    from neusky_amd.utils.checkpoints import load_reference_pipeline_state, save_checkpoint
    torch.manual_seed(1)
    cfg = synthetic_pipeline_config()
    cfg.datamanager = SyntheticDataManagerConfig(num_train_images=3, num_eval_images=2)
    pipe = cfg.setup(device=DEV)
    randomise(pipe)
    ckpt = save_checkpoint(tmp_path, 3, pipe)
    Hc, Wc = 16, 24
    m = np.eye(4)
    m[:3] = A.look_at()
    path_file = tmp_path / "camera_path.json"
    path_file.write_text(json.dumps({"render_width": Wc, "render_height": Hc, "camera_type": "perspective",
                                     "camera_path": [{"camera_to_world": m.reshape(-1).tolist(), "fov": 55.0}]}))
    props_file = tmp_path / "props.json"
    props_file.write_text(json.dumps([{"shape": "box", "position": [0.0, 0.15, 0.0], "size": [0.05, 0.06, 0.07], "yaw_deg": 25,
                                       "albedo": [0.2, 0.6, 0.9]},
                                      {"shape": "sphere", "position": [0.2, 0.3, 0.4], "size": 0.1, "visible": False}]))
    # (chunks of 512 hold the frame's 384 rays: the chunk graphs, here and in the runs, stay small)
    base = ["--checkpoint", str(ckpt), "--camera-path", str(path_file), "--latent-index", "1", "--chunk", "512"]
    ball = ["--prop-sphere", "0.05", "-0.05", "0.0", "0.1", "0.8", "0.3", "0.2"]
    sun = ["--sun-azimuth", "130", "--sun-elevation", "35"]
    # refused while the arguments are read, before anything touches the device
    for flags, words in ((ball + ["--transfer", "fp32"], ("--prop-sphere", "--transfer")), (["--prop-mask"], ("--prop-mask needs a prop",)),
                         (["--prop-bias", "0.1"], ("--prop-bias needs a prop",)),
                         (["--prop-path", "0", "0", "0", "1", "1", "1", "--prop-steps", "2"], ("--prop-path needs a prop",)),
                         (ball + ["--prop-path", "0", "0", "0", "1", "1", "1"], ("--prop-steps",)),
                         (ball + ["--prop-path", "0", "0", "0", "1", "1", "1", "--prop-steps", "2", "--turntable", "2"], ("--turntable",)),
                         (ball + ["--prop-path", "0", "0", "0", "1", "1", "1", "--prop-steps", "2", "--sun-path", "0", "10", "90", "40",
                                  "--sun-steps", "2"], ("--sun-steps",)),
                         (ball + ["--prop-bias", "-1"], ("--prop-bias",)),
                         (["--prop-sphere", "0", "0", "0", "-0.1", "1", "1", "1"], ("radius",)),
                         (["--prop-box", "0", "0", "0", "0.1", "0.1", "0.1", "0", "1", "2", "1"], ("albedo",)),
                         (ball * 65, ("at most 64",))):
        with pytest.raises(SystemExit) as refused:
            main(base + ["--output-dir", str(tmp_path / "refused")] + flags)
        message = capsys.readouterr().err
        assert refused.value.code not in (0, None) and all(w in message for w in words), (flags[:4], message[-300:])
    assert not (tmp_path / "refused").exists()
    runs = [base + ["--output-dir", str(tmp_path / "plain")],
            base + ["--output-dir", str(tmp_path / "ball"), "--prop-mask"] + ball,
            base + ["--output-dir", str(tmp_path / "file"), "--props", str(props_file), "--prop-bias", "0.02", "--prop-mask", "--shadow-map"]
            + ball + sun,
            base + ["--output-dir", str(tmp_path / "path"), "--prop-path", "0.05", "-0.05", "0.0", "-0.1", "0.2", "0.1", "--prop-steps", "3"] + ball]
    script = "import sys, json\nfrom neusky_amd.relight.__main__ import main\nfor argv in json.loads(sys.argv[1]):\n    assert main(argv) == 0\n"
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-c", script, json.dumps(runs)], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    closing = [line for line in r.stdout.splitlines() if line.startswith("props:")]
    assert len(closing) == 3 and closing[0].startswith("props: 1 prop | share of pixels with prop_weight > 0.5: smallest"), r.stdout
    assert closing[1].startswith("props: 3 props |") and closing[2].startswith("props: 1 prop |")
    assert sorted(os.listdir(tmp_path / "plain")) == ["frame_0000_000.png"]
    assert sorted(os.listdir(tmp_path / "ball")) == ["frame_0000_000.png", "prop_0000_000.png"]
    assert sorted(os.listdir(tmp_path / "file")) == ["frame_0000_000.png", "prop_0000_000.png", "shadow_0000_000.png"]
    assert sorted(os.listdir(tmp_path / "path")) == [f"frame_0000_{f:03d}.png" for f in range(3)]
    # the same frames from Python
    state = torch.load(ckpt, map_location="cpu", weights_only=False)["pipeline"]
    again = build_pipeline(state, DEV)
    load_reference_pipeline_state(again, state)
    again.eval()
    model = again.model
    with torch.no_grad():
        model.eval_illumination_latents[0].copy_(model.train_illumination_latents[1])
        model.eval_scale[0].copy_(model.train_scale[1])
    rb = camera_rays(load_camera_path(str(path_file)), 0, DEV)
    frame = lambda **kw: model.get_outputs_for_camera_ray_bundle(rb, camera_index=0, chunk=512, **kw)  # noqa: E731
    png = lambda *p: np.asarray(Image.open(os.path.join(tmp_path, *p)))  # noqa: E731
    as8 = lambda x: np.round(x.clamp(0.0, 1.0).cpu().numpy() * 255.0).astype(np.uint8)  # noqa: E731
    assert np.array_equal(png("plain", "frame_0000_000.png"), as8(frame()["rgb"]))  # without prop flags: the plain frame's bytes
    first = Prop("sphere", (0.05, -0.05, 0.0), 0.1, (0.8, 0.3, 0.2))
    seen = frame(props=first)
    assert np.array_equal(png("ball", "frame_0000_000.png"), as8(seen["rgb"]))
    assert np.array_equal(png("ball", "prop_0000_000.png"), as8(seen["prop_weight"][..., 0]))
    assert png("ball", "prop_0000_000.png").max() > 128 and not np.array_equal(png("ball", "frame_0000_000.png"), png("plain", "frame_0000_000.png"))
    share = float((seen["prop_weight"] > 0.5).float().mean())
    assert f"smallest {share:.4g} largest {share:.4g}" in closing[0]
    from neusky_amd.relight import SunLight
    three = frame(props=[first, *load_props(props_file)], prop_bias=0.02, sun=SunLight(130.0, 35.0, (1.0, 1.0, 1.0)))
    assert np.array_equal(png("file", "frame_0000_000.png"), as8(three["rgb"]))
    assert np.array_equal(png("file", "prop_0000_000.png"), as8(three["prop_weight"][..., 0]))
    assert np.array_equal(png("file", "shadow_0000_000.png"), as8(three["shadow_map"][..., 0]))
    assert np.array_equal(png("path", "frame_0000_000.png"), as8(seen["rgb"]))
    last = frame(props=first.moved_to((-0.1, 0.2, 0.1)))
    assert np.array_equal(png("path", "frame_0000_002.png"), as8(last["rgb"]))
    assert not np.array_equal(png("path", "frame_0000_000.png"), png("path", "frame_0000_002.png"))
    del frame, seen, three, last, model, again, pipe
    gc.collect()
    torch.cuda.empty_cache()  # (the full-size model's chunk graphs: handed back before the next test's processes start)
