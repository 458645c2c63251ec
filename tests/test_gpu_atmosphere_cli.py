"""python -m neusky_amd.relight with the fog flags: --fog-density writes the frame the Python call renders with `atmosphere=`, --fog-map its
transmittance in 8 bits, --save-linear its in-scatter; the closing line reports the mean transmittance and what the shafts cost; a run
without fog flags writes the files it always wrote."""
import dataclasses
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
from neusky_amd.relight import Atmosphere, SunLight, camera_rays, load_camera_path

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cli_with_the_fog_flags(tmp_path, capsys):
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
    del pipe
    Hc, Wc = 16, 24
    m = np.eye(4)
    m[:3] = A.look_at()
    path_file = tmp_path / "camera_path.json"
    path_file.write_text(json.dumps({"render_width": Wc, "render_height": Hc, "camera_type": "perspective",
                                     "camera_path": [{"camera_to_world": m.reshape(-1).tolist(), "fov": 55.0}]}))
    # (one chunk of 512 holds the frame's 384 rays; a chunk graph of the default 4096 takes eight times the memory for the same frame)
    base = ["--checkpoint", str(ckpt), "--camera-path", str(path_file), "--latent-index", "1", "--chunk", "512"]
    fog = ["--fog-density", "0.5", "1.0", "2.0", "--fog-scale-height", "0.4", "--fog-anisotropy", "0.5"]
    sun = ["--sun-azimuth", "130", "--sun-elevation", "35", "--sun-colour", "2", "1.7", "1.2"]
    # refused while the arguments are read, before anything touches the device
    for flags, words in ((fog + ["--transfer", "fp16"], ("--fog-density", "--transfer fp16")), (["--fog-map"], ("--fog-map needs --fog-density",)),
                         (fog + ["--fog-shafts", "4"], ("--fog-shafts", "needs a sun"))):
        with pytest.raises(SystemExit) as refused:
            main(base + ["--output-dir", str(tmp_path / "refused")] + flags)
        message = capsys.readouterr().err
        assert refused.value.code not in (0, None) and all(w in message for w in words), (flags[:4], message[-300:])
    assert not (tmp_path / "refused").exists()
    runs = [base + ["--output-dir", str(tmp_path / "clear")],
            base + ["--output-dir", str(tmp_path / "fog"), "--fog-map", "--save-linear"] + fog,
            base + ["--output-dir", str(tmp_path / "shafts"), "--fog-shafts", "3", "--fog-clear-background"] + fog + sun]
    script = "import sys, json\nfrom neusky_amd.relight.__main__ import main\nfor argv in json.loads(sys.argv[1]):\n    assert main(argv) == 0\n"
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-c", script, json.dumps(runs)], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    closing = [line for line in r.stdout.splitlines() if line.startswith("fog:")]
    assert len(closing) == 2 and closing[0].endswith("| no shafts"), r.stdout
    assert closing[1].endswith("| 3 shaft samples x 1 sun: 3 extra DDF rows per ray"), r.stdout
    assert sorted(os.listdir(tmp_path / "clear")) == ["frame_0000_000.png"]
    assert sorted(os.listdir(tmp_path / "fog")) == ["fog_0000_000.png", "frame_0000_000.inscatter.npy", "frame_0000_000.lin.npy", "frame_0000_000.png"]
    assert sorted(os.listdir(tmp_path / "shafts")) == ["frame_0000_000.png"]
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
    as8 = lambda rgb: np.round(rgb.clamp(0.0, 1.0).cpu().numpy() * 255.0).astype(np.uint8)  # noqa: E731
    clear = frame()
    assert np.array_equal(png("clear", "frame_0000_000.png"), as8(clear["rgb"]))  # no fog flags: the file the run always wrote
    medium = Atmosphere((0.5, 1.0, 2.0), scale_height=0.4, anisotropy=0.5)
    fogged = frame(atmosphere=medium)
    assert np.array_equal(np.load(tmp_path / "fog" / "frame_0000_000.lin.npy"), fogged["lin"].cpu().numpy())
    assert np.array_equal(np.load(tmp_path / "fog" / "frame_0000_000.inscatter.npy"), fogged["atmosphere_inscatter"].cpu().numpy())
    assert np.array_equal(png("fog", "fog_0000_000.png"), as8(fogged["atmosphere_transmittance"]))
    assert png("fog", "fog_0000_000.png").shape == (Hc, Wc, 3) and png("fog", "fog_0000_000.png").min() < 255
    assert np.abs(png("fog", "frame_0000_000.png").astype(int) - as8(fogged["rgb"]).astype(int)).max() <= 1  # (the display path's 8 bits)
    assert not np.array_equal(png("fog", "frame_0000_000.png"), png("clear", "frame_0000_000.png"))
    mean = float(fogged["atmosphere_transmittance"].mean())
    assert closing[0].startswith(f"fog: mean transmittance smallest {mean:.4g} largest {mean:.4g} |"), closing[0]
    shafts = frame(sun=SunLight(130.0, 35.0, (2.0, 1.7, 1.2)), atmosphere=dataclasses.replace(medium, shaft_samples=3, background=False))
    assert np.array_equal(png("shafts", "frame_0000_000.png"), as8(shafts["rgb"]))
    # the chunk graphs' pools go back to the device: the runs of other tests' command lines are processes of their own and need the room
    del frame, model, again, clear, fogged, shafts
    gc.collect()
    torch.cuda.empty_cache()
