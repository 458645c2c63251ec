"""Frames lit by the sun extracted from their environment map (relight.extract_sun): the projected light keeps the map's flux, a rolled
map with its own extraction is the original under a rotation with the sun turned back by it (which pins the R^T of SunExtraction.sun),
a turntable replays the captured chunk graphs, and `python -m neusky_amd.relight --extract-sun` from a saved checkpoint."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import envmap_sun_cpu as EC
from util_frames import frame_scene
from util_step import randomise
from neusky_amd.relight import EnvironmentMap, SunLight, extract_sun, project_envmap, z_rotation

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, CHUNK = 13, 16, 64  # the frame of test_gpu_sun_frame.py: 208 rays, three whole chunks and a padded one
MH, MW, SIGMA, RHO = 64, 128, 4.0, 12.0
AZ, EL = 130.7, 35.3  # not a texel centre
ROLL = 11


@pytest.fixture(scope="module")
def scene():
    pipe, rb = frame_scene(H, W, DEV)
    m = pipe.model

    def render(use_graph=True, **kw):
        return m.get_outputs_for_camera_ray_bundle(rb, camera_index=1, chunk=CHUNK, use_graph=use_graph, **kw)

    return pipe, render


@pytest.mark.parametrize("conv", ["blender", "neusky"])
def test_projected_light_keeps_the_flux(scene, conv):
    pipe, _ = scene
    dirs = pipe.model.illumination_sampler.directions
    env = EnvironmentMap(EC.synthetic_map(MH, MW, conv, AZ, EL, SIGMA), conv, exposure=0.8)
    ext = extract_sun(env, radius_deg=RHO)
    assert ext.found and EC.angle_deg(ext.direction, EC.direction(AZ, EL)) < 45.0 / MH
    rot = z_rotation(0.7).to(DEV)

    def flux(e):
        c, w = project_envmap(e, dirs, rot)
        assert (w > 0).all()  # every cell holds texels: no cell fell back to the lookup
        return (w.double()[:, None] * c.double()).sum(dim=0).cpu().numpy()

    before, after = flux(env), flux(ext.envmap) + 2.0 * np.pi * np.array(ext.colour) * 0.8
    rel = np.abs(before - after).max() / np.abs(before).max()
    print(f"{conv}: flux {before}, residual + sun {after}, rel {rel:.2e}; sun share {ext.flux_fraction:.3f}")
    assert rel < 1e-5
    np.testing.assert_allclose(ext.sun().colour, 0.8 * np.array(ext.colour), rtol=1e-15)


@pytest.mark.parametrize("conv", ["blender", "neusky"])
def test_rolled_map_is_a_rotation_with_the_sun_turned_back(scene, conv):
    _, render = scene
    m = EC.synthetic_map(MH, MW, conv, AZ, EL, SIGMA)
    angle = 2.0 * math.pi * ROLL / MW
    rolled = np.roll(m, -ROLL if conv == "neusky" else ROLL, axis=1)  # z_rotation's docstring: this map is the original turned by angle
    ext, ext_r = extract_sun(EnvironmentMap(m, conv), radius_deg=RHO), extract_sun(EnvironmentMap(rolled, conv), radius_deg=RHO)
    assert ext.found and ext_r.found
    az, az_r = SunLight.from_direction(ext.direction), SunLight.from_direction(ext_r.direction)
    assert abs((az_r.azimuth_deg - (az.azimuth_deg - math.degrees(angle)) + 180.0) % 360.0 - 180.0) < 1e-6  # R d = m: the sun at -angle
    assert abs(az_r.elevation_deg - az.elevation_deg) < 1e-6
    np.testing.assert_allclose(ext_r.colour, ext.colour, rtol=1e-6)
    R = z_rotation(angle)
    turned = ext.sun(R)
    assert EC.angle_deg(turned.direction, ext_r.sun().direction) < 1e-5  # (R is fp32)
    a = render(envmap=ext_r.envmap, sun=ext_r.sun())
    b = render(envmap=ext.envmap, rotation=R.to(DEV), sun=turned)
    for k in ("rgb", "shadow_map"):
        err = (a[k] - b[k]).abs().max().item()
        print(f"{conv} {k}: rolled map vs rotation {err:.2e}")
        assert err < 2e-6, k
    wrong = render(envmap=ext.envmap, rotation=R.to(DEV), sun=SunLight.from_direction(R.double().numpy() @ np.array(ext.direction), turned.colour))
    assert (a["rgb"] - wrong["rgb"]).abs().max().item() > 1e-3  # R instead of R^T is another frame
    no_sun = render(envmap=ext.envmap, rotation=R.to(DEV))
    assert (b["rgb"] - no_sun["rgb"]).abs().max().item() > 1e-2  # and the sun lights something


def test_turntable_replays_the_captured_chunks(scene):
    pipe, render = scene
    m = pipe.model
    ext = extract_sun(EnvironmentMap(EC.synthetic_map(MH, MW, "blender", AZ, EL, SIGMA), "blender"), radius_deg=RHO)
    r1, r2 = z_rotation(0.4), z_rotation(2.9)
    one = render(envmap=ext.envmap, rotation=r1.to(DEV), sun=ext.sun(r1))
    one = {k: v.clone() for k, v in one.items()}
    runners = dict(m.frames.runners)
    graphs = {k: r.graph for k, r in runners.items()}
    two = render(envmap=ext.envmap, rotation=r2.to(DEV), sun=ext.sun(r2))
    assert m.frames.runners.keys() == runners.keys()  # the cache did not grow: the residual map is one tensor for the whole run
    assert all(m.frames.runners[k] is r and r.graph is graphs[k] for k, r in runners.items())
    assert not torch.equal(one["rgb"], two["rgb"]) and not torch.equal(one["shadow_map"], two["shadow_map"])
    eager = render(use_graph=False, envmap=ext.envmap, rotation=r2.to(DEV), sun=ext.sun(r2))
    for k in ("rgb", "shadow_map"):
        assert (two[k] - eager[k]).abs().max().item() < 2e-6, k


def test_cli_extracts_the_sun(tmp_path):
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
    np.save(tmp_path / "sunny.npy", EC.synthetic_map(MH, MW, "blender", AZ, EL, SIGMA))
    np.save(tmp_path / "overcast.npy", EC.sky_map(MH, MW, "blender").astype(np.float32))

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
    base = ["--checkpoint", str(ckpt), "--camera-path", str(tmp_path / "camera_path.json"), "--turntable", "2"]
    runs = [base + ["--output-dir", str(tmp_path / "sunny"), "--envmap", str(tmp_path / "sunny.npy"), "--extract-sun", "--shadow-map",
                    "--sun-search-radius", str(RHO), "--exposure", "0.5"],
            base + ["--output-dir", str(tmp_path / "flagged"), "--envmap", str(tmp_path / "overcast.npy"), "--extract-sun", "--shadow-map",
                    "--sun-search-radius", str(RHO)],
            base + ["--output-dir", str(tmp_path / "plain"), "--envmap", str(tmp_path / "overcast.npy")]]
    script = "import sys, json\nfrom neusky_amd.relight.__main__ import main\nfor argv in json.loads(sys.argv[1]):\n    assert main(argv) == 0\n"
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-c", script, json.dumps(runs)], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    found = [line for line in r.stdout.splitlines() if line.startswith("sun found:")]
    assert len(found) == 1 and "azimuth" in found[0] and "elevation" in found[0] and "diameter" in found[0], r.stdout
    words = found[0].split()
    az, el = float(words[words.index("azimuth") + 1]), float(words[words.index("elevation") + 1])
    assert abs(az - AZ) < 0.05 + 45.0 / MH and abs(el - EL) < 0.05 + 45.0 / MH  # (two decimals are printed)
    assert r.stderr.count("no sun stands out") == 1
    names = [f"frame_0000_{f:03d}.png" for f in range(2)]
    assert sorted(os.listdir(tmp_path / "sunny")) == sorted(names + [f"shadow_0000_{f:03d}.png" for f in range(2)])
    frames = [np.asarray(Image.open(str(tmp_path / "sunny" / n))) for n in names]
    shadows = [np.asarray(Image.open(str(tmp_path / "sunny" / f"shadow_0000_{f:03d}.png"))) for f in range(2)]
    assert all(f.shape == (Hc, Wc, 3) and f.dtype == np.uint8 for f in frames) and all(s.shape == (Hc, Wc) for s in shadows)
    assert not np.array_equal(frames[0], frames[1])  # the sun turned with its sky
    assert sorted(os.listdir(tmp_path / "flagged")) == sorted(names) == sorted(os.listdir(tmp_path / "plain"))
    for n in names:
        assert (tmp_path / "flagged" / n).read_bytes() == (tmp_path / "plain" / n).read_bytes(), n
