"""`antialias=` through the frame render (a sky frame, one sun, a sun sweep, a daylight sweep, one sun with marched shadows) on a 9 x 13
pinhole bundle: with nothing marked every output keeps its bits; with every pixel marked the frame is the brute-force average of the
renders of the sub-pixel bundles; under an edge rule that marks a part of the frame the mask is the restatement's on the frame's own
first pass, unmarked pixels keep their bits and marked ones are the brute-force average; `display=` sees the resolved frame; no new chunk graph appears; and the
`python -m neusky_amd.relight` command line with and without the antialiasing flags."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import antialias_cpu as A
import display_cpu as D
from util_frames import frame_scene
from util_step import randomise
from neusky_amd.cameras.rays import RayBundle
from neusky_amd.relight import Antialias, CameraPath, DaylightSky, DisplayTransform, camera_rays, subpixel_rays
from neusky_amd.relight.sun import SunLight, sun_path

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, CHUNK = 9, 13, 64  # 117 rays: one whole chunk and a padded one; 351 second-pass rays under every_pixel: five chunks and a padded one
P = H * W
BAR = 2e-6  # the project's chunk-independence bar (test_gpu_render_frame.py): times max(1, max |value|) of the output
SUN = SunLight(130.0, 35.0, (40.0, 34.0, 24.0))
SKY = DaylightSky(turbidity=3.0, exposure=0.1)
CASES = ("sky", "one sun", "sun sweep", "daylight sweep", "sdf shadows")
RESOLVED = ("lin", "albedo", "accumulation", "shadow_map")
CENTRE = ("depth", "normal", "p2p_dist")
# thresholds so high that nothing is marked.  The randomised model's rendered normals lie up to 122 degrees apart between neighbours, and
# an angle of 90 degrees or more is marked under every normal_deg (d <= 0): `covered` above every accumulation switches the two tests
# between covered pixels off as well
NOTHING = dict(colour=1e30, depth=1e30, accumulation=1e30, normal_deg=89.9, covered=1e30)
# the randomised model is noise from pixel to pixel (median differences between neighbours: 0.2 of accumulation, 0.25 of depth, 40 degrees,
# 0.2 to 0.4 of luminance): the default thresholds mark 99 to 100 % of the 117 pixels in every case.  These mark 33 % (sky), 50 % (one
# sun), 73 % (sun sweep), 42 % (daylight sweep) and 55 % (marched shadows), by the restatement on the first pass' G-buffers
RULE = dict(colour=0.7, depth=1.0, accumulation=0.45, normal_deg=80.0)


@pytest.fixture(scope="module")
def scene():
    pipe, _ = frame_scene(H, W, DEV)
    m = pipe.model
    c2w = torch.from_numpy(A.look_at()).float()
    rb = camera_rays(CameraPath(W, H, c2w[None], torch.tensor([55.0])), 0, DEV, camera_index=1)
    lights = {
        "sky": {},
        "one sun": {"sun": SUN},
        "sun sweep": {"sun": sun_path(100.0, 8.0, 190.0, 62.0, 3, (40.0, 34.0, 24.0))},
        "daylight sweep": {"daylight": SKY, "sun": SKY.sun_path(100.0, 8.0, 190.0, 62.0, 3)},
        "sdf shadows": {"sun": SUN, "sun_shadows": "sdf"},
    }
    makers = {name: (lambda bundle=rb, _kw=kw, **more: m.get_outputs_for_camera_ray_bundle(bundle, camera_index=1, chunk=CHUNK, **_kw, **more))
              for name, kw in lights.items()}
    return pipe, rb, makers, {}


def brute_force(scene, name):
    """float64 {key: the average of the plain frame and of the frames rendered, through the public call, on each of the 3 bundles
    subpixel_rays returns for every pixel}, and the plain frame; made once per case"""
    _, rb, makers, cache = scene
    if name not in cache:
        plain = makers[name](display=DisplayTransform())  # (display: a sky frame's `lin`, the same bits as the plain frame's other keys)
        plain = {k: v.clone() for k, v in plain.items() if not k.startswith("display_")}
        offsets = Antialias(samples=4).sample_offsets(DEV)
        sub = subpixel_rays(rb, torch.arange(P, device=DEV), offsets)
        total = {k: plain[k].double() for k in RESOLVED if k in plain}
        for s in range(3):
            pick = lambda t: t[s::3].reshape(H, W, -1).contiguous()  # noqa: E731
            bundle = RayBundle(pick(sub.origins), pick(sub.directions), pick(sub.pixel_area), pick(sub.camera_indices),
                               metadata={"directions_norm": pick(sub.metadata["directions_norm"])})
            out = makers[name](bundle=bundle, display=DisplayTransform())
            for k in total:
                total[k] += out[k].double()
        cache[name] = ({k: v / 4.0 for k, v in total.items()}, plain)
    return cache[name]


def assert_average(name, got, want, where=None, what=""):
    """the resolved outputs against the brute force, at the pixels `where` [H, W] (all by default)"""
    for k, ref in want.items():
        g, r = got[k].double(), ref
        if where is not None:
            g, r = g[..., where, :], r[..., where, :]
        worst, scale = float((g - r).abs().max()), max(1.0, float(r.abs().max()))
        print(f"{name}{what}: {k} worst difference from the brute force {worst:.2e} (values up to {scale:.3g}, bar {BAR * scale:.2e})")
        assert worst <= BAR * scale, (k, worst, scale)


def assert_rgb_follows_lin(out, where=None):
    lin, rgb = out["lin"].cpu().numpy(), out["rgb"].double().cpu().numpy()
    err = np.abs(rgb - A.srgb(lin))
    assert (err if where is None else err[..., where.cpu().numpy(), :]).max() <= 1e-6


@pytest.mark.parametrize("name", CASES)
def test_nothing_marked_keeps_every_bit(scene, name):
    _, _, makers, _ = scene
    plain = {k: v.clone() for k, v in makers[name]().items()}
    out = makers[name](antialias=Antialias(**NOTHING))
    extra = {"aa_mask", "aa_fraction"} | ({"lin"} if name == "sky" else set())
    assert set(out) == set(plain) | extra and not extra & set(plain)
    for k, v in plain.items():
        assert out[k].dtype == v.dtype and out[k].shape == v.shape and torch.equal(out[k], v), k
    assert out["aa_fraction"] == 0 and isinstance(out["aa_fraction"], float)
    assert out["aa_mask"].dtype == torch.uint8 and tuple(out["aa_mask"].shape) == (H, W, 1) and not bool(out["aa_mask"].any())
    again = makers[name]()  # and the plain frame after an antialiased one
    assert set(again) == set(plain)
    for k, v in plain.items():
        assert torch.equal(again[k], v), k


@pytest.mark.parametrize("name", CASES)
def test_every_pixel_is_the_brute_force_average(scene, name):
    _, _, makers, _ = scene
    want, plain = brute_force(scene, name)
    assert ("shadow_map" in want) == (name != "sky") and "lin" in want
    out = makers[name](antialias=Antialias(samples=4, every_pixel=True))
    assert out["aa_fraction"] == 1.0 and bool(out["aa_mask"].all())
    assert_average(name, out, want)
    assert_rgb_follows_lin(out)
    for k in CENTRE + (("shadow_status",) if name == "sdf shadows" else ()) + (("shadow_difference",) if name != "sky" else ()):
        assert torch.equal(out[k], plain[k]), k  # the centre ray's bits
    assert not torch.equal(out["lin"], plain["lin"])
    # three slices, the last one partial: the same bits as one slice
    sliced = makers[name](antialias=Antialias(samples=4, every_pixel=True, batch_pixels=50))
    assert set(sliced) == set(out)
    for k, v in out.items():
        assert torch.equal(sliced[k], v) if torch.is_tensor(v) else sliced[k] == v, k
    # and on the host
    host = makers[name](antialias=Antialias(samples=4, every_pixel=True), to_cpu=True)
    for k, v in out.items():
        if torch.is_tensor(v):
            assert host[k].device.type == "cpu" and torch.equal(host[k], v.cpu()), k


@pytest.mark.parametrize("name", CASES)
def test_edge_rule_on_the_frames_own_first_pass(scene, name):
    _, _, makers, _ = scene
    want, plain = brute_force(scene, name)
    rule = RULE
    out = makers[name](antialias=Antialias(samples=4, **rule))
    names = {"depth": "depth_t"}
    mask = A.edge_mask(plain["depth"][..., 0].cpu().numpy(), plain["normal"].cpu().numpy(), plain["accumulation"][..., 0].cpu().numpy(),
                       plain["lin"].reshape(-1, H, W, 3).cpu().numpy(), **{names.get(k, k): v for k, v in rule.items()})
    share = float(mask.mean())
    print(f"{name}: the rule {rule} marks {mask.sum()} of {P} pixels ({share:.3f})")
    assert 0.05 <= share <= 0.95  # (so that neither half of this test is vacuous)
    assert np.array_equal(out["aa_mask"][..., 0].cpu().numpy(), mask)
    assert out["aa_fraction"] == mask.sum() / P
    marked = torch.from_numpy(mask.astype(bool)).to(DEV)
    for k, v in plain.items():  # unmarked pixels keep the plain frame's bits in every key
        assert torch.equal(out[k][..., ~marked, :], v[..., ~marked, :]), k
    assert_average(name, out, want, marked, " (marked pixels)")
    assert_rgb_follows_lin(out, marked)
    for k in CENTRE:
        assert torch.equal(out[k], plain[k]), k


@pytest.mark.parametrize("name", ("sky", "sun sweep"))
def test_display_sees_the_resolved_frame(scene, name):
    _, _, makers, _ = scene
    t = DisplayTransform(curve="aces", exposure="frame", key=0.25, ev=0.5, percentiles=(0.1, 0.9), meter_mask_threshold=0.5)
    out = makers[name](antialias=Antialias(samples=4, every_pixel=True), display=t)
    plain = makers[name](display=t)
    lin, acc = out["lin"].reshape(-1, H, W, 3).cpu().numpy(), out["accumulation"].reshape(H, W).cpu().numpy()
    K = lin.shape[0]
    want = np.array([D.exposure(D.histogram(lin[k], acc, 0.5), 0.25, 0.5, (0.1, 0.9)) for k in range(K)])
    got = out["display_exposure"].cpu().numpy().astype(np.float64)
    assert got.shape == (K,) and np.abs(got / want - 1.0).max() <= 2.0 ** -22, (got, want)
    ref = D.display_map(lin, out["display_exposure"].cpu().numpy().reshape(K, 1, 1, 1), "aces")
    assert np.abs(out["display_rgb"].reshape(-1, H, W, 3).cpu().numpy() - ref).max() <= 1e-4
    assert torch.equal(out["display_rgb8"], torch.round(out["display_rgb"] * 255).to(torch.uint8))
    assert out["display_rgb"].shape == out["rgb"].shape and not torch.equal(out["display_rgb"], plain["display_rgb"])


@pytest.mark.parametrize("name", CASES)
def test_no_new_chunk_graph_and_parameters_reuse_the_runners(scene, name):
    pipe, _, makers, _ = scene
    runners = pipe.model.frames.runners
    runners.clear()
    makers[name](display=DisplayTransform())
    shown = set(runners)
    first = makers[name](antialias=Antialias(samples=4, every_pixel=True))
    assert pipe.model.frames.runners is runners and set(runners) == shown  # no key beyond those of display= alone
    before = dict(runners)
    for kw in ({"samples": 7}, {"colour": 0.3}, {"depth": 0.1}, {"normal_deg": 40.0}, {"accumulation": 0.3}, {"covered": 0.1},
               {"batch_pixels": 17}, {"every_pixel": True, "samples": 2}):
        other = makers[name](antialias=Antialias(**kw), display=DisplayTransform())
        assert pipe.model.frames.runners is runners and runners.keys() == before.keys(), kw
        assert all(runners[k] is r for k, r in before.items()), kw
        assert torch.equal(other["depth"], first["depth"])
    assert pipe.model.frames.active is None


def test_errors(scene):
    pipe, rb, makers, _ = scene
    from neusky_amd.relight import FrameLighting
    with pytest.raises(ValueError, match="bake"):
        pipe.model.frames.render(rb, FrameLighting.of(bake="fp32"), antialias=Antialias())
    flat = rb.slice(0, 1 << 62)
    with pytest.raises(ValueError, match=r"\[H, W\]"):
        pipe.model.get_outputs_for_camera_ray_bundle(flat, camera_index=1, chunk=CHUNK, antialias=Antialias())
    with pytest.raises(ValueError, match="Antialias"):
        makers["sky"](antialias=4)
    assert pipe.model.frames.active is None


# ------------------------------------------------------------------------------------------ the command line
def test_cli_with_and_without_the_antialias_flags(tmp_path, capsys):
    from PIL import Image

    from neusky_amd.configs.neusky_config import synthetic_pipeline_config
    from neusky_amd.data.synthetic_datamanager import SyntheticDataManagerConfig
    from neusky_amd.relight import load_camera_path
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
    base = ["--checkpoint", str(ckpt), "--camera-path", str(path_file), "--latent-index", "1"]
    sun = ["--sun-azimuth", "130", "--sun-elevation", "35", "--sun-colour", "40", "34", "24"]
    # refused while the arguments are read, before anything touches the device
    with pytest.raises(SystemExit) as refused:
        main(base + ["--output-dir", str(tmp_path / "refused"), "--antialias", "4", "--transfer", "fp32"])
    message = capsys.readouterr().err
    assert refused.value.code not in (0, None) and "--antialias" in message and "--transfer" in message
    with pytest.raises(SystemExit):
        main(base + ["--output-dir", str(tmp_path / "refused"), "--aa-all"])
    assert "--aa-all needs --antialias" in capsys.readouterr().err
    assert not (tmp_path / "refused").exists()
    runs = [base + ["--output-dir", str(tmp_path / "plain")],
            base + ["--output-dir", str(tmp_path / "all"), "--antialias", "4", "--aa-all", "--save-linear"],
            base + ["--output-dir", str(tmp_path / "masked"), "--antialias", "4", "--aa-mask"] + sun]
    script = "import sys, json\nfrom neusky_amd.relight.__main__ import main\nfor argv in json.loads(sys.argv[1]):\n    assert main(argv) == 0\n"
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-c", script, json.dumps(runs)], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    closing = [line for line in r.stdout.splitlines() if line.startswith("antialias:")]
    assert len(closing) == 2 and all("4 samples" in line for line in closing), r.stdout
    share = lambda line: tuple(float(line.split()[line.split().index(w) + 1]) for w in ("smallest", "largest"))  # noqa: E731
    assert share(closing[0]) == (1.0, 1.0)
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
    frame = lambda **kw: model.get_outputs_for_camera_ray_bundle(rb, camera_index=0, chunk=4096, **kw)  # noqa: E731
    # no flag: the parent's files, byte for byte: the parent's host code on the plain frame
    assert sorted(os.listdir(tmp_path / "plain")) == ["frame_0000_000.png"]
    rgb = frame()["rgb"].clamp(0.0, 1.0).cpu().numpy()
    Image.fromarray(np.round(rgb * 255.0).astype(np.uint8)).save(str(tmp_path / "parent.png"))
    assert (tmp_path / "plain" / "frame_0000_000.png").read_bytes() == (tmp_path / "parent.png").read_bytes()
    # every pixel: the linear image is the Python call's, and the PNG its rgb
    assert sorted(os.listdir(tmp_path / "all")) == ["frame_0000_000.lin.npy", "frame_0000_000.png"]
    out = frame(antialias=Antialias(samples=4, every_pixel=True))
    lin = np.load(tmp_path / "all" / "frame_0000_000.lin.npy")
    assert lin.dtype == np.float32 and np.array_equal(lin, out["lin"].cpu().numpy())
    png = np.asarray(Image.open(str(tmp_path / "all" / "frame_0000_000.png")))
    assert np.array_equal(png, np.round(out["rgb"].clamp(0.0, 1.0).cpu().numpy() * 255.0).astype(np.uint8)) and not np.array_equal(png, np.round(rgb * 255.0))
    # the mask of a sun frame
    assert sorted(os.listdir(tmp_path / "masked")) == ["aa_0000_000.png", "frame_0000_000.png"]
    lit = frame(sun=SUN, antialias=Antialias(samples=4))
    grey = np.asarray(Image.open(str(tmp_path / "masked" / "aa_0000_000.png")))
    assert grey.dtype == np.uint8 and grey.shape == (Hc, Wc) and set(np.unique(grey)) <= {0, 255}
    assert np.array_equal(grey, lit["aa_mask"][..., 0].cpu().numpy() * np.uint8(255))
    assert share(closing[1])[0] == pytest.approx(lit["aa_fraction"], rel=1e-3) and share(closing[1])[0] == share(closing[1])[1]
    png = np.asarray(Image.open(str(tmp_path / "masked" / "frame_0000_000.png")))
    assert np.array_equal(png, np.round(lit["rgb"].clamp(0.0, 1.0).cpu().numpy() * 255.0).astype(np.uint8))
