"""`depth_of_field=` through the frame render (a sky frame, one sun, a sun sweep, a daylight sweep, one sun with marched shadows, a lamp, fog
with shafts) on a 9 x 13 pinhole bundle: with nothing marked every output keeps its bits; with every pixel marked the frame is the
brute-force average of the renders of the lens bundles; under a lens that blurs a part of the frame the mask is the restatement's on the
frame's own first pass, unmarked pixels keep their bits and marked ones are the brute-force average; the focus pixel is read on the device;
with `antialias=` as well the two masks are disjoint and each set is its own average; graph and eager frames agree; no new chunk graph
appears; and the `python -m neusky_amd.relight` command line with and without the depth-of-field flags."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import antialias_cpu as A
import dof_cpu as L
from util_frames import frame_scene
from util_step import randomise
from neusky_amd.cameras.rays import RayBundle
from neusky_amd.relight import (Antialias, Atmosphere, CameraPath, DaylightSky, DepthOfField, DisplayTransform, PointLight, camera_rays, lens_rays,
                                subpixel_rays)
from neusky_amd.relight.antialias import RESOLVED_KEYS
from neusky_amd.relight.sun import SunLight, sun_path

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, CHUNK = 9, 13, 64  # 117 rays: one whole chunk and a padded one; 351 second-pass rays under every_pixel: five chunks and a padded one
P = H * W
BAR = 2e-6  # the project's chunk-independence bar (test_gpu_render_frame.py): times max(1, max |value|) of the output
SUN = SunLight(130.0, 35.0, (40.0, 34.0, 24.0))
SKY = DaylightSky(turbidity=3.0, exposure=0.1)
LAMP = PointLight((0.3, 0.6, 0.2), (1.0, 0.8, 0.6))
FOG = Atmosphere(1.5, scale_height=0.3, base_height=-0.2, albedo=(0.9, 0.8, 1.0), anisotropy=0.6, shaft_samples=4)
CASES = ("sky", "one sun", "sun sweep", "daylight sweep", "sdf shadows", "lamp", "fog shafts")
CENTRE = ("depth", "normal", "p2p_dist")
EVERY = dict(aperture=0.02, focus_distance=0.5, samples=4, every_pixel=True)
# The randomised model's depth is noise from pixel to pixel (0.11 to 0.80 over the frame, median 0.43; accumulation 0.04 to 0.92), so the
# circle of confusion is too.  With f_px = 8.64 a lens of radius 0.05 focused at depth 0.5 has c = 0.432 |1 / depth - 2|: 0.5 pixel at depth
# 0.32, 1.5 at 0.18; `covered` 0.1 leaves few pixels at infinity (c = 0.864).  With threshold 0.8 and reach 2 the restatement marks, on the
# first pass' G-buffer (the same in every case: the lights do not move the geometry), 84 of the 117 pixels, 72 %, c from 0.0024 to 3.0
PARTIAL = dict(aperture=0.05, focus_distance=0.5, samples=4, threshold=0.8, reach=2, covered=0.1)


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
        "lamp": {"lights": LAMP},
        "fog shafts": {"sun": SUN, "atmosphere": FOG},
    }
    makers = {name: (lambda bundle=rb, _kw=kw, **more: m.get_outputs_for_camera_ray_bundle(bundle, camera_index=1, chunk=CHUNK, **_kw, **more))
              for name, kw in lights.items()}
    return pipe, rb, makers, {}


def plain_frame(scene, name):
    _, _, makers, cache = scene
    if ("plain", name) not in cache:
        plain = makers[name](display=DisplayTransform())  # (display: a sky frame's `lin`, the same bits as the plain frame's other keys)
        cache["plain", name] = {k: v.clone() for k, v in plain.items() if not k.startswith("display_")}
    return cache["plain", name]


def average_of(scene, name, sub, S):
    """float64 {key: the average of the plain frame and of the frames rendered, through the public call, on each of the S - 1 bundles in the
    pixel-major `sub` of every pixel}"""
    _, _, makers, _ = scene
    plain = plain_frame(scene, name)
    total = {k: plain[k].double() for k in RESOLVED_KEYS if k in plain}
    for s in range(S - 1):
        pick = lambda t: t[s::S - 1].reshape(H, W, -1).contiguous()  # noqa: E731
        bundle = RayBundle(pick(sub.origins), pick(sub.directions), pick(sub.pixel_area), pick(sub.camera_indices),
                           metadata={"directions_norm": pick(sub.metadata["directions_norm"])})
        out = makers[name](bundle=bundle, display=DisplayTransform())
        for k in total:
            total[k] += out[k].double()
    return {k: v / S for k, v in total.items()}


def lens_average(scene, name, dof, focus=None):
    """the brute force of a lens: made once per case and lens"""
    _, rb, _, cache = scene
    key = ("lens", name, dof.aperture, dof.focus_distance, dof.samples, None if focus is None else float(focus))
    if key not in cache:
        cache[key] = average_of(scene, name, lens_rays(rb, torch.arange(P, device=DEV), dof, focus=focus), dof.samples)
    return cache[key]


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


def restated(plain, dof, rb):
    """(coc, mask, 1 / z_f) of the restatement on the plain frame's own G-buffer"""
    depth, acc = plain["depth"][..., 0].cpu().numpy(), plain["accumulation"][..., 0].cpu().numpy()
    d, n = rb.directions.cpu().numpy(), rb.metadata["directions_norm"].cpu().numpy()
    izf = np.float32(1.0 / dof.focus_distance) if dof.focus_distance is not None else L.focus_of(depth, acc, dof.focus_index(H, W), dof.covered)
    afpx = np.float32(L.lens_block(d, n, dof.aperture, 0.0)[11])
    c = L.coc(depth, acc, afpx, izf, dof.covered)
    return c, L.mark(c, dof.threshold, dof.reach), izf


@pytest.mark.parametrize("name", CASES)
def test_nothing_marked_keeps_every_bit(scene, name):
    _, rb, makers, _ = scene
    plain = {k: v.clone() for k, v in makers[name]().items()}
    extra = {"dof_coc", "dof_mask", "dof_fraction", "dof_focus"} | ({"lin"} if "lin" not in plain else set())
    # a lens of radius 0, and a threshold above every circle of confusion
    for dof in (DepthOfField(0.0), DepthOfField(0.0, threshold=0.0), DepthOfField(0.02, focus_distance=0.5, threshold=1e30)):
        out = makers[name](depth_of_field=dof)
        assert set(out) == set(plain) | extra and not extra & set(plain)
        for k, v in plain.items():
            assert out[k].dtype == v.dtype and out[k].shape == v.shape and torch.equal(out[k], v), k
        assert out["dof_fraction"] == 0 and isinstance(out["dof_fraction"], float)
        assert out["dof_mask"].dtype == torch.uint8 and tuple(out["dof_mask"].shape) == (H, W, 1) and not bool(out["dof_mask"].any())
        assert out["dof_coc"].dtype == torch.float32 and tuple(out["dof_coc"].shape) == (H, W, 1)
        assert tuple(out["dof_focus"].shape) == (1,)
        c, _, izf = restated(plain_frame(scene, name), dof, rb)
        assert np.array_equal(out["dof_coc"][..., 0].cpu().numpy().view(np.uint32), c.view(np.uint32))
        assert (c == 0).all() == (dof.aperture == 0.0) and float(out["dof_focus"]) == float(izf)
    again = makers[name]()  # and the plain frame after one with a lens
    assert set(again) == set(plain)
    for k, v in plain.items():
        assert torch.equal(again[k], v), k


@pytest.mark.parametrize("name", CASES)
def test_every_pixel_is_the_brute_force_average(scene, name):
    _, _, makers, _ = scene
    dof = DepthOfField(**EVERY)
    want, plain = lens_average(scene, name, dof), plain_frame(scene, name)
    assert ("shadow_map" in want) == (name not in ("sky", "lamp")) and "lin" in want and ("light_lin" in want) == (name == "lamp")
    out = makers[name](depth_of_field=dof)
    assert out["dof_fraction"] == 1.0 and bool(out["dof_mask"].all())
    assert_average(name, out, want)
    assert_rgb_follows_lin(out)
    status = [k for k in ("shadow_status", "shadow_difference", "light_status", "atmosphere_transmittance", "atmosphere_inscatter") if k in plain]
    for k in list(CENTRE) + status:
        assert torch.equal(out[k], plain[k]), k  # the centre ray's bits
    assert not torch.equal(out["lin"], plain["lin"])
    # three slices, the last one partial: the same bits as one slice
    sliced = makers[name](depth_of_field=DepthOfField(**EVERY, batch_pixels=50))
    assert set(sliced) == set(out)
    for k, v in out.items():
        assert torch.equal(sliced[k], v) if torch.is_tensor(v) else sliced[k] == v, k
    # eager: the same bits as the graph's
    eager = makers[name](depth_of_field=dof, use_graph=False)
    differ = [k for k, v in out.items() if torch.is_tensor(v) and not torch.equal(eager[k], v)]
    print(f"{name}: keys whose eager frame differs from the graph's: {differ or 'none'}")
    for k, v in out.items():
        assert torch.equal(eager[k], v) if torch.is_tensor(v) else eager[k] == v, k
    # and on the host
    host = makers[name](depth_of_field=dof, to_cpu=True)
    for k, v in out.items():
        if torch.is_tensor(v):
            assert host[k].device.type == "cpu" and torch.equal(host[k], v.cpu()), k


@pytest.mark.parametrize("name", CASES)
def test_a_lens_that_blurs_a_part_of_the_frame(scene, name):
    _, rb, makers, _ = scene
    dof = DepthOfField(**PARTIAL)
    want, plain = lens_average(scene, name, dof), plain_frame(scene, name)
    out = makers[name](depth_of_field=dof)
    c, mask, izf = restated(plain, dof, rb)
    share = float(mask.mean())
    print(f"{name}: the lens {PARTIAL} marks {mask.sum()} of {P} pixels ({share:.3f}); c from {np.nanmin(c):.3g} to {np.nanmax(c):.3g}")
    assert 0.2 <= share <= 0.8  # (so that neither half of this test is vacuous)
    assert np.array_equal(out["dof_coc"][..., 0].cpu().numpy().view(np.uint32), c.view(np.uint32))
    assert np.array_equal(out["dof_mask"][..., 0].cpu().numpy(), mask)
    assert out["dof_fraction"] == mask.sum() / P and float(out["dof_focus"]) == float(izf)
    marked = torch.from_numpy(mask.astype(bool)).to(DEV)
    for k, v in plain.items():  # unmarked pixels keep the plain frame's bits in every key
        assert torch.equal(out[k][..., ~marked, :], v[..., ~marked, :]), k
    assert_average(name, out, want, marked, " (marked pixels)")
    assert_rgb_follows_lin(out, marked)
    for k in CENTRE:
        assert torch.equal(out[k], plain[k]), k
    sliced = makers[name](depth_of_field=DepthOfField(**PARTIAL, batch_pixels=50))
    for k, v in out.items():
        assert torch.equal(sliced[k], v) if torch.is_tensor(v) else sliced[k] == v, k


def test_the_focus_pixel_is_read_from_the_first_pass(scene):
    _, rb, makers, _ = scene
    plain = plain_frame(scene, "one sun")
    depth, acc = plain["depth"].view(-1), plain["accumulation"].view(-1)
    covered = [int(p) for p in torch.nonzero((acc > 0.5) & (depth > 0)).view(-1)[:3]]
    assert covered
    bare = [int(p) for p in torch.nonzero(~((acc > 0.5) & (depth > 0))).view(-1)[:1]]  # (an uncovered pixel, if the frame has one)
    for p in covered + bare:
        y, x = divmod(p, W)
        dof = DepthOfField(0.02, focus_pixel=(x, y), samples=4, every_pixel=True)
        out = makers["one sun"](depth_of_field=dof)
        want = L.focus_of(depth.cpu().numpy(), acc.cpu().numpy(), p)
        assert out["dof_focus"].cpu().numpy().view(np.uint32)[0] == np.asarray(want, np.float32).view(np.uint32)
        if p == covered[0]:
            assert float(want) > 0 and float(out["dof_coc"].view(-1)[p]) == 0.0  # in focus
            assert_average("one sun", out, lens_average(scene, "one sun", dof, focus=out["dof_focus"]), what=f" (focus pixel {x}, {y})")
    # the default is the centre pixel
    centre = makers["one sun"](depth_of_field=DepthOfField(0.02))
    assert float(centre["dof_focus"]) == float(L.focus_of(depth.cpu().numpy(), acc.cpu().numpy(), (H // 2) * W + W // 2))
    # covered above every accumulation: focus at infinity
    far = makers["one sun"](depth_of_field=DepthOfField(0.02, focus_pixel=(covered[0] % W, covered[0] // W), covered=1e30))
    assert float(far["dof_focus"]) == 0.0 and not bool(far["dof_coc"].any())


@pytest.mark.parametrize("name", ("sky", "one sun"))
def test_with_antialiasing_the_masks_are_disjoint(scene, name):
    _, rb, makers, _ = scene
    plain = plain_frame(scene, name)
    dof, aa = DepthOfField(**PARTIAL), Antialias(samples=4, every_pixel=True)
    out = makers[name](depth_of_field=dof, antialias=aa)
    _, mask, _ = restated(plain, dof, rb)
    lens, edge = out["dof_mask"][..., 0].bool(), out["aa_mask"][..., 0].bool()
    assert np.array_equal(lens.cpu().numpy(), mask.astype(bool))
    assert not bool((lens & edge).any()) and bool((lens | edge).all())  # every_pixel: the antialiasing pass takes exactly the rest
    assert out["aa_fraction"] == float(edge.sum()) / P and out["dof_fraction"] == float(lens.sum()) / P
    assert_average(name, out, lens_average(scene, name, dof), lens, " (lens pixels)")
    sub = subpixel_rays(rb, torch.arange(P, device=DEV), aa.sample_offsets(DEV))
    assert_average(name, out, average_of(scene, name, sub, 4), edge, " (edge pixels)")
    assert_rgb_follows_lin(out)
    # an edge rule that marks a part: the three sets, and the untouched one keeps its bits
    rule = Antialias(samples=4, colour=0.7, depth=1.0, accumulation=0.45, normal_deg=80.0)
    both = makers[name](depth_of_field=dof, antialias=rule)
    alone = makers[name](antialias=rule)["aa_mask"][..., 0].bool()  # the edges of the first pass
    lens, edge = both["dof_mask"][..., 0].bool(), both["aa_mask"][..., 0].bool()
    assert torch.equal(edge, alone & ~lens) and bool(edge.any()) and bool((~edge & ~lens).any())
    untouched = ~edge & ~lens
    for k, v in plain.items():
        assert torch.equal(both[k][..., untouched, :], v[..., untouched, :]), k
    assert_average(name, both, lens_average(scene, name, dof), lens, " (lens pixels, with an edge rule)")
    assert_average(name, both, average_of(scene, name, sub, 4), edge, " (edge pixels, with an edge rule)")


@pytest.mark.parametrize("name", ("sky", "sun sweep"))
def test_display_sees_the_resolved_frame(scene, name):
    _, _, makers, _ = scene
    dof = DepthOfField(**EVERY)
    out = makers[name](depth_of_field=dof, display=DisplayTransform())
    alone = makers[name](depth_of_field=dof)
    assert torch.equal(out["lin"], alone["lin"])
    assert torch.equal(out["display_rgb8"], torch.round(out["display_rgb"] * 255).to(torch.uint8))
    assert not torch.equal(out["display_rgb"], makers[name](display=DisplayTransform())["display_rgb"])


@pytest.mark.parametrize("name", CASES)
def test_no_new_chunk_graph_and_parameters_reuse_the_runners(scene, name):
    pipe, _, makers, _ = scene
    runners = pipe.model.frames.runners
    runners.clear()
    makers[name](display=DisplayTransform())
    shown = set(runners)
    first = makers[name](depth_of_field=DepthOfField(**EVERY))
    assert pipe.model.frames.runners is runners and set(runners) == shown  # no key beyond those of display= alone
    before = dict(runners)
    for kw in ({"aperture": 0.05}, {"aperture": 0.02, "focus_distance": 0.9}, {"aperture": 0.02, "focus_pixel": (3, 4)},
               {"aperture": 0.02, "samples": 7}, {"aperture": 0.02, "threshold": 0.1, "reach": 3}, {"aperture": 0.02, "rotate": False},
               {"aperture": 0.02, "batch_pixels": 17, "every_pixel": True, "samples": 2}):
        other = makers[name](depth_of_field=DepthOfField(**kw), display=DisplayTransform())
        assert pipe.model.frames.runners is runners and runners.keys() == before.keys(), kw
        assert all(runners[k] is r for k, r in before.items()), kw
        assert torch.equal(other["depth"], first["depth"])
    assert pipe.model.frames.active is None


def test_errors(scene):
    pipe, rb, makers, _ = scene
    from neusky_amd.relight import FrameLighting
    with pytest.raises(ValueError, match="bake"):
        pipe.model.frames.render(rb, FrameLighting.of(bake="fp32"), depth_of_field=DepthOfField(0.02))
    flat = rb.slice(0, 1 << 62)
    with pytest.raises(ValueError, match=r"\[H, W\]"):
        pipe.model.get_outputs_for_camera_ray_bundle(flat, camera_index=1, chunk=CHUNK, depth_of_field=DepthOfField(0.02))
    with pytest.raises(ValueError, match="DepthOfField"):
        makers["sky"](depth_of_field=0.02)
    with pytest.raises(ValueError, match="outside the frame"):
        makers["sky"](depth_of_field=DepthOfField(0.02, focus_pixel=(W, 0)))
    with pytest.raises(ValueError, match="exclude"):
        DepthOfField(0.02, focus_distance=0.5, focus_pixel=(1, 1))
    bent = RayBundle(rb.origins, rb.directions.clone(), rb.pixel_area, rb.camera_indices, metadata=dict(rb.metadata))
    bent.directions[H - 1, W - 1, 1] += 0.05  # one corner: not a pinhole's bundle
    with pytest.raises(ValueError, match="pinhole"):
        makers["sky"](bundle=bent, depth_of_field=DepthOfField(0.02))
    assert pipe.model.frames.active is None
    makers["sky"](depth_of_field=DepthOfField(0.02))  # and the renderer goes on


# ------------------------------------------------------------------------------------------ the command line
def test_cli_with_and_without_the_depth_of_field_flags(tmp_path, capsys):
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
        main(base + ["--output-dir", str(tmp_path / "refused"), "--dof-aperture", "0.02", "--transfer", "fp32"])
    message = capsys.readouterr().err
    assert refused.value.code not in (0, None) and "--dof-aperture" in message and "--transfer" in message
    with pytest.raises(SystemExit):
        main(base + ["--output-dir", str(tmp_path / "refused"), "--dof-all"])
    assert "--dof-all needs --dof-aperture" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        main(base + ["--output-dir", str(tmp_path / "refused"), "--dof-aperture", "0.02", "--dof-focus-pixel", str(Wc), "0"])
    assert "outside the frame" in capsys.readouterr().err
    assert not (tmp_path / "refused").exists()
    lens = ["--dof-aperture", "0.02", "--dof-focus-distance", "0.5", "--dof-samples", "8", "--dof-reach", "4", "--dof-map"]
    runs = [base + ["--output-dir", str(tmp_path / "plain")] + sun,
            base + ["--output-dir", str(tmp_path / "zero"), "--dof-aperture", "0"] + sun,
            base + ["--output-dir", str(tmp_path / "lens")] + lens + sun,
            base + ["--output-dir", str(tmp_path / "all"), "--dof-aperture", "0.02", "--dof-samples", "4", "--dof-all", "--save-linear"]]
    script = "import sys, json\nfrom neusky_amd.relight.__main__ import main\nfor argv in json.loads(sys.argv[1]):\n    assert main(argv) == 0\n"
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-c", script, json.dumps(runs)], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    closing = [line for line in r.stdout.splitlines() if line.startswith("depth of field:")]
    assert len(closing) == 3 and "16 samples" in closing[0] and "8 samples" in closing[1] and "4 samples through every pixel" in closing[2], r.stdout

    def pair(line, after):
        """the numbers behind `smallest` and `largest`, behind the word `after`"""
        words = line.split()
        start = words.index(after)
        return tuple(float(words[words.index(w, start) + 1]) for w in ("smallest", "largest"))

    assert pair(closing[1], "focus") == (0.5, 0.5)
    assert pair(closing[0], "share") == (0.0, 0.0) and pair(closing[2], "share") == (1.0, 1.0)
    # a lens of radius 0: every file is, byte for byte, what a run without the flag writes
    assert sorted(os.listdir(tmp_path / "plain")) == ["frame_0000_000.png"] == sorted(os.listdir(tmp_path / "zero"))
    assert (tmp_path / "plain" / "frame_0000_000.png").read_bytes() == (tmp_path / "zero" / "frame_0000_000.png").read_bytes()
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
    assert sorted(os.listdir(tmp_path / "lens")) == ["coc_0000_000.png", "frame_0000_000.png"]
    lit = frame(sun=SUN, depth_of_field=DepthOfField(0.02, focus_distance=0.5, samples=8, reach=4))
    png = np.asarray(Image.open(str(tmp_path / "lens" / "frame_0000_000.png")))
    assert np.array_equal(png, np.round(lit["rgb"].clamp(0.0, 1.0).cpu().numpy() * 255.0).astype(np.uint8))
    assert not np.array_equal(png, np.asarray(Image.open(str(tmp_path / "plain" / "frame_0000_000.png"))))
    grey = np.asarray(Image.open(str(tmp_path / "lens" / "coc_0000_000.png")))
    assert grey.dtype == np.uint8 and grey.shape == (Hc, Wc)
    want = torch.round((lit["dof_coc"][..., 0] / 4).clamp(0.0, 1.0).nan_to_num(0.0) * 255.0).to(torch.uint8).cpu().numpy()
    assert np.array_equal(grey, want) and grey.max() > 0
    assert pair(closing[1], "share")[0] == pytest.approx(lit["dof_fraction"], rel=1e-3)
    # every pixel: the linear image is the Python call's
    assert sorted(os.listdir(tmp_path / "all")) == ["frame_0000_000.lin.npy", "frame_0000_000.png"]
    out = frame(depth_of_field=DepthOfField(0.02, samples=4, every_pixel=True))
    lin = np.load(tmp_path / "all" / "frame_0000_000.lin.npy")
    assert lin.dtype == np.float32 and np.array_equal(lin, out["lin"].cpu().numpy())
