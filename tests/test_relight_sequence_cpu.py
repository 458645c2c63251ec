"""The run of python -m neusky_amd.relight (relight/sequence.py) without a device: the frame plan of each kind of camera, the files the
writer makes of a frame record when there is no display transform, and the closing lines of a tally filled by hand.  The lamps' picture
goes through DisplayTransform.apply, which is HIP kernels even for the default transform, so the writer's test here runs without
--light-map and `light_lin`: the run `lamp` of tests/test_gpu_relight_sequence_cli.py checks lights_*.png without a display transform."""
import math
import os

import numpy as np
import torch

from neusky_amd.relight import Antialias, DisplayTransform, PointLight, srgb_to_linear
from neusky_amd.relight.__main__ import build_parser, parse_lights, parse_suns
from neusky_amd.relight.sequence import Frame, FrameWriter, Shot, Tally, frame_plan
from neusky_amd.relight.transfer import LIGHTS_PER_PASS

BASE = ["--checkpoint", "c.ckpt", "--camera-path", "p.json", "--latent-index", "0"]
LAMP = ["--light", "0.3", "-0.2", "0.4", "1.5", "1.2", "0.9"]


def _plan(*flags):
    """the plan main() makes of a command line, and its parsed lamp path"""
    ap = build_parser()
    args = ap.parse_args(BASE + ["--output-dir", "o"] + list(flags))
    suns = parse_suns(ap, args)
    path = parse_lights(ap, args)[3]
    return frame_plan(args.turntable, args.rotation_deg, suns, args.sun_path is not None, path, args.transfer), path


def _covers(shots, frames):
    return [f for shot in shots for f in shot.frames] == list(range(frames))


def test_plan_of_a_turntable():
    shots, _ = _plan("--turntable", "3")
    assert [s.angles for s in shots] == [(None,), (2.0 * math.pi / 3,), (2.0 * math.pi * 2 / 3,)] and _covers(shots, 3)
    assert all(len(s.frames) == 1 and s.lamp is None and not s.sweep for s in shots)
    shots, _ = _plan("--rotation-deg", "30")
    assert shots == [Shot(range(0, 1), (math.radians(30.0),))]


def test_plan_of_a_sun_path():
    shots, _ = _plan("--sun-path", "120", "30", "240", "30", "--sun-steps", "4")
    assert shots == [Shot(range(0, 4), (None,), None, True)] and _covers(shots, 4)


def test_plan_of_a_moving_lamp():
    a, b = (0.3, -0.2, 0.4), (-0.3, 0.3, 0.2)
    shots, path = _plan("--sun-path", "120", "30", "240", "30", "--sun-steps", "1", "--rotation-deg", "30", *LAMP,
                        "--light-path", *map(str, a + b), "--light-steps", "3")
    assert _covers(shots, 3) and all(len(s.frames) == 1 and not s.sweep and s.angles == (math.radians(30.0),) for s in shots)  # (one sun: no sweep)
    want = [tuple(a[i] + (b[i] - a[i]) * t for i in range(3)) for t in (0.0, 0.5, 1.0)]
    assert [s.lamp for s in shots] == want and shots[0].lamp == a and shots[2].lamp == b
    shots, _ = _plan(*LAMP, "--light-path", *map(str, a + b), "--light-steps", "1")
    assert shots == [Shot(range(0, 1), (None,), a)]


def test_plan_of_a_baked_transfer():
    F = LIGHTS_PER_PASS + 1
    shots, _ = _plan("--transfer", "fp16", "--turntable", str(F))
    assert [len(s.frames) for s in shots] == [LIGHTS_PER_PASS, 1] and _covers(shots, F)
    assert shots[0].angles == (None,) + tuple(2.0 * math.pi * f / F for f in range(1, LIGHTS_PER_PASS))
    assert shots[1].angles == (2.0 * math.pi * LIGHTS_PER_PASS / F,) and not any(s.sweep or s.lamp for s in shots)
    shots, _ = _plan("--transfer", "off", "--turntable", str(F))
    assert [len(s.frames) for s in shots] == [1] * F and _covers(shots, F)


def _writer(tmp_path, *flags):
    args = build_parser().parse_args(BASE + ["--output-dir", str(tmp_path)] + list(flags))
    tally = Tally()
    return FrameWriter(args, None, tally), tally


def test_writer_without_a_display_transform(tmp_path):
    from PIL import Image
    g = torch.Generator().manual_seed(3)
    rgb = torch.rand(2, 3, 3, generator=g).numpy()
    rgb[0, 0], rgb[1, 2] = 0.0, 1.0
    shadow = torch.tensor([[-0.5, 0.0, 0.25], [0.5, 1.0, 1.5]]).view(2, 3, 1)
    marks = torch.tensor([[0, 1, 0], [1, 1, 0]], dtype=torch.uint8).view(2, 3, 1)
    writer, tally = _writer(tmp_path, "--save-hdr", "--shadow-map", "--aa-mask")
    writer.write(Frame(2, 5, rgb=rgb, shadow=shadow, aa_mask=marks))
    writer.end_camera()
    assert sorted(os.listdir(tmp_path)) == ["aa_0002_005.png", "frame_0002_005.npy", "frame_0002_005.png", "shadow_0002_005.png"]
    assert tally.frames == 1
    frame = Image.open(tmp_path / "frame_0002_005.png")
    assert frame.mode == "RGB" and np.array_equal(np.asarray(frame), np.round(rgb * 255.0).astype(np.uint8))
    hdr = np.load(tmp_path / "frame_0002_005.npy")
    assert hdr.dtype == np.float32 and np.array_equal(hdr, srgb_to_linear(rgb).astype(np.float32))
    grey = Image.open(tmp_path / "shadow_0002_005.png")
    assert grey.mode == "L" and np.asarray(grey).tolist() == [[0, 0, 64], [128, 255, 255]]  # round(clamp(shadow) * 255); 63.75 -> 64, 127.5 -> 128
    mask = Image.open(tmp_path / "aa_0002_005.png")
    assert mask.mode == "L" and np.asarray(mask).tolist() == [[0, 255, 0], [255, 255, 0]]


def test_writer_writes_only_what_the_frame_has(tmp_path):
    rgb = np.full((2, 3, 3), 0.5, np.float32)
    writer, tally = _writer(tmp_path, "--shadow-map", "--aa-mask", "--light-map")  # (--extract-sun that found nothing: no shadow; no lamps)
    writer.write(Frame(0, 0, rgb=rgb))
    writer.write(Frame(0, 1, rgb=rgb))
    assert sorted(os.listdir(tmp_path)) == ["frame_0000_000.png", "frame_0000_001.png"] and tally.frames == 2
    writer, _ = _writer(tmp_path / "plain")
    os.makedirs(tmp_path / "plain")
    writer.write(Frame(1, 0, rgb=rgb, shadow=torch.ones(2, 3, 1), aa_mask=torch.ones(2, 3, 1, dtype=torch.uint8), light_lin=torch.ones(2, 3, 3)))
    assert os.listdir(tmp_path / "plain") == ["frame_0001_000.png"]  # and nothing the command line did not ask for


def _report(capsys, tally, flags, **parsed):
    args = build_parser().parse_args(BASE + ["--output-dir", "o"] + flags)
    given = {"display": None, "antialias": None, "shadow_trace": None, "lights": None, "light_trace": None, **parsed}
    tally.report(args, (24, 16), **given)
    return capsys.readouterr().out.splitlines()


def test_tally_reports_every_closing_line(capsys):
    tally = Tally(t_load=1.5)
    tally.t_render, tally.frames = 2.0, 4
    tally.exposures = [torch.tensor([0.5]), torch.tensor([2.0, 1.25])]
    tally.marked = [0.25, 0.125]
    tally.shadow_rays, tally.exhausted = 1200, 3
    tally.light_rays, tally.light_exhausted = 768, 0
    lamps = (PointLight((0.0, 0.0, 1.0), (1.0, 1.0, 1.0)),) * 2
    lines = _report(capsys, tally, [], display=DisplayTransform(curve="aces", exposure="sequence"), antialias=Antialias(samples=4),
                    shadow_trace={"steps": 96}, lights=lamps, light_trace={"steps": 16})
    assert lines == [
        "o: 4 frames 24x16 | load 1.500s render 2.000s (0.500s/frame)",
        "display: tonemap aces | exposure metered per camera: smallest 0.5 largest 2",
        "antialias: 4 samples through the pixels its edge rule marks | share of marked pixels: smallest 0.125 largest 0.25",
        "sdf shadows: 3 of 1200 shadow rays (0.250%) were still marching after 96 steps (raise --shadow-steps if that is too many)",
        "lights: 2 lamps | 0 of 768 shadow rays (0.000%) were still marching after 16 steps (raise --light-shadow-steps if that is too many)"]
    lines = _report(capsys, tally, [], display=DisplayTransform(curve="hable", exposure="frame"), antialias=Antialias(samples=2, every_pixel=True),
                    lights=lamps[:1])
    assert lines[1:] == ["display: tonemap hable | exposure metered per frame: smallest 0.5 largest 2",
                         "antialias: 2 samples through every pixel | share of marked pixels: smallest 0.125 largest 0.25",
                         "lights: 1 lamp | no shadows"]


def test_tally_reports_the_first_line_alone(capsys):
    tally = Tally(t_load=0.25)
    tally.t_render, tally.t_bake, tally.t_relight, tally.frames = 4.5, 1.0, 0.125, 9
    tally.sh_residual, tally.sh_store = torch.tensor(0.03125, dtype=torch.float64), (9, 2_500_000)
    lines = _report(capsys, tally, ["--transfer", "fp16", "--sh-order", "2"])
    assert lines == ["o: 9 frames 24x16 | load 0.250s render 4.500s (0.500s/frame) | transfer fp16: bake 1.000s relight 0.125s | "
                     "sh order 2 (9 coefficients, 2.5 MB per camera): largest light_residual 3.125e-02"]
    assert _report(capsys, Tally(), []) == ["o: 0 frames 24x16 | load 0.000s render 0.000s (0.000s/frame)"]
    # a display transform that showed nothing, an antialias that marked nothing: no line
    assert len(_report(capsys, Tally(), [], display=DisplayTransform(), antialias=Antialias(samples=4))) == 1
