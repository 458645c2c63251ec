"""Frames seen through an atmosphere (get_outputs_for_camera_ray_bundle(..., atmosphere=)): without one every frame is what it was, bit
for bit, on a model that has rendered fog and on a fresh one, and no chunk graph appears; the fogged frame is atmosphere_cpu.py's rule
applied to the clear frame's own linear image, accumulation, depth, rays and background, under the sky alone, suns, a daylight sky,
marched shadows and a lamp; shafts take the visibilities the frame's shadow mode gives by hand at the segments' midpoints; graph and
eager frames agree to the bit; a new medium replays the captured chunk; antialiasing fogs every sub-pixel sample at its own depth; a
display transform sees the fogged frame.

The scene, the 32 x 48 frame and its three chunks are test_gpu_lights_frame.py's."""
import numpy as np
import pytest
import torch

import atmosphere_cpu as AC
import sun_cpu as SC
from util_shadows import camera_grid, grow_the_ball
from util_step import randomise, small_pipeline_config
from neusky_amd import hip
from neusky_amd.cameras.rays import RayBundle
from neusky_amd.relight import Antialias, Atmosphere, DaylightSky, DisplayTransform, PointLight, SunLight, shadows, subpixel_rays
from neusky_amd.relight.lighting import light_colours, ray_background

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W, CHUNK = 32, 48, 512  # 1536 rays: three whole chunks
N = H * W
CAM = 1
TRACE = {"steps": 16}
LAMP = PointLight((0.3, 0.6, 0.2), (1.0, 0.8, 0.6))
SUN = SunLight(130.0, 35.0, (2.0, 1.7, 1.2))
OTHER = SunLight(250.0, 15.0, (3.0, 2.0, 0.5))
LIN_BAR = 1e-5  # the bar of test_gpu_sun_frame.py on its linear image
AA_BAR = 2e-6  # the bar of test_gpu_antialias_frame.py: times max(1, max |value|) of the output
FOG = Atmosphere(1.5, scale_height=0.3, base_height=-0.2, albedo=(0.9, 0.8, 1.0), anisotropy=0.6)
FRAME_KEYS = ("rgb", "lin", "atmosphere_transmittance", "atmosphere_inscatter")


def _build():
    torch.manual_seed(0)
    pipe = small_pipeline_config(R=16, D=32, images=4, S=24).setup(device=DEV)
    randomise(pipe)
    grow_the_ball(pipe)  # something to cast a shadow
    m = pipe.model
    with torch.no_grad():
        g = torch.Generator().manual_seed(3)
        m.eval_illumination_latents.copy_((torch.randn(m.eval_illumination_latents.shape, generator=g) * 0.3).to(DEV))
        m.eval_scale.copy_((1 + 0.2 * torch.rand(m.eval_scale.shape, generator=g)).to(DEV))
    pipe.eval()
    return pipe


def _renderer(m, rb):
    def render(use_graph=True, bundle=rb, **kw):
        if kw.get("sun_shadows") == "sdf":
            kw.setdefault("shadow_trace", TRACE)
        if kw.get("lights"):
            kw.setdefault("light_trace", TRACE)
        out = m.get_outputs_for_camera_ray_bundle(bundle, camera_index=CAM, chunk=CHUNK, use_graph=use_graph, **kw)
        return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in out.items()}
    return render


@pytest.fixture(scope="module")
def scene():
    pipe = _build()
    rb = camera_grid(H, W, DEV)
    return pipe, rb, _renderer(pipe.model, rb)


def _f64(t):
    return t.detach().cpu().double().numpy()


def _sun_tensors(suns):
    dirs = torch.tensor([s.direction for s in suns], dtype=torch.float64).to(torch.float32).to(DEV)
    return dirs, torch.tensor([s.colour for s in suns], dtype=torch.float32).to(DEV)


def _frame_inputs(m, rb, clear, suns=None, daylight=None):
    """what the rule reads of a clear frame, in float64: its own lin [Kb, N, 3], accumulation and depth along the ray, the rays, the sky
    behind them (relight.lighting.ray_background) and the mean light colour of each base image's sky"""
    flat = rb.slice(0, 1 << 62)
    K = 1 if suns is None else len(suns)
    dirs = m.illumination_sampler.on_device(m.device, apply_random_rotation=False)[0]
    sun_dirs, sun_cols = (None, None) if suns is None else _sun_tensors(suns)
    with torch.no_grad():
        if daylight is None:
            bg = ray_background(m, flat.directions.contiguous(), CAM)
            abar = np.broadcast_to(_f64(light_colours(m, dirs, CAM)).mean(0), (K, 3))
        else:
            from neusky_amd.models.frame import FrameDaylight
            t = lambda *v: torch.tensor(v, dtype=torch.float32, device=DEV)  # noqa: E731
            day = FrameDaylight(None, t(daylight.turbidity), t(daylight.exposure), t(*daylight.ground), sun_dirs, None)
            bg = ray_background(m, flat.directions.contiguous(), CAM, daylight=day)
            lights = torch.empty(K, dirs.shape[0], 3, device=DEV)
            hip.daylight_eval(dirs, sun_dirs, day.turbidity, day.exposure, day.ground, lights)
            abar = _f64(lights).mean(1)
    return dict(origins=_f64(flat.origins), directions=_f64(flat.directions), depth=_f64(clear["p2p_dist"]).reshape(N),
                accumulation=_f64(clear["accumulation"]).reshape(N), lin=_f64(clear["lin"]).reshape(K, N, 3), background=_f64(bg), abar=abar,
                sun_dirs=None if suns is None else _f64(sun_dirs), sun_colours=None if suns is None else _f64(sun_cols))


def _check(name, fogged, clear, want, lead=()):
    """a fogged frame against the rule's outputs `want` of the clear frame; lead: (K,) under a sequence of suns"""
    assert fogged["lin"].shape == (*lead, H, W, 3) and fogged["atmosphere_inscatter"].shape == (*lead, H, W, 3), name
    assert fogged["atmosphere_transmittance"].shape == (H, W, 3) and fogged["rgb"].shape == fogged["lin"].shape
    errs = {k: float(np.abs(_f64(fogged[g]).reshape(np.shape(want[k])) - want[k]).max())
            for g, k in (("lin", "lin"), ("atmosphere_inscatter", "inscatter"), ("atmosphere_transmittance", "transmittance"))}
    moved = np.abs(_f64(fogged["lin"]) - _f64(clear["lin"])).reshape(-1, N, 3).max((0, 2))
    print(f"{name}: against the rule on the clear frame: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items())
          + f" (bar {LIN_BAR:.0e}); the fog moved lin by more than 100 bars on {100.0 * (moved > 100 * LIN_BAR).mean():.1f}% of the rays")
    assert max(errs.values()) < LIN_BAR, (name, errs)
    np.testing.assert_allclose(_f64(fogged["rgb"]), SC.linear_to_srgb(_f64(fogged["lin"])), rtol=1e-4, atol=1e-6)
    for k in ("albedo", "accumulation", "depth", "p2p_dist", "normal"):
        assert torch.equal(fogged[k], clear[k]), (name, k)


def test_without_an_atmosphere_every_frame_is_what_it_was(scene):
    pipe, rb, render = scene
    m = pipe.model
    render(atmosphere=FOG), render(sun=SUN, atmosphere=FOG), render(lights=LAMP, atmosphere=FOG)  # the model has rendered fog
    fresh = _build()
    clean = _renderer(fresh.model, rb)
    for kw in ({}, {"sun": SUN}, {"lights": LAMP}):
        absent = render(**kw)
        keys = set(m.frames.runners)
        same, untouched = render(atmosphere=None, **kw), clean(**kw)
        assert set(same) == set(absent) == set(untouched) and not any(k.startswith("atmosphere") for k in same)
        for k in absent:
            assert torch.equal(same[k], absent[k]) and torch.equal(untouched[k], absent[k]), (kw, k)
        assert set(m.frames.runners) == keys and len(m.frames.runners) == len(keys)  # no new chunk graph
    assert "lin" not in render()


MODES = {"the sky alone": {}, "one sun": {"sun": SUN}, "two suns": {"sun": [SUN, OTHER]},
         "daylight, two suns": {"daylight": True, "sun": [(130.0, 35.0), (250.0, 15.0)]},
         "a sun, sdf shadows": {"sun": SUN, "sun_shadows": "sdf"}, "a sun and a lamp": {"sun": SUN, "lights": LAMP}}


@pytest.mark.parametrize("mode", list(MODES))
def test_the_fogged_frame_is_the_rule_on_the_clear_frame(scene, mode):
    pipe, rb, render = scene
    m = pipe.model
    kw = dict(MODES[mode])
    sky = None
    if kw.pop("daylight", False):
        sky = DaylightSky()
        kw.update(daylight=sky, sun=[sky.sun(*p) for p in kw["sun"]])
    suns = kw.get("sun")
    suns = None if suns is None else list(suns) if isinstance(suns, (list, tuple)) else [suns]
    clear = render(**kw, **({} if suns else {"display": DisplayTransform()}))  # (display: a sky frame's `lin`)
    fogged = render(**kw, atmosphere=FOG)
    inputs = _frame_inputs(m, rb, clear, suns, sky)
    lamps = "lights" in kw
    want = AC.apply(**inputs, vis=None, params=_f64(FOG.block()), M=0, light_lin=_f64(clear["light_lin"]).reshape(N, 3) if lamps else None)
    _check(mode, fogged, clear, want, (len(suns),) if isinstance(kw.get("sun"), list) else ())
    moved = np.abs(_f64(fogged["lin"]) - _f64(clear["lin"])).reshape(-1, N, 3).max((0, 2))
    assert (moved > 100 * LIN_BAR).mean() >= 0.5  # a no-op cannot pass
    if lamps:
        assert np.abs(_f64(fogged["light_lin"]).reshape(N, 3) - want["light_lin"]).max() < LIN_BAR
        assert torch.equal(fogged["light_visibility"], clear["light_visibility"])
    for k in ("shadow_map", "shadow_difference", "shadow_status"):
        assert k not in clear or torch.equal(fogged[k], clear[k]), k
    if sky is None:
        assert set(fogged) - set(clear) == {"atmosphere_transmittance", "atmosphere_inscatter"}
    T = _f64(fogged["atmosphere_transmittance"])
    assert T.min() >= 0.0 and T.max() <= 1.0 and T.min() < 0.9


def _shaft_visibilities(m, rb, suns, M, far, mode):
    """V [M, K, N] by hand, chunk by chunk as the frame does: the frame's own shadow primitive on the rows (ray r at the midpoint of segment m)"""
    flat = rb.slice(0, 1 << 62)
    sun_dirs, _ = _sun_tensors(suns)
    K = len(suns)
    depths = torch.from_numpy(AC.midpoints(far, M).astype(np.float32)).to(DEV)
    params = shadows.trace_params(shadows.trace_settings(TRACE, {**shadows.SHADOW_DEFAULTS, "radius": 1.0})).to(DEV)
    p = shadows.trace_settings(TRACE, {**shadows.SHADOW_DEFAULTS, "radius": 1.0})
    out = []
    m.field.invalidate_weight_cache()
    with torch.no_grad():
        for a in range(0, N, CHUNK):
            b = min(a + CHUNK, N)
            n = b - a
            ro, rd = flat.origins[a:b].repeat(M, 1).contiguous(), flat.directions[a:b].repeat(M, 1).contiguous()
            rt = depths.repeat_interleave(n).contiguous()
            if mode == "sdf":
                march = shadows.trace_sun_shadows(m.field, ro, rd, rt, torch.zeros(M * n, 3, device=DEV), sun_dirs, params, p["steps"], p["grace"])
                out.append(march.visibility.view(K, M, n).permute(1, 0, 2))
            else:
                vd = m.compute_visibility_compact(ro, rd, rt[:, None], sun_dirs, m.visibility_threshold.detach(), float(m.sigmoid_scale),
                                                  sel=torch.arange(K, device=DEV, dtype=torch.int32))
                out.append(vd["visibility"].view(M, n, K).permute(0, 2, 1))
    return torch.cat(out, 2)


@pytest.mark.parametrize("mode", ("ddf", "sdf"))
def test_shafts_take_the_shadow_modes_visibilities(scene, mode):
    pipe, rb, render = scene
    m = pipe.model
    M = 4
    fog = Atmosphere((0.5, 1.0, 2.0), albedo=0.9, anisotropy=0.3, shaft_samples=M)
    kw = {"sun": [SUN, OTHER], "sun_shadows": mode}
    clear, fogged = render(**kw), render(**kw, atmosphere=fog)
    V = _shaft_visibilities(m, rb, [SUN, OTHER], M, fog.far, mode)
    assert V.shape == (M, 2, N) and float(V.min()) >= 0.0 and float(V.max()) <= 1.0
    want = AC.apply(**_frame_inputs(m, rb, clear, [SUN, OTHER]), vis=_f64(V), params=_f64(fog.block()), M=M)
    _check(f"shafts, {mode}", fogged, clear, want, (2,))
    spread = (V.max(0).values - V.min(0).values).max(0).values  # [N]: the widest difference between two segments of a ray
    print(f"shafts, {mode}: {int((spread > 0.5).sum())} of {N} rays have two segments whose visibility differs by more than 0.5")
    unshadowed = AC.apply(**_frame_inputs(m, rb, clear, [SUN, OTHER]), vis=None, params=_f64(fog.block()), M=M)
    if mode == "sdf":
        assert int((spread > 0.5).sum()) >= 1  # a shaft: the ray crosses the edge of the ball's shadow
        assert np.abs(unshadowed["lin"] - want["lin"]).max() > 100 * LIN_BAR  # and the frame shows it


def test_graph_and_eager_frames_are_the_same_bits(scene):
    _, _, render = scene
    for kw in ({}, {"sun": SUN}, {"sun": [SUN, OTHER], "lights": LAMP}):
        fog = Atmosphere(1.5, 0.3, shaft_samples=4 if "sun" in kw else 0)
        kw = {**kw, "atmosphere": fog}
        graph, eager = render(**kw), render(use_graph=False, **kw)
        assert set(graph) == set(eager) and set(FRAME_KEYS) <= set(graph)
        for k in graph:
            assert torch.equal(graph[k], eager[k]), (sorted(kw), k)


def test_a_new_medium_replays_the_captured_chunk(scene):
    pipe, rb, render = scene
    m = pipe.model
    clear = render(sun=SUN)
    first = render(sun=SUN, atmosphere=FOG)
    runners = dict(m.frames.runners)
    other = Atmosphere((0.4, 0.8, 1.6), scale_height=None, base_height=0.3, albedo=0.7, anisotropy=-0.4, far=1.5, background=False)
    got = render(sun=SUN, atmosphere=other)
    assert len(m.frames.runners) == len(runners) and all(m.frames.runners[k] is r for k, r in runners.items())
    want = AC.apply(**_frame_inputs(m, rb, clear, [SUN]), vis=None, params=_f64(other.block()), M=0)
    _check("a second medium through the first one's graph", got, clear, want)
    assert not torch.equal(got["lin"], first["lin"])
    eager = render(use_graph=False, sun=SUN, atmosphere=other)
    for k in FRAME_KEYS:
        assert torch.equal(got[k], eager[k]), k
    n = len(m.frames.runners)
    render(sun=SUN, atmosphere=Atmosphere(1.5, shaft_samples=2))  # the shaft samples are held by value: another runner
    assert len(m.frames.runners) in (n + 1, 1)  # (the cache holds four, and starts again when it is full)


def test_antialiasing_fogs_every_sample_at_its_own_depth(scene):
    _, rb, render = scene
    aa = Antialias(4, every_pixel=True)
    S1 = aa.samples - 1
    sub = subpixel_rays(rb, torch.arange(N, device=DEV), aa.sample_offsets(DEV))  # pixel-major: row e S1 + s
    centre = render(sun=SUN, atmosphere=FOG)
    total = centre["lin"].double()
    for s in range(S1):
        pick = lambda t: t.reshape(N, S1, -1)[:, s].reshape(H, W, -1).contiguous()  # noqa: E731
        bundle = RayBundle(pick(sub.origins), pick(sub.directions), pick(sub.pixel_area), pick(sub.camera_indices),
                           metadata={"directions_norm": pick(sub.metadata["directions_norm"])})
        total = total + render(bundle=bundle, sun=SUN, atmosphere=FOG)["lin"].double()
    want = total / aa.samples
    out = render(sun=SUN, atmosphere=FOG, antialias=aa)
    worst, scale = float((out["lin"].double() - want).abs().max()), max(1.0, float(want.abs().max()))
    print(f"antialiased fogged lin: worst difference from the brute-force average {worst:.2e} (values up to {scale:.3g}, bar {AA_BAR * scale:.2e})")
    assert out["aa_fraction"] == 1.0 and worst <= AA_BAR * scale
    for k in ("atmosphere_transmittance", "atmosphere_inscatter", "depth"):
        assert torch.equal(out[k], centre[k]), k  # the centre ray's
    np.testing.assert_allclose(_f64(out["rgb"]), SC.linear_to_srgb(_f64(out["lin"])), rtol=1e-4, atol=1e-6)


def test_display_sees_the_fogged_frame(scene):
    _, _, render = scene
    fogged = render(atmosphere=FOG)
    shown, plain = render(atmosphere=FOG, display=DisplayTransform()), render(display=DisplayTransform())
    assert torch.equal(shown["lin"], fogged["lin"]) and not torch.equal(shown["lin"], plain["lin"])
    assert not torch.equal(shown["display_rgb"], plain["display_rgb"])
