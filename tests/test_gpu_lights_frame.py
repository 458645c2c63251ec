"""Frames lit by point and spot lights inside the scene (get_outputs_for_camera_ray_bundle(..., lights=)): without lights every frame is
what it was, bit for bit, and no chunk graph appears; `light_visibility` is the bounded march called by hand on the frame's own depth,
normal and rays, and the lit frame is lights_cpu.py's composite of a float64 transfer of the chunks' samples; lamps add, scale with
their intensity and sit on top of suns and a daylight sky without touching the suns' shadows; graph and eager frames agree to the bit,
new lamp values replay the captured chunk; antialiasing resolves the lamps' image too.

The lamp stands beside the ball and in front of the camera, at (0.3, 0.6, 0.2).  With 16 rounds, of the 1536 rays (all accumulate) its
shadow rays end HIT on 269 (the side of the ball away from it), ESCAPED on 604 and EXHAUSTED on 663."""
import dataclasses

import numpy as np
import pytest
import torch

import lights_cpu as LC
import sun_cpu as SC
from util_shadows import camera_grid, grow_the_ball
from util_step import randomise, small_pipeline_config
from neusky_amd import hip
from neusky_amd.cameras.rays import RayBundle
from neusky_amd.relight import (Antialias, DaylightSky, DisplayTransform, FrameLighting, PointLight, SunLight, lights, lights_block, shadows,
                                subpixel_rays)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W, CHUNK = 32, 48, 512  # 1536 rays: three whole chunks
N = H * W
TRACE = {"steps": 16}
LAMP = PointLight((0.3, 0.6, 0.2), (1.0, 0.8, 0.6))
OTHER = PointLight((0.55, -0.45, 0.35), (0.3, 0.5, 0.9), radius=0.05, direction=(-0.5, 0.4, -0.3), inner_deg=20.0, outer_deg=50.0)
SUN = SunLight(130.0, 35.0, (2.0, 1.7, 1.2))
LIN_BAR = 1e-5  # the bar of test_gpu_sun_frame.py on its linear image
LIGHT_KEYS = ("rgb", "lin", "light_lin", "light_visibility", "light_status")


@pytest.fixture(scope="module")
def scene():
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
    rb = camera_grid(H, W, DEV)

    def render(use_graph=True, bundle=rb, **kw):
        if kw.get("lights") and kw.get("light_shadows", True):
            kw.setdefault("light_trace", TRACE)
        out = m.get_outputs_for_camera_ray_bundle(bundle, camera_index=1, chunk=CHUNK, use_graph=use_graph, **kw)
        return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in out.items()}

    lit = render(lights=LAMP)  # the frame every test reads and none writes
    return pipe, rb, render, lit


def _f64(t):
    return t.detach().cpu().double().numpy()


def _ulps(got, ref64, scale):
    return np.abs(got - ref64) / np.spacing(np.abs(scale).astype(np.float32)).astype(np.float64)


def _march_by_hand(m, rb, out, lamps, trace):
    """the frame's lamp-shadow rays marched outside it, chunk by chunk as the frame does: nsky_light_trace_begin on the frame's own rays,
    p2p_dist (its depth along the ray) and normal, then `steps` rounds of the field's sdf and the bounded step, and the finish
    -> visibility, status [L, N] before the accumulation rule"""
    flat = rb.slice(0, 1 << 62)
    p = shadows.trace_settings(trace, {**lights.LIGHT_TRACE_DEFAULTS, "radius": 1.0})
    params = shadows.trace_params(p).to(DEV)
    block = lights_block(lamps).to(DEV)
    L = block.shape[0]
    depth, normal = out["p2p_dist"].reshape(N), out["normal"].reshape(N, 3)
    vis, status = [], []
    m.field.invalidate_weight_cache()
    for a in range(0, N, CHUNK):
        b = min(a + CHUNK, N)
        T = L * (b - a)
        state, points, ray_dirs, bounds = (torch.empty(6, T, device=DEV), torch.empty(T, 3, device=DEV), torch.empty(T, 3, device=DEV),
                                           torch.empty(2, T, device=DEV))
        hip.light_trace_begin(flat.origins[a:b].contiguous(), flat.directions[a:b].contiguous(), depth[a:b].contiguous(),
                              normal[a:b].contiguous(), block, params, state, points, ray_dirs, bounds)
        with torch.no_grad():
            for i in range(p["steps"]):
                hip.sphere_trace_step(state, m.field.get_sdf_at_pos(points).reshape(-1), ray_dirs, 1, params, i, p["steps"], p["grace"],
                                      points, bounds)
        v, t, s = torch.empty(T, device=DEV), torch.empty(T, device=DEV), torch.empty(T, dtype=torch.int8, device=DEV)
        hip.sphere_trace_finish(state, v, s, t)
        vis.append(v.view(L, b - a))
        status.append(s.view(L, b - a))
    return torch.cat(vis, 1), torch.cat(status, 1)


def _transfer_by_hand(m, rb, lamps):
    """the float64 transfer [L, N, 3] of the chunks' own samples"""
    flat = rb.slice(0, 1 << 62)
    block = lights_block(lamps).double().numpy()
    t = []
    with torch.no_grad():
        m.begin_frame(1)
        try:
            m.begin_step()
            for a in range(0, N, CHUNK):
                c = flat.slice(a, min(a + CHUNK, N))
                c = type(c)(c.origins.contiguous(), c.directions.contiguous(), c.pixel_area.contiguous(), c.camera_indices.contiguous(),
                            metadata={k: v.contiguous() for k, v in c.metadata.items()})
                so = m.sample_and_forward_field(m.collider(c))
                fo = so["field_outputs"]
                albedo = [v for k, v in fo.items() if str(k).lower().endswith("albedo")][0]
                normals = [v for k, v in fo.items() if str(k).lower().endswith("normals")][0]
                x = so["ray_samples"].frustums.get_positions()
                t.append(LC.transfer(_f64(x), _f64(albedo), _f64(normals), _f64(so["weights"][..., 0]), block)[0])
        finally:
            m.end_frame()
    return np.concatenate(t, 1)


def test_without_lights_every_frame_is_what_it_was(scene):
    pipe, _, render, _ = scene
    m = pipe.model
    for kw in ({}, {"sun": SUN}, {"sun": SUN, "sun_shadows": "sdf", "shadow_trace": TRACE}):
        absent = render(**kw)
        keys = set(m.frames.runners)
        for none in (None, ()):
            same = render(lights=none, **kw)
            assert set(same) == set(absent) and not any(k.startswith("light_") for k in same)
            for k in absent:
                assert torch.equal(same[k], absent[k]), (kw, k)
            assert set(m.frames.runners) == keys  # no new chunk graph
        assert "lin" not in absent or "sun" in kw


def test_light_visibility_is_the_march_by_hand(scene):
    pipe, rb, _, lit = scene
    assert set(lit) >= set(LIGHT_KEYS) and lit["light_status"].dtype == torch.int8
    assert lit["light_status"].shape == (H, W, 1) and lit["light_visibility"].shape == (H, W, 1) and lit["light_lin"].shape == (H, W, 3)
    vis, status = _march_by_hand(pipe.model, rb, lit, [LAMP], TRACE)
    on = lit["accumulation"].reshape(-1) > 0.0
    got = lit["light_visibility"].reshape(-1)
    assert on.any() and torch.equal(got, torch.where(on, vis[0], torch.zeros((), device=DEV)))
    st = lit["light_status"].reshape(-1)
    assert torch.equal(st, status[0])
    counts = np.bincount(st[on].cpu().numpy(), minlength=4).tolist()
    print(f"lamp shadow rays: {int(on.sum())} of {N} rays accumulate; statuses {counts}; mean visibility {got[on].mean().item():.3f}")
    assert counts[shadows.HIT] >= 50 and counts[shadows.ESCAPED] >= 50  # 269 and 604
    assert ((st == shadows.HIT) | (st == shadows.ESCAPED) | (st == shadows.EXHAUSTED)).all()
    assert (got[on & (st == shadows.HIT)] == 0.0).all() and got.min().item() >= 0.0 and got.max().item() <= 1.0


def test_lit_frame_is_the_composite_of_the_transfer_by_hand(scene):
    pipe, rb, render, lit = scene
    m = pipe.model
    dark = render(lights=dataclasses.replace(LAMP, intensity=(0.0, 0.0, 0.0)))
    unlit = render(display=DisplayTransform())  # (display: a sky frame's `lin`)
    assert torch.equal(dark["lin"], unlit["lin"]) and torch.equal(dark["rgb"], unlit["rgb"])  # no intensity: the unlit frame's bits
    assert dark["light_lin"].abs().max().item() == 0.0 and torch.equal(dark["light_visibility"], lit["light_visibility"])
    vis, _ = _march_by_hand(m, rb, lit, [LAMP], TRACE)
    t = _transfer_by_hand(m, rb, [LAMP])
    rgb, lin, E, V = LC.composite(_f64(unlit["lin"]).reshape(N, 3), t, _f64(vis), _f64(lit["accumulation"]).reshape(N), 0.0,
                                  lights_block(LAMP).double().numpy())
    err = np.abs(_f64(lit["lin"]).reshape(N, 3) - lin[0]).max()
    err_l = np.abs(_f64(lit["light_lin"]).reshape(N, 3) - E).max()
    print(f"lin vs the composite of the transfer by hand: max err {err:.3e} (light_lin {err_l:.3e}), lamp term max {E.max():.3f}")
    assert err < LIN_BAR and err_l < LIN_BAR
    np.testing.assert_allclose(_f64(lit["rgb"]).reshape(N, 3), SC.linear_to_srgb(_f64(lit["lin"]).reshape(N, 3)), rtol=1e-4, atol=1e-6)
    assert np.array_equal(_f64(lit["light_visibility"]).reshape(N), V[0])
    assert (_f64(lit["lin"]) - _f64(unlit["lin"])).max() > 1e-2  # the lamp lit something
    for k in ("albedo", "accumulation", "depth", "p2p_dist", "normal"):
        assert torch.equal(lit[k], unlit[k]), k


def test_lamps_add_and_scale(scene):
    _, _, render, lit = scene
    b, both = render(lights=OTHER), render(lights=[LAMP, OTHER])
    assert both["light_visibility"].shape == (H, W, 2) and both["light_status"].shape == (H, W, 2) and both["light_lin"].shape == (H, W, 3)
    assert torch.equal(both["light_visibility"][..., 0], lit["light_visibility"][..., 0])
    assert torch.equal(both["light_visibility"][..., 1], b["light_visibility"][..., 0])
    x, y = _f64(lit["light_lin"]), _f64(b["light_lin"])
    u = _ulps(_f64(both["light_lin"]), x + y, np.maximum(x, y))
    print(f"two lamps: light_lin(A, B) vs light_lin(A) + light_lin(B): {u.max():.2f} ulp of the larger term; B lights up to {y.max():.3f}")
    assert u.max() <= 2 and y.max() > 1e-3
    v = b["light_visibility"]
    assert ((v > 0) & (v < 1)).sum() >= 20  # a spherical source: a penumbra
    twice = render(lights=dataclasses.replace(LAMP, intensity=tuple(2.0 * c for c in LAMP.intensity)))
    assert torch.equal(twice["light_lin"], 2.0 * lit["light_lin"]) and torch.equal(twice["light_visibility"], lit["light_visibility"])


@pytest.mark.parametrize("daylight", (False, True), ids=("latent sky", "daylight sky"))
def test_lamps_on_top_of_suns(scene, daylight):
    _, _, render, lit = scene
    sky = DaylightSky()
    if daylight:
        kw = dict(daylight=sky, sun=[sky.sun(130.0, 35.0), sky.sun(10.0, -5.0), sky.sun(250.0, 15.0)])
    else:
        kw = dict(sun=[SUN, SunLight(10.0, -5.0, (1.0, 1.0, 1.0)), SunLight(250.0, 15.0, (3.0, 2.0, 0.5))])
    for mode in ({}, {"sun_shadows": "sdf", "shadow_trace": TRACE}):
        suns, lamps = render(**kw, **mode), render(lights=LAMP, **kw, **mode)
        assert lamps["lin"].shape == (3, H, W, 3) and lamps["light_lin"].shape == (H, W, 3) and lamps["light_visibility"].shape == (H, W, 1)
        for k in ("shadow_map", "shadow_difference") + (("shadow_status",) if mode else ()):
            assert torch.equal(lamps[k], suns[k]), k  # the suns' shadows keep their bits
        assert torch.equal(lamps["light_lin"], lit["light_lin"]) and torch.equal(lamps["light_visibility"], lit["light_visibility"])
        want = _f64(suns["lin"]) + _f64(lamps["light_lin"])[None]
        u = _ulps(_f64(lamps["lin"]), want, want)
        print(f"{'daylight' if daylight else 'latent'} sky, 3 suns {mode.get('sun_shadows', 'ddf')}: lin[k] vs sun lin[k] + light_lin {u.max():.2f} ulp")
        assert u.max() <= 1
        np.testing.assert_allclose(_f64(lamps["rgb"]), SC.linear_to_srgb(_f64(lamps["lin"])), rtol=1e-4, atol=1e-6)
    one = render(lights=LAMP, sun=SUN)
    assert one["lin"].shape == (H, W, 3) and one["shadow_map"].shape == (H, W, 1)


def test_a_model_without_a_visibility_network_casts_a_lamp_shadow(scene):
    pipe, _, render, lit = scene
    m = pipe.model
    m.config.use_visibility = False
    try:
        out = render(use_graph=False, lights=LAMP)  # (eager: a chunk graph is not keyed on this flag, and none may be captured under it)
    finally:
        m.config.use_visibility = True
    on = out["accumulation"] > 0.0
    inside = out["light_visibility"][on]
    assert inside.min().item() < inside.max().item() and torch.equal(out["light_status"], lit["light_status"])


def test_graph_and_eager_frames_are_the_same_bits(scene):
    _, _, render, lit = scene
    eager = render(use_graph=False, lights=LAMP)
    assert set(eager) == set(lit)
    for k in lit:
        assert torch.equal(eager[k], lit[k]), k


def test_new_lamp_values_replay_the_captured_chunk(scene):
    pipe, _, render, lit = scene
    m = pipe.model
    render(lights=LAMP)
    runners = dict(m.frames.runners)
    moved = PointLight((0.5, -0.5, 0.4), (3.0, 0.2, 1.0), radius=0.06, direction=(-0.5, 0.5, -0.4), inner_deg=25.0, outer_deg=70.0)
    trace = {**TRACE, "eps": 2e-3, "bias": 0.02}
    got = render(lights=moved, light_trace=trace)
    assert len(m.frames.runners) == len(runners) and all(m.frames.runners[k] is r for k, r in runners.items())
    eager = render(use_graph=False, lights=moved, light_trace=trace)
    for k in LIGHT_KEYS:
        assert torch.equal(got[k], eager[k]), k
    assert not torch.equal(got["light_visibility"], lit["light_visibility"])
    n = len(m.frames.runners)
    longer = render(lights=moved, light_trace={**trace, "steps": 20})  # the march's length is held by value: another runner
    assert len(m.frames.runners) in (n + 1, 1)  # (the cache holds four, and starts again when it is full)
    n = len(m.frames.runners)
    two = render(lights=[moved, LAMP], light_trace={**trace, "steps": 20})  # and so is the number of lamps
    assert len(m.frames.runners) in (n + 1, 1)
    assert longer["light_visibility"].shape == got["light_visibility"].shape and two["light_visibility"].shape == (H, W, 2)


def test_lamps_without_shadows(scene):
    _, _, render, lit = scene
    out = render(lights=LAMP, light_shadows=False)
    assert "light_status" not in out and set(out) == set(lit) - {"light_status"}
    assert torch.equal(out["light_visibility"], (out["accumulation"] > 0.0).to(torch.float32))
    assert (out["light_lin"] >= lit["light_lin"]).all() and (out["light_lin"] > lit["light_lin"]).any()


def test_antialiasing_resolves_the_lamps_image(scene):
    _, rb, render, lit = scene
    aa = Antialias(2, every_pixel=True)
    sub = subpixel_rays(rb, torch.arange(N, device=DEV), aa.sample_offsets(DEV))
    pick = lambda t: t.reshape(H, W, -1).contiguous()  # noqa: E731
    bundle = RayBundle(pick(sub.origins), pick(sub.directions), pick(sub.pixel_area), pick(sub.camera_indices),
                       metadata={"directions_norm": pick(sub.metadata["directions_norm"])})
    second = render(bundle=bundle, lights=LAMP)
    out = render(lights=LAMP, antialias=aa)
    assert out["aa_fraction"] == 1.0
    for k in ("lin", "light_lin", "light_visibility"):
        want = (lit[k].double() + second[k].double()) / 2.0
        worst, scale = float((out[k].double() - want).abs().max()), max(1.0, float(want.abs().max()))
        print(f"antialiased {k}: worst difference from the brute-force average {worst:.2e} (values up to {scale:.3g})")
        assert worst <= 2e-6 * scale, k
    assert torch.equal(out["light_status"], lit["light_status"])  # the centre ray's
    np.testing.assert_allclose(_f64(out["rgb"]), SC.linear_to_srgb(_f64(out["lin"])), rtol=1e-4, atol=1e-6)


def test_display_sees_the_lit_frame(scene):
    _, _, render, lit = scene
    shown, plain = render(lights=LAMP, display=DisplayTransform()), render(display=DisplayTransform())
    assert torch.equal(shown["lin"], lit["lin"]) and not torch.equal(shown["display_rgb"], plain["display_rgb"])


def test_what_excludes_lamps_is_refused(scene):
    _, _, render, _ = scene
    with pytest.raises(ValueError):
        FrameLighting.of(lights=LAMP, bake="fp32")
    with pytest.raises(ValueError):
        render(light_trace=TRACE)
    with pytest.raises(ValueError):
        render(lights=[LAMP] * 65)
    with pytest.raises(ValueError):
        PointLight((0, 0, 1), (1, 1, 1), inner_deg=10.0, outer_deg=20.0)
