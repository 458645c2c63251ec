"""Frames whose sun shadows are sphere-traced through the SDF (get_outputs_for_camera_ray_bundle(..., sun_shadows="sdf")): the default
and "ddf" are the DDF frame bit for bit; the marched shadow map is relight.trace_visibility called by hand on the frame's own depth, normal
and rays under the composite's set-sun and accumulation rules, and the lit frame is sun_cpu.py's composite of that visibility; graph and
eager frames agree to the bit, a new sun and a new angular diameter replay the captured chunk; K suns, a daylight sky and an extracted
sun take the same shadows; and a model without a visibility network gets its first sun shadow."""
import numpy as np
import pytest
import torch

import envmap_sun_cpu as EC
import sun_cpu as SC
from util_shadows import camera_grid, grow_the_ball
from util_step import randomise, small_pipeline_config
from neusky_amd import hip
from neusky_amd.relight import DaylightSky, EnvironmentMap, SunLight, extract_sun, shadows, z_rotation

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W, CHUNK = 32, 48, 512  # 1536 rays: three whole chunks
TRACE = {"steps": 16}
SUN = SunLight(130.0, 35.0, (2.0, 1.7, 1.2))
DARK = SunLight(130.0, 35.0, (0.0, 0.0, 0.0))
LIN_BAR = 1e-5  # the bar of test_gpu_sun_frame.py on its linear image
SUN_KEYS = ("rgb", "lin", "shadow_map", "shadow_difference", "shadow_status")


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

    def render(use_graph=True, **kw):
        out = m.get_outputs_for_camera_ray_bundle(rb, camera_index=1, chunk=CHUNK, use_graph=use_graph, **kw)
        return {k: v.clone() for k, v in out.items()}

    def marched(use_graph=True, **kw):
        return render(use_graph, sun_shadows="sdf", shadow_trace=kw.pop("shadow_trace", TRACE), **kw)

    lit = marched(sun=SUN)  # the frame every test reads and none writes
    return pipe, rb, render, marched, lit


def _f64(t):
    return t.detach().cpu().double().numpy()


def _by_hand(m, rb, out, suns, trace):
    """the frame's shadow rays marched outside it, chunk by chunk as the frame does: the start points of nsky_sphere_trace_begin from the
    frame's own rays, p2p_dist (its depth along the ray) and normal, then relight.trace_visibility on them, one direction per ray
    -> visibility [K, N] before the composite's rules"""
    flat = rb.slice(0, 1 << 62)
    p = shadows.trace_settings(trace, shadows.SHADOW_DEFAULTS)
    params = shadows.trace_params(p).to(DEV)
    dirs = torch.tensor([s.direction for s in suns], dtype=torch.float64).to(torch.float32).to(DEV)
    K, N = len(suns), H * W
    depth, normal = out["p2p_dist"].reshape(N), out["normal"].reshape(N, 3)
    vis = []
    for a in range(0, N, CHUNK):
        b = min(a + CHUNK, N)
        R = b - a
        state, points = torch.empty(6, K * R, device=DEV), torch.empty(K * R, 3, device=DEV)
        hip.sphere_trace_begin(flat.origins[a:b].contiguous(), flat.directions[a:b].contiguous(), depth[a:b].contiguous(),
                               normal[a:b].contiguous(), dirs, params, state, points)
        tr = shadows.trace_visibility(m.field, points, dirs.repeat_interleave(R, 0), steps=p["steps"], eps=p["eps"], relax=p["relax"],
                                      min_step=p["min_step"], grace=p["grace"], radius=p["radius"],
                                      angular_diameter_deg=p["angular_diameter_deg"])
        vis.append(tr.visibility.view(K, R))
    return torch.cat(vis, 1), dirs


def test_ddf_is_the_default_and_is_what_it_was(scene):
    _, _, render, _, _ = scene
    first = render(sun=SUN)
    named = render(sun=SUN, sun_shadows="ddf")
    again = render(sun=SUN)
    assert set(first) == set(named) == set(again) and "shadow_status" not in first
    for k in first:
        assert torch.equal(first[k], named[k]) and torch.equal(first[k], again[k]), k
    assert first["shadow_difference"].abs().max().item() > 0.0
    plain, plain_named = render(), render(sun_shadows="ddf")  # and a frame without a sun
    for k in plain:
        assert torch.equal(plain[k], plain_named[k]), k


def test_shadow_map_is_the_march_by_hand(scene):
    pipe, rb, _, _, lit = scene
    m = pipe.model
    assert set(lit) >= set(SUN_KEYS) and lit["shadow_status"].dtype == torch.int8 and lit["shadow_status"].shape == (H, W, 1)
    vis, _ = _by_hand(m, rb, lit, [SUN], TRACE)
    on = lit["accumulation"].reshape(-1) > 0.0
    want = torch.where(on, vis[0], torch.zeros((), device=DEV))
    got = lit["shadow_map"].reshape(-1)
    status = lit["shadow_status"].reshape(-1)
    print(f"shadow map: {int(on.sum())} of {H * W} rays accumulate; statuses {np.bincount(status.cpu().numpy(), minlength=4).tolist()}; "
          f"differs from the march by hand by {(got - want).abs().max().item():.2e}; mean {got[on].mean().item():.3f}")
    assert on.any() and torch.equal(got, want)
    hit, lit_rays = on & (status == shadows.HIT), on & (status == shadows.ESCAPED)
    assert hit.sum() > 50 and lit_rays.sum() > 50  # the ball shadows itself on the side away from the sun, and not on the other
    assert lit["shadow_difference"].abs().max().item() == 0.0
    assert ((status == shadows.HIT) | (status == shadows.ESCAPED) | (status == shadows.EXHAUSTED)).all()
    assert (got[on & (status == shadows.HIT)] == 0.0).all()
    assert got.min().item() >= 0.0 and got.max().item() <= 1.0


def test_lit_frame_is_the_composite_of_the_marched_visibility(scene):
    pipe, rb, _, marched, lit = scene
    m = pipe.model
    dark = marched(sun=DARK)
    vis, dirs = _by_hand(m, rb, lit, [SUN], TRACE)
    flat = rb.slice(0, 1 << 62)
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
                t.append(SC.transfer(_f64(albedo), _f64(normals), _f64(so["weights"][..., 0]), _f64(dirs))[0][0])
        finally:
            m.end_frame()
    t = np.concatenate(t)[None]  # [1, N, 3]
    rgb, lin, V = SC.composite(_f64(dark["lin"]).reshape(-1, 3), t, _f64(vis), _f64(lit["accumulation"]).reshape(-1), 0.0, _f64(dirs),
                               np.array([SUN.colour], np.float32).astype(np.float64))
    err = np.abs(_f64(lit["lin"]).reshape(-1, 3) - lin[0]).max()
    print(f"lin vs the composite of the marched visibility: max err {err:.3e}, sun term max {(lin[0] - _f64(dark['lin']).reshape(-1, 3)).max():.3f}")
    assert err < LIN_BAR
    np.testing.assert_allclose(_f64(lit["rgb"]).reshape(-1, 3), SC.linear_to_srgb(_f64(lit["lin"]).reshape(-1, 3)), rtol=1e-4, atol=1e-6)
    assert np.array_equal(_f64(lit["shadow_map"]).reshape(-1), V[0])
    assert (_f64(lit["lin"]) - _f64(dark["lin"])).max() > 1e-2  # the sun lit something


def test_graph_and_eager_frames_are_the_same_bits(scene):
    _, _, _, marched, lit = scene
    eager = marched(use_graph=False, sun=SUN)
    assert set(eager) == set(lit)
    print({k: float((eager[k].double() - lit[k].double()).abs().max()) for k in lit})
    for k in lit:
        assert torch.equal(eager[k], lit[k]), k


def test_a_new_sun_and_diameter_replay_the_captured_chunk(scene):
    pipe, _, _, marched, lit = scene
    m = pipe.model
    marched(sun=SUN)
    runners = dict(m.frames.runners)
    other = SunLight(250.0, 15.0, (3.0, 2.0, 0.5))
    wide = {**TRACE, "angular_diameter_deg": 4.0, "eps": 2e-3, "bias": 0.02}
    got = marched(sun=other, shadow_trace=wide)
    assert len(m.frames.runners) == len(runners) and all(m.frames.runners[k] is r for k, r in runners.items())
    eager = marched(use_graph=False, sun=other, shadow_trace=wide)
    for k in SUN_KEYS:
        assert torch.equal(got[k], eager[k]), k
    assert not torch.equal(got["shadow_map"], lit["shadow_map"])
    n = len(m.frames.runners)
    longer = marched(sun=other, shadow_trace={**wide, "steps": 20})  # the march's length is held by value: another runner
    assert len(m.frames.runners) in (n + 1, 1)  # (the cache holds four, and starts again when it is full)
    assert longer["shadow_map"].shape == got["shadow_map"].shape


def test_three_suns_one_of_them_set(scene):
    pipe, rb, _, marched, lit = scene
    suns = [SUN, SunLight(10.0, -5.0, (1.0, 1.0, 1.0)), SunLight(250.0, 15.0, (3.0, 2.0, 0.5))]
    many = marched(sun=suns)
    assert many["shadow_map"].shape == (3, H, W, 1) and many["shadow_status"].shape == (3, H, W, 1) and many["rgb"].shape == (3, H, W, 3)
    assert many["shadow_status"].dtype == torch.int8
    assert many["shadow_map"][1].abs().max().item() == 0.0
    vis, _ = _by_hand(pipe.model, rb, many, suns, TRACE)
    on = (many["accumulation"].reshape(-1) > 0.0)[None] & torch.tensor([s.elevation_deg > 0.0 for s in suns], device=DEV)[:, None]
    assert torch.equal(many["shadow_map"].reshape(3, -1), torch.where(on, vis, torch.zeros((), device=DEV)))
    assert not torch.equal(many["shadow_map"][0], many["shadow_map"][2])


def test_daylight_and_extracted_suns_take_the_same_shadows(scene):
    _, _, _, marched, lit = scene
    sky = DaylightSky()
    day = marched(sun=sky.sun(SUN.azimuth_deg, SUN.elevation_deg), daylight=sky)
    assert torch.equal(day["shadow_map"], lit["shadow_map"]) and torch.equal(day["shadow_status"], lit["shadow_status"])
    ext = extract_sun(EnvironmentMap(EC.synthetic_map(64, 128, "blender", 130.7, 35.3, 4.0), "blender"), radius_deg=12.0)
    assert ext.found
    rot = z_rotation(0.4)
    found = ext.sun(rot)
    on_map = marched(envmap=ext.envmap, rotation=rot.to(DEV), sun=found)
    on_latent = marched(sun=found)
    assert torch.equal(on_map["shadow_map"], on_latent["shadow_map"])
    assert not torch.equal(on_map["rgb"], on_latent["rgb"])


def test_a_model_without_a_visibility_network_casts_a_shadow(scene):
    pipe, _, render, marched, _ = scene
    m = pipe.model
    m.config.use_visibility = False
    try:
        ddf = render(sun=SUN)
        sdf = marched(sun=SUN)
    finally:
        m.config.use_visibility = True
    on = ddf["accumulation"] > 0.0
    assert torch.equal(ddf["shadow_map"], on.to(torch.float32))  # no shadow: every accumulating ray sees the sun, as before
    inside = sdf["shadow_map"][on]
    print(f"without a visibility network: marched shadow map from {inside.min().item():.3f} to {inside.max().item():.3f}, mean {inside.mean().item():.3f}")
    assert inside.min().item() < inside.max().item()
    assert sdf["shadow_difference"].abs().max().item() == 0.0 and "shadow_status" in sdf and "shadow_status" not in ddf


def test_a_model_built_without_a_visibility_field_renders_its_suns():
    """not the flag flipped on a model that has a DDF: the pipeline is set up with no visibility field, so the model has neither
    `sigmoid_scale` nor `visibility_threshold`, and a sun frame must not ask for them (randomise() would: the ball is grown from the
    geometric initialisation instead)"""
    torch.manual_seed(0)
    cfg = small_pipeline_config(R=16, D=32, images=4, S=24)
    cfg.visibility_field = None
    cfg.model.use_visibility = False
    pipe = cfg.setup(device=DEV)
    grow_the_ball(pipe)
    m = pipe.model
    assert m.visibility_field is None and not hasattr(m, "sigmoid_scale") and not hasattr(m, "visibility_threshold")
    with torch.no_grad():
        g = torch.Generator().manual_seed(3)
        m.eval_illumination_latents.copy_((torch.randn(m.eval_illumination_latents.shape, generator=g) * 0.3).to(DEV))
        m.eval_scale.copy_((1 + 0.2 * torch.rand(m.eval_scale.shape, generator=g)).to(DEV))
    pipe.eval()
    rb = camera_grid(8, 12, DEV)  # 96 rays at chunk 64: a whole chunk and a padded one
    render = lambda **kw: m.get_outputs_for_camera_ray_bundle(rb, camera_index=1, chunk=64, **kw)  # noqa: E731
    with torch.no_grad():
        m.begin_frame(1, sun=SUN)
        key = m.frames.active.key
        m.end_frame()
    assert key == ((1, None), "sun", 1, 0.0)
    ddf = render(sun=SUN)
    on = ddf["accumulation"] > 0.0
    assert on.any() and torch.equal(ddf["shadow_map"], on.to(torch.float32))  # no DDF: every accumulating ray sees the sun
    sdf = render(sun=[SUN, DARK], sun_shadows="sdf", shadow_trace=TRACE)
    sky = render(sun=SUN, daylight=DaylightSky(), sun_shadows="sdf", shadow_trace=TRACE)
    for out in (ddf, sdf, sky):
        assert all(torch.isfinite(out[k]).all() for k in SUN_KEYS if k in out)
    assert sdf["shadow_status"].shape == (2, 8, 12, 1) and sdf["shadow_difference"].abs().max().item() == 0.0
    assert torch.equal(sky["shadow_map"], sdf["shadow_map"][0])  # the march does not depend on the sky


def test_what_excludes_the_march_is_refused(scene):
    _, _, render, marched, _ = scene
    with pytest.raises(ValueError):
        marched(sun=SUN, shadow_threshold=0.1)
    with pytest.raises(ValueError):
        marched()  # no sun
    with pytest.raises(ValueError):
        render(sun=SUN, shadow_trace=TRACE)  # the parameters without the mode
    with pytest.raises(ValueError):
        render(sun=SUN, sun_shadows="mesh")
    with pytest.raises(ValueError):
        marched(sun=SUN, shadow_trace={"step": 3})
