"""Frames with solid props in them (get_outputs_for_camera_ray_bundle(..., props=)): without props every frame is what it was, bit for bit
and key for key; the seam by hand: props_cpu's intersect and insert on a chunk's own samples give the frame's prop_id, prop_weight and
reductions, and the float64 hemisphere composite of the edited samples under visibility x restated occlusion gives its `lin`; a hidden
prop and a shadow caster the camera does not see; every lighting mode, graph against eager to the bit, with the suns' and the lamps'
visibilities the prop-free query by hand times the restated occlusion; new prop values replay the captured chunk; both second passes
resolve prop_weight.

The scene is the lamp frame test's: the grown ball (radius about 0.35) seen from (0.75, 0.1, 0.05), 1536 rays, chunks of 512.  A stands
between the ball and SunLight(130, 35), B in front of the ball, C behind it.  On the analytic ball a numpy run gives 40 rays that enter
A first, 20 that enter B first, none that reach C, and A's shadow on 72 sun-facing visible ball points; the field's ball is slightly
dented, so the tests assert at least half of these and print the frame's own counts."""
import dataclasses

import numpy as np
import pytest
import torch

import antialias_cpu as AC
import props_cpu as PC
from util_shadows import camera_grid, grow_the_ball
from util_step import randomise, small_pipeline_config
from neusky_amd.cameras.rays import RayBundle
from neusky_amd.relight import (Antialias, Atmosphere, CameraPath, DaylightSky, DepthOfField, DisplayTransform, EnvironmentMap, FrameLighting,
                                PointLight, Prop, SunLight, camera_rays, lens_rays, lights_block, props_block, shadows, subpixel_rays, z_rotation)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W, CHUNK = 32, 48, 512
N = H * W
TRACE = {"steps": 16}
SUN = SunLight(130.0, 35.0, (2.0, 1.7, 1.2))
LAMP = PointLight((0.3, 0.6, 0.2), (1.0, 0.8, 0.6))
A = Prop("sphere", (0.135, 0.299, 0.321), 0.08, (0.8, 0.3, 0.2))
B = Prop("box", (0.45, -0.2, -0.2), (0.05, 0.08, 0.06), (0.2, 0.7, 0.3), yaw_deg=30.0)
C = Prop("sphere", (-0.6, -0.08, -0.04), 0.1, (0.3, 0.3, 0.9))
D = Prop("sphere", (0.225, 0.45, 0.15), 0.06)  # between the ball and LAMP
BIAS = 1e-2
BAR, LIN_BAR, CHUNK_BAR = 1e-5, 1e-5, 2e-6


def _build():
    torch.manual_seed(0)
    pipe = small_pipeline_config(R=16, D=32, images=4, S=24).setup(device=DEV)
    randomise(pipe)
    grow_the_ball(pipe)
    m = pipe.model
    with torch.no_grad():
        g = torch.Generator().manual_seed(3)
        m.eval_illumination_latents.copy_((torch.randn(m.eval_illumination_latents.shape, generator=g) * 0.3).to(DEV))
        m.eval_scale.copy_((1 + 0.2 * torch.rand(m.eval_scale.shape, generator=g)).to(DEV))
    pipe.eval()
    return pipe


def _renderer(m, rb):
    def render(use_graph=True, bundle=rb, **kw):
        if kw.get("lights") and kw.get("light_shadows", True):
            kw.setdefault("light_trace", TRACE)
        if kw.get("sun_shadows") == "sdf":
            kw.setdefault("shadow_trace", TRACE)
        out = m.get_outputs_for_camera_ray_bundle(bundle, camera_index=1, chunk=CHUNK, use_graph=use_graph, **kw)
        return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in out.items()}
    return render


@pytest.fixture(scope="module")
def scene():
    pipe = _build()
    rb = camera_grid(H, W, DEV)
    yield pipe, rb, _renderer(pipe.model, rb), {}
    pipe.model.frames.runners.clear()
    torch.cuda.empty_cache()  # (the modes' chunk graphs: handed back before the next module's processes start)


def _f64(t):
    return t.detach().cpu().double().numpy()


def _f32(t):
    return t.detach().cpu().float().numpy()


def _rays(rb):
    flat = rb.slice(0, 1 << 62)
    return _f32(flat.origins), _f32(flat.directions)


def _points(rb, out):
    """the float32 points the frame looks a prop's shadow up from: o + d p2p_dist, the product and the sum rounded once each"""
    o, d = _rays(rb)
    return o + d * _f32(out["p2p_dist"]).reshape(N, 1)


def _occluded(rb, out, props, **towards):
    x, n = _points(rb, out), _f32(out["normal"]).reshape(N, 3)
    occ, margin = PC.occlude(x, n, BIAS, props_block(props).numpy(), **towards)
    keep = margin >= PC.MARGIN
    assert (~keep).sum() <= 1e-3 * keep.size
    return occ, keep


def _sun_dirs(suns):
    return torch.tensor([s.direction for s in suns], dtype=torch.float64).to(torch.float32)


# ---------------------------------------------------------------- unchanged without props
def test_without_props_every_frame_is_what_it_was(scene):
    pipe, rb, render, _ = scene
    m = pipe.model
    render(props=[A, B], sun=SUN), render(props=C)  # the model has rendered props
    untouched = _build()  # a model that never has
    clean = _renderer(untouched.model, rb)
    for name, kw in (("sky", {}), ("sun", {"sun": SUN})):
        fresh, absent = clean(**kw), render(**kw)
        keys = set(m.frames.runners)
        assert set(absent) == set(fresh) and not any("props" in str(k) for k in untouched.model.frames.runners)
        for k, v in fresh.items():
            assert torch.equal(absent[k], v), (name, k)
        for none in (None, (), []):
            same = render(props=none, **kw)
            assert set(same) == set(fresh) and not any(k.startswith("prop_") for k in same)
            for k, v in fresh.items():
                assert torch.equal(same[k], v), (name, k)
            assert set(m.frames.runners) == keys  # no new chunk graph, no new key


# ---------------------------------------------------------------- the seam, by hand
def _hemi_f64(albedo, normals, weights, dirs, colours, vis, bg):
    """nsky_hemi_composite_fwd's linear image in float64 (include/neusky_hip.h, the transfer's form of it)"""
    cos = np.clip(np.einsum("rsi,di->rsd", normals, dirs), 0.0, 1.0)
    cnt = np.maximum((cos > 0).sum(-1), 1)
    T = vis[:, :, None] * np.einsum("rs,rsc,rsd->rdc", weights / cnt, albedo, cos)
    return np.einsum("rdc,dc->rc", T, colours) + bg * (1.0 - weights.sum(1))[:, None]


def test_the_seam_by_hand(scene):
    pipe, rb, render, _ = scene
    m = pipe.model
    props = [A, B, C]
    block = props_block(props).numpy()
    got = render(props=props, display=DisplayTransform())  # (display: a sky frame's `lin`)
    o, d = _rays(rb)
    t_hit, who, hn, ha, margin = PC.intersect(o, d, block)
    assert (margin >= PC.MARGIN).all()
    assert got["prop_id"].dtype == torch.int32 and got["prop_id"].shape == (H, W, 1) and got["prop_weight"].shape == (H, W, 1)
    assert np.array_equal(got["prop_id"].cpu().numpy().reshape(N), who)
    flat = rb.slice(0, 1 << 62)
    rows = []
    with torch.no_grad():
        m.begin_frame(1)  # the plain frame's own samples
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
                fr = so["ray_samples"].frustums
                s = slice(a, a + c.origins.shape[0])
                w1, s1, e1, a1, n1, near = PC.insert(_f32(so["weights"][..., 0]), _f32(fr.starts[..., 0]), _f32(fr.ends[..., 0]), _f32(albedo),
                                                     _f32(normals), t_hit[s], who[s], hn[s], ha[s])
                mid = (s1.astype(np.float64) + e1) / 2.0  # nerfstudio's expected depth, clipped to the chunk's own bounds
                p2p = np.clip((w1 * mid).sum(1) / (w1.astype(np.float64).sum(1) + 1e-10), mid.min(), mid.max())
                rows.append(dict(p2p=p2p[:, None], w=w1.astype(np.float64), s=s1.astype(np.float64), e=e1.astype(np.float64), a=a1.astype(np.float64),
                                 n=n1.astype(np.float64), near=near, dirs=_f64(so["illumination_directions"]),
                                 cols=_f64(so["hdr_illumination_colours"])[0], bg=_f64(so["hdr_background_colours"])))
        finally:
            m.end_frame()
    cat = lambda k: np.concatenate([r[k] for r in rows])  # noqa: E731
    w, near = cat("w"), cat("near")
    keep = ~near
    print(f"the seam by hand: {int(near.sum())} of {N} rays have a midpoint within 4 ulp of t_hit and are left out")
    assert near.sum() <= 0.01 * N
    acc = w.sum(1)
    want = {"prop_weight": w[:, -1:], "accumulation": acc[:, None], "p2p_dist": cat("p2p")}
    nrm = (w[..., None] * cat("n")).sum(1)
    for k, ref in want.items():
        err = np.abs(_f64(got[k]).reshape(N, -1) - ref)[keep].max()
        print(f"the seam by hand: {k} max err {err:.3e}")
        assert err < BAR, k
    err = np.abs(_f64(got["normal"]).reshape(N, 3) - nrm)[keep].max()
    print(f"the seam by hand: normal max err {err:.3e}")
    assert err < BAR
    first = [int(((who == p) & (w[:, -1] > 0.5)).sum()) for p in range(3)]
    print(f"rays that enter a prop first with more than half their weight: A {first[0]} B {first[1]} C {first[2]}; entered at all "
          f"{[int((who == p).sum()) for p in range(3)]}")
    assert first[0] >= 20 and first[1] >= 10  # 40 and 20 on the analytic ball
    # under the sky alone: the hemisphere composite of the edited samples under visibility x restated occlusion
    plain_vis = []
    with torch.no_grad():
        m.begin_step()
        for a in range(0, N, CHUNK):
            s = slice(a, min(a + CHUNK, N))
            vd = m.compute_visibility_compact(flat.origins[s].contiguous(), flat.directions[s].contiguous(), got["p2p_dist"].reshape(N, 1)[s],
                                              torch.from_numpy(rows[0]["dirs"]).float().to(DEV), m.visibility_threshold, m.sigmoid_scale)
            plain_vis.append(_f64(vd["visibility"]))
    occ, ok = _occluded(rb, got, props, directions=rows[0]["dirs"].astype(np.float32))
    vis = np.where(occ, 0.0, np.concatenate(plain_vis))
    lin = _hemi_f64(cat("a"), cat("n"), w, rows[0]["dirs"], rows[0]["cols"], vis, cat("bg"))
    use = keep & ok.all(1)
    err = np.abs(_f64(got["lin"]).reshape(N, 3) - lin)[use].max()
    print(f"the seam by hand: lin max err {err:.3e} on {int(use.sum())} rays; the props shadow {int(occ.sum())} of {occ.size} sky entries")
    assert err < LIN_BAR and occ.sum() > 100


# ---------------------------------------------------------------- a hidden prop, a shadow caster only
def test_a_hidden_prop_leaves_the_frame(scene):
    _, _, render, _ = scene
    plain, got = render(display=DisplayTransform()), render(props=C, prop_bias=BIAS, display=DisplayTransform())
    entered = got["prop_id"] == 0
    opaque = plain["accumulation"] > 0.99
    pw = got["prop_weight"]
    print(f"hidden prop: entered by {int(entered.sum())} rays, {int((entered & opaque).sum())} of them opaque; largest prop_weight on an opaque "
          f"ray {float(pw[opaque].max()):.3e}; largest 1 - accumulation there {float((1 - plain['accumulation'][opaque]).max()):.3e}")
    assert int((entered & opaque).sum()) >= 10  # 20 on the analytic ball
    assert (pw[opaque] == 0).all()
    for k in ("lin", "accumulation", "albedo"):
        err = float((got[k] - plain[k]).abs()[opaque.expand_as(got[k])].max())
        print(f"hidden prop: {k} differs from the plain frame by at most {err:.3e} on the opaque rays")
        assert err <= CHUNK_BAR * max(1.0, float(plain[k].abs().max())), k


@pytest.mark.parametrize("mode", ("ddf", "sdf", "no visibility network"))
def test_a_shadow_caster_the_camera_does_not_see(scene, mode):
    pipe, rb, render, _ = scene
    m = pipe.model
    caster = dataclasses.replace(A, visible=False)
    kw = {"sun": SUN, "sun_shadows": "sdf" if mode == "sdf" else "ddf"}
    eager = mode == "no visibility network"  # (a chunk graph is not keyed on the flag, and none may be captured under it)
    if eager:
        m.config.use_visibility = False
    try:
        plain, got = render(use_graph=not eager, **kw), render(use_graph=not eager, props=caster, prop_bias=BIAS, **kw)
    finally:
        m.config.use_visibility = True
    assert (got["prop_id"] == -1).all() and (got["prop_weight"] == 0).all()
    for k in ("depth", "normal", "albedo", "accumulation"):
        assert float((got[k] - plain[k]).abs().max()) <= CHUNK_BAR * max(1.0, float(plain[k].abs().max())), k
    assert (got["shadow_map"] <= plain["shadow_map"]).all()
    occ, keep = _occluded(rb, got, [caster], directions=_sun_dirs([SUN]).numpy())
    shadowed = torch.from_numpy(occ[:, 0] & keep[:, 0]).to(DEV)
    lit_before = shadowed & (plain["shadow_map"].reshape(N) > 0.5)
    print(f"shadow caster only ({mode}): the restatement shadows {int(shadowed.sum())} rays, {int(lit_before.sum())} of them lit in the plain "
          f"frame; on the visible ball {int((shadowed & (plain['accumulation'].reshape(N) > 0.5)).sum())}")
    assert (got["shadow_map"].reshape(N)[shadowed] == 0).all()
    assert int((shadowed & (plain["accumulation"].reshape(N) > 0.5)).sum()) >= 36  # 72 on the analytic ball
    free = torch.from_numpy(~occ[:, 0] & keep[:, 0]).to(DEV)
    assert float((got["shadow_map"] - plain["shadow_map"]).reshape(N)[free].abs().max()) <= CHUNK_BAR


# ---------------------------------------------------------------- every mode
def _modes():
    sky = DaylightSky()
    g = torch.Generator().manual_seed(5)
    env = torch.rand(16, 32, 3, generator=g) * 2.0
    fog = Atmosphere(1.5, scale_height=0.3, base_height=-0.2, shaft_samples=2)
    return {
        "sky": {},
        "envmap": {"envmap": ("map", env), "rotation": z_rotation(0.7)},
        "one sun": {"sun": SUN},
        "two suns": {"sun": [SUN, SunLight(250.0, 15.0, (3.0, 2.0, 0.5))]},
        "daylight": {"daylight": sky, "sun": [sky.sun(130.0, 35.0)]},
        "sdf shadows": {"sun": SUN, "sun_shadows": "sdf"},
        "lamp": {"lights": LAMP},
        "fog shafts ddf": {"sun": SUN, "atmosphere": fog},
        "fog shafts sdf": {"sun": SUN, "atmosphere": fog, "sun_shadows": "sdf"},
        "display": {"sun": SUN, "display": DisplayTransform(curve="aces")},
    }


@pytest.mark.parametrize("name", list(_modes()))
def test_every_mode(scene, name):
    pipe, rb, render, _ = scene
    m = pipe.model
    kw = dict(_modes()[name])
    if "envmap" in kw:
        kw["envmap"] = EnvironmentMap(kw["envmap"][1], device=DEV)
        kw["rotation"] = kw["rotation"].to(DEV)
    props = [A, B, C] + ([D] if name == "lamp" else [])
    graph, eager = render(props=props, **kw), render(use_graph=False, props=props, **kw)
    assert set(graph) == set(eager) and {"prop_id", "prop_weight"} <= set(graph)
    for k, v in graph.items():
        if torch.is_tensor(v):
            assert torch.equal(v, eager[k]), (name, k)
    plain = render(**kw)
    assert not torch.equal(plain["rgb"], graph["rgb"]) and (graph["prop_weight"] > 0.5).sum() >= 30
    flat = rb.slice(0, 1 << 62)
    on = graph["accumulation"].reshape(N) > 0.0
    if name in ("one sun", "two suns", "sdf shadows"):
        suns = kw["sun"] if isinstance(kw["sun"], list) else [kw["sun"]]
        dirs = _sun_dirs(suns).to(DEV)
        K = len(suns)
        depth, normal = graph["p2p_dist"].reshape(N, 1), graph["normal"].reshape(N, 3)
        by_hand = []
        with torch.no_grad():
            m.begin_step()
            m.field.invalidate_weight_cache()
            for a in range(0, N, CHUNK):
                s = slice(a, min(a + CHUNK, N))
                o, d = flat.origins[s].contiguous(), flat.directions[s].contiguous()
                if name == "sdf shadows":
                    p = shadows.trace_settings(TRACE, shadows.SHADOW_DEFAULTS)
                    march = shadows.trace_sun_shadows(m.field, o, d, depth[s], normal[s].contiguous(), dirs, shadows.trace_params(p).to(DEV),
                                                      p["steps"], p["grace"])
                    by_hand.append(march.visibility.reshape(K, -1))
                else:
                    vd = m.compute_visibility_compact(o, d, depth[s], dirs, m.visibility_threshold, m.sigmoid_scale, compute_shadow_map=True,
                                                      sel=torch.arange(K, dtype=torch.int32, device=DEV))
                    by_hand.append(vd["visibility"].t())
        vis = torch.cat(by_hand, 1)  # [K, N]
        occ, keep = _occluded(rb, graph, props, directions=dirs.cpu().numpy())
        up = (dirs[:, 2] > 0)[:, None] & on[None]
        want = torch.where(up & ~torch.from_numpy(occ.T.copy()).to(DEV), vis, torch.zeros((), device=DEV))
        got = graph["shadow_map"].reshape(K, N)
        err = float((got - want).abs()[torch.from_numpy(keep.T.copy()).to(DEV)].max())
        print(f"{name}: shadow_map vs the query by hand x restated occlusion: max err {err:.3e}; props shadow {int((occ.T & _f32(up).astype(bool)).sum())}")
        assert err <= (0.0 if name == "sdf shadows" else float(m.sigmoid_scale) / 4.0 * 1e-5)
        assert (occ.T & _f32(up).astype(bool)).sum() >= 36
    if name == "lamp":
        from test_gpu_lights_frame import _march_by_hand
        vis, _ = _march_by_hand(m, rb, graph, [LAMP], TRACE)
        block = lights_block([LAMP]).numpy()
        occ, keep = _occluded(rb, graph, props, targets=block[:, 0:3], clearance=block[:, 9])
        want = torch.where(on & ~torch.from_numpy(occ[:, 0]).to(DEV), vis[0], torch.zeros((), device=DEV))
        k = torch.from_numpy(keep[:, 0]).to(DEV)
        assert torch.equal(graph["light_visibility"].reshape(N)[k], want[k])
        beyond = Prop("sphere", (0.3, 1.0, 0.2), 0.15)  # behind the lamp as the ball sees it, and outside the camera's view
        behind = render(props=beyond, lights=LAMP)
        ball = (plain["accumulation"].reshape(N) > 0.99) & (behind["prop_id"].reshape(N) < 0)
        occ_b, _ = _occluded(rb, behind, [beyond], targets=block[:, 0:3], clearance=block[:, 9])
        # (the appended zero sample may change a summation order, and with it a march's start point by a rounding)
        same = (behind["light_visibility"].reshape(N)[ball] - plain["light_visibility"].reshape(N)[ball]).abs() <= 1e-4
        print(f"lamp: props stand between {int(occ.sum())} points and the lamp; a prop behind the lamp changes {int((~same).sum())} of "
              f"{int(ball.sum())} visibilities on the ball")
        assert occ.sum() >= 10 and ball.sum() >= 100 and not occ_b[ball.cpu().numpy(), 0].any() and (~same).sum() <= 0.01 * ball.sum()
    if name.startswith("fog shafts"):
        caster = [dataclasses.replace(p, visible=False) for p in (A, B)]
        shade = render(props=caster, **kw)
        assert (shade["atmosphere_inscatter"] <= plain["atmosphere_inscatter"] + CHUNK_BAR).all()
        assert float((plain["atmosphere_inscatter"] - shade["atmosphere_inscatter"]).max()) > 1e-4  # the props' shafts


# ---------------------------------------------------------------- the shafts, by hand
@pytest.mark.parametrize("mode", ("ddf", "sdf", "no visibility network"))
def test_shaft_visibilities_are_the_query_by_hand_times_the_restated_occlusion(scene, mode):
    """the fogged prop frame is atmosphere_cpu's rule on the clear prop frame, fed V [M, K, N]: the frame's own shadow primitive by hand on
    the rows nsky_atmosphere_rows writes (ray r at the midpoint of segment m; ones on a model without a visibility field), times
    props_cpu.occlude from the rows' points, with no normal, along each sun.  A wrong row order, stride or subset of rows or suns moves
    the in-scatter by far more than the bar."""
    import atmosphere_cpu as FC
    from test_gpu_atmosphere_frame import _check, _frame_inputs, _shaft_visibilities
    pipe, rb, render, _ = scene
    m = pipe.model
    M, suns, props = 4, [SUN, SunLight(250.0, 15.0, (3.0, 2.0, 0.5))], [A, B, C]
    fog = Atmosphere((0.5, 1.0, 2.0), albedo=0.9, anisotropy=0.3, shaft_samples=M)
    kw = {"sun": suns, "sun_shadows": "sdf" if mode == "sdf" else "ddf", "props": props, "prop_bias": BIAS}
    bare = mode == "no visibility network"  # (eager: a chunk graph is not keyed on the flag, and none may be captured under it)
    if bare:
        m.config.use_visibility = False
    try:
        clear, fogged = render(use_graph=not bare, **kw), render(use_graph=not bare, atmosphere=fog, **kw)
        V = torch.ones(M, 2, N, device=DEV) if bare else _shaft_visibilities(m, rb, suns, M, fog.far, mode)
    finally:
        m.config.use_visibility = True
    o, d = _rays(rb)
    depths = FC.midpoints(fog.far, M).astype(np.float32)
    occ, keep = [], np.ones(N, bool)
    for t in depths:  # the rows' points as the frame forms them: o + d t in float32, the product and the sum rounded once each
        hit, margin = PC.occlude(o + d * t, None, BIAS, props_block(props).numpy(), directions=_sun_dirs(suns).numpy())
        occ.append(hit.T)
        keep &= (margin >= PC.MARGIN).all(1)
    occ = np.stack(occ)  # [M, K, N]
    assert (~keep).sum() <= 1e-3 * N
    inputs = _frame_inputs(m, rb, clear, suns)
    want = FC.apply(**inputs, vis=np.where(occ, 0.0, _f64(V)), params=_f64(fog.block()), M=M)
    unoccluded = FC.apply(**inputs, vis=_f64(V), params=_f64(fog.block()), M=M)
    for k in want:  # (a margin case may go either way: its ray takes the frame's own value)
        g = {"lin": "lin", "inscatter": "atmosphere_inscatter", "transmittance": "atmosphere_transmittance"}.get(k)
        if g is not None and not keep.all():
            want[k][..., ~keep, :] = _f64(fogged[g]).reshape(np.shape(want[k]))[..., ~keep, :]
    _check(f"prop shafts, {mode}", fogged, clear, want, (2,))
    moved = np.abs(unoccluded["inscatter"] - want["inscatter"]).max()
    print(f"prop shafts, {mode}: the props shadow {int(occ.sum())} of {occ.size} shaft entries ({int((~keep).sum())} rays left out); they move "
          f"the in-scatter by up to {moved:.3e}")
    assert occ.sum() >= 100 and moved > 100 * LIN_BAR


# ---------------------------------------------------------------- replay
def test_new_prop_values_replay_the_captured_chunk(scene):
    pipe, _, render, _ = scene
    m = pipe.model
    m.frames.runners.clear()  # (the cache holds four and starts again when it is full: from here the counts are certain)
    first = render(props=A, sun=SUN)
    render(use_graph=False, props=A, sun=SUN)  # (the eager runner, which every frame shares)
    runners = dict(m.frames.runners)
    n = len(runners)
    changed = [Prop("sphere", (0.2, 0.25, 0.35), 0.08), dataclasses.replace(A, size=0.12), dataclasses.replace(A, albedo=(0.1, 0.9, 0.9)),
               dataclasses.replace(A, visible=False), dataclasses.replace(A, casts_shadows=False),
               Prop("box", A.position, (0.05, 0.08, 0.06), yaw_deg=10.0), Prop("box", A.position, (0.05, 0.08, 0.06), yaw_deg=55.0)]
    for prop in changed:
        got = render(props=prop, sun=SUN)
        assert len(m.frames.runners) == n and all(m.frames.runners[k] is r for k, r in runners.items()), prop
        eager = render(use_graph=False, props=prop, sun=SUN)
        for k in ("rgb", "lin", "shadow_map", "prop_id", "prop_weight"):
            assert torch.equal(got[k], eager[k]), (prop, k)
        assert not torch.equal(got["lin"], first["lin"])
    got = render(props=A, sun=SUN, prop_bias=0.05)
    assert len(m.frames.runners) == n and all(m.frames.runners[k] is r for k, r in runners.items())
    assert torch.equal(got["shadow_map"], render(use_graph=False, props=A, sun=SUN, prop_bias=0.05)["shadow_map"])
    assert not torch.equal(got["shadow_map"], first["shadow_map"])
    two = render(props=[A, B], sun=SUN)  # the number of props is held by value: one new key
    new = [k for k in m.frames.runners if k not in runners]
    assert len(m.frames.runners) == n + 1 and len(new) == 1 and str(("props", 2)) in str(new[0]) and two["prop_id"].max().item() == 1
    assert all(str(("props", 1)) in str(k) for k in runners if k[1])  # (and the one-prop graph was keyed on its one prop)


# ---------------------------------------------------------------- the second passes
def _brute_force(render, bundle, sub, S, **kw):
    first = render(bundle=bundle, display=DisplayTransform(), **kw)
    total = {k: first[k].double() for k in ("lin", "albedo", "accumulation", "shadow_map", "prop_weight")}
    for s in range(S - 1):
        pick = lambda t: t[s::S - 1].reshape(H, W, -1).contiguous()  # noqa: E731
        bundle = RayBundle(pick(sub.origins), pick(sub.directions), pick(sub.pixel_area), pick(sub.camera_indices),
                           metadata={"directions_norm": pick(sub.metadata["directions_norm"])})
        out = render(bundle=bundle, display=DisplayTransform(), **kw)
        for k in total:
            total[k] += out[k].double()
    return first, {k: v / S for k, v in total.items()}


@pytest.mark.parametrize("second", ("antialias", "depth of field"))
def test_second_passes_resolve_the_props(scene, second):
    _, rb, render, _ = scene
    kw = dict(props=[A, B], sun=SUN)
    if second == "antialias":
        how = {"antialias": Antialias(4, every_pixel=True)}
        sub = subpixel_rays(rb, torch.arange(N, device=DEV), how["antialias"].sample_offsets(DEV))
    else:
        how = {"depth_of_field": DepthOfField(0.02, focus_distance=0.5, samples=4, every_pixel=True)}
        c2w = torch.from_numpy(AC.look_at(angle=0.13, radius=0.76, height=0.05)).float()  # a pinhole about where the grid's eye is
        rb = camera_rays(CameraPath(W, H, c2w[None], torch.tensor([55.0])), 0, DEV, camera_index=1)
        sub = lens_rays(rb, torch.arange(N, device=DEV), how["depth_of_field"])
    first, want = _brute_force(render, rb, sub, 4, **kw)
    got = render(bundle=rb, **kw, **how)
    assert (first["prop_weight"] > 0.5).sum() >= 30
    for k, ref in want.items():
        worst, scale = float((got[k].double() - ref).abs().max()), max(1.0, float(ref.abs().max()))
        print(f"{second}: {k} worst difference from the brute-force average {worst:.2e} (values up to {scale:.3g})")
        assert worst <= CHUNK_BAR * scale, k
    assert torch.equal(got["prop_id"], first["prop_id"])  # the centre ray's
    partial = lambda out: int(((out["prop_weight"] > 0.05) & (out["prop_weight"] < 0.95)).sum())  # noqa: E731
    assert partial(got) > partial(first)  # the props' edges are resolved


# ---------------------------------------------------------------- errors
def test_what_props_exclude_is_refused(scene):
    pipe, rb, render, _ = scene
    m = pipe.model
    with pytest.raises(ValueError):
        m.frames.begin(1, FrameLighting.of(bake="fp32"), props=A)
    assert m.frames.active is None
    with pytest.raises(ValueError):
        render(props=[A] * 65)
    with pytest.raises(TypeError):
        render(props=["sphere"])
    with pytest.raises(ValueError):
        render(props=A, prop_bias=-1.0)
    with pytest.raises(ValueError):
        Prop("sphere", (0, 0, 0), 0.0)
    with pytest.raises(ValueError):
        Prop("box", (0, 0, 0), (0.1, -0.1, 0.1))
    with pytest.raises(ValueError):
        Prop("sphere", (0, 0, 0), 0.1, visible=False, casts_shadows=False)
