"""The sphere-trace kernels (csrc/sphere_trace.hip) and relight.trace_visibility against the float64 restatement of the march rule
(sphere_trace_cpu.py): one `step` launch on hand-made states, one per branch of the rule, at the scalar and the 16-byte launch shape; the
step given bounds against the step without them, at every edge of its dispatch, and what it refuses; the whole march through the analytic plane-and-sphere scene at sizes on both sides of the shapes' divide; and the march through a model's
SDF field, whose first points are the rendered surface points lifted along their normals."""
import numpy as np
import pytest
import torch

import sphere_trace_cpu as ST
import test_gpu_lights as TL  # the hand-made rays of the step with bounds: a direction, a t_end and a tan_half each
from neusky_amd import hip
from neusky_amd.relight import shadows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ulps(got, ref64):
    """distance of fp32 `got` from the fp32 rounding of the float64 `ref64`, in ulps of that rounding"""
    ref32 = np.asarray(ref64, np.float64).astype(np.float32)
    return np.abs(got.astype(np.float64) - ref32.astype(np.float64)) / np.spacing(np.abs(ref32)).astype(np.float64)


# ---------------------------------------------------------------------------------------------- one step launch
# eps, relax, min_step, tan_half, radius, bias (fp32 values: the restatement reads the same numbers)
PARAMS = np.array([1e-3, 0.8, 1e-3, 0.05, 1.0, 0.0], np.float32)
GRACE, STEPS = 4, 10
# name: x, s, t, m, status, outside, f
RAYS = {
    "escapes: its next point is beyond the radius": ((0.9, 0.0, 0.0), (1.0, 0.0, 0.0), 0.05, 1.0, ST.ALIVE, 1, 0.2),
    "hit after it has been outside": ((0.1, 0.2, 0.3), (0.0, 0.6, 0.8), 0.3, 0.6, ST.ALIVE, 1, 5e-4),
    "inside and not yet out: a hit in grace only": ((0.1, 0.2, 0.3), (0.0, 0.6, 0.8), 0.004, 1.0, ST.ALIVE, 0, -2e-3),
    "penumbra: m falls to f / (t tan_half)": ((-0.2, 0.1, 0.0), (0.6, 0.0, 0.8), 0.5, 0.7, ST.ALIVE, 1, 0.01),
    "penumbra that does not beat the m it has": ((-0.2, 0.1, 0.0), (0.6, 0.0, 0.8), 0.5, 0.3, ST.ALIVE, 1, 0.01),
    "comes outside this round, and the penumbra sees it": ((0.0, 0.0, 0.1), (0.0, 0.0, 1.0), 0.2, 1.0, ST.ALIVE, 0, 0.002),
    "min_step floor (and no penumbra at t = 0)": ((0.3, 0.3, 0.0), (0.0, 0.6, 0.8), 0.0, 1.0, ST.ALIVE, 0, 1.1e-3),
    "a long step": ((-0.5, 0.0, 0.0), (1.0, 0.0, 0.0), 0.1, 1.0, ST.ALIVE, 1, 0.37),
    "dead: hit": ((0.1, 0.2, 0.3), (0.0, 0.6, 0.8), 0.25, 0.0, ST.HIT, 1, 0.3),
    "dead: escaped": ((0.5, 0.5, 0.5), (0.6, 0.0, 0.8), 0.4, 0.9, ST.ESCAPED, 1, -0.3),
    "dead: escaped before it was ever outside": ((0.5, 0.5, 0.5), (0.6, 0.0, 0.8), 0.4, 1.0, ST.ESCAPED, 0, 0.3),
}


def _hand_made(copies):
    rays = list(RAYS.values()) * copies
    col = lambda j, dt: np.array([r[j] for r in rays], dt)  # noqa: E731
    return col(0, np.float32), col(1, np.float32), col(2, np.float32), col(3, np.float32), col(4, np.int32), col(5, np.int32), col(6, np.float32)


def _state(x, t, m, status, outside):
    state = torch.empty(6, x.shape[0], device=DEV)
    state[:3] = torch.from_numpy(x.T.copy()).to(DEV)
    state[3], state[4] = torch.from_numpy(t).to(DEV), torch.from_numpy(m).to(DEV)
    state.view(torch.int32)[5] = torch.from_numpy(status | (outside << 8)).to(DEV)
    return state


@pytest.mark.parametrize("copies", (1, 4), ids=("11 rays: 4-byte accesses", "44 rays: 16-byte accesses"))
@pytest.mark.parametrize("it", (2, GRACE, STEPS - 1), ids=("in grace", "grace over", "last round"))
def test_one_step_on_hand_made_states(it, copies):
    x, s, t, m, status, outside, f = _hand_made(copies)
    T = x.shape[0]
    state = _state(x, t, m, status, outside)
    before = state.clone()
    points = torch.full((T, 3), 7.0, device=DEV)
    params = torch.from_numpy(PARAMS).to(DEV)
    dirs = torch.from_numpy(s).to(DEV)
    hip.sphere_trace_step(state, torch.from_numpy(f).to(DEV), dirs, 1, params, it, STEPS, GRACE, points)
    vis, t_out, st_out = torch.empty(T, device=DEV), torch.empty(T, device=DEV), torch.empty(T, dtype=torch.int8, device=DEV)
    hip.sphere_trace_finish(state, vis, st_out, t_out)
    torch.cuda.synchronize()

    P = PARAMS.astype(np.float64)
    t2, m2, status2, outside2 = ST.rule_step(f.astype(np.float64), it, t.astype(np.float64), m.astype(np.float64), status.astype(np.int8),
                                             outside.astype(bool), eps=P[0], relax=P[1], min_step=P[2], grace=GRACE, tan_half=P[3])
    p2, escaped = ST.escape(x.astype(np.float64), s.astype(np.float64), t2, status2, P[4])
    if it + 1 < STEPS:
        status2 = escaped
    got = state.cpu()
    flags = got[5].view(torch.int32).numpy()
    names = list(RAYS) * copies
    bad = [names[i] for i in range(T) if (flags[i] & 0xff) != status2[i] or (flags[i] >> 8) != int(outside2[i])]
    assert not bad, bad
    ut, um = _ulps(got[3].numpy(), t2), _ulps(got[4].numpy(), m2)
    scale = np.maximum(np.abs(p2), np.maximum(np.abs(x), np.abs(t2[:, None] * s)))
    up = np.abs(points.cpu().numpy().astype(np.float64) - p2) / np.spacing(scale.astype(np.float32)).astype(np.float64)
    print(f"round {it}, {T} rays: t {ut.max():.2f} ulp, m {um.max():.2f} ulp, points {up.max():.2f} ulp of their terms")
    assert ut.max() <= 4 and um.max() <= 4 and up.max() <= 4
    dead = status != ST.ALIVE
    assert torch.equal(got[:, dead], before.cpu()[:, dead]) and torch.equal(got[:3], before.cpu()[:3])  # a dead ray is left as it was
    # what the rule says of these rays, spelled out (round 2 is inside the leaving phase of 4)
    by = dict(zip(names[:len(RAYS)], zip(status2[:len(RAYS)], m2[:len(RAYS)], t2[:len(RAYS)])))
    assert by["escapes: its next point is beyond the radius"][0] == (ST.ESCAPED if it + 1 < STEPS else ST.ALIVE)
    assert by["hit after it has been outside"][:2] == (ST.HIT, 0.0)
    assert by["inside and not yet out: a hit in grace only"][0] == (ST.ALIVE if it < GRACE else ST.HIT)
    assert abs(by["penumbra: m falls to f / (t tan_half)"][1] - 0.4) < 1e-6 and abs(by["penumbra that does not beat the m it has"][1] - 0.3) < 1e-7
    assert abs(by["comes outside this round, and the penumbra sees it"][1] - 0.2) < 1e-6
    assert abs(by["min_step floor (and no penumbra at t = 0)"][2] - 1e-3) < 1e-9 and by["min_step floor (and no penumbra at t = 0)"][1] == 1.0
    # finish: m, t and the status, a ray still marching reported as exhausted
    assert torch.equal(vis.cpu(), got[4]) and torch.equal(t_out.cpu(), got[3])
    assert np.array_equal(st_out.cpu().numpy(), np.where(status2 == ST.ALIVE, ST.EXHAUSTED, status2).astype(np.int8))


# ---------------------------------------------------------------------------------------------- one step kernel, with and without bounds
def _lamp_rays(T):
    """the first T of the hand-made rays of test_gpu_lights, four times over -> state, sdf, directions [T, 3], bounds [2, T], params"""
    col = lambda j, dt: np.array([r[j] for r in list(TL.RAYS.values()) * 4][:T], dt)  # noqa: E731
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    state = _state(col(0, np.float32), col(2, np.float32), col(3, np.float32), col(4, np.int32), col(5, np.int32))
    return state, dev(col(6, np.float32)), dev(col(1, np.float32)), dev(np.stack([col(7, np.float32), col(8, np.float32)])), dev(TL.PARAMS)


def _step(state, sdf, dirs, bounds, params, it, dir_div=1):
    """one step on a copy of `state` -> the state and the points it leaves"""
    state, points = state.clone(), torch.full((state.shape[1], 3), 7.0, device=DEV)
    hip.sphere_trace_step(state, sdf, dirs, dir_div, params, it, TL.STEPS, TL.GRACE, points, bounds)
    return state, points


def _one_float_in(t):
    """`t` as a contiguous view that starts 4 bytes into a larger allocation: no 16-byte access may touch it"""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    out = buf[1:1 + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.is_contiguous() and out.data_ptr() % 16 == 4
    return out


@pytest.mark.parametrize("T", (11, 44), ids=("11 rays: 4-byte accesses", "44 rays: 16-byte accesses"))
@pytest.mark.parametrize("it", (2, TL.GRACE, TL.STEPS - 1), ids=("in grace", "grace over", "last round"))
def test_bounds_that_never_bind_are_the_step_without_them(it, T):
    """march_ray with t_end = +inf and each ray's tan_half equal to the block's computes the expressions of its unbounded branch"""
    state, sdf, dirs, _, params = _lamp_rays(T)
    bounds = torch.stack([torch.full((T,), float("inf"), device=DEV), params[3].expand(T)]).contiguous()
    with_bounds, without = _step(state, sdf, dirs, bounds, params, it), _step(state, sdf, dirs, None, params, it)
    assert torch.equal(with_bounds[0], without[0]) and torch.equal(with_bounds[1], without[1])
    assert not torch.equal(without[0], state) and not (without[1] == 7.0).any()  # (the step ran)


@pytest.mark.parametrize("it", (2, TL.STEPS - 1), ids=("in grace", "last round"))
def test_the_access_width_changes_no_result(it):
    state, sdf, dirs, bounds, params = _lamp_rays(44)
    wide = _step(state, sdf, dirs, bounds, params, it)
    plain = _step(state, sdf, dirs, None, params, it)
    assert not torch.equal(wide[0], plain[0])  # (these bounds bind)
    for name, args in (("bounds", (sdf, dirs, _one_float_in(bounds))), ("directions", (sdf, _one_float_in(dirs), bounds)),
                       ("sdf", (_one_float_in(sdf), dirs, bounds))):
        got = _step(state, *args, params, it)
        assert torch.equal(got[0], wide[0]) and torch.equal(got[1], wide[1]), name
    got = _step(state, _one_float_in(sdf), dirs, None, params, it)
    assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1])
    # 43 rays: no group of four; the rays are those of the 44-ray call
    got = _step(*_lamp_rays(43)[:4], params, it)
    assert torch.equal(got[0], wide[0][:, :43]) and torch.equal(got[1], wide[1][:43])
    got = _step(*_lamp_rays(43)[:3], None, params, it)
    assert torch.equal(got[0], plain[0][:, :43]) and torch.equal(got[1], plain[1][:43])


def test_the_step_refuses_bounds_it_cannot_take():
    state, sdf, dirs, bounds, params = _lamp_rays(44)
    before, points = state.clone(), torch.full((44, 3), 7.0, device=DEV)
    for d, dir_div, b in ((dirs[:22].contiguous(), 2, bounds),  # rays that share a direction
                          (dirs, 1, bounds.t().contiguous()),  # bounds [T, 2]
                          (dirs[:4].contiguous(), 1, bounds)):  # directions [K, 3]
        with pytest.raises(hip.NeuSkyHipError):
            hip.sphere_trace_step(state, sdf, d, dir_div, params, 2, TL.STEPS, TL.GRACE, points, b)
    torch.cuda.synchronize()
    assert torch.equal(state, before) and (points == 7.0).all()  # nothing was launched


# ---------------------------------------------------------------------------------------------- the whole march, analytic scene
S64 = ST.sun_direction()
STARTS = np.concatenate([ST.scene_starts(64, z) for z in (1e-2, 0.0, -5e-3)])  # [12288, 3]: the grid at the three start offsets
SIZES = (1, 63, 4096, 4097, 12288)  # one ray; a tail; the 64 x 64 grid (16-byte accesses); one more (4-byte ones); all offsets
DIAMETERS = (0.0, 0.533, 4.0)
_REF = {}


def _reference(deg):
    """the float64 march of all the start points, once per angular diameter; read, never written"""
    if deg not in _REF:
        _REF[deg] = ST.march(ST.scene_sdf, STARTS, S64, tan_half=ST.tan_half(deg))
    return _REF[deg]


def _torch_scene(points):
    c = torch.tensor(ST.CENTRE, dtype=torch.float32, device=points.device)
    return torch.minimum(points[:, 2], (points - c).norm(dim=1) - ST.SPHERE_RADIUS)


@pytest.mark.parametrize("deg", DIAMETERS)
@pytest.mark.parametrize("M", SIZES)
def test_trace_visibility_on_the_analytic_scene(M, deg):
    m64, status64, t64 = (a[:M] for a in _reference(deg))
    x = torch.from_numpy(STARTS[:M]).to(torch.float32).to(DEV)
    s = torch.from_numpy(S64).to(torch.float32).to(DEV)[None].expand(M, 3).contiguous()
    a = shadows.trace_visibility(_torch_scene, x, s, angular_diameter_deg=deg)
    b = shadows.trace_visibility(_torch_scene, x, s, angular_diameter_deg=deg)
    assert a.visibility.shape == (M,) and a.status.dtype == torch.int8 and a.t.dtype == torch.float32
    for u, v in zip(a, b):
        assert torch.equal(u, v)  # bitwise repeatable
    status, vis = a.status.cpu().numpy(), a.visibility.cpu().numpy().astype(np.float64)
    differ = status != status64
    same = ~differ
    err = np.abs(vis - m64)[same].max() if same.any() else 0.0
    print(f"M {M}, {deg} degrees: {int(differ.sum())} statuses differ, visibility differs by {err:.2e} on the others, "
          f"{int((status == ST.EXHAUSTED).sum())} exhausted")
    assert differ.sum() <= 0.005 * M
    assert err <= 1e-4
    assert vis.min() >= 0.0 and vis.max() <= 1.0 and (vis[status == ST.HIT] == 0.0).all()
    if deg == 0.0:
        assert np.array_equal(vis, np.where(status == ST.HIT, 0.0, 1.0))


def test_k_directions_over_m_points_are_k_marches():
    M = 63
    x = torch.from_numpy(STARTS[:M]).to(torch.float32).to(DEV)
    dirs = torch.tensor(np.stack([S64, ST.sun_direction(200.0, 15.0), ST.sun_direction(75.0, 80.0)]), dtype=torch.float32, device=DEV)
    many = shadows.trace_visibility(_torch_scene, x, dirs, angular_diameter_deg=4.0)
    assert many.visibility.shape == (3, M) and many.status.shape == (3, M) and many.t.shape == (3, M)
    for k in range(3):
        one = shadows.trace_visibility(_torch_scene, x, dirs[k][None].expand(M, 3), angular_diameter_deg=4.0)
        for u, v in zip(many, one):
            assert torch.equal(u[k], v), k
    assert not torch.equal(many.visibility[0], many.visibility[1])


def test_a_start_beyond_the_radius_escapes_at_once():
    x = torch.tensor([[0.9, 0.9, 0.1], [-0.5, -0.5, 0.3]], device=DEV)  # beyond the radius; inside it and lit
    s = torch.from_numpy(S64).to(torch.float32).to(DEV)[None].expand(2, 3)
    out = shadows.trace_visibility(_torch_scene, x, s)
    assert out.status.tolist() == [ST.ESCAPED, ST.ESCAPED] and out.t[0].item() == 0.0 and out.t[1].item() > 0.3
    assert out.visibility.tolist() == [1.0, 1.0]


def test_bad_arguments_are_refused():
    x = torch.zeros(4, 3, device=DEV)
    with pytest.raises(ValueError):
        shadows.trace_visibility(_torch_scene, x, x[:, :2])
    with pytest.raises(ValueError):
        shadows.trace_visibility(_torch_scene, x, x, steps=0)
    with pytest.raises(ValueError):
        shadows.trace_visibility(lambda p: p, x, x + 1.0, steps=2)  # [M, 3] is no sdf


# ---------------------------------------------------------------------------------------------- the model's field
def test_march_through_the_models_field():
    from util_shadows import grow_the_ball
    from util_step import randomise, small_pipeline_config
    torch.manual_seed(0)
    pipe = small_pipeline_config(R=16, D=32, images=4).setup(device=DEV)
    randomise(pipe)
    grow_the_ball(pipe)  # the start points lie about its surface, inside and outside
    pipe.eval()
    field = pipe.model.field
    R, K, steps = 150, 2, 16  # 300 shadow rays
    g = torch.Generator().manual_seed(11)
    o = (torch.rand(R, 3, generator=g) - 0.5) * 1.2
    d = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=1)
    depth = 0.1 + 0.4 * torch.rand(R, generator=g)
    n = torch.randn(R, 3, generator=g) * 0.7  # rendered normals are not unit vectors
    n[5] = 0.0  # and may be none at all
    suns = torch.tensor(np.stack([ST.sun_direction(130.0, 35.0), ST.sun_direction(20.0, 60.0)]), dtype=torch.float32)
    p = shadows.trace_settings({"steps": steps, "angular_diameter_deg": 2.0, "bias": 0.02}, shadows.SHADOW_DEFAULTS)
    params = shadows.trace_params(p)
    args = [t.to(DEV) for t in (o, d, depth, n, suns, params)]
    seen = []

    def recording(points):
        seen.append(points.clone())
        return field.get_sdf_at_pos(points).reshape(-1)

    field.invalidate_weight_cache()
    direct = shadows.trace_sun_shadows(field, *args, steps, p["grace"])
    wrapped = shadows.trace_sun_shadows(recording, *args, steps, p["grace"])
    for u, v in zip(direct, wrapped):
        assert torch.equal(u, v)
    assert direct.visibility.shape == (K, R) and len(seen) == steps
    # round 0 starts at o + depth d + bias n^ (the sun's direction where there is no normal)
    o64, d64, n64, s64 = o.double().numpy(), d.double().numpy(), n.double().numpy(), suns.double().numpy()
    nh = n64 / np.maximum(np.linalg.norm(n64, axis=1, keepdims=True), 1e-300)
    nh = np.broadcast_to(nh[None], (K, R, 3)).copy()
    nh[:, 5] = s64
    bias = float(params[5].double())
    surf = d64 * depth.double().numpy()[:, None]
    ref = o64[None] + surf[None] + bias * nh
    mag = np.maximum(np.maximum(np.abs(ref), np.abs(bias * nh)), np.maximum(np.abs(o64), np.abs(surf))[None])
    err = np.abs(seen[0].cpu().double().numpy().reshape(K, R, 3) - ref) / np.spacing(mag.astype(np.float32)).astype(np.float64)
    print(f"first points vs o + depth d + bias n^: {err.max():.2f} ulp of the coordinates' magnitude; statuses "
          f"{np.bincount(direct.status.cpu().numpy().reshape(-1), minlength=4).tolist()}")
    assert err.max() <= 2.0
    status = direct.status.cpu().numpy().reshape(-1)
    assert (status == ST.HIT).sum() >= 10 and (status == ST.ESCAPED).sum() >= 10  # the ball is there
    # later rounds move alive rays only, along their sun's direction
    moved = (seen[1] - seen[0]).reshape(K, R, 3)
    assert (torch.linalg.cross(moved, args[4][:, None].expand(K, R, 3)).norm(dim=-1) < 1e-6).all()
