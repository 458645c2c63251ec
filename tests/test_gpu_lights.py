"""The kernels of point and spot lights (csrc/lights.hip, the bounded step of csrc/sphere_trace.hip) and relight.trace_visibility_to
against the float64 restatement of their rules (lights_cpu.py): the transfer within its stated bound at sizes about every edge of its
launch shape, one bounded step on hand-made states at both access widths, the begin of the shadow rays, the whole march through the
analytic plane-and-sphere scene, and the composite."""
import numpy as np
import pytest
import torch

import lights_cpu as LC
import sphere_trace_cpu as ST
import sun_cpu
from neusky_amd import hip
from neusky_amd.relight import PointLight, lights, lights_block, shadows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ulps(got, ref64, scale=None):
    """distance of fp32 `got` from the fp32 rounding of the float64 `ref64`, in ulps of that rounding; with `scale`: from `ref64` itself,
    in fp32 ulps of `scale` (the magnitude of the terms it is formed from)"""
    ref64 = np.asarray(ref64, np.float64)
    if scale is None:
        ref32 = ref64.astype(np.float32)
        return np.abs(got.astype(np.float64) - ref32.astype(np.float64)) / np.spacing(np.abs(ref32)).astype(np.float64)
    return np.abs(got.astype(np.float64) - ref64) / np.spacing(np.abs(np.asarray(scale, np.float64)).astype(np.float32)).astype(np.float64)


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


# ---------------------------------------------------------------------------------------------- transfer
def _mixed_lights(L, g):
    """points and spots by turns, inside the unit ball"""
    out = []
    for l in range(L):  # noqa: E741
        p = g.uniform(-0.6, 0.6, 3)
        kw = dict(position=p, intensity=g.uniform(0.5, 3.0, 3), radius=float(g.uniform(0.0, 0.05)))
        if l % 2:
            kw.update(direction=g.normal(size=3), inner_deg=float(g.uniform(5, 40)), outer_deg=float(g.uniform(40, 120)))
        out.append(PointLight(**kw))
    return out


# one ray; a sample tail; a full pass of 8 lights; a pass boundary; rays across workgroups; then the pass rule and the ray loop the kernel
# shares with the suns' (a full pass, a pass of one behind it, two passes and one) at R = 5 (a second workgroup with one live wave) and
# S = 65 (one sample behind a full lane stride)
@pytest.mark.parametrize("R, S, L", ((1, 1, 1), (3, 63, 1), (65, 96, 8), (17, 65, 9), (257, 24, 3), (5, 65, 8), (5, 65, 9), (5, 65, 17)))
def test_transfer_is_within_its_bound(R, S, L):
    g = np.random.default_rng(100 * R + S + L)
    x = g.normal(size=(R, S, 3))
    x = (x / np.linalg.norm(x, axis=-1, keepdims=True) * g.random((R, S, 1)) ** (1 / 3)).astype(np.float32)  # in the unit ball
    alb = g.random((R, S, 3)).astype(np.float32)
    n = (g.normal(size=(R, S, 3)) * 0.7).astype(np.float32)
    w = (g.random((R, S)) / S).astype(np.float32)
    block = lights_block(_mixed_lights(L, g)).numpy().copy()
    block[0, :3] = x[0, 0]  # this light sits exactly on a sample
    r1, s1 = R - 1, S - 1
    if (r1, s1) != (0, 0):  # and this sample lies inside the last light's min_distance (>= 0.01)
        x[r1, s1] = block[L - 1, :3] + np.float32(0.003)
        assert 0.0 < np.linalg.norm(x[r1, s1].astype(np.float64) - block[L - 1, :3]) < block[L - 1, 10]
    ref, scale = LC.transfer(x, alb, n, w, block)
    args = [_dev(v) for v in (x, alb, n, w, block)]
    out, again = torch.full((L, R, 3), 7.0, device=DEV), torch.empty(L, R, 3, device=DEV)
    hip.light_transfer(*args, out)
    hip.light_transfer(*args, again)
    assert torch.equal(out, again)  # bitwise repeatable
    got = out.cpu().numpy().astype(np.float64)
    bound = (3 + S / 64 + 6) * 2.0 ** -24 * scale
    err = np.abs(got - ref)
    worst = (err / np.maximum(bound, 1e-300)).max() if bound.max() > 0 else 0.0
    print(f"R {R}, S {S}, L {L}: largest error {err.max():.2e}, {worst:.3f} of its bound; largest entry {np.abs(ref).max():.2e}")
    assert np.isfinite(got).all() and (err <= bound).all()
    if (R, S) == (1, 1):
        assert got.tolist() == [[[0.0, 0.0, 0.0]]]  # the only sample is at the lamp


# ---------------------------------------------------------------------------------------------- one bounded step
# eps, relax, min_step, tan_half (of the sun's march: not read here), radius, bias; relax is a power of two: t + |f| relax is exact
PARAMS = np.array([1e-3, 0.5, 1e-3, 0.3, 1.0, 0.0], np.float32)
GRACE, STEPS = 4, 10
NEXT = float(np.nextafter(np.float32(0.375), np.float32(1.0)))
# name: x, s, t, m, status, outside, f, t_end, tan_half
RAYS = {
    "reaches t_end this round": ((0.0, 0.0, 0.1), (0.0, 0.6, 0.8), 0.25, 1.0, LC.ALIVE, 1, 0.25, 0.375, 0.0),
    "one ulp short of t_end": ((0.0, 0.0, 0.1), (0.0, 0.6, 0.8), 0.25, 1.0, LC.ALIVE, 1, 0.25, NEXT, 0.0),
    "penumbra of a narrow source": ((-0.2, 0.1, 0.0), (0.6, 0.0, 0.8), 0.5, 0.7, LC.ALIVE, 1, 0.01, 5.0, 0.05),
    "penumbra of a wide source": ((-0.2, 0.1, 0.0), (0.6, 0.0, 0.8), 0.5, 0.7, LC.ALIVE, 1, 0.01, 5.0, 0.1),
    "a point source has no penumbra": ((-0.2, 0.1, 0.0), (0.6, 0.0, 0.8), 0.5, 0.7, LC.ALIVE, 1, 0.01, 5.0, 0.0),
    "escapes: its next point is beyond the radius": ((0.9, 0.0, 0.0), (1.0, 0.0, 0.0), 0.05, 1.0, LC.ALIVE, 1, 0.4, 5.0, 0.02),
    "hit after it has been outside": ((0.1, 0.2, 0.3), (0.0, 0.6, 0.8), 0.3, 0.6, LC.ALIVE, 1, 5e-4, 5.0, 0.02),
    "inside and not yet out: a hit in grace only": ((0.1, 0.2, 0.3), (0.0, 0.6, 0.8), 0.004, 1.0, LC.ALIVE, 0, -2e-3, 5.0, 0.02),
    "dead: hit": ((0.1, 0.2, 0.3), (0.0, 0.6, 0.8), 0.25, 0.0, LC.HIT, 1, 0.3, 0.1, 0.02),
    "dead: escaped at its light": ((0.5, 0.5, 0.5), (0.6, 0.0, 0.8), 0.4, 0.9, LC.ESCAPED, 1, -0.3, 0.4, 0.02),
    "dead: escaped before it was ever outside": ((0.5, 0.5, 0.5), (0.6, 0.0, 0.8), 0.4, 1.0, LC.ESCAPED, 0, 0.3, 0.4, 0.0),
}


@pytest.mark.parametrize("copies", (1, 4), ids=("11 rays: 4-byte accesses", "44 rays: 16-byte accesses"))
@pytest.mark.parametrize("it", (2, GRACE, STEPS - 1), ids=("in grace", "grace over", "last round"))
def test_one_bounded_step_on_hand_made_states(it, copies):
    rays = list(RAYS.values()) * copies
    col = lambda j, dt: np.array([r[j] for r in rays], dt)  # noqa: E731
    x, s, t, m, status, outside, f = col(0, np.float32), col(1, np.float32), col(2, np.float32), col(3, np.float32), col(4, np.int32), \
        col(5, np.int32), col(6, np.float32)
    t_end, tan_half = col(7, np.float32), col(8, np.float32)
    T = x.shape[0]
    state = torch.empty(6, T, device=DEV)
    state[:3] = _dev(x.T)
    state[3], state[4] = _dev(t), _dev(m)
    state.view(torch.int32)[5] = _dev(status | (outside << 8), torch.int32)
    before = state.clone()
    points = torch.full((T, 3), 7.0, device=DEV)
    bounds = _dev(np.stack([t_end, tan_half]))
    hip.sphere_trace_step(state, _dev(f), _dev(s), 1, _dev(PARAMS), it, STEPS, GRACE, points, bounds)
    torch.cuda.synchronize()

    P, d = PARAMS.astype(np.float64), np.float64
    t2, m2, status2, outside2 = LC.rule_step(f.astype(d), it, t.astype(d), m.astype(d), status.astype(np.int8), outside.astype(bool),
                                             tan_half.astype(d), eps=P[0], relax=P[1], min_step=P[2], grace=GRACE)
    p2, escaped = LC.escape(x.astype(d), s.astype(d), t2, status2, P[4], t_end.astype(d))
    if it + 1 < STEPS:
        status2 = escaped
    got = state.cpu()
    flags = got[5].view(torch.int32).numpy()
    names = list(RAYS) * copies
    bad = [names[i] for i in range(T) if (flags[i] & 0xff) != status2[i] or (flags[i] >> 8) != int(outside2[i])]
    assert not bad, bad
    ut, um = _ulps(got[3].numpy(), t2), _ulps(got[4].numpy(), m2)
    scale = np.maximum(np.abs(p2), np.maximum(np.abs(x), np.abs(t2[:, None] * s)))
    up = _ulps(points.cpu().numpy(), p2, scale)
    print(f"round {it}, {T} rays: t {ut.max():.2f} ulp, m {um.max():.2f} ulp, points {up.max():.2f} ulp of their terms")
    assert ut.max() <= 4 and um.max() <= 4 and up.max() <= 4
    dead = status != LC.ALIVE
    assert torch.equal(got[:, dead], before.cpu()[:, dead]) and torch.equal(got[:3], before.cpu()[:3])  # a dead ray is left as it was
    by = dict(zip(names[:len(RAYS)], zip(status2[:len(RAYS)], m2[:len(RAYS)], t2[:len(RAYS)])))
    last = it + 1 >= STEPS
    assert by["reaches t_end this round"][0] == (LC.ALIVE if last else LC.ESCAPED) and by["reaches t_end this round"][2] == 0.375
    assert by["one ulp short of t_end"][0] == LC.ALIVE and by["one ulp short of t_end"][2] == 0.375
    assert abs(by["penumbra of a narrow source"][1] - 0.4) < 1e-6 and abs(by["penumbra of a wide source"][1] - 0.2) < 1e-6
    assert by["a point source has no penumbra"][1] == np.float64(np.float32(0.7))
    assert by["escapes: its next point is beyond the radius"][0] == (LC.ALIVE if last else LC.ESCAPED)
    assert by["hit after it has been outside"][:2] == (LC.HIT, 0.0)
    assert by["inside and not yet out: a hit in grace only"][0] == (LC.ALIVE if it < GRACE else LC.HIT)


# ---------------------------------------------------------------------------------------------- the begin
def _begin_buffers(T):
    return (torch.empty(6, T, device=DEV), torch.empty(T, 3, device=DEV), torch.empty(T, 3, device=DEV), torch.empty(2, T, device=DEV))


def test_the_begin_of_the_shadow_rays():
    g = torch.Generator().manual_seed(11)
    R = 150
    o = (torch.rand(R, 3, generator=g) - 0.5) * 1.2
    d = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=1)
    depth = 0.1 + 0.4 * torch.rand(R, generator=g)
    n = torch.randn(R, 3, generator=g) * 0.7  # rendered normals are not unit vectors
    n[5] = 0.0  # and may be none at all
    n[6, 1] = float("nan")
    block = lights_block([PointLight((0.2, -0.3, 0.5), (1, 1, 1), radius=0.04), PointLight((-0.9, 0.9, 0.9), (1, 1, 1), clearance=0.3)])
    L = 2
    p = shadows.trace_settings({"bias": 0.02}, lights.LIGHT_TRACE_DEFAULTS)
    params = shadows.trace_params(p)
    state, points, ray_dirs, bounds = _begin_buffers(L * R)
    hip.light_trace_begin(*(v.to(DEV) for v in (o, d, depth, n, block, params)), state, points, ray_dirs, bounds)
    torch.cuda.synchronize()
    x = state[:3].t().cpu().numpy()
    assert np.array_equal(x, points.cpu().numpy()) and (state[3] == 0).all() and (state[4] == 1).all()
    # x = o + depth d + bias n^, the direction to the lamp where there is no normal
    b64 = block.double().numpy()
    o64, d64, n64, t64 = o.double().numpy(), d.double().numpy(), n.double().numpy(), depth.double().numpy()
    x64, s64, t_end64, tan64, st64 = LC.begin(b64, 1.0, origins=o64, directions=d64, depth=t64, normals=n64, bias=float(params[5].double()))
    surf = t64[:, None] * d64
    mag = np.maximum(np.maximum(np.abs(x64.reshape(L, R, 3)), float(params[5])), np.maximum(np.abs(o64), np.abs(surf))[None]).reshape(L * R, 3)
    ux = _ulps(x, x64, mag)
    lift = (x.astype(np.float64) - (o64 + surf)[None].repeat(L, 0).reshape(L * R, 3)).reshape(L, R, 3)
    to = b64[:, None, :3] - (o64 + surf)[None]
    for r in (5, 6):  # lifted straight towards each lamp
        cos = (lift[:, r] * to[:, r]).sum(-1) / (np.linalg.norm(lift[:, r], axis=-1) * np.linalg.norm(to[:, r], axis=-1))
        assert (cos > 1.0 - 1e-4).all() and np.allclose(np.linalg.norm(lift[:, r], axis=-1), 0.02, rtol=1e-3), (r, cos)
    # s, t_end, tan_half: formed in fp64 from the start point the kernel wrote, and rounded once
    pl = np.repeat(b64, R, axis=0)
    v = pl[:, :3] - x.astype(np.float64)
    ln = np.linalg.norm(v, axis=1)
    us = _ulps(ray_dirs.cpu().numpy(), v / ln[:, None], np.ones_like(v))
    ut = _ulps(bounds[0].cpu().numpy(), ln - pl[:, 9], np.maximum(ln, pl[:, 9]))
    uh = _ulps(bounds[1].cpu().numpy(), pl[:, 8] / ln)
    uh = np.where(pl[:, 8] > 0.0, uh, 0.0)
    assert (bounds[1].cpu().numpy()[pl[:, 8] == 0.0] == 0.0).all()
    status = state[5].view(torch.int32).cpu().numpy()
    print(f"begin: x {ux.max():.2f}, s {us.max():.2f}, t_end {ut.max():.2f}, tan_half {uh.max():.2f} ulp of their terms; "
          f"statuses {np.bincount(status, minlength=4).tolist()}")
    assert ux.max() <= 2 and us.max() <= 2 and ut.max() <= 2 and uh.max() <= 2
    norm = np.linalg.norm(x.astype(np.float64), axis=1)
    want = np.where((bounds[0].cpu().numpy() <= 0.0) | (norm >= 1.0), LC.ESCAPED, LC.ALIVE)
    clear = np.abs(norm - 1.0) > 1e-6  # (the kernel's |x|^2 is an fp32 sum: a start within its rounding of the radius may fall either way)
    assert np.array_equal(status[clear], want[clear]) and (status == st64).mean() >= 0.99
    assert (status == LC.ALIVE).sum() >= 100 and (status == LC.ESCAPED).sum() >= 5


def test_a_start_at_its_lamp():
    starts = torch.tensor([[0.25, -0.5, 0.125], [0.25, -0.5, 0.0], [0.9, 0.9, 0.0]], device=DEV)
    block = lights_block(PointLight((0.25, -0.5, 0.125), (1, 1, 1), radius=0.05, clearance=0.05)).to(DEV)
    params = shadows.trace_params(shadows.trace_settings(None, lights.LIGHT_TRACE_DEFAULTS)).to(DEV)
    state, points, ray_dirs, bounds = _begin_buffers(3)
    hip.light_trace_begin_points(starts, block, params, state, points, ray_dirs, bounds)
    assert torch.equal(points, starts) and torch.equal(state[:3].t(), starts)
    assert ray_dirs[0].tolist() == [0.0, 0.0, 1.0] and bounds[:, 0].tolist() == [0.0, 0.0]  # len == 0
    assert ray_dirs[1].tolist() == [0.0, 0.0, 1.0] and bounds[0, 1].item() == np.float32(0.125 - np.float64(np.float32(0.05)))
    assert bounds[1, 1].item() == np.float32(np.float64(np.float32(0.05)) / 0.125)
    assert state[5].view(torch.int32).tolist() == [LC.ESCAPED, LC.ALIVE, LC.ESCAPED]  # at the lamp; marching; beyond the radius
    out = lights.trace_visibility_to(lambda p: p[:, 2] + 1.0, starts, block)
    assert out.status.tolist() == [[LC.ESCAPED] * 3] and out.visibility.tolist() == [[1.0] * 3] and out.t[0, 0].item() == 0.0


# ---------------------------------------------------------------------------------------------- the whole march, analytic scene
LAMPS = {"above": (0.1, -0.05, 0.9), "under": (0.1, -0.05, 0.08), "low side": (-0.45, 0.3, 0.15), "outside the collider": (0.9, 0.9, 0.9)}
RHOS = (0.0, 0.02, 0.08)
STARTS = np.concatenate([ST.scene_starts(32, z) for z in (1e-2, 0.0, -5e-3)])[:1025]  # the 32 x 32 grid, and one point of the next height
SIZES = (1, 63, 1024, 1025)  # one ray; a tail; the grid (16-byte accesses); one more (4-byte ones)
_REF = {}


def _lamp(name, rho):
    return PointLight(LAMPS[name], (1, 1, 1), radius=rho, clearance=rho)


def _reference(name, rho):
    """the float64 march of all the start points, once per lamp; read, never written"""
    if (name, rho) not in _REF:
        _REF[name, rho] = LC.march_to(ST.scene_sdf, STARTS, lights_block(_lamp(name, rho)).double().numpy())
    return _REF[name, rho]


def _torch_scene(points):
    c = torch.tensor(ST.CENTRE, dtype=torch.float32, device=points.device)
    return torch.minimum(points[:, 2], (points - c).norm(dim=1) - ST.SPHERE_RADIUS)


@pytest.mark.parametrize("rho", RHOS)
@pytest.mark.parametrize("name", LAMPS)
@pytest.mark.parametrize("M", SIZES)
def test_trace_visibility_to_on_the_analytic_scene(M, name, rho):
    m64, status64, t64, _ = (a[0, :M] for a in _reference(name, rho))
    x = _dev(STARTS[:M])
    a = lights.trace_visibility_to(_torch_scene, x, _lamp(name, rho))
    b = lights.trace_visibility_to(_torch_scene, x, _lamp(name, rho))
    assert a.visibility.shape == (1, M) and a.status.dtype == torch.int8 and a.t.dtype == torch.float32
    for u, v in zip(a, b):
        assert torch.equal(u, v)  # bitwise repeatable
    status, vis = a.status[0].cpu().numpy(), a.visibility[0].cpu().numpy().astype(np.float64)
    differ = status != status64
    same = ~differ
    err = np.abs(vis - m64)[same].max() if same.any() else 0.0
    print(f"M {M}, {name}, rho {rho}: {int(differ.sum())} statuses differ, visibility differs by {err:.2e} on the others, "
          f"{int((status == LC.EXHAUSTED).sum())} exhausted")
    assert differ.sum() <= 0.005 * M
    assert err <= 1e-4
    assert vis.min() >= 0.0 and vis.max() <= 1.0 and (vis[status == LC.HIT] == 0.0).all()
    if rho == 0.0:
        assert np.array_equal(vis, np.where(status == LC.HIT, 0.0, 1.0))
    if name == "under":
        assert (status == LC.ESCAPED).all()


def test_geometry_behind_a_lamp_does_not_shadow_it():
    M = 1024
    x = _dev(STARTS[:M])
    out = lights.trace_visibility_to(_torch_scene, x, _lamp("under", 0.0))
    assert (out.status == LC.ESCAPED).all() and (out.visibility == 1.0).all()
    v = torch.tensor(LAMPS["under"], dtype=torch.float64, device=DEV) - x.double()
    dirs = (v / v.norm(dim=1, keepdim=True)).float()
    unbounded = shadows.trace_visibility(_torch_scene, x, dirs)
    hits = int((unbounded.status == ST.HIT).sum())
    print(f"the unbounded march reports HIT on {hits} of {M} rays that see the lamp")
    assert hits >= 1


def test_l_lamps_over_m_points_are_l_marches():
    M = 63
    x = _dev(STARTS[:M])
    lamps = [_lamp(name, rho) for name, rho in zip(LAMPS, (0.08, 0.0, 0.02, 0.08))]
    many = lights.trace_visibility_to(_torch_scene, x, lamps)
    assert many.visibility.shape == (4, M) and many.status.shape == (4, M) and many.t.shape == (4, M)
    for l, lamp in enumerate(lamps):  # noqa: E741
        one = lights.trace_visibility_to(_torch_scene, x, lamp)
        for u, v in zip(many, one):
            assert torch.equal(u[l], v[0]), l
    assert not torch.equal(many.visibility[0], many.visibility[3])
    with pytest.raises(ValueError):
        lights.trace_visibility_to(_torch_scene, x, [lamps[0]] * 65)
    with pytest.raises(ValueError):
        lights.trace_visibility_to(_torch_scene, x[:, :2], lamps)


# ---------------------------------------------------------------------------------------------- composite
@pytest.mark.parametrize("given", (False, True), ids=("vis NULL", "vis given"))
@pytest.mark.parametrize("R", (1, 65, 1000))
@pytest.mark.parametrize("L", (1, 9))
@pytest.mark.parametrize("Kb, strided", ((1, False), (1, True), (3, False), (3, True)),
                         ids=("one image", "one image [1,R,3]", "one base under 3 images", "3 bases"))
def test_composite(Kb, strided, L, R, given):
    g = np.random.default_rng(7 * R + L + Kb)
    base = (g.random((Kb, R, 3) if strided else (R, 3)) * 2.0).astype(np.float32)
    t = (g.random((L, R, 3)) * 3.0).astype(np.float32)
    vis = g.random((L, R)).astype(np.float32) if given else None
    acc = g.random(R).astype(np.float32)
    acc[0] = 0.5  # exactly at the threshold: not above it
    thr = np.float32(0.5)
    block = lights_block(_mixed_lights(L, g)).numpy()
    rgb64, lin64, E64, V64 = LC.composite(base, t, vis, acc, thr, block)
    lin64 = np.broadcast_to(lin64, (Kb, R, 3))
    rgb, lin = torch.empty(Kb, R, 3, device=DEV), torch.empty(Kb, R, 3, device=DEV)
    light_lin, V = torch.empty(R, 3, device=DEV), torch.empty(L, R, device=DEV)
    args = (_dev(base), _dev(t), None if vis is None else _dev(vis), _dev(acc), _dev(np.array([thr])), _dev(block))
    hip.lights_composite(*args, rgb, lin, light_lin, V)
    rgb2 = torch.empty_like(rgb)
    hip.lights_composite(*args, rgb2)  # the optional outputs left out
    assert torch.equal(rgb, rgb2)
    assert np.array_equal(V.cpu().numpy().astype(np.float64), V64) and (V64[:, acc <= thr] == 0.0).all()
    assert R == 1 or ((acc > thr).any() and (acc < thr).any())  # rays on both sides of the threshold, and one on it
    ul, ue = _ulps(lin.cpu().numpy(), lin64), _ulps(light_lin.cpu().numpy(), E64)
    print(f"Kb {Kb}, L {L}, R {R}: lin {ul.max():.2f} ulp, light_lin {ue.max():.2f} ulp")
    assert ul.max() <= 1 and ue.max() <= 1
    want = sun_cpu.linear_to_srgb(lin.cpu().numpy().astype(np.float64))
    assert np.allclose(rgb.cpu().numpy(), want, rtol=1e-4, atol=1e-6)
    # no intensity: the base's bits
    dark = block.copy()
    dark[:, 12:15] = 0.0
    hip.lights_composite(*args[:5], _dev(dark), rgb, lin, light_lin, V)
    assert torch.equal(lin, args[0].expand(Kb, R, 3) if not strided else args[0]) and (light_lin == 0).all()
