"""numpy restatement of the point and spot lights (include/neusky_hip.h, "Point and spot lights inside the scene"): transfer, the begin
of the shadow rays, the bounded march and the composite, the reference the kernels of csrc/lights.hip, the bounded step of
csrc/sphere_trace.hip and the frame render with `lights=` are tested against, in float64 (or, with dtype=, in float32, to see what the
number format alone does).  It marches through sphere_trace_cpu's analytic scene.  Nothing here imports the package."""
import numpy as np

import sphere_trace_cpu as ST

ALIVE, HIT, ESCAPED, EXHAUSTED = ST.ALIVE, ST.HIT, ST.ESCAPED, ST.EXHAUSTED
# columns of a light's row
P, A, COS_INNER, COS_OUTER, RHO, CLEARANCE, MIN_DISTANCE, I = slice(0, 3), slice(3, 6), 6, 7, 8, 9, 10, slice(12, 15)


def light_row(p, intensity=(1.0, 1.0, 1.0), rho=0.0, clearance=None, min_distance=None, axis=None, inner_deg=None, outer_deg=None):
    """one row [16] in float64, with the defaults clearance = max(rho, 0.02), min_distance = max(rho, 0.01) and no cone"""
    row = np.zeros(16)
    row[P], row[I], row[RHO] = p, intensity, rho
    row[CLEARANCE] = max(rho, 0.02) if clearance is None else clearance
    row[MIN_DISTANCE] = max(rho, 0.01) if min_distance is None else min_distance
    if axis is None:
        row[A], row[COS_INNER], row[COS_OUTER] = (0.0, 0.0, -1.0), -1.0, -1.0
    else:
        a = np.asarray(axis, np.float64)
        row[A] = a / np.linalg.norm(a)
        row[COS_INNER], row[COS_OUTER] = np.cos(np.radians(np.float64(inner_deg))), np.cos(np.radians(np.float64(outer_deg)))
    return row


def spot(c, cos_inner, cos_outer):
    """the cone's factor at c = -<u, a>: 1 at and above cos_inner, else 0 at and below cos_outer, else the smoothstep; in this order"""
    c = np.asarray(c, np.float64)
    out = np.ones_like(c)
    rest = ~(c >= cos_inner)
    dark = rest & (c <= cos_outer)
    mid = rest & ~dark
    out[dark] = 0.0
    if mid.any():
        h = (c[mid] - cos_outer) / (cos_inner - cos_outer)
        out[mid] = h * h * (3.0 - 2.0 * h)
    return out


def factor(positions, normals, light):
    """cosine g [..]: positions, normals [.., 3]; light: a row"""
    x, n, q_ = np.asarray(positions, np.float64), np.asarray(normals, np.float64), np.asarray(light, np.float64)
    v = q_[P] - x
    q = (v * v).sum(-1)
    safe = np.where(q > 0.0, q, 1.0)
    u = v / np.sqrt(safe)[..., None]
    cosine = np.clip((n * u).sum(-1), 0.0, 1.0)
    c = -(u * q_[A]).sum(-1)
    g = spot(c, q_[COS_INNER], q_[COS_OUTER]) / np.maximum(safe, q_[MIN_DISTANCE] ** 2)
    return np.where(q > 0.0, cosine * g, 0.0)


def transfer(positions, albedo, normals, weights, lights):
    """positions, albedo, normals [R,S,3]; weights [R,S]; lights [L,16] -> t [L,R,3] and the tolerance scale
    sum_s |weights albedo| cosine g [L,R,3]"""
    a, w = np.asarray(albedo, np.float64), np.asarray(weights, np.float64)
    f = np.stack([factor(positions, normals, q) for q in np.asarray(lights, np.float64)])  # [L,R,S]
    return np.einsum("lrs,rs,rsc->lrc", f, w, a), np.einsum("lrs,rs,rsc->lrc", f, np.abs(w), np.abs(a))


def begin(lights, radius, *, starts=None, origins=None, directions=None, depth=None, normals=None, bias=0.0, dtype=np.float64):
    """the shadow rays i = l R + r of L lights over R start points (`starts`, or o + depth d + bias n^ with a zero or non-finite normal
    replaced by the unit vector to the light) -> x, s [L R, 3], t_end, tan_half [L R], status [L R] (rule step 1 of iteration 0).
    s, t_end and tan_half are formed in float64 from x in `dtype`, and rounded to it once."""
    q = np.asarray(lights, dtype).astype(np.float64)  # (the lights as the device holds them when dtype is float32)
    L = q.shape[0]
    if starts is not None:
        x = np.broadcast_to(np.asarray(starts, dtype)[None], (L,) + np.asarray(starts).shape).copy()
    else:
        o, d, t, n = (np.asarray(v, dtype) for v in (origins, directions, depth, normals))
        surf = o + t[:, None] * d
        nn = (n.astype(np.float64) ** 2).sum(1)
        ok = (nn > 0.0) & np.isfinite(nn)
        nh = n.astype(np.float64) / np.sqrt(np.where(ok, nn, 1.0))[:, None]
        nh = np.broadcast_to(nh[None], (L,) + nh.shape).copy()
        to = q[:, None, P] - surf.astype(np.float64)[None]
        ln = np.linalg.norm(to, axis=2, keepdims=True)
        to = np.where(ln > 0.0, to / np.where(ln > 0.0, ln, 1.0), np.array([0.0, 0.0, 1.0]))
        nh[:, ~ok] = to[:, ~ok]
        x = (surf[None] + dtype(bias) * nh.astype(dtype)).astype(dtype)
    R = x.shape[1]
    x = x.reshape(L * R, 3)
    ql = np.repeat(q, R, axis=0)
    v = ql[:, P] - x.astype(np.float64)
    ln = np.linalg.norm(v, axis=1)
    some = ln > 0.0
    safe = np.where(some, ln, 1.0)
    s = np.where(some[:, None], v / safe[:, None], np.array([0.0, 0.0, 1.0])).astype(dtype)
    t_end = np.where(some, ln - ql[:, CLEARANCE], 0.0).astype(dtype)
    tan_half = np.where(some, ql[:, RHO] / safe, 0.0).astype(dtype)
    status = np.full(L * R, ALIVE, np.int8)
    status[(dtype(0.0) >= t_end) | (np.linalg.norm(x, axis=1) >= dtype(radius))] = ESCAPED
    return x, s, t_end, tan_half, status


def rule_step(f, i, t, m, status, outside, tan_half, *, eps, relax, min_step, grace):
    """sphere_trace_cpu.rule_step with a tan_half of each ray's own [T]"""
    t, m, status, outside = t.copy(), m.copy(), status.copy(), outside.copy()
    alive = status == ALIVE
    outside |= alive & (f >= eps)
    hit = alive & (f < eps) & (outside | (i >= grace))
    status[hit] = HIT
    m[hit] = 0.0
    alive &= ~hit
    pen = alive & outside & (tan_half > 0.0) & (t > 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        m[pen] = np.minimum(m[pen], np.clip(f[pen] / (t[pen] * tan_half[pen]), 0.0, 1.0))
    t[alive] = t[alive] + np.maximum(np.abs(f[alive]) * t.dtype.type(relax), t.dtype.type(min_step))
    return t, m, status, outside


def escape(x, s, t, status, radius, t_end):
    """rule step 1 of the bounded march: the points x + t s, and the status with the ALIVE rays that reached t_end, or the radius,
    ESCAPED"""
    p = x + t[:, None] * s
    status = status.copy()
    status[(status == ALIVE) & ((t >= t_end) | (np.linalg.norm(p, axis=1) >= radius))] = ESCAPED
    return p, status


def march_from(sdf, x, s, t_end, tan_half, status, *, steps=96, eps=1e-3, relax=1.0, min_step=1e-3, grace=16, radius=1.0, dtype=np.float64):
    """the bounded march from a begun state -> (visibility [T], status [T] int8, t [T])"""
    x, s, t_end, tan_half = (np.asarray(v, dtype) for v in (x, s, t_end, tan_half))
    T = x.shape[0]
    t, m = np.zeros(T, dtype), np.ones(T, dtype)
    status, outside = status.copy(), np.zeros(T, bool)
    for i in range(steps):
        p, status = escape(x, s, t, status, dtype(radius), t_end)
        f = np.asarray(sdf(p), dtype)
        t, m, status, outside = rule_step(f, i, t, m, status, outside, tan_half, eps=dtype(eps), relax=relax, min_step=min_step, grace=grace)
    status[status == ALIVE] = EXHAUSTED
    return m, status, t


def march_to(sdf, starts, lights, *, dtype=np.float64, radius=1.0, **params):
    """starts [M,3], lights [L,16] -> (visibility, status, t), each [L, M]; and the rays' directions [L, M, 3]"""
    L, M = np.asarray(lights).shape[0], np.asarray(starts).shape[0]
    x, s, t_end, tan_half, status = begin(lights, radius, starts=starts, dtype=dtype)
    m, status, t = march_from(sdf, x, s, t_end, tan_half, status, radius=radius, dtype=dtype, **params)
    return m.reshape(L, M), status.reshape(L, M), t.reshape(L, M), s.reshape(L, M, 3)


def linear_to_srgb(x):
    x = np.asarray(x, np.float64)
    return np.clip(np.where(x <= 0.0031308, 12.92 * x, 1.055 * np.abs(x) ** (1.0 / 2.4) - 0.055), 0.0, 1.0)


def composite(base, t, vis, acc, acc_threshold, lights):
    """base [Kb,R,3], or [R,3] (one base under every output: the results then have Kb = 1 and broadcast); t [L,R,3]; vis [L,R] or None;
    acc [R]; lights [L,16]  ->  (rgb [Kb,R,3], lin [Kb,R,3], light_lin [R,3], V [L,R]), all float64"""
    t, q = np.asarray(t, np.float64), np.asarray(lights, np.float64)
    L, R = t.shape[:2]
    v = np.ones((L, R)) if vis is None else np.asarray(vis, np.float64)
    V = np.where((np.asarray(acc, np.float64) > np.float64(acc_threshold))[None], v, 0.0)
    E = np.zeros((R, 3))
    for l in range(L):  # noqa: E741
        E = E + q[l, I][None] * V[l][:, None] * t[l]
    base = np.asarray(base, np.float64)
    lin = (base if base.ndim == 3 else base[None]) + E[None]
    return linear_to_srgb(lin), lin, E, V
