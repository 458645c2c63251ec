"""Float64 numpy restatement of the props' rules (include/neusky_hip.h, "Solid props placed in a frame"): the interval of a line inside a
sphere or a yawed box, the nearest entered prop of a ray, the insertion of its hit as one more sample, and the occlusion of a visibility
entry.  Every product, sum and quotient is rounded once in float64 from the float32 inputs, in the order the header gives, so a kernel
that follows the header differs from this only where a decision is closer than float64 rounding: each function also returns the
`margin` of its decisions, and a comparison leaves out the cases whose margin is below MARGIN.

Margins, all relative: a sphere's |disc| / b^2; a box's |t_out - t_in| / |t_out|, the gap of an axis with d'_i == 0 to its slab, and
the gap between its two largest per-axis minima (which decides the entry axis); for an entered or occluding interval of length
L = t_out - t_in the gaps |t_in| / L (seen: t_in > 0), |t_out| / L and |t_in - t_max| / max(|t_max|, L) (shadow).  Two entered props
whose t_in differ by less than TIE relative, but are not equal, are a tie: margin 0."""
import numpy as np

MARGIN = 1e-9
TIE = 1e-12
KIND, C, H, COS, SIN, ALBEDO, VISIBLE, CASTS = 0, 1, 4, 7, 8, 9, 12, 13
INF = np.inf


def _rel(a, b):
    """|a| / |b| with 0 / 0 = 0 and x / 0 = inf"""
    a, b = np.abs(a), np.abs(b)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(b > 0, a / np.where(b > 0, b, 1.0), np.where(a > 0, INF, 0.0))


def interval(o, d, row):
    """o, d: float64 [..., 3] (broadcast against each other); row: one prop's 16 columns -> (has [...], t_in, t_out, axis, margin): the
    interval of the line o + t d inside the prop; t_in, t_out are nan where there is none"""
    row = np.asarray(row, np.float64)
    o, d = np.broadcast_arrays(np.asarray(o, np.float64), np.asarray(d, np.float64))
    ocx, ocy, ocz = o[..., 0] - row[C], o[..., 1] - row[C + 1], o[..., 2] - row[C + 2]
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    with np.errstate(all="ignore"):
        if row[KIND] == 0.0:
            r = row[H]
            a = dx * dx + dy * dy + dz * dz
            b = ocx * dx + ocy * dy + ocz * dz
            q = ocx * ocx + ocy * ocy + ocz * ocz - r * r
            disc = b * b - a * q
            has = disc > 0
            s = np.sqrt(np.where(has, disc, 0.0))
            t_in, t_out = np.where(has, (-b - s) / a, np.nan), np.where(has, (-b + s) / a, np.nan)
            return has, t_in, t_out, np.full(has.shape, -1), _rel(disc, b * b)
        cy, sy = row[COS], row[SIN]
        ol = (cy * ocx + sy * ocy, cy * ocy - sy * ocx, ocz)
        dl = (cy * dx + sy * dy, cy * dy - sy * dx, dz)
        t_in, t_out = np.full(dx.shape, -INF), np.full(dx.shape, INF)
        second = np.full(dx.shape, -INF)  # the second largest per-axis minimum
        axis, has = np.full(dx.shape, -1), np.ones(dx.shape, bool)
        margin = np.full(dx.shape, INF)
        for i in range(3):
            h = row[H + i]
            moving = dl[i] != 0
            div = np.where(moving, dl[i], 1.0)
            t0, t1 = (-h - ol[i]) / div, (h - ol[i]) / div
            lo, hi = np.where(moving, np.minimum(t0, t1), -INF), np.where(moving, np.maximum(t0, t1), INF)
            up = lo > t_in
            second = np.where(up, t_in, np.maximum(second, lo))
            axis = np.where(up, i, axis)
            t_in = np.where(up, lo, t_in)
            t_out = np.minimum(t_out, hi)
            has &= moving | (np.abs(ol[i]) < h)
            margin = np.where(moving, margin, np.minimum(margin, np.abs(np.abs(ol[i]) - h) / h))
        has &= t_in < t_out
        finite = np.isfinite(t_in) & np.isfinite(t_out)
        margin = np.where(finite, np.minimum(margin, _rel(t_out - t_in, t_out)), margin)
        # the entry axis: how far the runner-up minimum is behind (only where the interval exists and two axes constrain)
        two = has & np.isfinite(second)
        margin = np.where(two, np.minimum(margin, _rel(t_in - second, np.maximum(np.abs(t_in), np.abs(t_out - t_in)))), margin)
        return has, np.where(has, t_in, np.nan), np.where(has, t_out, np.nan), axis, margin


def intersect(origins, directions, block):
    """origins, directions: float32 [R, 3]; block float32 [P, 16] -> (t_hit float32 [R] (+inf), id int32 [R] (-1), normal, albedo float32
    [R, 3], margin float64 [R])"""
    o, d = np.asarray(origins, np.float32).astype(np.float64), np.asarray(directions, np.float32).astype(np.float64)
    block = np.asarray(block, np.float32)
    R = o.shape[0]
    best, who, ax = np.full(R, INF), np.full(R, -1, np.int32), np.full(R, -1)
    margin = np.full(R, INF)
    entered = []
    with np.errstate(all="ignore"):
        for p, row in enumerate(block):
            if row[VISIBLE] == 0:
                continue
            has, t_in, t_out, axis, m = interval(o, d, row)
            m = np.where(has, np.minimum(m, _rel(t_in, t_out - t_in)), m)
            margin = np.minimum(margin, m)
            enters = has & (t_in > 0)
            entered.append(np.where(enters, t_in, INF))
            win = enters & (t_in < best)
            best, who, ax = np.where(win, t_in, best), np.where(win, p, who).astype(np.int32), np.where(win, axis, ax)
        if len(entered) > 1:
            e = np.sort(np.stack(entered, 1), 1)
            near = np.isfinite(e[:, 1]) & (e[:, 1] != e[:, 0]) & ((e[:, 1] - e[:, 0]) < TIE * np.abs(e[:, 0]))
            margin = np.where(near, 0.0, margin)
        normal, albedo = np.zeros((R, 3)), np.zeros((R, 3), np.float32)
        for r in np.nonzero(who >= 0)[0]:
            row = block[who[r]].astype(np.float64)
            if row[KIND] == 0.0:
                v = [(o[r, c] - row[C + c] + best[r] * d[r, c]) / row[H] for c in range(3)]
                length = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
                normal[r] = [v[0] / length, v[1] / length, v[2] / length]
            else:
                cy, sy = row[COS], row[SIN]
                dl = (cy * d[r, 0] + sy * d[r, 1], cy * d[r, 1] - sy * d[r, 0], d[r, 2])
                s = -1.0 if dl[ax[r]] > 0 else 1.0
                normal[r] = [(s * cy, s * sy, 0.0), (-s * sy, s * cy, 0.0), (0.0, 0.0, s)][ax[r]]
            albedo[r] = block[who[r], ALBEDO:ALBEDO + 3]
    return best.astype(np.float32), who, normal.astype(np.float32), albedo, margin


def insert(weights, starts, ends, albedo, normals, t_hit, prop_id, hit_normal, hit_albedo):
    """weights, starts, ends: float32 [R, S]; albedo, normals [R, S, 3]; intersect's outputs -> (weights', starts', ends' [R, S + 1],
    albedo', normals' [R, S + 1, 3], near bool [R]: some midpoint is within 4 ulp of t_hit, where the float32 test could go either way in
    an implementation that forms the midpoint differently)"""
    f = lambda a: np.asarray(a, np.float32)  # noqa: E731
    weights, starts, ends, albedo, normals, t_hit = f(weights), f(starts), f(ends), f(albedo), f(normals), f(t_hit)
    R, S = weights.shape
    entered = np.asarray(prop_id) >= 0
    mid = (starts + ends) / np.float32(2)
    front = mid < t_hit[:, None]
    kept = np.where(front, weights, np.float32(0))
    total = np.cumsum(kept.astype(np.float64), axis=1)[:, -1]  # in sample order
    slot = np.where(entered, np.clip(1.0 - total, 0.0, 1.0), 0.0).astype(np.float32)
    at = np.where(entered, t_hit, ends[:, -1]).astype(np.float32)
    cat = lambda a, b: np.concatenate([a, b], 1)  # noqa: E731
    zero = np.zeros((R, 3), np.float32)
    with np.errstate(invalid="ignore"):
        near = (np.isfinite(t_hit)[:, None] & (np.abs(mid - t_hit[:, None]) <= 4 * np.spacing(np.abs(t_hit))[:, None])).any(1)
    return (cat(kept, slot[:, None]), cat(starts, at[:, None]), cat(ends, at[:, None]),
            cat(albedo, np.where(entered[:, None], f(hit_albedo), zero)[:, None]),
            cat(normals, np.where(entered[:, None], f(hit_normal), zero)[:, None]), near)


def lifted(x, normals, bias):
    """x' = x + bias n^ in float64 [M, 3]; a zero or non-finite normal, or None, gives no lift"""
    x = np.asarray(x, np.float32).astype(np.float64)
    if normals is None:
        return x
    n = np.asarray(normals, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        nn = n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2]
        ok = (nn > 0) & (nn < INF)
        length = np.sqrt(np.where(ok, nn, 1.0))
        lift = float(np.float32(bias))
        return np.where(ok[:, None], x + lift * (n / length[:, None]), x)


def occlude(x, normals, bias, block, directions=None, targets=None, clearance=None):
    """x: float32 [M, 3]; normals [M, 3] or None; directions [N, 3], or targets [N, 3] with clearance [N]; bias: a number -> (occluded bool
    [M, N], margin float64 [M, N]): entry (m, n) of a visibility tensor is multiplied by 0 where occluded and left otherwise"""
    assert (directions is None) != (targets is None) and (targets is None) == (clearance is None)
    xl = lifted(x, normals, bias)[:, None, :]
    M = xl.shape[0]
    with np.errstate(all="ignore"):
        if directions is not None:
            d = np.asarray(directions, np.float32).astype(np.float64)[None]
            N = d.shape[1]
            t_max, live = np.full((M, N), INF), np.ones((M, N), bool)
        else:
            v = np.asarray(targets, np.float32).astype(np.float64)[None] - xl
            N = v.shape[1]
            length = np.sqrt(v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2])
            live = length > 0
            d = v / np.where(live, length, 1.0)[..., None]
            t_max = length - np.asarray(clearance, np.float32).astype(np.float64)[None]
        occluded, margin = np.zeros((M, N), bool), np.full((M, N), INF)
        for row in np.asarray(block, np.float32):
            if row[CASTS] == 0:
                continue
            has, t_in, t_out, _, m = interval(xl, d, row)
            span = t_out - t_in
            m = np.where(has, np.minimum(m, _rel(t_out, span)), m)
            m = np.where(has & np.isfinite(t_max), np.minimum(m, _rel(t_in - t_max, np.maximum(np.abs(t_max), span))), m)
            margin = np.minimum(margin, m)
            occluded |= has & (t_out > 0) & (t_in < t_max)
    return occluded & live, np.where(live, margin, INF)


# ---- the drawn cases the CPU and the GPU tests share (fixed seeds: test_props_cpu asserts that the restatement leaves out none of them)
INTERSECT_R, INTERSECT_P = (1, 63, 64, 65, 257), (1, 3, 64)
INSERT_S, INSERT_R = (1, 24, 65), (1, 65, 257)
OCCLUDE_M, OCCLUDE_N = (1, 65, 513), (1, 32, 257)


def draw_block(seed, P):
    """float32 [P, 16]: spheres and yawed boxes in [-1, 1]^3; prop 1 is an invisible shadow caster, prop 2 is seen and casts none"""
    from neusky_amd.relight import Prop, props_block
    rng = np.random.default_rng(seed)
    props = []
    for p in range(P):
        c, alb = rng.uniform(-1, 1, 3), rng.uniform(0, 1, 3)
        flags = dict(visible=p != 1, casts_shadows=p != 2)
        if p % 2 == 0:
            props.append(Prop("sphere", c, rng.uniform(0.1, 0.4), alb, **flags))
        else:
            props.append(Prop("box", c, rng.uniform(0.05, 0.4, 3), alb, yaw_deg=rng.uniform(-180, 180), **flags))
    return props_block(props).numpy()


def draw_rays(seed, R, block):
    """float32 origins, directions [R, 3]: aimed near a prop from outside, directions not exactly unit; of every 8 rows one starts at a
    prop's centre (inside it), one points away from a prop just behind it, one runs along +-z through a prop's column (d'_x = d'_y = 0
    inside the slabs) and one along +-z beside it (outside a slab)"""
    rng = np.random.default_rng(seed)
    P = block.shape[0]
    o = rng.uniform(-2, 2, (R, 3))
    which = rng.integers(0, P, R)
    c, h = block[which, C:C + 3].astype(np.float64), block[which, H:H + 3].astype(np.float64)
    d = c + rng.uniform(-1.2, 1.2, (R, 3)) * h.max(1, keepdims=True) - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    u = rng.normal(size=(R, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    for r in range(R):
        kind = r % 8
        if kind == 0:
            o[r] = c[r]
        elif kind == 1:
            o[r], d[r] = c[r] + 2.5 * h[r].max() * u[r], u[r]
        elif kind in (2, 3):
            side = h[r, :2].min() * 0.45 if kind == 2 else h[r, :2].max() * 3.0
            o[r] = c[r] + np.array([side * np.cos(r), side * np.sin(r), -3.0 if r % 16 < 8 else 3.0])
            d[r] = (0.0, 0.0, 1.0 if r % 16 < 8 else -1.0)
    return o.astype(np.float32), d.astype(np.float32)


def draw_samples(seed, R, S, t_hit):
    """float32 weights, starts, ends [R, S], albedo, normals [R, S, 3] of rays whose samples lie around their t_hit [R]"""
    rng = np.random.default_rng(seed)
    far = np.where(np.isfinite(t_hit), 2.0 * t_hit, 4.0).astype(np.float64) + 0.5
    edges = np.sort(rng.uniform(0.0, 1.0, (R, S + 1)), 1) * far[:, None]
    alpha = rng.uniform(0, 0.3, (R, S))
    T = np.cumprod(np.concatenate([np.ones((R, 1)), 1 - alpha], 1), 1)[:, :-1]
    f = lambda a: a.astype(np.float32)  # noqa: E731
    return f(alpha * T), f(edges[:, :-1]), f(edges[:, 1:]), f(rng.uniform(0, 1, (R, S, 3))), f(rng.normal(size=(R, S, 3)))


def draw_points(seed, M, N, block):
    """float32 x, normals [M, 3], directions [N, 3], targets [N, 3], clearance [N]: of every 8 points one is a prop's centre; of every 8
    normals one is zero and one is not finite"""
    rng = np.random.default_rng(seed)
    P = block.shape[0]
    x = rng.uniform(-1.5, 1.5, (M, 3))
    n = rng.normal(size=(M, 3)) * rng.uniform(0.1, 3.0, (M, 1))
    for m in range(M):
        if m % 8 == 0:
            x[m] = block[m // 8 % P, C:C + 3]
        if m % 8 == 3:
            n[m] = 0.0
        if m % 8 == 5:
            n[m, m % 3] = np.inf
    d = rng.normal(size=(N, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    f = lambda a: a.astype(np.float32)  # noqa: E731
    return f(x), f(n), f(d), f(rng.uniform(-2, 2, (N, 3))), f(rng.uniform(0, 0.05, N))
