"""numpy restatement of the sphere-traced shadow march (include/neusky_hip.h, "Sphere-traced shadow rays"): the reference the kernels of
csrc/sphere_trace.hip and relight.trace_visibility are tested against, in float64 (or in float32, to see what the number format alone
does), and the analytic scene the tests march through.  Nothing here imports the package."""
import numpy as np

ALIVE, HIT, ESCAPED, EXHAUSTED = 0, 1, 2, 3
DEFAULTS = dict(steps=96, eps=1e-3, relax=1.0, min_step=1e-3, grace=16, radius=1.0)


def tan_half(angular_diameter_deg):
    return float(np.tan(np.radians(np.float64(angular_diameter_deg)) / 2.0))


def rule_step(f, i, t, m, status, outside, *, eps, relax, min_step, grace, tan_half):
    """rule steps 3-6 of iteration i on copies of the state arrays, for the sdf values f: -> t, m, status, outside"""
    t, m, status, outside = t.copy(), m.copy(), status.copy(), outside.copy()
    alive = status == ALIVE
    outside |= alive & (f >= eps)
    hit = alive & (f < eps) & (outside | (i >= grace))
    status[hit] = HIT
    m[hit] = 0.0
    alive &= ~hit
    pen = alive & outside & (tan_half > 0.0) & (t > 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        m[pen] = np.minimum(m[pen], np.clip(f[pen] / (t[pen] * m.dtype.type(tan_half)), 0.0, 1.0))
    t[alive] = t[alive] + np.maximum(np.abs(f[alive]) * t.dtype.type(relax), t.dtype.type(min_step))
    return t, m, status, outside


def escape(x, s, t, status, radius):
    """rule step 1: the points x + t s, and the status with the ALIVE rays at or beyond the radius ESCAPED"""
    p = x + t[:, None] * s
    status = status.copy()
    status[(status == ALIVE) & (np.linalg.norm(p, axis=1) >= radius)] = ESCAPED
    return p, status


def march(sdf, x, s, *, steps=96, eps=1e-3, relax=1.0, min_step=1e-3, grace=16, radius=1.0, tan_half=0.0, dtype=np.float64):
    """x [M, 3] start points, s [M, 3] or [3] unit directions, sdf: points [M, 3] -> [M]  ->  (visibility [M], status [M] int8, t [M])"""
    x = np.asarray(x, dtype)
    s = np.broadcast_to(np.asarray(s, dtype), x.shape)
    M = x.shape[0]
    t, m = np.zeros(M, dtype), np.ones(M, dtype)
    status, outside = np.full(M, ALIVE, np.int8), np.zeros(M, bool)
    for i in range(steps):
        p, status = escape(x, s, t, status, dtype(radius))
        f = np.asarray(sdf(p), dtype)
        t, m, status, outside = rule_step(f, i, t, m, status, outside, eps=dtype(eps), relax=relax, min_step=min_step, grace=grace,
                                          tan_half=tan_half)
    status[status == ALIVE] = EXHAUSTED
    return m, status, t


# ---- the analytic scene: the plane z = 0 and a sphere above it
CENTRE, SPHERE_RADIUS = np.array([0.1, -0.05, 0.4]), 0.25
BAND = 0.01


def scene_sdf(p):
    p = np.asarray(p)
    c = CENTRE.astype(p.dtype)
    return np.minimum(p[:, 2], np.linalg.norm(p - c, axis=1) - p.dtype.type(SPHERE_RADIUS))


def sun_direction(azimuth_deg=30.0, elevation_deg=40.0):
    az, el = np.radians(np.float64(azimuth_deg)), np.radians(np.float64(elevation_deg))
    return np.array([np.cos(az) * np.cos(el), np.sin(az) * np.cos(el), np.sin(el)])


def scene_starts(n=64, z=0.0, half=0.6):
    g = np.linspace(-half, half, n)
    X, Y = np.meshgrid(g, g, indexing="ij")
    return np.stack([X.reshape(-1), Y.reshape(-1), np.full(n * n, np.float64(z))], 1)


def analytic_shadow(x, s):
    """-> (in the sphere's shadow [M] bool, distance of the ray's line from the sphere's silhouette [M])"""
    v = CENTRE[None] - x
    along = v @ s
    perp = np.linalg.norm(v - along[:, None] * s[None], axis=1)
    return (perp < SPHERE_RADIUS) & (along > 0.0), np.abs(perp - SPHERE_RADIUS)
