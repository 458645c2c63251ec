"""A float64 numpy restatement of the sun extraction's definitions (include/neusky_hip.h, the section after the environment map's):
what csrc/envmap_sun.hip is tested against, and the synthetic maps of those tests.  Test infrastructure: nothing here is on the
product path."""
import math
from types import SimpleNamespace

import numpy as np

LUM = np.array([0.2126, 0.7152, 0.0722])
SKY_TINT = np.array([0.5, 0.7, 1.0])
SUN_TINT = np.array([1.0, 0.9, 0.7])
SUN_PEAK = 500.0

# (H, W, convention, azimuth, elevation, sigma, rho) in degrees; the last two are the seam cases
CASES = [(128, 256, "blender", 37.3, 41.7, 2.0, 6.0),
         (128, 256, "neusky", 179.6, 20.2, 2.0, 6.0),
         (128, 256, "blender", 10.0, 88.9, 2.0, 6.0),  # the cap closes over the pole
         (37, 91, "neusky", -120.0, 55.0, 5.0, 15.0),
         (16, 32, "blender", 60.0, 45.0, 10.0, 25.0),
         (128, 256, "neusky", 0.4, 30.0, 2.0, 6.0),
         (128, 256, "blender", 179.7, 30.0, 2.0, 6.0)]


def case_id(c):
    return f"{c[0]}x{c[1]}-{c[2]}-az{c[3]:g}-el{c[4]:g}"


def texel_directions(H, W, convention):
    """e [H, W, 3] and omega [H, W]"""
    th = np.pi * (np.arange(H, dtype=np.float64) + 0.5) / H
    u = (np.arange(W, dtype=np.float64) + 0.5) / W
    ph = np.pi - 2.0 * np.pi * u if convention == "blender" else 2.0 * np.pi * u
    st, ct = np.sin(th), np.cos(th)
    e = np.stack([st[:, None] * np.cos(ph)[None], st[:, None] * np.sin(ph)[None], np.broadcast_to(ct[:, None], (H, W))], axis=-1)
    omega = np.broadcast_to((st * ((2.0 * np.pi / W) * 2.0 * math.sin(np.pi / (2.0 * H))))[:, None], (H, W))
    return e, omega


def direction(az_deg, el_deg):
    az, el = math.radians(az_deg), math.radians(el_deg)
    return np.array([math.cos(az) * math.cos(el), math.sin(az) * math.cos(el), math.sin(el)])


def sky_map(H, W, convention):
    e, _ = texel_directions(H, W, convention)
    return (0.6 + 0.4 * e[..., 2:3]) * SKY_TINT + 0.05 * np.sin(3.0 * e[..., 0:1])


def sun_lobe(H, W, convention, az_deg, el_deg, sigma_deg, amplitude=SUN_PEAK):
    e, _ = texel_directions(H, W, convention)
    ang = np.arccos(np.clip(e @ direction(az_deg, el_deg), -1.0, 1.0))
    return amplitude * np.exp(-ang ** 2 / (2.0 * math.radians(sigma_deg) ** 2))[..., None] * SUN_TINT


def synthetic_map(H, W, convention, az_deg, el_deg, sigma_deg, amplitude=SUN_PEAK):
    """the sky plus a Gaussian sun, fp32"""
    return (sky_map(H, W, convention) + sun_lobe(H, W, convention, az_deg, el_deg, sigma_deg, amplitude)).astype(np.float32)


def luminance(L):
    return 0.2126 * L[..., 0] + 0.7152 * L[..., 1] + 0.0722 * L[..., 2]


def extract(map32, convention, rho_deg, min_peak_ratio=10.0):
    """the definitions, on an fp32 [H, W, 3] map.  Returns a namespace: peak (flat index, -1 without one), peak_row, peak_col, Y_p,
    e_p, dots [H, W] (<e_t, e_p>), tau, ring_omega, ring_omega_Y, found, residual (fp32), excess (bool [H, W]), m, C, solid_angle,
    Y [H, W] (NaN where excluded)."""
    assert map32.dtype == np.float32 and map32.ndim == 3 and map32.shape[2] == 3
    H, W, _ = map32.shape
    rho = math.radians(rho_deg)
    L = map32.astype(np.float64)
    e, omega = texel_directions(H, W, convention)
    ok = np.isfinite(L).all(axis=-1)
    with np.errstate(invalid="ignore", over="ignore"):
        Y = np.where(ok, luminance(np.where(ok[..., None], L, 0.0)), np.nan)
    upper = ((np.arange(H) + 0.5) / H < 0.5)[:, None] & ok
    out = SimpleNamespace(Y=Y, residual=map32.copy(), excess=np.zeros((H, W), bool), C=np.zeros(3), solid_angle=0.0, tau=0.0,
                          ring_omega=0.0, ring_omega_Y=0.0, found=False, dots=None)
    if not upper.any():
        out.peak, out.peak_row, out.peak_col, out.Y_p, out.e_p = -1, -1, -1, 0.0, np.array([0.0, 0.0, 1.0])
        out.m = out.e_p
        return out
    masked = np.where(upper, Y, -np.inf).reshape(-1)
    p = int(np.argmax(masked))  # the first of equal maxima: the lowest flat index
    out.peak, out.peak_row, out.peak_col, out.Y_p = p, p // W, p % W, float(masked[p])
    e_p = e[p // W, p % W]
    out.e_p = out.m = e_p
    dots = e @ e_p
    out.dots = dots
    cap = (dots >= math.cos(rho)) & ok
    ring = (dots >= math.cos(2.0 * rho)) & (dots < math.cos(rho)) & ok
    out.ring_omega = float(omega[ring].sum())
    out.ring_omega_Y = float((omega[ring] * Y[ring]).sum())
    out.tau = out.ring_omega_Y / out.ring_omega if out.ring_omega > 0.0 else 0.0
    out.found = bool(out.ring_omega > 0.0 and out.Y_p > 0.0 and out.Y_p >= min_peak_ratio * out.tau)
    if not out.found:
        return out
    ex = cap & (np.where(ok, Y, -np.inf) > out.tau)
    out.excess = ex
    out.residual[ex] = (L[ex] * out.tau / Y[ex][:, None]).astype(np.float32)
    x = L[ex] - out.residual[ex].astype(np.float64)
    out.C = (omega[ex][:, None] * x).sum(axis=0) / (2.0 * np.pi)
    s = ((omega[ex] * luminance(x))[:, None] * e[ex]).sum(axis=0)
    n = float(np.linalg.norm(s))
    if n > 0.0:
        out.m = s / n
    out.solid_angle = float(omega[ex].sum())
    return out


def flux(map32, H, W, convention):
    """sum_t omega_t L_t [3] over the finite texels, float64"""
    _, omega = texel_directions(H, W, convention)
    L = map32.astype(np.float64)
    ok = np.isfinite(L).all(axis=-1)
    return (omega[ok][:, None] * L[ok]).sum(axis=0)


def boundary_margin(ref, rho_deg):
    """the least distance of any <e_t, e_p> from cos rho and cos 2 rho: set membership must not hang on rounding"""
    rho = math.radians(rho_deg)
    return min(float(np.abs(ref.dots - math.cos(rho)).min()), float(np.abs(ref.dots - math.cos(2.0 * rho)).min()))


def peak_margin(ref):
    """by how much the peak exceeds the second brightest texel of the upper hemisphere, relative to the peak"""
    H, W = ref.Y.shape
    y = np.where(((np.arange(H) + 0.5) / H < 0.5)[:, None], np.nan_to_num(ref.Y, nan=-np.inf), -np.inf).reshape(-1).copy()
    y[ref.peak] = -np.inf
    return (ref.Y_p - float(y.max())) / ref.Y_p


def angle_deg(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return math.degrees(math.atan2(np.linalg.norm(np.cross(a, b)), float(a @ b)))
