"""The height-fog rule of include/neusky_hip.h restated in numpy: float64 by default, the tests' reference; `dtype=np.float32` runs the
same statements in float32, which is where the kernel tests' bar comes from.  Test infrastructure: the product path has no CPU side."""
import numpy as np

from sun_cpu import linear_to_srgb

FLOATS = 12  # density (0..2), albedo (3..5), H (0: homogeneous), base_height, g, far, background (1 or 0), pad


def block(density, scale_height=None, base_height=0.0, albedo=1.0, anisotropy=0.0, far=2.0, background=True):
    """the kernels' parameter block, rounded to float32 as the device holds it, in float64"""
    three = lambda v: list(np.broadcast_to(np.asarray(v, np.float64), (3,)))  # noqa: E731
    p = [*three(density), *three(albedo), 0.0 if scale_height is None else scale_height, base_height, anisotropy, far, 1.0 if background else 0.0, 0.0]
    return np.asarray(p, np.float64).astype(np.float32).astype(np.float64)


def phi(u):
    """(1 - exp(-u)) / u in u's dtype"""
    u = np.asarray(u)
    one = u.dtype.type(1.0)
    safe = np.where(np.abs(u) < 1e-4, one, u)
    return np.where(np.abs(u) < 1e-4, one - u / 2 + u * u / 6, -np.expm1(-safe) / safe)


def phi_series(u):
    return 1.0 - u / 2 + u * u / 6


def phi_closed(u):
    return -np.expm1(-u) / u


class Medium:
    """a parameter block and the rays' own factors, in `dtype`"""

    def __init__(self, params, origins, directions, dtype=np.float64):
        f = lambda x: np.asarray(x).astype(dtype)  # noqa: E731
        p = f(params)
        self.dtype = dtype
        self.density, self.albedo, self.H, self.base, self.g, self.far, self.background = p[0:3], p[3:6], p[6], p[7], p[8], p[9], bool(p[10] != 0)
        o, self.d = f(origins), f(directions)
        self.dz = self.d[:, 2]
        if self.H > 0:
            self.E = np.exp(np.clip(-(o[:, 2] - self.base) / self.H, dtype(-80.0), dtype(80.0)))
        else:
            self.E = np.ones(o.shape[0], dtype)

    def path(self, t):
        """E t phi(d_z t / H) [R]; t alone in a homogeneous medium"""
        t = np.broadcast_to(np.asarray(t, self.dtype), self.dz.shape)
        if not self.H > 0:
            return t
        return self.E * t * phi(self.dz * t / self.H)

    def tau(self, t):
        return self.density[None, :] * self.path(t)[:, None]

    def T(self, t):
        """[R, 3]"""
        return np.exp(-self.tau(t))

    def phase(self, mu):
        g = self.g
        q = 1 + g * g - 2 * g * mu
        return self.dtype(1.0 / (4.0 * np.pi)) * (1 - g * g) / (q * np.sqrt(q))


def apply(origins, directions, depth, accumulation, lin, background, abar, sun_dirs, sun_colours, vis, params, M, light_lin=None,
          dtype=np.float64):
    """origins, directions [R,3]; depth, accumulation [R]; lin [Kb,R,3]; background [R,3] or [Kb,R,3]; abar [Kb,3]; sun_dirs, sun_colours
    [Kb,3] or None; vis [M,Kb,R] or None; params [12]; M -> dict: lin, rgb, inscatter [Kb,R,3], transmittance [R,3], light_lin [R,3] or None,
    and `scale` [Kb,R,3] = max(|lin|, |B|, J with V = 1), the pixel's scale"""
    f = lambda x: np.asarray(x).astype(dtype)  # noqa: E731
    md = Medium(params, origins, directions, dtype)
    lin, abar = f(lin), f(abar)
    Kb, R = lin.shape[0], lin.shape[1]
    B = np.broadcast_to(f(background), (Kb, R, 3))
    ts = np.clip(f(depth).reshape(R), dtype(0.0), md.far)
    A = np.clip(f(accumulation).reshape(R), dtype(0.0), dtype(1.0))[None, :, None]
    sun = np.zeros((Kb, R, 3), dtype)  # 2 pi p_g(<d, s_k>) C_k up_k
    if sun_dirs is not None:
        s, C = f(sun_dirs), f(sun_colours)
        up = (s[:, 2] > 0).astype(dtype)
        mu = np.einsum("ri,ki->kr", md.d, s)
        sun = dtype(2.0 * np.pi) * md.phase(mu)[:, :, None] * C[:, None, :] * up[:, None, None]
    Mseg = max(int(M), 1)
    far = np.full(R, md.far, dtype)
    Ss, Sf = np.zeros((Kb, R, 3), dtype), np.zeros((Kb, R, 3), dtype)
    for m in range(Mseg):
        t0, t1 = dtype(m) * md.far / dtype(Mseg), dtype(m + 1) * md.far / dtype(Mseg)
        v = f(vis)[m][:, :, None] if (vis is not None and M > 0) else dtype(1.0)
        J = md.albedo[None, None, :] * (abar[:, None, :] + sun * v)
        Ss = Ss + J * (md.T(np.minimum(t0, ts)) - md.T(np.minimum(t1, ts)))[None]
        Sf = Sf + J * (md.T(np.minimum(t0, far)) - md.T(np.minimum(t1, far)))[None]
    Ts, Tf = md.T(ts), md.T(far)
    X = Tf[None] * B + Sf if md.background else B
    out = Ts[None] * (lin - (1 - A) * B) + A * Ss + (1 - A) * X
    inscatter = A * Ss + (1 - A) * Sf if md.background else A * Ss
    J1 = md.albedo[None, None, :] * (abar[:, None, :] + sun)
    return {"lin": out, "rgb": linear_to_srgb(out), "inscatter": inscatter, "transmittance": Ts,
            "light_lin": None if light_lin is None else f(light_lin) * Ts,
            "scale": np.maximum(np.maximum(np.abs(lin), np.abs(B)), J1).astype(np.float64)}


def midpoints(far, M):
    """the float64 depths [M] of the shaft queries: (m + 0.5) (far / M), far as the device holds it"""
    return (np.arange(M, dtype=np.float64) + 0.5) * (np.float64(np.float32(far)) / M)
