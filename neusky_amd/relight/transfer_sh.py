"""A baked frame's radiance transfer in a spherical-harmonic basis of the light directions: (order + 1)^2 coefficients per ray and
channel in place of D directions (precomputed radiance transfer, Sloan, Kautz, Snyder 2002).

The relight of a baked frame is linear in the light L [D, 3] (transfer.py).  With an orthonormal basis Q [D, J] of the directions,
    sum_d T[r,d,c] L[d,c] = sum_j C[r,j,c] l[j,c],     C = T Q,   l = Q^T L
for every light in the span of Q; for any other light the right-hand side is the relight under the projected light Q Q^T L.  Q is the
thin QR of the real spherical harmonics up to `order` sampled at the frame's directions (J = (order + 1)^2), so the span is the
band-limited lights.  A sky without its sun is smooth; the sun has paths of its own (SunLight, extract_sun, DaylightSky).

How close an order comes depends on the light, and has not been measured on a trained sky.  Every relight therefore reports
`light_residual` = |L - Q Q^T L|_F / |L|_F of the light it was given: that is what to read before trusting a frame.  The default order
(5, 36 coefficients) and the maximum (8, 81) are design choices, not measurements.

Kernels: csrc/transfer_sh.hip (nsky_transfer_project, nsky_transfer_relight_short); both take any basis."""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import math

import torch

from .transfer import BakedFrame, RadianceTransfer, _bake_chunks, _storage_dtype

DEFAULT_ORDER = 5  # a design choice (36 coefficients: a 1080p frame in 0.9 GB of fp32), not a measurement
MAX_ORDER = 8      # likewise (81 coefficients; the kernels take up to 128)
MAX_CONDITION = 1.0e3


def sh_basis(directions: torch.Tensor, order: int) -> torch.Tensor:
    """float64 [D, (order + 1)^2]: the orthonormal real spherical harmonics Y_l^m, l <= order, at unit `directions` [D, 3], z up,
    column j = l (l + 1) + m; no Condon-Shortley phase (Y_1^1 = sqrt(3 / 4 pi) x).  With P_l^m(z) = (1 - z^2)^(m/2) p_l^m(z),
        Y_l^{+m} = sqrt(2) K_l^m Re (x + i y)^m p_l^m(z),  Y_l^{-m} = sqrt(2) K_l^m Im (x + i y)^m p_l^m(z),  Y_l^0 = K_l^0 p_l^0(z),
    K_l^m = sqrt((2 l + 1) / (4 pi) (l - m)! / (l + m)!), and p by the Legendre recurrences in l: polynomials in x, y, z, no angle."""
    if order < 0:
        raise ValueError(f"order must be >= 0, got {order}")
    d = directions.to(torch.float64)
    d = d / d.norm(dim=1, keepdim=True)  # (fp32 directions are unit to 1e-7 only)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    out = torch.empty(d.shape[0], (order + 1) ** 2, dtype=torch.float64, device=d.device)
    re, im = torch.ones_like(x), torch.zeros_like(x)  # (x + i y)^m
    pmm = 1.0  # p_m^m = (2 m - 1)!!
    for m in range(order + 1):
        if m > 0:
            re, im = re * x - im * y, re * y + im * x
            pmm *= 2 * m - 1
        below = torch.zeros_like(z)           # p_{l-2}^m
        here = torch.full_like(z, pmm)        # p_{l-1}^m, starting at p_m^m
        for l in range(m, order + 1):  # noqa: E741
            if l > m:
                below, here = here, ((2 * l - 1) * z * here - (l + m - 1) * below) / (l - m)
            k = math.sqrt((2 * l + 1) / (4.0 * math.pi) * math.factorial(l - m) / math.factorial(l + m))
            if m == 0:
                out[:, l * (l + 1)] = k * here
            else:
                out[:, l * (l + 1) + m] = math.sqrt(2.0) * k * re * here
                out[:, l * (l + 1) - m] = math.sqrt(2.0) * k * im * here
    return out


def light_basis(directions: torch.Tensor, order: int) -> torch.Tensor:
    """Q fp32 [D, J], J = (order + 1)^2, on the directions' device: the thin QR (float64, on the host) of sh_basis(directions, order)
    with the diagonal of R positive, so that Q is unique.  Its columns are orthonormal over the D directions and span the harmonics
    up to `order`.  ValueError when the directions cannot hold them: J > D, or the sampled harmonics' condition number above 1e3."""
    if not 0 <= int(order) <= MAX_ORDER:
        raise ValueError(f"order must lie in 0..{MAX_ORDER}, got {order}")
    D, J = directions.shape[0], (int(order) + 1) ** 2
    if J > D:
        raise ValueError(f"order {order} has {J} coefficients: more than the {D} light directions")
    Y = sh_basis(directions.detach().to("cpu", torch.float64), int(order))
    sv = torch.linalg.svdvals(Y)
    cond = float(sv[0] / sv[-1]) if float(sv[-1]) > 0.0 else math.inf
    if not cond <= MAX_CONDITION:
        raise ValueError(f"the {D} light directions do not resolve order {order}: the sampled harmonics' condition number is {cond:.3g}")
    Q, Rm = torch.linalg.qr(Y, mode="reduced")
    sign = torch.where(torch.diagonal(Rm) < 0, -1.0, 1.0).to(torch.float64)
    return (Q * sign[None, :]).to(torch.float32).contiguous().to(directions.device)  # (LAPACK's Q is column-major)


def project_lights(Q: torch.Tensor, lights: torch.Tensor):
    """lights [K, D, 3] -> (l [K, J, 3] fp32 = Q^T L, light_residual [K] float64 = |L - Q Q^T L|_F / |L|_F), formed in float64 on the
    lights' device"""
    Q64, L64 = Q.to(torch.float64), lights.to(torch.float64)
    l = torch.einsum("dj,kdc->kjc", Q64, L64)  # noqa: E741
    rest = L64 - torch.einsum("dj,kjc->kdc", Q64, l)
    norm = L64.flatten(1).norm(dim=1)
    residual = rest.flatten(1).norm(dim=1) / torch.where(norm > 0, norm, torch.ones_like(norm))
    return l.to(torch.float32).contiguous(), residual


class SHRadianceTransfer(BakedFrame):
    """One baked frame in a light basis: C [R, J, 3] = T Q (fp32, or fp16 with int32 row exponents [R]), acc [R], the basis Q [D, J]
    over the bake's light directions dirs [D, 3], the rays' directions [R, 3] (for the background), the frame shape and the
    light-independent outputs of the frame render.

    `relight` takes RadianceTransfer.relight's arguments and returns its keys, the light projected onto the basis, plus "light_residual"
    ([K], or 0-d for a single light): |L - Q Q^T L|_F / |L|_F, a device tensor (nothing synchronises with the host).  The frame is the
    dense relight under Q Q^T L: exact where the residual is zero.  Its linear image may be negative where the basis rings: a `display`
    transform takes such a value as 0, like a NaN, and does not meter it."""
    ROWS, FORMAT, EXTRA_KEYS, HAS_RESIDUAL = "C", 2, ("Q", "order"), True

    def __init__(self, C: torch.Tensor, exponents: Optional[torch.Tensor], acc: torch.Tensor, Q: torch.Tensor, dirs: torch.Tensor,
                 ray_directions: torch.Tensor, shape: Sequence[int], outputs: Dict[str, torch.Tensor], camera_index: int = 0,
                 order: Optional[int] = None):
        super().__init__(C, exponents, acc, dirs, ray_directions, shape, outputs, camera_index,
                         fits=tuple(Q.shape) == (dirs.shape[0], *C.shape[1:2]), others=f"Q {tuple(Q.shape)}, ")
        self.Q = Q.to(torch.float32).contiguous()
        self.order = math.isqrt(C.shape[1]) - 1 if order is None else int(order)

    def _relight_pass(self, lights, bg, rgb, lin) -> torch.Tensor:
        from .. import hip
        l, residual = project_lights(self.Q, lights)  # noqa: E741
        hip.transfer_relight_short(self.C, self.exponents, self.acc, l, bg, rgb, lin)
        return residual

    @torch.no_grad()
    def relight_from_lights(self, lights: torch.Tensor, bg: torch.Tensor, return_linear: bool = False) -> Dict[str, torch.Tensor]:
        """lights [K, D, 3] at the bake's directions and bg [K, R, 3] -> {"rgb" [K, *shape, 3], "light_residual" [K], "linear"}: the
        frame under each light's projection onto the basis.  Nothing synchronises with the host."""
        R, D = self.C.shape[0], self.dirs.shape[0]
        K = lights.shape[0]
        if tuple(lights.shape) != (K, D, 3) or tuple(bg.shape) != (K, R, 3):
            raise ValueError(f"lights {tuple(lights.shape)} and bg {tuple(bg.shape)} for {D} directions and {R} rays")
        lights = lights.to(self.device, torch.float32).contiguous()
        bg = bg.to(self.device, torch.float32).contiguous()
        rgb = torch.empty(K, R, 3, dtype=torch.float32, device=self.device)
        lin = torch.empty(K, R, 3, dtype=torch.float32, device=self.device) if return_linear else None
        out = {"rgb": rgb.view(K, *self.shape, 3), "light_residual": self._relight_pass(lights, bg, rgb, lin)}
        if lin is not None:
            out["linear"] = lin.view(K, *self.shape, 3)
        return out


def _coefficients(R: int, J: int, storage: str, dev):
    C = torch.empty(R, J, 3, dtype=_storage_dtype(storage), device=dev)
    return C, (torch.empty(R, dtype=torch.int32, device=dev) if storage == "fp16" else None)


@torch.no_grad()
def compress_transfer(baked: RadianceTransfer, order: int = DEFAULT_ORDER, storage: Optional[str] = None) -> SHRadianceTransfer:
    """Project a dense bake onto the harmonics up to `order`: C = T Q, stored as `storage` (default: the bake's)."""
    from .. import hip
    storage = baked.storage if storage is None else storage
    Q = light_basis(baked.dirs, order)
    C, exps = _coefficients(baked.T.shape[0], Q.shape[1], storage, baked.device)
    hip.transfer_project(baked.T, baked.exponents, Q, C, 0, exps)
    return SHRadianceTransfer(C, exps, baked.acc, Q, baked.dirs, baked.ray_directions, baked.shape, baked.outputs, baked.camera_index, order)


@torch.no_grad()
def bake_transfer_sh(model, camera_ray_bundle, order: int = DEFAULT_ORDER, storage: str = "fp32", chunk: Optional[int] = None,
                     use_graph: bool = True, camera_index: Optional[int] = None) -> SHRadianceTransfer:
    """bake_transfer straight into the basis: the same chunked bake (in fp32 chunks), each chunk's rows projected into C as soon as they
    exist.  The dense [R, D, 3] transfer is never allocated; C and acc are bit for bit those of
    compress_transfer(bake_transfer(..., "fp32"), order, storage)."""
    from .. import hip
    _storage_dtype(storage)
    kept = {}

    def open_sink(R, dirs, dev):
        Q = kept["Q"] = light_basis(dirs, order)
        C, exps = kept["C"], kept["exps"] = _coefficients(R, Q.shape[1], storage, dev)

        def take(a, b, res):
            hip.transfer_project(res["transfer"][:b - a], None, Q, C, a, exps)
        return take

    shape, dirs, acc, rays, outputs, camera_index = _bake_chunks(model, camera_ray_bundle, "fp32", chunk, use_graph, camera_index, open_sink)
    return SHRadianceTransfer(kept["C"], kept["exps"], acc, kept["Q"], dirs, rays, shape, outputs, camera_index, order)
