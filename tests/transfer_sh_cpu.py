"""float64 numpy restatement of the transfer in a spherical-harmonic basis (relight/transfer_sh.py, csrc/transfer_sh.hip): the real
harmonics from the associated Legendre functions in angles (the package builds them as polynomials in x, y, z), the light basis, the
projection of a transfer and the relight of coefficient rows.  The tone curve and the fp16 packing are transfer_cpu's."""
from __future__ import annotations

import math

import numpy as np

from transfer_cpu import linear_to_srgb, pack_fp16, unpack_fp16  # noqa: F401  (shared with the tests)


def legendre(l: int, m: int, z: np.ndarray) -> np.ndarray:  # noqa: E741
    """associated Legendre function P_l^m(z), m >= 0, WITHOUT the Condon-Shortley phase: P_m^m = (2m-1)!! (1-z^2)^(m/2),
    P_{m+1}^m = (2m+1) z P_m^m, (l-m) P_l^m = (2l-1) z P_{l-1}^m - (l+m-1) P_{l-2}^m"""
    pmm = np.ones_like(z)
    root = np.sqrt(np.maximum(1.0 - z * z, 0.0))
    for i in range(1, m + 1):
        pmm = pmm * (2 * i - 1) * root
    if l == m:
        return pmm
    pm1 = (2 * m + 1) * z * pmm
    for n in range(m + 2, l + 1):
        pmm, pm1 = pm1, ((2 * n - 1) * z * pm1 - (n + m - 1) * pmm) / (n - m)
    return pm1


def real_sh(directions: np.ndarray, order: int) -> np.ndarray:
    """[D, (order+1)^2]: orthonormal real spherical harmonics, z up, column l(l+1)+m:
    Y_l^m = sqrt(2) K cos(m phi) P_l^m(cos theta) (m > 0), sqrt(2) K sin(|m| phi) P_l^|m| (m < 0), K P_l^0 (m = 0)"""
    d = np.asarray(directions, dtype=np.float64)
    z = d[:, 2] / np.linalg.norm(d, axis=1)
    phi = np.arctan2(d[:, 1], d[:, 0])
    out = np.empty((d.shape[0], (order + 1) ** 2))
    for l in range(order + 1):  # noqa: E741
        for m in range(-l, l + 1):
            a = abs(m)
            k = math.sqrt((2 * l + 1) / (4.0 * math.pi) * math.factorial(l - a) / math.factorial(l + a))
            p = legendre(l, a, z)
            if m == 0:
                y = k * p
            elif m > 0:
                y = math.sqrt(2.0) * k * np.cos(a * phi) * p
            else:
                y = math.sqrt(2.0) * k * np.sin(a * phi) * p
            out[:, l * (l + 1) + m] = y
    return out


def light_basis(directions: np.ndarray, order: int) -> np.ndarray:
    """float64 [D, J]: the thin QR of real_sh with the diagonal of R positive"""
    Q, R = np.linalg.qr(real_sh(directions, order))
    return Q * np.where(np.diag(R) < 0, -1.0, 1.0)[None, :]


def project(T: np.ndarray, B: np.ndarray) -> np.ndarray:
    """T [R, D, 3], B [D, J] -> C [R, J, 3] = sum_d T[r,d,c] B[d,j]"""
    return np.einsum("rdc,dj->rjc", np.asarray(T, dtype=np.float64), np.asarray(B, dtype=np.float64))


def project_magnitude(T: np.ndarray, B: np.ndarray) -> np.ndarray:
    """sum_d |T| |B| [R, J, 3]: what the rounding of a projected value is relative to"""
    return np.einsum("rdc,dj->rjc", np.abs(np.asarray(T, dtype=np.float64)), np.abs(np.asarray(B, dtype=np.float64)))


def relit_linear(C, acc, l, bg) -> np.ndarray:  # noqa: E741
    """C [R, J, 3], acc [R], l [K, J, 3], bg [K, R, 3] -> lin [K, R, 3] = sum_j C l + bg (1 - acc)"""
    C, acc, l, bg = (np.asarray(t, dtype=np.float64) for t in (C, acc, l, bg))  # noqa: E741
    return np.einsum("rjc,kjc->krc", C, l) + bg * (1.0 - acc)[None, :, None]


def relit_magnitude(C, l, bg) -> np.ndarray:  # noqa: E741
    C, l, bg = (np.abs(np.asarray(t, dtype=np.float64)) for t in (C, l, bg))  # noqa: E741
    return np.einsum("rjc,kjc->krc", C, l) + bg


def light_residual(Q: np.ndarray, L: np.ndarray) -> float:
    """|L - Q Q^T L|_F / |L|_F for one light L [D, 3]"""
    L = np.asarray(L, dtype=np.float64)
    return float(np.linalg.norm(L - Q @ (Q.T @ L)) / np.linalg.norm(L))
