"""float64 restatement of the radiance-transfer definitions (include/neusky_hip.h, relight/transfer.py): the transfer of a batch of rays,
the relit frame, and the scaled-fp16 packing (numpy); plus the input generator the transfer tests share."""
from __future__ import annotations

import numpy as np
import torch


def transfer(albedo, normals, weights, dirs, vis=None):
    """albedo, normals [R,S,3]; weights [R,S]; dirs [D,3]; vis [R,D] or None -> (T [R,D,3], acc [R]), float64
    T[r,d,c] = vis[r,d] sum_s w[r,s] alb[r,s,c] clamp(n[r,s].dir[d], 0, 1) / cnt[r,s]"""
    albedo, normals, weights, dirs = albedo.double(), normals.double(), weights.double(), dirs.double()
    cos = torch.einsum("rsi,di->rsd", normals, dirs).clamp(0.0, 1.0)
    cnt = (cos > 0).double().sum(-1, keepdim=True)
    cnt = torch.where(cnt > 0, cnt, torch.ones_like(cnt))
    T = torch.einsum("rs,rsc,rsd->rdc", weights, albedo, cos / cnt)
    if vis is not None:
        T = T * vis.double()[:, :, None]
    return T, weights.sum(-1)


def relit_linear(T, acc, lights, bg):
    """T [R,D,3], acc [R], lights [K,D,3], bg [K,R,3] -> lin [K,R,3] = sum_d T L + bg (1 - acc)"""
    return torch.einsum("rdc,kdc->krc", T.double(), lights.double()) + bg.double() * (1.0 - acc.double())[None, :, None]


def relit_magnitude(T, lights, bg):
    """sum_d |T L| + |bg| [K,R,3]: what the rounding of a relit value is relative to"""
    return torch.einsum("rdc,kdc->krc", T.double().abs(), lights.double().abs()) + bg.double().abs()


def linear_to_srgb(x):
    y = torch.where(x <= 0.0031308, 12.92 * x, 1.055 * torch.pow(torch.abs(x), 1 / 2.4) - 0.055)
    return y.clamp(0.0, 1.0)


def relit(T, acc, lights, bg):
    return linear_to_srgb(relit_linear(T, acc, lights, bg))


def pack_fp16(T: np.ndarray):
    """(half [R,...], e int32 [R]): row r stored as half(T[r] 2^e[r]), the row maximum of |T[r]| 2^e[r] in [0.5, 1); a zero row takes 0"""
    T = np.asarray(T, dtype=np.float64)
    R = T.shape[0]
    mx = np.abs(T.reshape(R, -1)).max(axis=1)
    _, x = np.frexp(mx)
    e = np.where(mx > 0, -x, 0).astype(np.int32)
    scaled = np.ldexp(T, e.reshape((R,) + (1,) * (T.ndim - 1)))
    return scaled.astype(np.float16), e


def unpack_fp16(half: np.ndarray, e: np.ndarray) -> np.ndarray:
    R = half.shape[0]
    return np.ldexp(half.astype(np.float64), -e.reshape((R,) + (1,) * (half.ndim - 1)).astype(np.int64))


def random_inputs(R: int, S: int, D: int, seed: int, with_vis: bool = True, margin: float = 1e-5):
    """fp32 renderer inputs that exercise the corners: samples facing no direction (zero normals: cnt = 0), one ray with acc = 0 and one
    with acc = 1.  No cosine lies within `margin` of zero, so fp32 and fp64 agree on which directions a sample faces (cnt is a step)."""
    g = torch.Generator().manual_seed(seed)
    dirs = torch.nn.functional.normalize(torch.randn(D, 3, generator=g), dim=-1)
    normals = torch.nn.functional.normalize(torch.randn(R, S, 3, generator=g), dim=-1)
    for _ in range(64):
        near = (torch.einsum("rsi,di->rsd", normals.double(), dirs.double()).abs() < margin).any(-1)
        if not near.any():
            break
        normals[near] = torch.nn.functional.normalize(torch.randn(int(near.sum()), 3, generator=g), dim=-1)
    else:
        raise RuntimeError("could not separate the cosines from zero")
    normals[torch.rand(R, S, generator=g) < 0.1] = 0.0
    albedo = torch.rand(R, S, 3, generator=g)
    weights = torch.rand(R, S, generator=g) ** 4
    weights = weights / weights.sum(-1, keepdim=True) * torch.rand(R, 1, generator=g)
    weights[0] = 0.0  # acc = 0
    if R > 1:
        weights[1] = 0.0
        weights[1, S // 2] = 1.0  # acc = 1
    vis = torch.rand(R, D, generator=g) if with_vis else None
    return albedo, normals, weights, dirs, vis


def random_lights(K: int, D: int, R: int, seed: int, sun: bool = True):
    g = torch.Generator().manual_seed(seed)
    lights = torch.rand(K, D, 3, generator=g) ** 2 * 2.0
    if sun:
        lights[0, D // 3, 1] = 3.0e4
    bg = torch.rand(K, R, 3, generator=g) * 1.5
    return lights, bg
