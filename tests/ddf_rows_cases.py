"""Inputs and references for the tests of the DDF query rows: the sphere position and the 16-column encoded row
[d_loc | NeRF2(d_loc) | 0] that every DDF evaluation starts from, written by visibility_rays_kernel (csrc/render.hip) and by
ddf_fit_rows_fwd/bwd_kernel (csrc/samplers.hip), and the two autograd nodes around them (ops.DDFQueryRowsFn, ops.DDFFitRowsFn).

Deterministic builders (torch.Generator seeds on the CPU, float32 tensors) and the restatement of each operation, run in float64
(the reference the kernels are held to) and in float32 (what plain float32 arithmetic makes of the same inputs: the conditioning
of a case, and the unit of every bar).  Every restatement is the oracle's: O.ddf_model_outputs and O.compute_visibility with a
capturing ddf_fn that records the position and the row (O.ddf_local_direction + O.nerf_encoding, pinned by G5 / G6) of every
evaluation and returns a fixed linear read-out of the row, so that each of the 15 columns is observed.  Nothing here needs a GPU:
test_ddf_rows_cases_cpu.py proves what the cases are meant to be, test_gpu_ddf_rows.py runs the kernels.

One quirk of the reference is kept on purpose: the multi-view points are drawn from the UNIT sphere whatever ddf_radius is
(ddf_model.py:290), so at radius 2.5 the multi-view rows start 1.5 inside the DDF sphere.  The cases do the same."""
import functools
import math

import numpy as np
import torch

from oracle import neusky_oracle as O

RADII = (1.0, 2.5)
EPS32 = 2.0 ** -23
F32 = lambda v: float(np.float32(v))  # noqa: E731  (a Python float as the C ABI's `float` argument sees it)
# the read-out of the capturing ddf_fn: 15 fixed weights, none of them 0, no two alike
READOUT = 0.11 * torch.cos(0.7 * torch.arange(15, dtype=torch.float64) + 0.3) + 0.02

# case -> seed, where the first seed missed a condition of test_ddf_rows_cases_cpu.py (none had to move)
RESEEDED = {}


def _seed(*key):
    if key in RESEEDED:
        return RESEEDED[key]
    return int(sum((j + 1) * 7919 * round(1000 * float(v)) for j, v in enumerate(key[1:]))) % (2 ** 31) + len(key[0])


def bar(ref32, ref64):
    """the bar of one compared array: 4 x the largest difference between the float32 and the float64 run of the restatement on
    the same inputs (the factor covers a second, differently ordered float32 evaluation: fma contraction, the device sinf, another
    reduction order), with a floor of 4 float32 roundings of the array's largest entry"""
    ref64 = ref64.double()
    if ref64.numel() == 0:
        return 0.0
    return max(4.0 * (ref32.double() - ref64).abs().max().item(), 4.0 * EPS32 * ref64.abs().max().item())


def max_err(got, ref64):
    return (got.double() - ref64.double()).abs().max().item() if ref64.numel() else 0.0


# ---- the row and the capturing ddf_fn ----------------------------------------------------------------------------------------------
def rows(pos, dirs, dtype):
    """the 15 columns [d_loc | sin(2 pi d_i {1, 4}) | sin(.. + pi / 2)] of DDF queries at sphere positions `pos` along world
    directions `dirs` (ddf_model.py:158-200, directional_distance_field.py:188-191, 270-271)"""
    if pos.shape[0] == 0:  # (an absent section: the oracle's encoding cannot reshape no rows)
        return torch.zeros(0, 15, dtype=dtype)
    dl = O.ddf_local_direction(pos.to(dtype), dirs.to(dtype))
    return torch.cat([dl, O.nerf_encoding(dl, 2, 0.0, 2.0, False)], -1)


class Capture:
    """ddf_fn(sphere_pos, world_dir) -> read-out [M]; keeps (sphere_pos, row [M,15]) of every call, in call order"""

    def __init__(self, dtype, as_dict=False):
        self.dtype, self.as_dict, self.calls = dtype, as_dict, []

    def __call__(self, pos, dirs):
        r = rows(pos, dirs, self.dtype)
        self.calls.append((pos, r))
        t = r @ READOUT.to(self.dtype)
        return {"expected_termination_dist": t} if self.as_dict else t


def _unit(n, g):
    return torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)


def _ball(n, g):
    return _unit(n, g) * torch.rand(n, 1, generator=g) ** (1.0 / 3.0)


# ---- fit rows ----------------------------------------------------------------------------------------------------------------------
# (N, Ns, want_mv, radius, ldx): every value of every axis; E = N + n_mv + Ns below one workgroup (2, 2, 64, 226), one past a
# multiple of 256 (257 and 2 * 256 + 1) and many workgroups with a partly filled last one
FIT_CASES = ((1, 0, True, 1.0, 16), (1, 1, False, 2.5, 20), (63, 100, True, 2.5, 16), (63, 1, False, 1.0, 20),
             (257, 0, False, 1.0, 16), (257, 255, False, 2.5, 20), (257, 100, True, 2.5, 20), (1312, 1, True, 1.0, 20),
             (1312, 100, True, 2.5, 16), (1312, 0, False, 1.0, 16))
WEIGHT_MODES = tuple((z, e) for z in (False, True) for e in (3.0, 1.0, 2.5))
BWD_CASES = ((1, 1.0, 16), (1, 2.5, 20), (257, 1.0, 20), (257, 2.5, 16), (1312, 1.0, 16), (1312, 2.5, 20))  # (N, radius, ldx)
# column groups of the row: the raw, the sin and the shifted-sin columns of each of the three local axes
COLUMN_GROUPS = tuple((f"{kind}{i}", cols) for i in range(3)
                      for kind, cols in (("raw", (i,)), ("sin", (3 + 2 * i, 4 + 2 * i)), ("shifted", (9 + 2 * i, 10 + 2 * i))))
NODE_FIT, NODE_VIS = (24, 7, 2.5), (5, 51, 2.5)  # the autograd nodes' case: M = 255 is no multiple of N = 24, and N != Ns = 7
MV_MIN_LEN = 0.1  # x radius: the shortest multi-view ray of a case (1 / len is the backward's factor)


def fit_launch_rows(N, Ns, want_mv):
    return N + (N if want_mv else 0) + Ns


@functools.lru_cache(maxsize=None)
def fit_inputs(N, Ns, radius):
    """positions [N,3] on the upper half of the sphere of `radius`; directions [N,3] (unit) towards a point inside 0.7 radius and
    t [N] the distance to it; mv [N,3] UNIT vectors on the whole sphere (the kernel folds z; the reference's quirk, see the module
    docstring); sky_o [Ns,3] inside 0.5 radius and unit sky_d [Ns,3].  An inner point closer than 0.12 radius to its (folded)
    multi-view point is drawn again: MV_MIN_LEN is a condition on the inputs, and at radius 2.5 the unit sphere lies inside the
    ball the inner points come from."""
    g = torch.Generator().manual_seed(_seed("fit", N, Ns, radius))
    pos = _unit(N, g)
    pos[:, 2] = pos[:, 2].abs()
    pos = pos * radius
    mv = _unit(N, g)
    folded = mv.clone()
    folded[:, 2] = folded[:, 2].abs()
    inner = _ball(N, g) * (0.7 * radius)
    for _ in range(64):
        near = (inner - folded).norm(dim=-1) < 0.12 * radius
        if not near.any():
            break
        inner[near] = _ball(int(near.sum()), g) * (0.7 * radius)
    dv = inner - pos
    t = dv.norm(dim=-1)
    return dict(positions=pos.contiguous(), directions=(dv / t[:, None]).contiguous(), t=t.contiguous(), mv=mv.contiguous(),
                sky_o=(_ball(Ns, g) * (0.5 * radius)).contiguous(), sky_d=_unit(Ns, g).contiguous(),
                d_xrow=torch.randn(N, 15, generator=g))


def fold(mv):
    out = mv.clone()
    out[:, 2] = out[:, 2].abs()
    return out


def distance_weight(positions, radius, exp, include_z, dtype):
    """1 - (|p| / r)^e over (x, y) or (x, y, z) (ddf_model.py:224-238)"""
    p = positions.to(dtype)
    return 1.0 - ((p if include_z else p[:, :2]).norm(dim=-1) / radius) ** exp


def fit_reference(inp, radius, dtype, d_rows=None):
    """O.ddf_model_outputs in `dtype` with the capturing ddf_fn -> per section (fit, mv, sky) the sphere positions and the rows,
    the read-outs, sky_gt, the distance weight of the `neusky` config and, with d_rows [N,15], the gradient of
    sum(mv rows * d_rows) to t [N]"""
    c = lambda k: inp[k].to(dtype)  # noqa: E731
    t = c("t").clone().requires_grad_(d_rows is not None)  # (a clone: .to() of a float32 tensor to float32 is the cached input itself)
    cap = Capture(dtype)
    out = O.ddf_model_outputs(c("positions"), c("directions"), t[:, None], c("mv"), c("sky_o"), c("sky_d"), radius, cap,
                              lambda x: x[:, :1] * 0.0)
    (p_fit, r_fit), (p_mv, r_mv), (p_sky, r_sky) = cap.calls
    ref = dict(pos_fit=p_fit, rows_fit=r_fit, pos_mv=p_mv, rows_mv=r_mv, pos_sky=p_sky, rows_sky=r_sky,
               t_fit=out["expected_termination_dist"], t_mv=out["multi_view_expected_termination_dist"],
               t_sky=out["sky_ray_expected_termination_dist"], sky_gt=out["sky_ray_termination_dist"],
               distance_weight=out["distance_weight"],
               mv_len=(c("positions") + c("directions") * t[:, None] - p_mv).norm(dim=-1))
    if d_rows is not None:
        ref["d_t"], = torch.autograd.grad((r_mv * d_rows.to(dtype)).sum(), t)
    return {k: v.detach() for k, v in ref.items()}


def mv_rows_of_t(inp, t, dtype):
    """the multi-view rows [N,15] as a differentiable function of t [N] (`dtype`): ddf_model.py:286-298 through the oracle"""
    c = lambda k: inp[k].to(dtype)  # noqa: E731
    cap = Capture(dtype)
    none = torch.zeros(0, 3, dtype=dtype)
    O.ddf_model_outputs(c("positions"), c("directions"), t[:, None], c("mv"), none, none, 1.0, cap, lambda x: x[:, :1] * 0.0)
    return cap.calls[1][1]


def mv_t_gradient(inp, d_rows, dtype):
    """gradient of sum(mv rows * d_rows [N,15]) to t, in `dtype` (the radius takes no part in the multi-view rows)"""
    t = inp["t"].to(dtype).clone().requires_grad_(True)
    g, = torch.autograd.grad((mv_rows_of_t(inp, t, dtype) * d_rows.to(dtype)).sum(), t)
    return g


FIT_SECTIONS = ("fit", "mv", "sky")


@functools.lru_cache(maxsize=None)
def fit_case(N, Ns, radius):
    """-> inputs, float64 reference, float32 run of the same restatement (both with the gradient under inp['d_xrow'])"""
    inp = fit_inputs(N, Ns, radius)
    return inp, fit_reference(inp, radius, torch.float64, inp["d_xrow"]), fit_reference(inp, radius, torch.float32, inp["d_xrow"])


def group_probe(inp, cols):
    """inp['d_xrow'] with every column outside `cols` zeroed"""
    keep = torch.zeros(15)
    keep[list(cols)] = 1.0
    return inp["d_xrow"] * keep


# ---- G6: the reference's own recorded DDF-model outputs ----------------------------------------------------------------------------
G6_OUTPUTS = ("expected_termination_dist", "multi_view_expected_termination_dist", "sky_ray_expected_termination_dist",
              "sky_ray_termination_dist", "distance_weight")
G6_RTOL, G6_ATOL = 2e-5, 2e-6  # test_oracle_golden.test_g6_ddf_model_plumbing


def g6_head(g, dtype):
    """G6's stand-in DDF head on a sphere position p [M,3] and a row x [M,15]: sigmoid(x Wd + tanh(cat(p, sin(p Wp)) Wc)) 2"""
    Wp, Wd, Wc = (torch.from_numpy(g[k]).to(dtype) for k in ("Wp", "Wd", "Wc"))
    return lambda p, x: torch.sigmoid((x @ Wd + torch.tanh(torch.cat([p, torch.sin(p @ Wp)], -1) @ Wc))[..., 0]) * 2.0


def g6_oracle(g, inp, dtype):
    """test_g6_ddf_model_plumbing's evaluation of the oracle in `dtype` -> the five outputs the kernel's rows are pinned to"""
    head = g6_head(g, dtype)
    c = lambda a: torch.from_numpy(a).to(dtype)  # noqa: E731
    out = O.ddf_model_outputs(c(inp["positions"]), c(inp["directions"]), c(g["term"]), c(g["mv_points"]), c(g["sky_o"]), c(g["sky_d"]),
                              1.0, lambda pos, dirs: head(pos, rows(pos, dirs, dtype)), lambda x: x.norm(dim=-1, keepdim=True) - 0.5)
    return {k: out[k] for k in G6_OUTPUTS}


# ---- visibility rows ---------------------------------------------------------------------------------------------------------------
VIS_SHAPES = ((1, 1), (5, 51), (37, 7), (16, 256))  # (R, Dv)
BOUNDARY_MARGIN = 1e-5


def vis_cases():
    return [(R, Dv, radius) for R, Dv in VIS_SHAPES for radius in RADII]


def vis_scale(R, Dv, radius):
    """the sigmoid's sharpness: the configured 25 (most rows saturate) and 2 / radius (none does), in turn; the single row of
    (1, 1) is never saturated"""
    return 25.0 if R * Dv > 1 and (VIS_SHAPES.index((R, Dv)) + RADII.index(radius)) % 2 == 0 else F32(2.0 / radius)


@functools.lru_cache(maxsize=None)
def vis_inputs(R, Dv, radius):
    """origins / ray_dirs [R,3], depth [R]: ray 0 ends EXACTLY on the sphere (origin 0, direction (1,0,0), depth = radius: its norm
    is radius in float32 and in float64, so `!(norm < radius)` takes the fix-up branch in both), rays 1 .. R // 8 end outside it
    (depth 3 radius), the others inside.  dirs [D,3] of length 0.5 .. 1.5 with D = Dv + Dv // 2 + 1, of which the Dv at the
    ascending indices sel_index have z > 0; d_vis [R,D] the probe of the finish backward."""
    g = torch.Generator().manual_seed(_seed("vis", R, Dv, radius))
    o = (torch.rand(R, 3, generator=g) * 0.6 - 0.3) * radius  # |o| <= 0.52 radius: with a depth below 0.45 radius the ray ends inside
    d = _unit(R, g)
    depth = (0.1 + 0.35 * torch.rand(R, generator=g)) * radius
    n_out = R // 8 if R > 8 else min(R - 1, 1)
    depth[1:1 + n_out] = 3.0 * radius
    o[0] = 0.0
    d[0] = torch.tensor([1.0, 0.0, 0.0])
    depth[0] = radius
    D = Dv + Dv // 2 + 1
    dirs = _unit(D, g) * (0.5 + torch.rand(D, 1, generator=g))
    sel = torch.sort(torch.randperm(D, generator=g)[:Dv]).values
    upper = torch.zeros(D, dtype=torch.bool)
    upper[sel] = True
    dirs[:, 2] = torch.where(upper, dirs[:, 2].abs(), -dirs[:, 2].abs())
    return dict(origins=o.contiguous(), ray_dirs=d.contiguous(), depth=depth.contiguous(), dirs=dirs.contiguous(), sel_index=sel,
                n_outside=n_out, threshold=F32(0.35 * radius), scale=vis_scale(R, Dv, radius), d_vis=torch.randn(R, D, generator=g))


def vis_reference(inp, radius, dtype):
    """O.compute_visibility (upper hemisphere, lower value 1) in `dtype` with the capturing ddf_fn -> sphere_points [M,3],
    termination_dist [M], the clamped surf_dist [M], rows [M,15], the read-out t_hat [M], visibility [R,D], the end points of the
    rays before the fix-up and their norm"""
    c = lambda k: inp[k].to(dtype)  # noqa: E731
    cap = Capture(dtype, as_dict=True)
    out = O.compute_visibility(c("origins"), c("ray_dirs"), c("depth")[:, None], c("dirs"), torch.tensor(inp["threshold"], dtype=dtype),
                               inp["scale"], radius, cap)
    assert torch.equal(torch.nonzero(out["upper_mask"])[:, 0], inp["sel_index"])
    (pos, r), = cap.calls
    ends = c("origins") + c("ray_dirs") * c("depth")[:, None]
    return dict(sphere_points=out["sphere_points"], termination_dist=out["termination_dist"],
                surf_dist=out["termination_dist"].clamp(max=2.0 * radius), rows=r, t_hat=out["expected_termination_dist"],
                visibility=out["visibility"], end_norm=ends.norm(dim=-1))


def finish_reference(t_hat, surf_dist, inp, dtype):
    """vis = 1 - sigmoid(scale (surf_dist - t_hat - threshold)) on the selected directions (neusky_model.py:1730-1740; the
    formulation of test_gpu_render.test_visibility_geometry_golden) in `dtype` -> vis [R,Dv], the gradients of sum(vis d_vis) to
    t_hat [M] and to the threshold, and the per-row terms that the threshold's gradient sums"""
    R, Dv = inp["origins"].shape[0], inp["sel_index"].numel()
    t = t_hat.to(dtype).clone().requires_grad_(True)
    thr = torch.tensor(inp["threshold"], dtype=dtype)
    thr_rows = thr.expand(R * Dv).clone().requires_grad_(True)  # one threshold per row: its gradient is the per-row term
    v = 1.0 - torch.sigmoid(inp["scale"] * (surf_dist.to(dtype) - t - thr_rows))
    g_t, g_thr = torch.autograd.grad((v.view(R, Dv) * inp["d_vis"][:, inp["sel_index"]].to(dtype)).sum(), [t, thr_rows])
    return dict(vis=v.detach().view(R, Dv), d_t_hat=g_t, d_threshold_terms=g_thr, d_threshold=g_thr.sum())


@functools.lru_cache(maxsize=None)
def vis_case(R, Dv, radius):
    """-> inputs, float64 and float32 run of the rays' restatement, and the finish kernels' inputs (float32 roundings of the float64
    read-out and surf_dist: the finish test does not depend on the rays kernel) with their float64 and float32 references"""
    inp = vis_inputs(R, Dv, radius)
    ref, ref32 = vis_reference(inp, radius, torch.float64), vis_reference(inp, radius, torch.float32)
    t_hat, sdist = ref["t_hat"].float(), ref["surf_dist"].float()
    return inp, ref, ref32, dict(t_hat=t_hat, surf_dist=sdist, ref=finish_reference(t_hat, sdist, inp, torch.float64),
                                 ref32=finish_reference(t_hat, sdist, inp, torch.float32))


def threshold_bar(terms64):
    """the bar of d_threshold, a sum of R Dv terms by float32 atomics in no fixed order: 4 x the distance between a float32 sum of
    the float64 per-row terms and their float64 sum, with a floor of 4 float32 roundings of sum |terms|"""
    return max(4.0 * abs(terms64.float().sum().double().item() - terms64.sum().item()), 4.0 * EPS32 * terms64.abs().sum().item())


# ---- the drawn multi-view points ---------------------------------------------------------------------------------------------------
DRAW_N, DRAW_CALLS = 4096, 64


def oracle_hemisphere_draws(calls, n, seed):
    """float64 draws of the oracle's construction of a point on the upper unit hemisphere (O.vmf_ddf_rays: theta = 2 pi u,
    cos(phi) = 2 u - 1, then fold z) -> [calls, n, 3]"""
    pts, _ = O.vmf_ddf_rays(calls * n, 1, 20.0, 1.0, torch.Generator().manual_seed(seed))
    return pts.view(calls, n, 3)


def _corr(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    a, b = a - a.mean(), b - b.mean()
    return ((a * b).mean() / (a.std(unbiased=False) * b.std(unbiased=False))).item()


def hemisphere_statistics(pts):
    """pts [calls, N, 3] -> [(name, value, expected, bound)]: z uniform on [0, 1), the azimuth uniform, the two independent, and
    no correlation of z between successive calls or neighbouring rows.  Every bound is six standard errors of its estimator,
    computed from n = calls * N."""
    pts = pts.double()
    calls, N, _ = pts.shape
    n = calls * N
    z = pts[..., 2]
    theta = torch.atan2(pts[..., 1], pts[..., 0])
    xy = pts[..., :2].norm(dim=-1)
    out = [("mean z", z.mean().item(), 0.5, 6.0 * math.sqrt(1.0 / 12.0) / math.sqrt(n)),
           ("var z", z.var(unbiased=False).item(), 1.0 / 12.0, 6.0 * math.sqrt((1.0 / 80.0 - 1.0 / 144.0) / n)),
           ("mean cos theta", (pts[..., 0] / xy).mean().item(), 0.0, 6.0 * math.sqrt(0.5) / math.sqrt(n)),
           ("mean sin theta", (pts[..., 1] / xy).mean().item(), 0.0, 6.0 * math.sqrt(0.5) / math.sqrt(n))]
    az = torch.clamp(((theta + math.pi) / (2.0 * math.pi) * 16.0).floor().long(), 0, 15)
    zc = torch.clamp((z * 8.0).floor().long(), 0, 7)
    hist = torch.bincount((az * 8 + zc).reshape(-1), minlength=128).double()
    p = 1.0 / 128.0
    worst = (hist - n * p).abs().max().item()
    out.append(("histogram cell 16 x 8 (largest deviation)", n * p + worst, n * p, 6.0 * math.sqrt(n * p * (1.0 - p))))
    out.append(("corr z, call k / k + 1", _corr(z[:-1], z[1:]), 0.0, 6.0 / math.sqrt(n)))
    out.append(("corr z, row j / j + 1", _corr(z[:, :-1], z[:, 1:]), 0.0, 6.0 / math.sqrt(n)))
    return out


# ---- the generator behind the draws ------------------------------------------------------------------------------------------------
MV_STREAM = 0x6d76  # the stream id of the multi-view draw (csrc/samplers.hip: mv_point); the sampler's positions use stream 0


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al. 2011) on uint32 arrays counter [n,4] and key [2] -> [n,4]"""
    c = [np.asarray(counter[:, i], dtype=np.uint64) for i in range(4)]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    m32 = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & m32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return np.stack(c, 1).astype(np.uint32)


def philox_mv_points(seed, call, n, dtype):
    """the multi-view points of call number `call` as csrc/samplers.hip documents them: words of Philox4x32-10 under the key
    (seed low, seed high) at the counter (row, MV_STREAM, call low, call high); u = ((w >> 9) + 1 / 2) / 2^23 strictly inside (0, 1);
    theta = 2 pi u0, cos(phi) = 2 u1 - 1, then the fold z = |z| (ddf_model.py:290-295) -> [n,3] in `dtype`"""
    ctr = np.zeros((n, 4), dtype=np.uint32)
    ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3] = np.arange(n), MV_STREAM, call & 0xFFFFFFFF, call >> 32
    w = philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    u = (torch.from_numpy((w[:, :2] >> 9).astype(np.int64)).to(dtype) + 0.5) / 8388608.0  # exact in float32 and in float64
    theta = (2.0 * math.pi) * u[:, 0]
    cphi = 2.0 * u[:, 1] - 1.0
    sphi = torch.sqrt((1.0 - cphi * cphi).clamp(min=0.0))
    return torch.stack([sphi * torch.cos(theta), sphi * torch.sin(theta), cphi.abs()], 1)
