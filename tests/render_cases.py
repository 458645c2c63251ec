"""Inputs and references for the edge tests of the render kernels (neusky_amd/csrc/render.hip): NeuS alpha -> transmittance ->
weights, the hash-grid probe's point alphas, the hemisphere composite, the proposal density weights and the interlevel loss.

Deterministic builders (torch.Generator / numpy seeds, float32 tensors) and the restatements of each operation, run in float64
(the reference the kernels are held to) and in float32 (what plain float32 arithmetic makes of the same inputs: the conditioning
of a case, and the unit of the kernels' gradient bar).  Every restatement is an oracle function that exists -- O.neus_alpha,
O.weights_from_alphas, O.lambertian_render, O._outer, ray_samplers.weights_from_density -- under torch autograd; nothing here
needs a GPU.  test_render_cases_cpu.py proves what the cases are meant to reach, test_gpu_render_edges.py runs the kernels."""
import functools
import math

import numpy as np
import torch

import inputs as gi
from oracle import neusky_oracle as O

VARIANCES = (0.32, 0.6, 0.9, 1.2, 1.5)  # inv_s = e^(10 v): 24.5, 403, 8103, 1.6e5 and, past the clamp, 1e6 (e^15 = 3.3e6)
ANNEALS = (0.0, 0.37, 1.0)
NEUS_S = (1, 63, 64, 65, 129, 192, 256)  # CH = ceil(S / 64) = 1, 1, 1, 2, 3, 3, 4; last_lane = (S - 1) / CH = 0, 62, 63, 32, 42, 63, 63
POINT_P = (1, 63, 64, 65, 257)
F32 = lambda v: float(np.float32(v))  # noqa: E731  (a Python float as the C ABI's `float` argument sees it)


def inv_s_of(variance):
    return min(max(math.exp(10.0 * F32(variance)), 1e-6), 1e6)


def rel_to_max(got, ref):
    """largest |got - ref| over the largest |ref| (0 where both tensors vanish)"""
    err, scale = (got.double() - ref.double()).abs().max().item(), ref.double().abs().max().item()
    return 0.0 if err == 0.0 else err / scale if scale > 0 else float("inf")


# ---- NeuS weights ----------------------------------------------------------------------------------------------------------------
def neus_cases():
    """(family, variance, anneal, R, S).  Under every anneal: every S, every variance, both R (R = 9: the third workgroup holds one
    ray) in the resolved family; the coarse family at variance 0.6 and 0.9 with CH = 3 and S = 256."""
    cases = []
    for k, an in enumerate(ANNEALS):
        for i, S in enumerate(NEUS_S):
            cases.append(("resolved", VARIANCES[(i + k) % 5], an, (1, 9)[(i + k) % 2], S))
        # (finer bins saturate fewer samples: at variance 0.6 the required tenth of alphas >= 0.999 is there up to S = 192, and
        # S = 256 goes with variance 0.9, where half of them are)
        cases.append(("coarse", 0.6, an, 37, (129, 192, 129)[k]))
        cases.append(("coarse", 0.9, an, 9, (256, 192, 256)[k]))
    return cases


# case -> seed, where the first seed missed a condition of test_render_cases_cpu.py.  No NeuS or point case had to move; the
# D = 1024 hemisphere case had one |n.l| = 8.7e-6 among its 30 720 dots under seed 1129, below the 1e-5 margin (2.3e-5 under 1134).
RESEEDED = {("hemi", 6, 5, 1024, 2): 1134}


def _seed(*key):
    if key in RESEEDED:
        return RESEEDED[key]
    return int(sum((j + 1) * 7919 * round(1000 * float(v)) for j, v in enumerate(key[1:]))) % (2 ** 31) + len(key[0])


def _ray_geometry(R, S, g):
    """unit ray directions; gradients of norm 1 +- 0.1 that mostly face the ray (a falling sdf), some turned away from it"""
    dirs = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1)
    grad = torch.nn.functional.normalize(-dirs[:, None, :] + 0.8 * torch.randn(R, S, 3, generator=g), dim=-1)
    return dirs, grad * (1.0 + 0.1 * (2.0 * torch.rand(R, S, 1, generator=g) - 1.0))


@functools.lru_cache(maxsize=None)
def neus_inputs(family, variance, anneal, R, S):
    """sdf [R,S], grad [R,S,3], dirs [R,3], starts / ends [R,S], variance [1], the probes gw [R,S] and gT [R] of the loss
    sum(w gw) + sum(T_bg gT).  Both families: the sdf falls along the ray from + to - (ramp + a per-ray offset + noise).
    resolved: sdf in units of 8 / inv_s and intervals of 16 / (inv_s S) (0.5 .. 1.5 of it), so the sigmoid's argument runs
    over +-8 and the crossing spans several samples whatever the sharpness.  coarse: sdf at the fixed scale 0.05 and sorted random
    bins over [0.05, 2.05] (the bins of test_gpu_render._alpha_inputs): from variance 0.6 on the sigmoid is a step, alphas reach 1
    and the transmittance behind the surface leaves the normal float32 range."""
    g = torch.Generator().manual_seed(_seed(family, variance, anneal, R, S))
    inv_s = inv_s_of(variance)
    ramp = 1.0 - 2.0 * (torch.arange(S, dtype=torch.float64) + 0.5) / S
    offset = (torch.rand(R, 1, generator=g, dtype=torch.float64) - 0.5) * 0.3
    noise = torch.randn(R, S, generator=g, dtype=torch.float64)
    if family == "resolved":
        sdf = (ramp + offset + 0.05 * noise) * (8.0 / inv_s)
        delta = (16.0 / (inv_s * S)) * (0.5 + torch.rand(R, S, generator=g, dtype=torch.float64))
        bins = 0.05 + torch.cat([torch.zeros(R, 1, dtype=torch.float64), torch.cumsum(delta, dim=1)], dim=1)
    else:
        assert family == "coarse"
        sdf = (ramp + offset + 0.1 * noise) * 0.05
        bins = torch.sort(torch.rand(R, S + 1, generator=g, dtype=torch.float64) * 2 + 0.05, dim=1).values
    bins = bins.float()
    dirs, grad = _ray_geometry(R, S, g)
    return dict(sdf=sdf.float(), grad=grad, dirs=dirs, starts=bins[:, :-1].contiguous(), ends=bins[:, 1:].contiguous(),
                variance=torch.tensor([variance], dtype=torch.float32), anneal=F32(anneal),
                gw=torch.randn(R, S, generator=g), gT=torch.randn(R, generator=g))


KINK_R, KINK_S = 5, 12


@functools.lru_cache(maxsize=None)
def kink_inputs(anneal):
    """the resolved family at variance 0.32 with dirs = (0,0,1) and the gradients of samples 0, 1, 2, 0, ... exactly (0,0,1), (1,0,0),
    (0,0,-1): cos = 1, 0, -1 with no rounding, the kinks of relu(-cos / 2 + 1 / 2) and relu(-cos) and a point off both"""
    inp = dict(neus_inputs("resolved", 0.32, anneal, KINK_R, KINK_S))
    three = torch.tensor([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 0.0, -1.0]])
    inp["grad"] = three[torch.arange(KINK_S) % 3][None].expand(KINK_R, KINK_S, 3).contiguous()
    inp["dirs"] = torch.tensor([0.0, 0.0, 1.0]).expand(KINK_R, 3).contiguous()
    return inp


def neus_reference(inp, dtype):
    """O.neus_alpha + O.weights_from_alphas in `dtype`, with accumulation, expected depth and the gradients of
    sum(w gw) + sum(T_bg gT) to sdf, gradients and variance.  T [R,S+1] is the whole transmittance: T[:, 0] = 1, T[:, -1] = T_bg."""
    c = lambda k: inp[k].to(dtype)  # noqa: E731
    R, S = inp["sdf"].shape
    sd, gd, vd = c("sdf").requires_grad_(True), c("grad").requires_grad_(True), c("variance").requires_grad_(True)
    a = O.neus_alpha(sd[..., None], gd, c("dirs")[:, None, :].expand(R, S, 3), (c("ends") - c("starts"))[..., None], vd, inp["anneal"])
    w, T = O.weights_from_alphas(a)
    w, T = w[..., 0], T[..., 0]
    acc = w.sum(1)
    mid = (c("starts") + c("ends")) / 2
    depth = (w * mid).sum(1) / (acc + 1e-10)
    loss = (w * c("gw")).sum() + (T[:, -1] * c("gT")).sum()
    gs, gg, gv = torch.autograd.grad(loss, [sd, gd, vd])
    return dict(alpha=a[..., 0].detach(), weights=w.detach(), T=T.detach(), T_bg=T[:, -1].detach(), accumulation=acc.detach(),
                depth=depth.detach(), mid=mid, d_sdf=gs, d_grad=gg, d_variance=gv)


NEUS_FORWARD = ("alpha", "weights", "T", "accumulation", "depth")
NEUS_GRADS = ("d_sdf", "d_grad", "d_variance")
DEPTH_MIN_ACC = 1e-3  # below it sum(w mid) / (sum(w) + 1e-10) is a ratio of two roundings: depth is compared only on rays above it


def restatement_error(ref32, ref64, names):
    """float32 run of a restatement against its float64 run, relative to the largest reference entry of each tensor.  The NeuS
    depth counts on the rays the reference gives an accumulation above DEPTH_MIN_ACC only.  T_bg is judged as part of T, whose
    scale is T[:, 0] = 1: behind a surface T_bg is a product of (1 - alpha + 1e-7) factors that float32 resolves to a few digits,
    of a size (1e-10 and below) nothing downstream can see."""
    out = {}
    for k in names:
        a, b = ref32[k], ref64[k]
        if k == "depth":
            on = ref64["accumulation"] > DEPTH_MIN_ACC
            a, b = a[on], b[on]
        out[k] = rel_to_max(a, b) if b.numel() else 0.0
    return out


@functools.lru_cache(maxsize=None)
def neus_case(family, variance, anneal, R, S):
    """-> inputs, float64 reference, float32-restatement error of each forward quantity and gradient"""
    inp = neus_inputs(family, variance, anneal, R, S)
    ref = neus_reference(inp, torch.float64)
    return inp, ref, restatement_error(neus_reference(inp, torch.float32), ref, NEUS_FORWARD + NEUS_GRADS)


@functools.lru_cache(maxsize=None)
def neus_case_without_gT(family, variance, anneal, R, S):
    """the same case under the loss sum(w gw) alone: what a null d_trans_bg means.  -> float64 reference, restatement errors"""
    inp = dict(neus_inputs(family, variance, anneal, R, S), gT=torch.zeros(R))
    ref = neus_reference(inp, torch.float64)
    return ref, restatement_error(neus_reference(inp, torch.float32), ref, NEUS_GRADS)


@functools.lru_cache(maxsize=None)
def kink_case(anneal):
    inp = kink_inputs(anneal)
    ref = neus_reference(inp, torch.float64)
    return inp, ref, restatement_error(neus_reference(inp, torch.float32), ref, NEUS_FORWARD + NEUS_GRADS)


# ---- point alphas ----------------------------------------------------------------------------------------------------------------
def point_cases():
    """(variance, anneal, P): every P and every variance under every anneal"""
    return [(VARIANCES[(i + k) % 5], an, P) for k, an in enumerate(ANNEALS) for i, P in enumerate(POINT_P)]


@functools.lru_cache(maxsize=None)
def point_inputs(variance, anneal, P):
    """P isolated samples scaled as the resolved family: sdf within 8 / inv_s of the surface, three gaps of order 16 / inv_s"""
    g = torch.Generator().manual_seed(_seed("point", variance, anneal, P))
    inv_s = inv_s_of(variance)
    sdf = ((2.0 * torch.rand(P, generator=g, dtype=torch.float64) - 1.0) * (8.0 / inv_s)).float()
    dirs, grad = _ray_geometry(P, 1, g)
    gaps = [F32(16.0 / inv_s * f) for f in (0.06, 0.11, 0.23)]
    return dict(sdf=sdf, grad=grad[:, 0].contiguous(), dirs=dirs, gaps=gaps, variance=torch.tensor([variance], dtype=torch.float32),
                anneal=F32(anneal), probe=torch.randn(P, 3, generator=g))


def point_reference(inp, dtype):
    """O.neus_alpha itself on sdf [P,1] and deltas = gaps[None,:] -> alphas [P,3], and the gradients of sum(alphas probe)"""
    c = lambda k: inp[k].to(dtype)  # noqa: E731
    sd, gd, vd = c("sdf").requires_grad_(True), c("grad").requires_grad_(True), c("variance").requires_grad_(True)
    a = O.neus_alpha(sd[:, None], gd, c("dirs"), torch.tensor(inp["gaps"], dtype=dtype)[None, :], vd, inp["anneal"])
    gs, gg, gv = torch.autograd.grad((a * c("probe")).sum(), [sd, gd, vd])
    return dict(alpha=a.detach(), d_sdf=gs, d_grad=gg, d_variance=gv)


@functools.lru_cache(maxsize=None)
def point_case(variance, anneal, P):
    inp = point_inputs(variance, anneal, P)
    ref = point_reference(inp, torch.float64)
    return inp, ref, restatement_error(point_reference(inp, torch.float32), ref, ("alpha",) + NEUS_GRADS)


# ---- hemisphere composite --------------------------------------------------------------------------------------------------------
HEMI_SHAPES = ((6, 1, 1, 1), (9, 3, 65, 3), (9, 4, 64, 3), (7, 5, 63, 2), (6, 5, 1024, 2))  # (R, S, D, U), U < R: rays share cameras
HEMI_SCALES = (1.0, 0.05, 0.002)  # on bg and cam_colours: composites above 1 (outdoor light), inside the curve, on its linear segment
HEMI_KEYS = ("albedo", "normals", "cam_colours", "vis", "bg", "weights")
SRGB_KNEE = 0.0031308


def hemi_cases():
    return [shape + (scale,) for shape in HEMI_SHAPES for scale in HEMI_SCALES]


HEMI_OPTIONAL = ((9, 3, 65, 3, 1.0), (6, 5, 1024, 2, 0.05))  # the cases also run without vis, without d_vis, without d_cam_colours


@functools.lru_cache(maxsize=None)
def hemi_inputs(R, S, D, U, scale):
    """inputs.lambertian_inputs with its one zeroed normal replaced (n.l = 0 on every direction is the kink of the clamp) and the
    light scaled; float32 tensors, cam_of_ray int64, d_rgb the probe of the backward"""
    inp = gi.lambertian_inputs(seed=RESEEDED.get(("hemi", R, S, D, U), 100 + D + S), R=R, S=S, D=D, U=U)
    inp["normals"][0, 0] = inp["normals"][-1, -1] if R * S > 1 else gi.unit(np.array([0.3, -0.5, 0.8], np.float32))
    out = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in inp.items()}
    out["bg"] = out["bg"] * scale
    out["cam_colours"] = out["cam_colours"] * scale
    out["d_rgb"] = torch.randn(R, 3, generator=torch.Generator().manual_seed(R + S + D))
    return out


def _hemi_render(td, dirs, cam_of_ray, with_vis):
    return O.lambertian_render(td["albedo"], td["normals"], dirs, td["cam_colours"], cam_of_ray, td["vis"] if with_vis else None,
                               td["bg"], td["weights"])


def hemi_reference(inp, dtype=torch.float64, with_vis=True):
    """O.lambertian_render (training) in `dtype`: rgb, the linear composite the curve is applied to, and the gradients of
    sum(rgb d_rgb) to every input (vis: None without it)"""
    td = {k: inp[k].to(dtype).requires_grad_(True) for k in HEMI_KEYS}
    dirs = inp["dirs"].to(dtype)
    rgb = _hemi_render(td, dirs, inp["cam_of_ray"], with_vis)
    keys = [k for k in HEMI_KEYS if with_vis or k != "vis"]
    grads = dict(zip(keys, torch.autograd.grad((rgb * inp["d_rgb"].to(dtype)).sum(), [td[k] for k in keys])))
    curve = O.linear_to_srgb
    O.linear_to_srgb = lambda colour: colour  # the same composite with the curve taken out, not a second statement of it
    try:
        with torch.no_grad():
            lin = _hemi_render(td, dirs, inp["cam_of_ray"], with_vis)
    finally:
        O.linear_to_srgb = curve
    return dict(rgb=rgb.detach(), lin=lin, grads=grads, dot=torch.einsum("rsi,ji->rsj", td["normals"].detach(), dirs))


@functools.lru_cache(maxsize=None)
def hemi_case(R, S, D, U, scale, with_vis=True):
    inp = hemi_inputs(R, S, D, U, scale)
    return inp, hemi_reference(inp, torch.float64, with_vis)


# ---- proposal density weights ----------------------------------------------------------------------------------------------------
DENSITY_N = (1, 64, 65, 130, 192)  # CH = 1, 1, 2, 3, 3


def density_cases():
    return [(n, R, ld) for n in DENSITY_N for R in (1, 9) for ld in (1, 4)]


def density_edge_slots(n, R, ld):
    """per ray (index of the raw = -30 entry or None, index of the raw = 40 entry or None).  Lane l owns bins [l CH, (l + 1) CH)
    that lie below n: both entries sit in the LAST slot a lane owns.  The -30 entry (below trunc_exp's backward clamp at -15) is
    lane 1's last slot, ahead of the saturated one, so it keeps a transmittance and a gradient; the saturated entry (alpha = 1,
    every later weight exactly 0) is the last slot of a middle lane on even rays and bin n - 1, the last lane's last owned slot
    (a partly filled chunk when n is no multiple of CH), on odd rays.  n = 1 has one slot: -30 on odd rays (ld 4 where R = 1)."""
    CH = (n + 63) // 64
    last_lane = (n - 1) // CH
    slots = []
    for r in range(R):
        if n == 1:
            low = (r % 2 == 1) if R > 1 else ld == 4
            slots.append((0, None) if low else (None, 0))
        else:
            slots.append((2 * CH - 1, (last_lane // 2) * CH + CH - 1 if r % 2 == 0 else n - 1))
    return slots


@functools.lru_cache(maxsize=None)
def density_inputs(n, R, ld):
    g = torch.Generator().manual_seed(_seed("density", n, R, ld))
    raw = torch.zeros(R * n, ld)
    raw[:, 0] = torch.randn(R * n, generator=g) * 2.0
    for r, (low, sat) in enumerate(density_edge_slots(n, R, ld)):
        if low is not None:
            raw[r * n + low, 0] = -30.0
        if sat is not None:
            raw[r * n + sat, 0] = 40.0
    ebins = torch.sort(torch.rand(R, n + 1, generator=g) * 2 + 0.05, dim=1).values
    return dict(raw=raw, ebins=ebins, probe=torch.randn(R, n, generator=g))


@functools.lru_cache(maxsize=None)
def density_case(n, R, ld):
    """-> inputs, float64 weights [R,n] and gradient of sum(w probe) to raw[:, 0]: trunc_exp + ray_samplers.weights_from_density,
    the formulation of test_gpu_render.test_density_weights_matches_torch_formulation"""
    from neusky_amd import ops
    from neusky_amd.model_components.ray_samplers import weights_from_density
    inp = density_inputs(n, R, ld)
    r64 = inp["raw"].double().requires_grad_(True)
    dens = ops.TruncExpFn.apply(r64[:, :1]).view(R, n, 1)
    w = weights_from_density(dens, (inp["ebins"][:, 1:] - inp["ebins"][:, :-1]).double()[..., None])[..., 0]
    (w * inp["probe"].double()).sum().backward()
    return inp, dict(weights=w.detach(), d_raw=r64.grad[:, 0])


# ---- interlevel loss -------------------------------------------------------------------------------------------------------------
def interlevel_cases():
    """(R, S, n, ties): one sample and one bin; a partly filled last workgroup with S > 64 (the lane-stride loop's second pass);
    the LDS limit n = 1023; and the proposal sizes' (96, 64) with and without final-level edges ON proposal edges"""
    return [(1, 1, 1, False), (9, 65, 5, False), (5, 130, 1023, False), (9, 96, 64, False), (9, 96, 64, True)]


@functools.lru_cache(maxsize=None)
def interlevel_inputs(R, S, n, ties):
    g = torch.Generator().manual_seed(_seed("interlevel", R, S, n, ties))

    def edges(m, given=None):
        inner = torch.rand(R, m - 2 - (0 if given is None else given.shape[1]), generator=g)
        e = torch.cat([torch.zeros(R, 1), inner, torch.ones(R, 1)] + ([] if given is None else [given]), dim=1)
        return torch.sort(e, dim=1).values.contiguous()

    sb = edges(n + 1)
    # ties: every fourth proposal edge is a final-level edge too (the ends 0 and 1 always are), so searchsorted(right) meets equal
    # values in the middle of the row
    c = edges(S + 1, sb[:, 4:-1:4] if ties else None)
    wp = torch.rand(R, n, generator=g) / n  # sums to ~0.5 whatever n
    w = torch.rand(R, S, generator=g) * (1.5 / S)  # around the outer measure: intervals on both sides of max(w - w_outer, 0)
    if S > 1:
        w[:, S // 3:S // 3 + 2] += 0.3
    else:
        w += 0.4
    return dict(c=c, w=w, sb=sb, wp=wp, probe=torch.rand(R, generator=g) + 0.5)


@functools.lru_cache(maxsize=None)
def interlevel_case(R, S, n, ties):
    """-> inputs, float64 per-ray sums of max(w - w_outer, 0)^2 / (w + 1e-7) with w_outer = O._outer, the gradient of
    sum(per_ray probe) to the proposal weights, w - w_outer, and `covered` [R,n]: the bins inside [lo, hi] of an ACTIVE interval
    (w > w_outer), lo / hi being the two searchsorted(right) indices of O._outer.  Every other bin takes no part in the loss: its
    gradient is 0 (autograd's reverse cumsum leaves +-1e-15 there; the kernel must write exactly 0).  A covered bin's terms all
    carry the sign of -probe < 0, so they cannot cancel."""
    inp = interlevel_inputs(R, S, n, ties)
    c, w, sb = inp["c"].double(), inp["w"].double(), inp["sb"].double()
    wp = inp["wp"].double().requires_grad_(True)
    w_outer = O._outer(c[..., :-1], c[..., 1:], sb[..., :-1], sb[..., 1:], wp)
    per_ray = (torch.clip(w - w_outer, min=0) ** 2 / (w + 1e-7)).sum(-1)
    (per_ray * inp["probe"].double()).sum().backward()
    margin = (w - w_outer).detach()
    lo = torch.clamp(torch.searchsorted(sb[..., :-1].contiguous(), c[..., :-1].contiguous(), side="right") - 1, 0, n - 1)
    hi = torch.clamp(torch.searchsorted(sb[..., 1:].contiguous(), c[..., 1:].contiguous(), side="right"), 0, n - 1)
    j = torch.arange(n)[None, None, :]
    covered = ((j >= lo[..., None]) & (j <= hi[..., None]) & (margin > 0)[..., None]).any(1)
    return inp, dict(per_ray=per_ray.detach(), d_wp=wp.grad, margin=margin, covered=covered)
