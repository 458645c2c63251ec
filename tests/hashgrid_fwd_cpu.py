"""float64 restatement of the hash-grid encode FORWARD (neusky_amd/csrc/hashgrid.hip: encode_fwd_kernel in its three forms, and the
input gradient of encode_bwd_kernel) and the cases the kernels are held to, column group by column group.

One row is [x | PE(x) | hash(pos(x))]; its tangent rows are T_k = d row / d x_k, the directional row is Td = sum_k d_k T_k and the
input gradient under a row gradient dY is dx_b = sum_c dY_c T_b,c.  Everything is written out (no autograd) and runs in the dtype it
is handed: float64 is the reference, float32 is what plain float32 arithmetic (torch's operation order) makes of the same inputs --
the unit of every bar.  The CELL of a point is not part of the arithmetic under test: it is the one O.hash_grid_indices picks for the
position evaluated in float32 (test_gpu_hashgrid.test_indices_bit_exact pins the kernel to that choice), in both dtypes; with it
t = pos * scale + 0.5 - floor extrapolates across a face exactly as the kernel's cell does.

Columns are grouped as `x`, each PE frequency (its sin and shifted-sin columns on all three axes) and each hash level (its two
features).  Per group and quantity,  bar = max(4 max|ref32 - ref64| over the case's whole pool, 4 * 2^-23 * largest |ref64|)  (the
convention of ddf_rows_cases.bar); for dx the floor is per entry, 4 * 2^-23 * A_b with A_b = sum_c |dY_c| |T_b,c|.  Nothing measured
on a kernel goes into a bar.

Three kinds of pool point are compared for less than everything, by construction of the point and not of the result:
  * the L-infinity tie (1.5, 1.5, 0.2): its tangent is a subgradient -- values and finiteness only;
  * (3e38, 1, 1) under the L2 norm: x . x overflows float32 (the kernel and the float32 oracle both see m = inf), so float64 is no
    reference for it -- finiteness only; (1e18, 1, 1) takes its place as the point whose position reaches 1.0;
  * |x| > PE_MAX_X: 2 pi x 2^5 has an ulp of 0.016 and more there (inf at 3e38), so the PE columns of far points say nothing about
    the kernel and are left out of the PE groups (bars and comparisons); their x and hash columns are compared as any other.
    Where that argument overflows float32 ((3e38, 1, 1)) a PE column is NaN, and in the input gradient a zero row gradient does not
    remove it (0 * NaN): a case WITH PE columns compares no dx at that point, in any group.
Nothing here needs a GPU or imports the package: test_hashgrid_fwd_cpu.py proves the cases and the bars fit to test with,
test_gpu_hashgrid_fwd.py runs the kernels."""
import functools
import math
from dataclasses import dataclass

import numpy as np
import torch

import hashgrid_bwd_cpu as HB
from oracle import neusky_oracle as O

EPS32 = 2.0 ** -23
POOL = 4096          # seeded points of a case, after its edge points
PE_MAX_X = 4.0       # largest |x_i| whose PE columns are compared (the scene lives inside |x| < 2 or so)
CELL_CAP_LINF = 1e-4  # of a mode-1 case's (point, level) pairs may sit in another cell than the reference's; modes 0 and 2: none
TABLE_SCALE = 0.5
DEFECTS = ("dk", "no_quarter", "level0_scale", "smoothstep_derivative", "pe_step", "identity_entry", "shifted_sin_sign", "neighbour_dir")
SMOOTH_DEFECT_LEVEL = 3


@dataclass(frozen=True)
class Case:
    name: str
    n_levels: int
    log2T: int
    max_res: int
    smooth: bool
    mode: int
    include_x: bool
    pe: int
    pe_max_exp: float
    points: str  # "box": uniform in [-1.3, 1.3]^3 (mode 0: [-1, 1]^3); "sphere": unit-sphere points
    seed: int

    @property
    def width(self):
        return (3 if self.include_x else 0) + 6 * self.pe + 2 * self.n_levels

    @property
    def ldy(self):
        return (self.width + 3) // 4 * 4

    @property
    def feat0(self):
        return (3 if self.include_x else 0) + 6 * self.pe

    def cfg(self):
        return O.HashGridCfg(n_levels=self.n_levels, log2_hashmap_size=self.log2T, base_res=16, max_res=self.max_res, smoothstep=self.smooth)

    def groups(self):
        """[(name, columns)]"""
        out = []
        if self.include_x:
            out.append(("x", (0, 1, 2)))
        pe0, F = (3 if self.include_x else 0), self.pe
        for f in range(F):
            out.append((f"pe{f}", tuple(pe0 + half * 3 * F + i * F + f for half in (0, 1) for i in range(3))))
        for l in range(self.n_levels):
            out.append((f"level{l}", (self.feat0 + 2 * l, self.feat0 + 2 * l + 1)))
        return out


CASES = {c.name: c for c in (
    # the SDF field's call (sdf_albedo_field.py: [x | PE6 | hash], smoothstep), under both contraction norms
    Case("sdf_linf", 16, 19, 2048, True, 1, True, 6, 5.0, "box", 101),
    Case("sdf_l2", 16, 19, 2048, True, 2, True, 6, 5.0, "box", 102),
    # the DDF's call (directional_distance_field.py: [p | hash(p)] of raw unit-sphere points)
    Case("ddf", 16, 19, 2048, False, 0, True, 0, 0.0, "sphere", 103),
    # the two proposal networks (ray_samplers.py: hash only)
    Case("prop64", 5, 17, 64, False, 1, False, 0, 0.0, "box", 104),
    Case("prop256", 5, 17, 256, False, 1, False, 0, 0.0, "box", 105),
    # fewer levels than waves of a workgroup; a row with no pad column
    Case("small1", 1, 19, 16, False, 0, False, 0, 0.0, "box", 106),
    Case("small3", 3, 12, 64, True, 1, False, 0, 0.0, "box", 107),
    Case("small6", 6, 14, 128, True, 2, False, 0, 0.0, "box", 108),
)}
# geometry -> (resolutions, dense?) as the issue's table states them
GEOMETRY = {"prop64": ([16, 23, 32, 46, 64], [True, True, True, True, False]),
            "prop256": ([16, 32, 64, 128, 256], [True, True, False, False, False])}
TANGENT_CASES = ("sdf_linf", "sdf_l2", "small3")
DIR_CASES = ("sdf_linf", "sdf_l2")
DX_CASES = ("sdf_linf", "sdf_l2", "ddf")


# ---- the points ---------------------------------------------------------------------------------------------------------------------
STEP_IN, STEP_OUT = float(np.nextafter(np.float32(1), np.float32(0))), float(np.nextafter(np.float32(1), np.float32(2)))
_U2 = (0.36, -0.48, 0.8)  # a unit vector in the reals; in float32 its norm lands beside 1


def edge_points(mode):
    """[(name, (x, y, z))], prepended to a case's pool"""
    pts = []
    if mode == 0:
        pts += [("plus_one", (1.0, 1.0, 1.0)), ("minus_one", (-1.0, -1.0, -1.0)), ("mixed_one", (1.0, -1.0, 0.25)), ("origin", (0.0, 0.0, 0.0))]
        g = torch.Generator().manual_seed(64)
        k = torch.randint(-(HB.LATTICE - 1), HB.LATTICE, (64, 3), generator=g)
        pts += [(f"lattice{i}", tuple((k[i].double() / HB.LATTICE).tolist())) for i in range(64)]
        # cell faces of level 0 (scale 15): 15 x + 0.5 integral
        pts += [(f"face{j}", ((2 * j + 1) / 30.0, -(2 * j + 3) / 30.0, (2 * j + 5) / 30.0)) for j in (0, 4, 9)]
        return pts
    if mode == 1:
        pts += [("surface", (1.0, 0.3, -0.5)), ("surface_neg", (-0.25, -1.0, 0.75)),
                ("step_inside", (STEP_IN, 0.3, -0.5)), ("step_outside", (STEP_OUT, 0.3, -0.5))]
        far = (1.0, -0.35, 0.6)
    else:
        # the only float32 points of Euclidean norm exactly 1 are on the axes (x^2 + y^2 + z^2 = 4^n has no other integer solutions)
        pts += [("surface", (0.0, -1.0, 0.0)), ("step_inside", (0.0, -STEP_IN, 0.0)), ("step_outside", (0.0, -STEP_OUT, 0.0)),
                ("near_surface", _U2), ("near_surface_in", tuple(STEP_IN * v for v in _U2)), ("near_surface_out", tuple(STEP_OUT * v for v in _U2))]
        far = _U2
    pts += [("far_1e3", tuple(1e3 * v for v in far)), ("far_1e6", tuple(1e6 * v for v in far)), ("far_3e38", (3e38, 1.0, 1.0)),
            ("far_1e18", (1e18, 1.0, 1.0)), ("origin", (0.0, 0.0, 0.0)), ("negative_zero", (-0.0, 0.25, -0.0)),
            ("axis_inside", (0.0, 0.0, 0.5)), ("axis_outside", (2.5, 0.0, 0.0)), ("linf_tie", (1.5, 1.5, 0.2))]
    # cell faces of level 0 (scale 15): pos = (x + 2) / 4 with 15 pos + 0.5 integral
    pts += [(f"face{j}", (4.0 * (2 * j + 1) / 30.0 - 2.0, 4.0 * (2 * j + 3) / 30.0 - 2.0, 4.0 * (2 * j - 1) / 30.0 - 2.0)) for j in (5, 7, 9)]
    return pts


def norm_of(x, mode):
    x = x.double()
    return x.abs().max(-1).values if mode == 1 else x.norm(dim=-1)


@functools.lru_cache(maxsize=None)
def pool(name):
    """-> x [N,3] float32 (edge points first), edge names, and the per-point masks described in the module docstring"""
    case = CASES[name]
    edges = edge_points(case.mode)
    g = torch.Generator().manual_seed(case.seed)
    if case.points == "sphere":
        body = torch.nn.functional.normalize(torch.randn(POOL, 3, generator=g), dim=-1)
    else:
        body = (torch.rand(POOL, 3, generator=g) * 2 - 1) * (1.0 if case.mode == 0 else 1.3)
    x = torch.cat([torch.tensor([p for _, p in edges], dtype=torch.float64).to(torch.float32), body]).contiguous()
    names = [n for n, _ in edges]
    N = x.shape[0]
    srt = x.abs().sort(-1).values
    tie = (srt[:, 2] == srt[:, 1]) & (srt[:, 2] >= 1) if case.mode == 1 else torch.zeros(N, dtype=torch.bool)
    overflow = (x.abs().max(-1).values > 1e19) if case.mode == 2 else torch.zeros(N, dtype=torch.bool)
    pe_finite = 2.0 * math.pi * x.double().abs().max(-1).values * 2.0 ** case.pe_max_exp < float(np.finfo(np.float32).max)
    return dict(x=x, names=names, n_edges=len(edges), values=~overflow, tangents=~overflow & ~tie,
                pe=x.abs().max(-1).values <= PE_MAX_X, pe_finite=pe_finite if case.pe else torch.ones(N, dtype=torch.bool), dirs=torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1).contiguous())


def prefix_sizes(name):
    return (1, 63, 64, 65, pool(name)["x"].shape[0])


@functools.lru_cache(maxsize=None)
def table32(n_params):
    """the table the kernels read: float32, uniform in +-TABLE_SCALE; every 16-level case shares one (n_params is its only key)"""
    g = torch.Generator().manual_seed(n_params % 65521)
    return ((torch.rand(n_params, 2, generator=g) * 2 - 1) * TABLE_SCALE).contiguous()


@functools.lru_cache(maxsize=None)
def table64(n_params):
    return table32(n_params).double()


def position32(x, mode):
    """the float32 position that decides the cell: the oracle's own operation order (test_indices_bit_exact)"""
    x = x.to(torch.float32)
    return x if mode == 0 else (O.scene_contraction(x, float("inf") if mode == 1 else 2) + 2.0) / 4.0


def cells(x, case):
    """corner rows [N,L,8] and cell origin [N,L,3] of the float32 position"""
    return O.hash_grid_indices(position32(x, case.mode), case.cfg())


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def position(x, mode, dtype, defect=None):
    pos, J = HB.grid_position(x, mode, dtype)
    if mode and defect == "dk":  # J = k I / 4: the term x_a (dk / dm) (dm / dx_k) dropped
        m = x.to(dtype).abs().max(-1).values if mode == 1 else (x.to(dtype) ** 2).sum(-1).sqrt()
        ms = torch.where(m >= 1, m, torch.ones_like(m))
        k = torch.where(m >= 1, (2 - 1 / ms) / ms, torch.ones_like(m))
        J = k[:, None, None] * torch.eye(3, dtype=dtype) / 4
    if mode and defect == "no_quarter":
        J = J * 4
    return pos, J


def encode(case, x, dtype, cell, table, defect=None):
    """x [N,3] -> Y [N,width], T [3,N,width] in `dtype`; cell = cells(x, case); table [n_params,2] in `dtype`"""
    x = x.detach().to(dtype)
    N, W, F = x.shape[0], case.width, case.pe
    pos, J = position(x, case.mode, dtype, defect)
    idx, fl = cell
    Y, T = torch.zeros(N, W, dtype=dtype), torch.zeros(3, N, W, dtype=dtype)
    if case.include_x:
        Y[:, :3] = x
        for k in range(3):
            T[k, :, k] = 1.0
        if defect == "identity_entry":
            T[1, :, 1] = 0.0
    if F:
        pe0, npe = (3 if case.include_x else 0), 3 * F
        expo = torch.linspace(0.0, case.pe_max_exp, F, dtype=dtype)  # step max_exp / (F - 1)
        if defect == "pe_step":
            expo = torch.arange(F, dtype=dtype) * (case.pe_max_exp / F)
        freqs = 2.0 ** expo
        arg = 2.0 * math.pi * x[..., None] * freqs  # [N,3,F], column i F + f
        arg2 = arg + math.pi / 2.0
        Y[:, pe0:pe0 + npe] = torch.sin(arg).reshape(N, npe)
        Y[:, pe0 + npe:pe0 + 2 * npe] = torch.sin(arg2).reshape(N, npe)
        d1, d2 = torch.cos(arg) * (2.0 * math.pi * freqs), torch.cos(arg2) * (2.0 * math.pi * freqs)
        if defect == "shifted_sin_sign":  # d sin(arg + pi / 2) = -sin(arg) d arg, given the sign of sin
            d2 = -d2
        for i in range(3):
            T[i, :, pe0 + i * F:pe0 + (i + 1) * F] = d1[:, i]
            T[i, :, pe0 + npe + i * F:pe0 + npe + (i + 1) * F] = d2[:, i]
    cfg = case.cfg()
    for l in range(case.n_levels):
        s = float(np.float32(cfg.scales[l]))
        t = pos * s + 0.5 - fl[:, l].to(dtype)
        if case.smooth:
            w = t * t * (3.0 - 2.0 * t)
            dw = 6.0 * t * (1.0 - t) * s
            if defect == "smoothstep_derivative" and l == SMOOTH_DEFECT_LEVEL:
                dw = 6.0 * t * (1.0 - t) ** 2 * s
        else:
            w, dw = t, torch.full_like(t, s)
        vals = table[idx[:, l].reshape(-1)].view(N, 8, 2)
        feat = torch.zeros(N, 2, dtype=dtype)
        dfeat = torch.zeros(N, 3, 2, dtype=dtype)  # d feat / d pos_a
        for c in range(8):
            f = [w[:, d] if (c >> d) & 1 else 1.0 - w[:, d] for d in range(3)]
            df = [dw[:, d] if (c >> d) & 1 else -dw[:, d] for d in range(3)]
            feat = feat + (f[0] * f[1] * f[2])[:, None] * vals[:, c]
            dfeat[:, 0] += (df[0] * f[1] * f[2])[:, None] * vals[:, c]
            dfeat[:, 1] += (f[0] * df[1] * f[2])[:, None] * vals[:, c]
            dfeat[:, 2] += (f[0] * f[1] * df[2])[:, None] * vals[:, c]
        c0 = case.feat0 + 2 * l
        Y[:, c0:c0 + 2] = feat
        Tl = torch.einsum("paf,pak->kpf", dfeat, J)  # T_k = sum_a (d feat / d pos_a) J[a][k]
        if defect == "level0_scale" and l == 0:
            Tl = Tl * 1.02
        T[:, :, c0:c0 + 2] = Tl
    return Y, T


def point_dirs(dirs, N, spr):
    """dirs [R,3] -> the direction of each of N points: point p takes dirs[p // spr]"""
    return dirs[torch.arange(N) // spr]


def directional(T, d, defect=None):
    """Td [N,W] = sum_k d_k T_k, d [N,3] the direction of each point"""
    d = d.to(T.dtype)
    if defect == "neighbour_dir":
        d = torch.roll(d, -1, 0)
    return d[:, 0, None] * T[0] + d[:, 1, None] * T[1] + d[:, 2, None] * T[2]


def input_gradient(T, dY, cols=None):
    """dx [N,3] with dx_b = sum_c dY_c T_b,c over the columns `cols` (all when None), and A [N,3] = sum_c |dY_c| |T_b,c|"""
    dY = dY.to(T.dtype)
    if cols is not None:
        cols = list(cols)
        T, dY = T[:, :, cols], dY[:, cols]
    prod = T * dY[None]
    return prod.sum(-1).t().contiguous(), prod.abs().sum(-1).t().contiguous()


# ---- references and bars ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(name):
    """-> the pool of the case with its cells and the float64 and float32 runs of the restatement over all of it"""
    case, pl = CASES[name], pool(name)
    cell = cells(pl["x"], case)
    n = case.cfg().n_params
    Y64, T64 = encode(case, pl["x"], torch.float64, cell, table64(n))
    Y32, T32 = encode(case, pl["x"], torch.float32, cell, table32(n))
    g = torch.Generator().manual_seed(case.seed + 1000)
    return dict(pl, cell=cell, Y64=Y64, T64=T64, Y32=Y32, T32=T32, dY=torch.randn(pl["x"].shape[0], case.width, generator=g))


def point_mask(ref, quantity, group):
    """the points of the pool that take part in `quantity` of column group `group`"""
    m = ref["values"] if quantity == "value" else ref["tangents"]
    return m & ref["pe"] if group.startswith("pe") else m


def _bar(r32, r64):
    if r64.numel() == 0:
        return 0.0
    return max(4.0 * (r32.double() - r64).abs().max().item(), 4.0 * EPS32 * r64.abs().max().item())


@functools.lru_cache(maxsize=None)
def value_bars(name):
    ref = reference(name)
    return {g: _bar(ref["Y32"][point_mask(ref, "value", g)][:, list(c)], ref["Y64"][point_mask(ref, "value", g)][:, list(c)])
            for g, c in CASES[name].groups()}


@functools.lru_cache(maxsize=None)
def tangent_bars(name):
    ref = reference(name)
    return {g: _bar(ref["T32"][:, point_mask(ref, "tangent", g)][:, :, list(c)], ref["T64"][:, point_mask(ref, "tangent", g)][:, :, list(c)])
            for g, c in CASES[name].groups()}


@functools.lru_cache(maxsize=None)
def directional_reference(name, spr):
    """Td of the whole pool in float64 and float32, point p along ref['dirs'][p // spr]"""
    ref = reference(name)
    d = point_dirs(ref["dirs"], ref["x"].shape[0], spr)
    return directional(ref["T64"], d), directional(ref["T32"], d)


@functools.lru_cache(maxsize=None)
def directional_bars(name, spr):
    ref = reference(name)
    d64, d32 = directional_reference(name, spr)
    return {g: _bar(d32[point_mask(ref, "tangent", g)][:, list(c)], d64[point_mask(ref, "tangent", g)][:, list(c)]) for g, c in CASES[name].groups()}


def dx_groups(name):
    return CASES[name].groups() + [("all", tuple(range(CASES[name].width)))]


def dx_point_mask(ref, group):
    m = ref["tangents"] & ref["pe_finite"]
    return m & ref["pe"] if group.startswith("pe") or group == "all" else m


@functools.lru_cache(maxsize=None)
def dx_reference(name, group):
    """-> dx64 [N,3], A [N,3], and the noise part of the bar (a number): 4 max|dx32 - dx64| over the pool, with the row gradient
    ref['dY'] restricted to the columns of `group`"""
    ref = reference(name)
    cols = dict(dx_groups(name))[group]
    dx64, A = input_gradient(ref["T64"], ref["dY"], cols)
    dx32, _ = input_gradient(ref["T32"], ref["dY"], cols)
    m = dx_point_mask(ref, group)
    return dx64, A, 4.0 * (dx32.double() - dx64)[m].abs().max().item()


def dx_bar(name, group):
    """-> dx64 and the bar per entry [N,3]"""
    dx64, A, noise = dx_reference(name, group)
    return dx64, torch.clamp(4.0 * EPS32 * A, min=noise)


def group_probe(ref, case, group):
    """ref['dY'] with every column outside the group zeroed, padded to the row's leading dimension: [N, ldy] float32"""
    cols = list(dict(dx_groups(case.name))[group])
    out = torch.zeros(ref["x"].shape[0], case.ldy)
    out[:, cols] = ref["dY"][:, cols]
    return out


def cell_disagreements(idx_a, idx_b):
    """[N,L] bool: the (point, level) pairs whose eight corner rows differ"""
    return (idx_a != idx_b).any(-1)


def cell_cap(case, n_points):
    """the largest number of (point, level) pairs that may sit in another cell than the reference's"""
    return int(CELL_CAP_LINF * n_points * case.n_levels) if case.mode == 1 else 0
