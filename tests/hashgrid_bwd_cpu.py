"""float64 restatement of the hash-grid TABLE gradient (neusky_amd/csrc/hashgrid.hip, nsky_encode_bwd) and a Python restatement of
the chunk-owner dispatch (host plan, bitmap pre-pass, phase choice): the reference the owner kernel is tested against and the
proof that a test input reaches the branch it is meant for.  No autograd; nothing here imports the package."""
import os
import re

import numpy as np
import torch

from oracle import neusky_oracle as O

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "neusky_amd", "csrc", "hashgrid.hip")
_HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "neusky_hip.h")
M32 = 0xFFFFFFFF

# The per-entry bar of the lattice cases of test_gpu_hashgrid_owner.py, |got - base - G| <= C_LATTICE * (A + |base|): 4 x the largest
# figure measured on an MI355X over those cases (4.00e-7, at P = 32 800; the others 1.2e-7 .. 3.7e-7).  It lives here because the
# CPU test that injects defects needs it too: a defect has to break it tenfold.
C_LATTICE = 1.6e-6


# ---- the gradient ---------------------------------------------------------------------------------------------------------------
def grid_position(x, mode, dtype=torch.float64):
    """x [P,3] -> pos [P,3] fed to the grid and J [P,3,3], J[p,a,k] = d pos_a / d x_k, in float64 (or in `dtype`:
    float32 gives what plain float32 arithmetic makes of the same formulas).
    mode 0: pos = x.  mode 1 / 2: the L-infinity / L2 scene contraction c(x), then pos = (c + 2) / 4."""
    x = x.detach().to(dtype)
    P = x.shape[0]
    eye = torch.eye(3, dtype=dtype).expand(P, 3, 3)
    if mode == 0:
        return x.clone(), eye.clone()
    if mode == 1:
        m, im = x.abs().max(-1)
        dm = torch.zeros(P, 3, dtype=dtype)  # d m / d x_k
        dm[torch.arange(P), im] = torch.sign(x[torch.arange(P), im])
    else:
        m = (x * x).sum(-1).sqrt()
        dm = x / torch.where(m > 0, m, torch.ones_like(m))[:, None]
    out = m >= 1
    ms = torch.where(out, m, torch.ones_like(m))
    k = torch.where(out, (2 - 1 / ms) / ms, torch.ones_like(m))
    dk = torch.where(out, (-2 + 2 / ms) / (ms * ms), torch.zeros_like(m))
    c = k[:, None] * x
    J = k[:, None, None] * eye + dk[:, None, None] * x[:, :, None] * dm[:, None, :]
    return (c + 2) / 4, J / 4


def table_gradient(x, mode, cfg, dY, dT=None, smoothstep=None, corner_scale=None):
    """x [P,3]; dY [P,2L] (the hash columns of the row gradient); dT [3,P,2L] or None (the tangent rows' gradient).
    -> G, A [n_params,2] float64.

    Per level l and corner c (bit d of c: the +1 neighbour along axis d), with t = pos * scale_l + 0.5 - floor in float64,
    w the (smooth)step of t and w_c the product of the three per-axis factors, point p adds to row idx[p,l,c] the FOUR TERMS
        w_c dY_l   and, for a = 0..2,   (d w_c / d pos_a) * sum_k J[a][k] dT_k,l .
    G is their sum (index_add_), A the sum of their absolute values: what an fp32 evaluation rounds is each term and each
    partial sum, so |error_e| <= c * A_e is a bound per ENTRY, judged against the points that touch that entry.  (The absolute
    value of a point's summed terms would not do: where the four terms cancel, their fp32 rounding does not.)
    The corner rows and floor come from O.hash_grid_indices: the fp32 cell choice and tcnn's uint32 wrap.
    corner_scale [P,L,8] multiplies the contributions (tests inject defects with it)."""
    P, L = x.shape[0], cfg.n_levels
    smooth = cfg.smoothstep if smoothstep is None else smoothstep
    pos, J = grid_position(x, mode)
    idx, fl = O.hash_grid_indices(pos, cfg)
    dY = dY.detach().to(torch.float64)
    G = torch.zeros(cfg.n_params, 2, dtype=torch.float64)
    A = torch.zeros(cfg.n_params, 2, dtype=torch.float64)
    for l in range(L):
        s = float(np.float32(cfg.scales[l]))
        t = pos * s + 0.5 - fl[:, l]
        w = t * t * (3.0 - 2.0 * t) if smooth else t
        dw = 6.0 * t * (1.0 - t) * s if smooth else torch.full_like(t, s)
        gy = dY[:, 2 * l:2 * l + 2]
        if dT is not None:  # g[a] = sum_k J[a][k] dT_k : [P,3,2]
            g = torch.einsum("pak,kpf->paf", J, dT[:, :, 2 * l:2 * l + 2].detach().to(torch.float64))
        for c in range(8):
            f = [w[:, d] if (c >> d) & 1 else 1.0 - w[:, d] for d in range(3)]
            df = [dw[:, d] if (c >> d) & 1 else -dw[:, d] for d in range(3)]
            terms = [(f[0] * f[1] * f[2])[:, None] * gy]
            if dT is not None:
                terms += [(df[0] * f[1] * f[2])[:, None] * g[:, 0], (f[0] * df[1] * f[2])[:, None] * g[:, 1],
                          (f[0] * f[1] * df[2])[:, None] * g[:, 2]]
            if corner_scale is not None:
                terms = [tm * corner_scale[:, l, c, None] for tm in terms]
            G.index_add_(0, idx[:, l, c], sum(terms))
            A.index_add_(0, idx[:, l, c], sum(tm.abs() for tm in terms))
    return G, A


def autograd_table_gradient(x, mode, cfg, table, dY, dT=None):
    """the same gradient from the oracle's differentiable forward: d/d table of <dY, row> + sum_k <dT_k, d row / d x_k>, the
    tangent rows by the double-backward construction.  Also returns d <dY, row> / d x (hash columns only)."""
    xd = x.detach().to(torch.float64).requires_grad_(True)
    tb = table.detach().to(torch.float64).requires_grad_(True)
    pos = xd if mode == 0 else (O.scene_contraction(xd, float("inf") if mode == 1 else 2) + 2.0) / 4.0
    row = O.hash_grid_encode(pos, tb, cfg)
    loss = (row * dY.to(torch.float64)).sum()
    gx = torch.autograd.grad(loss, xd, retain_graph=True)[0]
    if dT is not None:
        v = torch.ones_like(row, requires_grad=True)
        gg = torch.autograd.grad(row, xd, v, create_graph=True)[0]
        for k in range(3):
            ek = torch.zeros_like(xd); ek[:, k] = 1.0
            jvp = torch.autograd.grad(gg, v, ek, create_graph=True)[0]  # d row / d x_k
            loss = loss + (jvp * dT[k].to(torch.float64)).sum()
    return torch.autograd.grad(loss, tb)[0], gx


# ---- test inputs ----------------------------------------------------------------------------------------------------------------
LATTICE = 2048  # x = k / 2048, |k| < 2048


def g4_cfg(smoothstep):
    """4 levels with exactly integral scales 15, 63, 255, 1023: every owner regime (one-chunk dense, many-chunk dense, hashed with
    split points, hashed) in a 10.5 MB table"""
    return O.HashGridCfg(n_levels=4, log2_hashmap_size=19, base_res=16, max_res=1024, smoothstep=smoothstep)


def lattice_points(P, f, seed=0):
    """P points k / 2048; a fraction f of them on the 8 x 8 x 8 lattice nodes of ONE finest-level cell of g4 (a crowd, as a scene's
    termination points form), the rest uniform"""
    g = torch.Generator().manual_seed(seed)
    k = torch.randint(-(LATTICE - 1), LATTICE, (P, 3), generator=g)
    n = int(P * f)
    sel = torch.randperm(P, generator=g)[:n]
    k[sel] = torch.tensor([642, -557, 331]) + torch.randint(0, 8, (n, 3), generator=g)
    return k.to(torch.float32) / LATTICE


# ---- the owner dispatch ---------------------------------------------------------------------------------------------------------
def owner_constants():
    """the kernel's constants, read from the source: a change there moves this plan with it, a vanished name fails here"""
    src = open(_CSRC).read()
    out = {}
    for name in ("OWN_CH", "OWN_SHIFT", "OWN_THREADS", "OWN_QCAP", "OWN_WG_PER_LEVEL", "OWN_DENSE_SPLITS", "OWN_MAX_CHUNKS", "BM_POINTS"):
        m = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*([0-9+\-*/() ]+);", src)
        assert m, f"{name} not found in hashgrid.hip"
        out[name] = int(eval(m.group(1), {"__builtins__": {}}))  # digits and + - * / ( ) only
    m = re.search(r"#define\s+NSKY_ENCODE_BWD_OWNER_MIN_POINTS\s+(\d+)", open(_HEADER).read())
    assert m, "NSKY_ENCODE_BWD_OWNER_MIN_POINTS not found in neusky_hip.h"
    out["MIN_POINTS"] = int(m.group(1))
    return out


def owner_plan(cfg, P, K=None):
    """nsky_encode_bwd's host plan: bitmap words, and per level (finest first) chunks, dense?, splits"""
    K = K or owner_constants()
    words = -(-P // K["BM_POINTS"]) * (K["BM_POINTS"] // 32)
    levels = []
    for l in range(cfg.n_levels - 1, -1, -1):
        size, res = cfg.offsets[l + 1] - cfg.offsets[l], cfg.resolutions[l]
        nch = -(-size // K["OWN_CH"])
        dense = res ** 3 <= size
        if dense:
            sp = max(2 * K["OWN_WG_PER_LEVEL"] // nch, K["OWN_DENSE_SPLITS"])
        else:
            sp = K["OWN_WG_PER_LEVEL"] // nch
            sp *= min(max(512 // res, 1), 4)
        sp = min(max(sp, 1), max(words // 32, 1))
        levels.append(dict(level=l, res=res, size=size, chunks=nch, dense=dense, splits=sp))
    return words, levels


def owner_bitmaps(x, mode, cfg, level, K=None):
    """owner_bitmaps_kernel for one level: bool [chunks, P], bit (c, p) set when point p may have a corner in chunk c"""
    K = K or owner_constants()
    pos, _ = grid_position(x, mode)
    idx, fl = O.hash_grid_indices(pos, cfg)
    size, res = cfg.offsets[level + 1] - cfg.offsets[level], cfg.resolutions[level]
    nch = -(-size // K["OWN_CH"])
    pg = fl[:, level].to(torch.int64) & M32
    ch = ((idx[:, level] - cfg.offsets[level]) >> K["OWN_SHIFT"]).numpy()  # [P,8]: the chunk of every corner
    if res ** 3 <= size:
        everywhere = ~((pg < res - 1).all(-1)).numpy()  # a cell not inside the grid: every owner looks
        lo, hi = ch.min(1), ch.max(1)                   # inside: corner 0 .. corner 7 bound the range
        c = np.arange(nch)[:, None]
        return ((c >= lo[None]) & (c <= hi[None])) | everywhere[None]
    everywhere = ((pg[:, 0] & (K["OWN_CH"] - 1)) == K["OWN_CH"] - 1).numpy()  # x + 1 carries into the chunk bits
    bits = np.zeros((nch, x.shape[0]), bool)
    for k in range(8):
        bits[ch[:, k], np.arange(x.shape[0])] = True
    return bits | everywhere[None]


def owner_phases(x, mode, cfg, K=None):
    """encode_bwd_owner_kernel's control flow per level: {level: dict(sizes = set of phase sizes taken (bitmap words),
    empty = workgroups that return before their first phase, busy = the others)}"""
    K = K or owner_constants()
    P = x.shape[0]
    words, levels = owner_plan(cfg, P, K)
    T, Q = K["OWN_THREADS"], K["OWN_QCAP"]
    out = {}
    for lv in levels:
        bits = owner_bitmaps(x, mode, cfg, lv["level"], K)
        pc = np.zeros((lv["chunks"], words * 32), bool)
        pc[:, :P] = bits
        pc = pc.reshape(lv["chunks"], words, 32).sum(-1)  # popcount per bitmap word
        sp = lv["splits"]
        wper = -(-words // sp)
        sizes, empty, busy = set(), 0, 0
        for c in range(lv["chunks"]):
            for ps in range(sp):
                wb, we = ps * wper, min(words, ps * wper + wper)
                if sp > 1 and pc[c, wb:we].sum() == 0:
                    empty += 1
                    continue
                busy += 1
                while wb < we:
                    half0, total1 = pc[c, wb:min(we, wb + T)].sum(), pc[c, min(we, wb + T):min(we, wb + 2 * T)].sum()
                    quarter0 = pc[c, wb:min(we, wb + T // 2)].sum()
                    if half0 + total1 <= Q: nw = 2 * T
                    elif half0 <= Q: nw = T
                    elif quarter0 <= Q: nw = 512
                    else: nw = 256
                    sizes.add(nw)
                    wb += nw
        out[lv["level"]] = dict(sizes=sizes, empty=empty, busy=busy)
    return out
