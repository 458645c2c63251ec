"""The sdf value chain (SDFAlbedoField.get_sdf_at_pos, sdf_albedo_field.py:169-174: Linear + Softplus(beta), Linear + Softplus(beta), the
sdf row of the last Linear) restated on the CPU with its hand-written backward and no autograd: every quantity the chain kernels
(csrc/sdf_chain.hip) store, in the three arithmetics of film_chain_cpu.py.

    float64   the reference
    float32   the noise measure: every product and elementwise step in float32 (torch CPU matmuls and sums)
    split     a rough emulation of the kernels' products for defect injection only (film_chain_cpu._Arith.prod), the sigmoid recovered
              from the saved softplus output as the kernels do (1 - exp(-beta a)); `defect` names one product or constant to damage.

The float64 and float32 modes take sigmoid(beta z) from z: the kernels' recovery from the saved output is what is under test.  Also the
launch plan of the eight-wave kernels (chain.h tail_plan / tail_tile) restated, and one row count per class of plan.

Needs no GPU and does not import neusky_amd.  Shared by test_sdf_chain_cpu.py and test_gpu_sdf_chain_parity.py, which both take a
quantity group's bar from `bars` below (the rule and the constants are film_chain_cpu's)."""
import torch

from film_chain_cpu import NOISE_FACTOR, NOISE_FLOOR, _Arith, distance

PRODUCTS = ("fwd0", "fwd1", "bwd1", "bwd0")
CONSTANT_DEFECTS = ("beta", "threshold")
HIDDEN = 256
BETA = 100.0
ROW_MATRICES = ("sdf", "a0", "a1", "dz1", "dz0", "dE")  # one batch row per row: a row's values depend on that row's inputs only
BATCH_SUMS = ("dw2", "db2")                             # summed over the batch inside the backward kernel (fp32 atomics)
SUM_ALLOWANCE = 1e-6  # x sum of magnitudes: what test_gpu_wgrad_native.py allows a batch sum of M fp32 terms added in another order


def param_grads(S, E):
    """the parameter gradients the weight-gradient kernels form, here in float64 from the stored matrices: dz1^T a0, dz0^T E, column sums"""
    d = lambda t: t.detach().cpu().double()  # noqa: E731
    return {"dW1": d(S["dz1"]).t() @ d(S["a0"]), "db1": d(S["dz1"]).sum(0), "dW0": d(S["dz0"]).t() @ d(E), "db0": d(S["dz0"]).sum(0)}


def _softplus(z, defect):
    """torch semantics: beta z > 20 returns z.  defect "threshold": log(1 + exp(beta z)) / beta whatever beta z is"""
    if defect == "threshold":
        return torch.log1p(torch.exp(BETA * z)) / BETA
    return torch.nn.functional.softplus(z, beta=BETA, threshold=20.0)


def sdf_chain(weights, E, g_sdf, beta=BETA, mode="float64", defect=None):
    """forward and hand-written backward.  weights: W0 [H, in_dim], b0 [H], W1 [H, H], b1 [H], w2 [H] (the sdf row), b2 [1]; E [M, >= in_dim]
    (further columns are ignored), g_sdf [M].  defect (split mode): a name of PRODUCTS or of CONSTANT_DEFECTS.
    -> dict, row-major: sdf [M], a0, a1, dz1, dz0 [M, H], dE [M, in_dim], dw2 [H], db2 [1], gmax [2], grads{dW1, db1, dW0, db0} (float64),
       sum_abs{dw2, db2}: sum over rows of |g a1| and of |g| (what the batch sums' allowance scales with)"""
    assert beta == BETA
    A = _Arith(mode, defect)
    W0, b0, W1, b1, w2, b2 = (t.detach().cpu().to(A.dtype) for t in weights)
    E = E.detach().cpu().to(A.dtype)[:, :W0.shape[1]]
    g = g_sdf.detach().cpu().to(A.dtype).reshape(-1)
    # ---- forward
    z0 = A.prod(E, W0, b0, "fwd0")
    a0 = _softplus(z0, defect)
    z1 = A.prod(a0, W1, b1, "fwd1")
    a1 = _softplus(z1, defect)
    sdf = a1 @ w2 + b2
    # ---- backward
    if mode == "split":
        bs = A.const("beta", BETA, 1e-3)
        s1, s0 = -torch.expm1(-bs * a1), -torch.expm1(-bs * a0)
    else:
        # (torch semantics again: above the threshold the softplus is the identity and its derivative 1, not sigmoid(20) = 1 - 2e-9)
        sg = lambda z: torch.where(BETA * z > 20.0, torch.ones_like(z), torch.sigmoid(BETA * z))  # noqa: E731
        s1, s0 = sg(z1), sg(z0)
    dz1 = g[:, None] * w2[None, :] * s1
    dz0 = A.prod(dz1, W1.t(), None, "bwd1") * s0
    dE = A.prod(dz0, W0.t(), None, "bwd0")
    ga1 = g[:, None] * a1
    out = dict(sdf=sdf, a0=a0, a1=a1, dz1=dz1, dz0=dz0, dE=dE, dw2=ga1.sum(0), db2=g.sum().reshape(1),
               gmax=torch.stack([dz1.abs().max(), dz0.abs().max()]),
               sum_abs={"dw2": ga1.double().abs().sum(0), "db2": g.double().abs().sum().reshape(1)})
    out["grads"] = param_grads(out, E)
    return out


# ---------------------------------------------------------------------------------------------------------- groups and bars
def groups(S):
    """the quantity groups of one evaluation (or of the kernels' stored quantities in the same dict form), each float64"""
    d = lambda t: t.detach().cpu().double()  # noqa: E731
    g = {k: d(S[k]) for k in ROW_MATRICES + BATCH_SUMS}
    for k, v in S["grads"].items():
        g[f"grad:{k}"] = d(v)
    return g


def _per_row(key, per_row):
    return per_row and key in ROW_MATRICES


def bars(ref64, ref32, per_row=False):
    """relative bar of every group: NOISE_FACTOR x (the float32 restatement's distance from the float64 one, same normaliser), floored at
    NOISE_FACTOR x 2^-24 (film_chain_cpu.bars).  Sums over the batch are never per row."""
    g64, g32 = groups(ref64), groups(ref32)
    return {k: NOISE_FACTOR * max(distance(g32[k], g64[k], _per_row(k, per_row)), NOISE_FLOOR) for k in g64}


def ratios(got, ref64, bar, per_row=False):
    """err / bar of every group.  The batch sums dw2 and db2 (M terms added by fp32 atomics in the kernel, pairwise in torch's float32):
    entry by entry against the group bar applied to the largest reference entry plus SUM_ALLOWANCE x the sum of the terms' magnitudes"""
    gg, g64 = groups(got), groups(ref64)
    r = {}
    for k in g64:
        if k in BATCH_SUMS:
            tol = bar[k] * float(g64[k].abs().max()) + SUM_ALLOWANCE * ref64["sum_abs"][k].double()
            r[k] = float(((gg[k] - g64[k]).abs() / tol.clamp_min(1e-300)).max())
        else:
            r[k] = distance(gg[k], g64[k], _per_row(k, per_row)) / bar[k]
    return r


def reference_and_bars(weights, E, g_sdf, per_row=False):
    """-> (float64 restatement, relative bar of every group)"""
    ref64 = sdf_chain(weights, E, g_sdf, BETA, "float64")
    return ref64, bars(ref64, sdf_chain(weights, E, g_sdf, BETA, "float32"), per_row)


# ---------------------------------------------------------------------------------------------------------- launch plans (chain.h)
def tail_plan(n_tiles, cus):
    """(full_wgs, tail_wgs, tail_k) of a launch of n_tiles wave tiles on cus CUs; the tail workgroups come first in the grid"""
    full = n_tiles // (8 * cus) * cus
    rem = n_tiles - 8 * full
    if rem >= 7 * cus:
        return full + (rem + 7) // 8, 0, 0
    k = (rem + cus - 1) // cus
    return full, ((rem + k - 1) // k if k else 0), k


def tail_tile(full_wgs, tail_wgs, tail_k, n_tiles, block, wave):
    """wave tile of wave `wave` of workgroup `block`, or -1"""
    if block >= tail_wgs:
        return (block - tail_wgs) * 8 + wave
    t = 8 * full_wgs + block * tail_k + wave
    return t if wave < tail_k and t < n_tiles else -1


def plan_class(n_tiles, cus):
    """the classes of launch plan a parity run has to cover, each other than P1 with eight-wave hand-shakes of its own kind:
    P1 one live wave per workgroup, P2:k tail workgroups of k live waves of which the last is ragged, P3 full workgroups only with dead
    waves in the last, P4 exactly 8 cus tiles, P5 full workgroups behind tail workgroups; None: another plan"""
    full, tail, k = tail_plan(n_tiles, cus)
    if full and tail:
        return "P5"
    if tail:
        if k == 1:
            return "P1"
        return f"P2:{k}" if n_tiles % k else None
    if n_tiles == 8 * cus:
        return "P4"
    return "P3" if 7 * cus <= n_tiles < 8 * cus and n_tiles % 8 else None


def plan_rows(cus):
    """{name: (class, M)}: one row count per class; every M but P4's leaves the last wave tile ragged.  A tail of k live waves with a
    ragged last workgroup needs k cus - 1 tiles not divisible by k: on fewer than 2 CUs there is none, and the class is left out"""
    ragged = lambda n: 32 * n - 5  # noqa: E731
    rows = {"P1": ("P1", ragged(cus))}
    for k in (2, 5, 7):
        if cus >= 2:
            rows[f"P2:{k}"] = (f"P2:{k}", ragged(k * cus - 1))
    rows["P3"] = ("P3", ragged(7 * cus + min(3, cus - 1)))
    rows["P4"] = ("P4", 32 * 8 * cus)
    rows["P5:1"] = ("P5", ragged(8 * cus + 1))
    rows["P5:41"] = ("P5", ragged(8 * cus + 41))
    return rows


def chunk_rows(cus):
    """rows of a P1 launch that the larger plans' per-row results are compared with: at most 8192, at most one wave tile per CU"""
    return min(8192, 32 * cus)


# ---------------------------------------------------------------------------------------------------------- cases
ROW_EDGES = (1, 31, 32, 33, 255, 256, 257, 582)
DIM_EDGES = (4, 16, 20, 32, 36, 64, 68, 72, 80)  # k-steps 1 1 2 2 3 4 5 5 5; W0^T tiles 1 1 1 1 2 2 3 3 3, the last of 4 16 20 32 4 32 4 8 16 rows
DIM_M = 129
DDF_DIM = 72
DEFECT_CASE = (DDF_DIM, 257)


def all_shapes():
    """(in_dim, M, steep) of every parity case against float64"""
    return [(DDF_DIM, M, False) for M in ROW_EDGES] + [(k, DIM_M, False) for k in DIM_EDGES] + [(DDF_DIM, 257, True)]


def make_weights(in_dim, steep=False):
    """W0, b0, W1, b1, w2, b2 on the CPU at the scales of test_gpu_sdf_chain.py (N(0, 1 / fan-in) weights, biases in +-0.1): with beta =
    100, beta z spans both softplus branches; steep: that test's scale = 2.0, which reaches beta z far beyond +-20"""
    g = torch.Generator().manual_seed(100 * in_dim + (7 if steep else 0))
    scale = 2.0 if steep else 1.0
    W0 = torch.randn(HIDDEN, in_dim, generator=g) * (scale / in_dim ** 0.5)
    b0 = torch.rand(HIDDEN, generator=g) * 0.2 - 0.1
    W1 = torch.randn(HIDDEN, HIDDEN, generator=g) * (scale / HIDDEN ** 0.5)
    b1 = torch.rand(HIDDEN, generator=g) * 0.2 - 0.1
    w2 = torch.randn(HIDDEN, generator=g) * (1.0 / HIDDEN ** 0.5)
    b2 = torch.rand(1, generator=g) * 0.2 - 0.1
    return [W0, b0, W1, b1, w2, b2]


def make_inputs(M, in_dim, steep=False):
    """E [M, in_dim] ~ N(0, 0.25) (steep: N(0, 1)), g_sdf [M] ~ N(0, 1)"""
    g = torch.Generator().manual_seed(7 + M + 1000 * in_dim)
    E = torch.randn(M, in_dim, generator=g) * (1.0 if steep else 0.5)
    return E, torch.randn(M, generator=g)
