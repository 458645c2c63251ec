"""The FiLM-SIREN chain (neusky/utils/siren.py:108-208) restated on the CPU with its hand-written backward and no autograd: every
matrix the chain kernels (csrc/film_chain.hip) store, in three arithmetics.

    float64   the reference
    float32   the noise measure: every product and elementwise step in float32 (torch CPU matmuls)
    split     a rough emulation of the kernels' products for defect injection only: both operands pre-scaled by powers of two (batch
              rows per row, weights per output row -- the kernels scale weights per 32-row tile), split into fp16 hi + fp16 residual,
              hi hi + hi lo + lo hi accumulated in float64 and rounded to float32; elementwise steps in float32.  `defect` names one
              product or constant to damage.

Needs no GPU and does not import neusky_amd.  Shared by test_film_chain_cpu.py and test_gpu_film_chain_parity.py, which both take a
quantity group's bar from `bars` below."""
import torch

PRODUCT_CLASSES = ("fwd_map", "fwd_head", "fwd_z", "fwd_out", "bwd_out", "bwd_film", "bwd_head", "bwd_map", "bwd_cond")
CONSTANT_DEFECTS = ("dF15", "freq30", "leaky", "cos")
NOISE_FACTOR = 4.0          # allowance over float32 noise for another summation order and the sin / cos polynomials
NOISE_FLOOR = 2.0 ** -24    # half a float32 ulp: a group the float32 restatement happens to hit exactly still gets 4 x this
FLIP_REL = 2e-5             # a LeakyReLU decision may differ from float64's only below this share of the layer's largest |pre|


def flip_cap(numel: int) -> int:
    return 1 + numel // 200000


def unpack_net(net, dtype=torch.float64):
    """-> dict(map_w, map_b, mo_w, mo_b, film_w, film_b, out_w, out_b) of CPU tensors in `dtype`.  net: the oracle's parameter dictionary
    ("ddf.map_w0", ...) or the (padded) weight list FilmChainFn takes: map_w0, map_b0, ..., map_wo, map_bo, film_w0, film_b0, ..., out_w, out_b"""
    c = lambda t: t.detach().cpu().to(dtype)  # noqa: E731
    if isinstance(net, dict):
        prefix = next(k for k in net if k.endswith("map_w0"))[:-len("map_w0")]
        n_map = sum(1 for k in net if k.startswith(prefix + "map_w") and k[len(prefix) + 5:].isdigit())
        n_film = sum(1 for k in net if k.startswith(prefix + "film_w"))
        g = lambda k: c(net[prefix + k])  # noqa: E731
        return dict(map_w=[g(f"map_w{i}") for i in range(n_map)], map_b=[g(f"map_b{i}") for i in range(n_map)], mo_w=g("map_wo"), mo_b=g("map_bo"),
                    film_w=[g(f"film_w{i}") for i in range(n_film)], film_b=[g(f"film_b{i}") for i in range(n_film)], out_w=g("out_w"), out_b=g("out_b"))
    wb = list(net)
    H = wb[0].shape[0]
    n_map = next(i for i in range(len(wb) // 2) if wb[2 * i].shape[0] != H)  # the mapping head has 2 n_film H rows
    n_film = (len(wb) - 2 * n_map - 4) // 2
    o = 2 * n_map + 2
    return dict(map_w=[c(wb[2 * i]) for i in range(n_map)], map_b=[c(wb[2 * i + 1]) for i in range(n_map)], mo_w=c(wb[2 * n_map]), mo_b=c(wb[2 * n_map + 1]),
                film_w=[c(wb[o + 2 * i]) for i in range(n_film)], film_b=[c(wb[o + 2 * i + 1]) for i in range(n_film)],
                out_w=c(wb[o + 2 * n_film]), out_b=c(wb[o + 2 * n_film + 1]))


def _planes(a):
    """float32 [R, K] -> fp16 hi, fp16 residual (as float64) of the rows scaled by 2^(15 - e), max |row| < 2^e (numerics.h pow2_scale), and 1 / scale"""
    m = a.abs().amax(1, keepdim=True)
    e = torch.frexp(m).exponent.clamp(-100, 100)
    s = torch.ldexp(torch.ones_like(m), 15 - e)
    s = torch.where((m > 0) & (m < 3.0e38), s, torch.ones_like(s))
    xs = a * s
    hi = xs.to(torch.float16).to(torch.float32)
    lo = (xs - hi).to(torch.float16).to(torch.float32)
    return hi.double(), lo.double(), (1.0 / s).double()


class _Arith:
    def __init__(self, mode, defect):
        assert mode in ("float64", "float32", "split")
        assert defect is None or mode == "split", "defects exist in the emulated split mode only"
        self.mode = mode
        self.dtype = torch.float64 if mode == "float64" else torch.float32
        self.defect = defect  # None, (product class, layer index) or a name of CONSTANT_DEFECTS

    def const(self, name, value, rel):
        return value * (1.0 + rel) if self.defect == name else value

    def prod(self, X, W, bias, tag):
        """X [M, K] W[N, K]^T (+ bias)"""
        if self.mode != "split":
            out = X @ W.t()
            return out if bias is None else out + bias
        xh, xl, xi = _planes(X)
        wh, wl, wi = _planes(W)
        acc = xh @ wh.t() + xl @ wh.t()
        if self.defect != tag:  # the damaged product loses its (weight residual) x (activation hi) term
            acc = acc + xh @ wl.t()
        out = acc * xi * wi.t()
        return (out if bias is None else out + bias.double()).float()


def param_grads(S, cond, x, d_res):
    """every parameter gradient, formed in float64 from the matrices the kernels store: dz_i^T y_{i-1}, dpre_l^T h_{l-1}, dfp^T h_last and the
    column sums (the head's from d_res and the last FiLM output).  S: dict with lists h, y, dz, dpre and the matrix dfp"""
    d = lambda t: t.double()  # noqa: E731
    g = {}
    y_prev = [d(x)] + [d(t) for t in S["y"][:-1]]
    for i, dz in enumerate(S["dz"]):
        g[f"film_w{i}"], g[f"film_b{i}"] = d(dz).t() @ y_prev[i], d(dz).sum(0)
    h_prev = [d(cond)] + [d(t) for t in S["h"][:-1]]
    for l, dp in enumerate(S["dpre"]):
        g[f"map_w{l}"], g[f"map_b{l}"] = d(dp).t() @ h_prev[l], d(dp).sum(0)
    g["map_wo"], g["map_bo"] = d(S["dfp"]).t() @ d(S["h"][-1]), d(S["dfp"]).sum(0)
    g["out_w"], g["out_b"] = d(d_res).t() @ d(S["y"][-1]), d(d_res).sum(0)
    return g


def film_chain(net, cond, x, d_res, mode="float64", leaky_masks=None, defect=None):
    """forward and hand-written backward of the chain.  cond [M, >= cond_dim], x [M, >= x_dim], d_res [M, >= out_dim] (further columns are
    ignored: the widths are the weights').  leaky_masks: per mapping layer a bool [M, H] of the signs (h_l > 0) the backward uses instead of
    its own.  defect (split mode): (class of PRODUCT_CLASSES, layer index) or a name of CONSTANT_DEFECTS.
    -> dict: res, h[l], z[i], y[i], dz[i], dfp = [dF_0.. | dphase_0..], dfp_rowmax, dpre[l], d_cond, d_x, grads{name} (float64),
       flips[l] = (signs that differ from this evaluation's own, largest |pre-activation| among them, largest |pre-activation| of the layer)"""
    A = _Arith(mode, defect)
    p = unpack_net(net, A.dtype)
    n_map, n_film, H = len(p["map_w"]), len(p["film_w"]), p["film_w"][0].shape[0]
    cond = cond.detach().cpu().to(A.dtype)[:, :p["map_w"][0].shape[1]]
    x = x.detach().cpu().to(A.dtype)[:, :p["film_w"][0].shape[1]]
    d_res = d_res.detach().cpu().to(A.dtype)[:, :p["out_w"].shape[0]]
    c15, c30 = A.const("dF15", 15.0, 2.0 ** -13), A.const("freq30", 30.0, 2.0 ** -14)
    slope_bwd = A.const("leaky", 0.2, 2.0 ** -13)
    cos_err = 2e-6 if defect == "cos" else 0.0
    # ---- forward
    h, hs, pres = cond, [], []
    for l in range(n_map):
        pre = A.prod(h, p["map_w"][l], p["map_b"][l], ("fwd_map", l))
        h = torch.where(pre > 0, pre, 0.2 * pre)
        pres.append(pre); hs.append(h)
    fo = A.prod(h, p["mo_w"], p["mo_b"], ("fwd_head", 0))
    F = [fo[:, i * H:(i + 1) * H] for i in range(n_film)]
    P = [fo[:, (n_film + i) * H:(n_film + i + 1) * H] for i in range(n_film)]
    y, zs, ys, fs, args = x, [], [], [], []
    for i in range(n_film):
        z = A.prod(y, p["film_w"][i], p["film_b"][i], ("fwd_z", i))
        f = 15.0 * F[i] + c30
        arg = f * z + P[i]
        y = torch.sin(arg)
        zs.append(z); ys.append(y); fs.append(f); args.append(arg)
    res = A.prod(y, p["out_w"], p["out_b"], ("fwd_out", 0))
    # ---- backward
    dY = A.prod(d_res, p["out_w"].t(), None, ("bwd_out", 0))
    dzs, dFs, dPs, d_x = [None] * n_film, [None] * n_film, [None] * n_film, None
    for i in range(n_film - 1, -1, -1):
        g = dY * (torch.cos(args[i]) + cos_err)
        dzs[i], dFs[i], dPs[i] = g * fs[i], c15 * g * zs[i], g
        nxt = A.prod(dzs[i], p["film_w"][i].t(), None, ("bwd_film", i))
        if i > 0:
            dY = nxt
        else:
            d_x = nxt
    dfp = torch.cat(dFs + dPs, 1)
    dh = A.prod(dfp, p["mo_w"].t(), None, ("bwd_head", 0))
    dpres, flips, d_cond = [None] * n_map, [None] * n_map, None
    for l in range(n_map - 1, -1, -1):
        own = pres[l] > 0
        mask = own if leaky_masks is None else leaky_masks[l].cpu()
        diff = own != mask
        flips[l] = (int(diff.sum()), float(pres[l][diff].abs().max()) if diff.any() else 0.0, float(pres[l].abs().max()))
        dpres[l] = torch.where(mask, dh, slope_bwd * dh)
        nxt = A.prod(dpres[l], p["map_w"][l].t(), None, ("bwd_map", l) if l > 0 else ("bwd_cond", 0))
        if l > 0:
            dh = nxt
        else:
            d_cond = nxt
    out = dict(res=res, h=hs, z=zs, y=ys, dz=dzs, dfp=dfp, dfp_rowmax=dfp.abs().amax(1), dpre=dpres, d_cond=d_cond, d_x=d_x, flips=flips)
    out["grads"] = param_grads(out, cond, x, d_res)
    return out


# ---------------------------------------------------------------------------------------------------------- groups and bars
def groups(S):
    """the quantity groups of one evaluation (or of the kernels' stored matrices in the same dict form), each float64"""
    n_film = len(S["z"])
    H = S["z"][0].shape[1]
    d = lambda t: t.detach().cpu().double()  # noqa: E731
    g = {"res": d(S["res"]), "d_cond": d(S["d_cond"]), "d_x": d(S["d_x"]), "dfp_rowmax": d(S["dfp_rowmax"])}
    for l, (h, dp) in enumerate(zip(S["h"], S["dpre"])):
        g[f"h{l}"], g[f"dpre{l}"] = d(h), d(dp)
    for i in range(n_film):
        g[f"z{i}"], g[f"y{i}"], g[f"dz{i}"] = d(S["z"][i]), d(S["y"][i]), d(S["dz"][i])
        g[f"dF{i}"], g[f"dphase{i}"] = d(S["dfp"][:, i * H:(i + 1) * H]), d(S["dfp"][:, (n_film + i) * H:(n_film + i + 1) * H])
    for k, v in S["grads"].items():
        g[f"grad:{k}"] = d(v)
    return g


def distance(got, ref, per_row=False):
    """max-norm distance relative to the reference's largest entry; per_row (row matrices of a batch whose rows differ in scale): every row by
    its own largest reference entry, rows whose reference is all zero left to the caller"""
    if per_row:
        if ref.dim() == 1:
            got, ref = got[:, None], ref[:, None]
        norm = ref.abs().amax(1)
        live = norm > 0
        if not live.any():
            return 0.0
        return float(((got - ref).abs().amax(1)[live] / norm[live]).max())
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)


def bars(ref64, ref32, per_row=False):
    """relative bar of every group: NOISE_FACTOR x (the float32 restatement's distance from the float64 one, same normaliser), floored at
    NOISE_FACTOR x 2^-24.  Gradients of parameters are sums over the batch: never per row."""
    g64, g32 = groups(ref64), groups(ref32)
    return {k: NOISE_FACTOR * max(distance(g32[k], g64[k], per_row and not k.startswith("grad:")), NOISE_FLOOR) for k in g64}


def ratios(got, ref64, bar, per_row=False):
    """err / bar of every group"""
    gg, g64 = groups(got), groups(ref64)
    return {k: distance(gg[k], g64[k], per_row and not k.startswith("grad:")) / bar[k] for k in g64}


# ---------------------------------------------------------------------------------------------------------- cases
# networks as (H, n_map, n_film, cond_dim, x_dim, out_dim)
DDF_NET = (256, 5, 5, 35, 15, 1)      # the DDF network (neusky_config.py:163-177)
RENI_NET = (128, 5, 9, 300, 10, 3)    # the RENI-shaped illumination decoder (latent 100 x 3)
# the wave's 32-row tile, the 128-row forward / FiLM-backward workgroups, the 256-row mapping-backward workgroup, two of those plus a tail
ROW_EDGES = (1, 31, 32, 33, 127, 128, 129, 255, 256, 257, 582)
DIM_M = 129
# every cond_dim of {1, 4, 15, 16, 17, 33, 128, 129, 320} (k-step 16, DMA group 8 slabs = 128, the limit), x_dim of {1, 3, 4, 13, 16},
# out_dim of {1, 2, 3, 4}, depth (1, 1) at both widths
DIM_NETS = ((128, 1, 1, 1, 1, 1), (256, 1, 1, 4, 3, 2), (128, 2, 2, 15, 4, 3), (256, 2, 3, 16, 13, 4), (128, 3, 2, 17, 16, 1),
            (256, 2, 2, 33, 1, 2), (128, 2, 3, 128, 3, 3), (256, 3, 2, 129, 4, 4), (128, 2, 2, 320, 13, 1))
MAX_LAYERS = 12
BIAS_TABLE_FLOATS = 6144


def table_fits(H, n_map, n_film):
    """the chain kernels' bias table: every mapping bias, three rows (F, phase, z) per FiLM layer, the head's 32"""
    return 1 <= n_map <= MAX_LAYERS and 1 <= n_film <= MAX_LAYERS and n_map * H + 3 * n_film * H + 32 <= BIAS_TABLE_FLOATS


def deepest(H, accepts=table_fits):
    """the (n_map, n_film) with the most layers that accepts(H, n_map, n_film) takes; among equals the one with more FiLM layers"""
    ok = [(m + f, f, m) for m in range(1, MAX_LAYERS + 2) for f in range(1, MAX_LAYERS + 2) if accepts(H, m, f)]
    _, f, m = max(ok)
    return m, f


def deepest_net(H, accepts=table_fits):
    return (H, *deepest(H, accepts), 36, 8, 2)


def all_shapes():
    """(network, M) of every launched parity case"""
    return ([(net, M) for net in (DDF_NET, RENI_NET) for M in ROW_EDGES] + [(net, DIM_M) for net in DIM_NETS]
            + [(deepest_net(H), DIM_M) for H in (128, 256)])


def pad4(n):
    return (n + 3) // 4 * 4


def make_weights(H, n_map, n_film, cond_dim, x_dim, out_dim):
    """the padded weight list FilmChainFn takes, on the CPU, at the scales of test_gpu_film_frozen.py (uniform; the FiLM layers' at 1/25 of
    the SIREN initialisation so that frequencies ~30 give arguments ~1e1..1e2); pad rows and columns zero"""
    g = torch.Generator().manual_seed(1000 * H + 10 * n_film + n_map + 7 * cond_dim + x_dim)

    def padded(rows, cols, real_rows, real_cols, scale):
        w = torch.zeros(rows, cols)
        w[:real_rows, :real_cols] = (torch.rand(real_rows, real_cols, generator=g) * 2 - 1) * scale
        return w
    wb = []
    for l in range(n_map):
        k = cond_dim if l == 0 else H
        wb += [padded(H, pad4(k), H, k, (6.0 / k) ** 0.5), padded(H, 1, H, 1, 0.3).reshape(H)]
    wb += [padded(2 * n_film * H, H, 2 * n_film * H, H, 0.25 * (6.0 / H) ** 0.5), padded(2 * n_film * H, 1, 2 * n_film * H, 1, 0.3).reshape(-1)]
    for i in range(n_film):
        k = x_dim if i == 0 else H
        wb += [padded(H, pad4(k), H, k, (1.0 / k) if i == 0 else (6.0 / k) ** 0.5 / 25.0), padded(H, 1, H, 1, 0.3).reshape(H)]
    wb += [padded(4, H, out_dim, H, (6.0 / H) ** 0.5), padded(4, 1, out_dim, 1, 0.3).reshape(4)]
    return wb


def make_inputs(M, cond_dim, x_dim, out_dim):
    """cond [M, pad4(cond_dim)], x [M, pad4(x_dim)], d_res [M, 4] ~ N(0, 1); pad columns zero"""
    g = torch.Generator().manual_seed(7 + M + 1000 * cond_dim)
    cond = torch.zeros(M, pad4(cond_dim)); cond[:, :cond_dim] = torch.randn(M, cond_dim, generator=g) * 0.5
    x = torch.zeros(M, pad4(x_dim)); x[:, :x_dim] = torch.rand(M, x_dim, generator=g) * 2 - 1
    d_res = torch.zeros(M, 4); d_res[:, :out_dim] = torch.randn(M, out_dim, generator=g)
    return cond, x, d_res


def oracle_params(wb, n_map, n_film, cond_dim, x_dim, out_dim, dtype=torch.float64):
    """the padded weight list as oracle.film_siren's parameter dictionary (pads cropped)"""
    u = unpack_net(wb, dtype)
    p = {}
    for l in range(n_map):
        p[f"ddf.map_w{l}"], p[f"ddf.map_b{l}"] = (u["map_w"][l][:, :cond_dim] if l == 0 else u["map_w"][l]).clone(), u["map_b"][l].clone()
    p["ddf.map_wo"], p["ddf.map_bo"] = u["mo_w"].clone(), u["mo_b"].clone()
    for i in range(n_film):
        p[f"ddf.film_w{i}"], p[f"ddf.film_b{i}"] = (u["film_w"][i][:, :x_dim] if i == 0 else u["film_w"][i]).clone(), u["film_b"][i].clone()
    p["ddf.out_w"], p["ddf.out_b"] = u["out_w"][:out_dim].clone(), u["out_b"][:out_dim].clone()
    return p


def reference_and_bars(wb, cond, x, d_res, leaky_masks=None, per_row=False):
    """-> (float64 restatement under leaky_masks, relative bar of every group).  The noise behind the bars is the float32 restatement's
    distance from the float64 restatement that differentiates the branches float32 took (a flipped LeakyReLU decision is no rounding)"""
    ref32 = film_chain(wb, cond, x, d_res, "float32")
    masks32 = [h > 0 for h in ref32["h"]]
    bar = bars(film_chain(wb, cond, x, d_res, "float64", leaky_masks=masks32), ref32, per_row)
    return film_chain(wb, cond, x, d_res, "float64", leaky_masks=leaky_masks), bar
