"""The FiLM-SIREN chain kernels (csrc/film_chain.hip: nsky_film_chain_fwd / _bwd_film / _bwd_map, through the C ABI) against the float64
restatement film_chain_cpu.py, per stored quantity, at bars tied to float32 noise.

Every matrix the kernels store is its own group: res, each h_l, z_i, y_i, dz_i, the dF and dphase halves of dfp per layer, dfp_rowmax, each
dpre_l, d_cond, d_x, and every parameter gradient formed in float64 on the host from those matrices.  A group's bar is 4 x the float32
restatement's distance from the float64 one (same inputs, same normaliser), floored at 4 x 2^-24, applied to the group's largest reference
entry (film_chain_cpu.reference_and_bars).  The reference differentiates the LeakyReLU branches the kernel took (signs of its saved h_l);
the decisions that differ from float64's are capped as in test_gpu_field_chain.py.

The buffers are laid out to show any access outside the ABI: tile-native saves pre-filled with NaN; row-major inputs with one NaN guard row
behind row M and NaN in the columns beyond pad4(dim) of a wider leading dimension; row-major outputs with 64 sentinel guard rows and sentinel
columns beyond pad4(dim) that must come back bit-unchanged.

Measured on an MI355X (worst err / bar over a case's groups; run with -s for every group of every case): row edges 0.30 .. 0.54, dimension
edges 0.25 .. 0.68 (h0 of the (1, 1)-deep network with one conditioning column), deepest networks 0.52 / 0.36, row-scaled gradient 0.29
(per row), 1e-7 gradient 0.38, end to end 0.25 .. 0.28; by kind of group: res 0.43, h 0.68, z 0.42, y 0.32, dz 0.52, dF 0.42, dphase 0.48,
dfp_rowmax 0.54, dpre 0.46, d_cond 0.35, d_x 0.49, parameter gradients 0.51.  No LeakyReLU decision differed from float64's in any case; the
row-scaled run is the unscaled run times the row's power of two to the bit.  The guards found the d_cond / d_x stores running up to the leading
dimension (every case failed on them before the stores were bounded by pad4(dim)).  With the (weight residual) x (dz hi) term of ONE backward
product removed in a scratch build (W_2^T dz_2 of the FiLM backward), every case with three or more FiLM layers fails: dz, dF, dphase of
layers 1 and 0, dfp_rowmax, every dpre, d_cond, d_x and the gradients formed from them at 2.4 .. 26 x their bars, where the older bars of
test_gpu_film_chain.py (2e-4 / 3e-4 of the largest entry) stand at 0.66 .. 1.29."""
import functools

import pytest
import torch

import film_chain_cpu as FC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 7.0e37
GUARD_ROWS = 64


def _id(v):
    return "-".join(map(str, v)) if isinstance(v, tuple) else str(v)


@functools.lru_cache(maxsize=None)
def _weights(net):
    return tuple(w.to(DEV) for w in FC.make_weights(*net))


def _desc(net, wb):
    from neusky_amd import hip
    H, n_map, n_film, cond_dim, x_dim, out_dim = net
    o = 2 * n_map + 2
    return hip.film_net(cond_dim, x_dim, out_dim, [wb[2 * l] for l in range(n_map)], [wb[2 * l + 1] for l in range(n_map)], wb[2 * n_map], wb[2 * n_map + 1],
                        [wb[o + 2 * i] for i in range(n_film)], [wb[o + 2 * i + 1] for i in range(n_film)], wb[o + 2 * n_film], wb[o + 2 * n_film + 1])


@functools.lru_cache(maxsize=None)
def _streams(net):
    """descriptor and the three packed streams (forward, FiLM backward, mapping backward) of a network"""
    from neusky_amd import hip
    desc = _desc(net, _weights(net))
    packs = []
    for direction in (0, 1, 2):
        nbytes, _ = hip.film_stream_layout(desc, direction)
        stream = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
        table = torch.empty(hip.FILM_TABLE_FLOATS, device=DEV)
        hip.film_pack(desc, stream, table, direction)
        packs.append((stream, table))
    return desc, packs


def _guarded_input(t, width):
    """[M, pad4(dim)] -> device [M + 1, width] view of its first M rows: NaN in the columns beyond and in the row behind"""
    M, w = t.shape
    buf = torch.full((M + 1, width), float("nan"), device=DEV)
    buf[:M, :w] = t.to(DEV)
    return buf[:M]


def _guarded_output(M, width):
    return torch.full((M + GUARD_ROWS, width), SENTINEL, device=DEV)


def _touched(buf, M, written, what):
    """what of a row-major output's guards was written (asserted empty once the case's figures are printed)"""
    bits = buf.view(torch.int32)
    want = torch.full((1,), SENTINEL, device=DEV).view(torch.int32)
    out = []
    if not bool((bits[M:] == want).all()):
        out.append(f"{what}: guard rows behind row {M} were written")
    if not bool((bits[:M, written:] == want).all()):
        cols = torch.nonzero((bits[:M, written:] != want).any(0)).flatten() + written
        out.append(f"{what}: columns {cols.tolist()} beyond pad4(dim) = {written} (leading dimension {buf.shape[1]}) were written")
    return out


def _run_kernels(net, M, cond, x, d_res):
    """the three kernels through the C ABI on guarded buffers -> the stored matrices in film_chain_cpu's dict form (CPU, row-major) + gmax"""
    from neusky_amd import hip
    H, n_map, n_film, cond_dim, x_dim, out_dim = net
    desc, ((s0, t0), (s1, t1), (s2, t2)) = _streams(net)
    pc, px = FC.pad4(cond_dim), FC.pad4(x_dim)
    ldx_out = min(16, px + 4)  # (nsky_film_chain_bwd_film takes ldx <= 16)
    cond_d, x_d, dres_d = _guarded_input(cond, pc + 8), _guarded_input(x, px + 8), _guarded_input(d_res, 8)
    Mp = hip.film_rows(M)
    mk = lambda n, w=H: [torch.full((Mp, w), float("nan"), device=DEV) for _ in range(n)]  # noqa: E731
    hs, zs, ys, dzs, dpres = mk(n_map), mk(n_film), mk(n_film), mk(n_film), mk(n_map)
    dfp = torch.full((Mp, 2 * n_film * H), float("nan"), device=DEV)
    rowmax = torch.full((Mp,), float("nan"), device=DEV)
    res, d_cond, d_x = _guarded_output(M, 8), _guarded_output(M, pc + 8), _guarded_output(M, ldx_out)
    gmax = torch.zeros(n_film + 1 + n_map, device=DEV)
    hip.film_chain_fwd(desc, s0, t0, cond_d, x_d, M, hs, zs, ys, res[:M])
    hip.film_chain_bwd_film(desc, s1, t1, M, dres_d, hs[-1], zs, dzs, dfp, rowmax, gmax[:n_film + 1], d_x[:M])
    hip.film_chain_bwd_map(desc, s2, t2, M, dfp, rowmax, hs, dpres, d_cond[:M], gmax[n_film + 1:])
    torch.cuda.synchronize()
    touched = _touched(res, M, 4, "res") + _touched(d_cond, M, pc, "d_cond") + _touched(d_x, M, px, "d_x")
    rows = lambda t, w=H: hip.film_native_to_rows(t, M, w).cpu()  # noqa: E731
    S = dict(res=res[:M, :4].cpu(), h=[rows(t) for t in hs], z=[rows(t) for t in zs], y=[rows(t) for t in ys], dz=[rows(t) for t in dzs],
             dfp=rows(dfp, 2 * n_film * H), dfp_rowmax=rowmax[:M].cpu(), dpre=[rows(t) for t in dpres], d_cond=d_cond[:M, :pc].cpu(),
             d_x=d_x[:M, :px].cpu())
    for k, v in S.items():
        for t in (v if isinstance(v, list) else [v]):
            assert bool(torch.isfinite(t).all()), f"{k}: not finite (a NaN pre-fill or guard was read, or a live row was not stored)"
    S["grads"] = FC.param_grads(S, cond, x, d_res[:, :4])
    S["gmax"] = gmax.cpu()
    S["touched"] = touched
    S["native"] = dict(hs=hs, ys=ys, dzs=dzs, dpres=dpres, dfp=dfp, gmax=gmax)
    return S


def _check_gmax(S):
    """the published maxima are the largest stored magnitudes, exactly (maxima of the stored floats themselves)"""
    want = [t.abs().max() for t in S["dz"]] + [S["dfp"].abs().max()] + [t.abs().max() for t in S["dpre"]]
    assert torch.equal(S["gmax"], torch.stack(want)), (S["gmax"], want)
    assert torch.equal(S["dfp_rowmax"], S["dfp"].abs().amax(1))


def _check_flips(ref):
    flips = []
    for l, (count, worst, largest) in enumerate(ref["flips"]):
        assert count <= FC.flip_cap(ref["h"][l].numel()) and worst < FC.FLIP_REL * largest, ("LeakyReLU decisions", l, count, worst, largest)
        flips.append(count)
    return flips


def _parity(name, net, M, cond, x, d_res, per_row=False):
    S = _run_kernels(net, M, cond, x, d_res)
    wb = [w.cpu() for w in _weights(net)]
    ref, bar = FC.reference_and_bars(wb, cond, x, d_res, leaky_masks=[h > 0 for h in S["h"]], per_row=per_row)
    flips = _check_flips(ref)
    _check_gmax(S)
    r = FC.ratios(S, ref, bar, per_row)
    worst = max(r, key=r.get)
    print(f"{name}: worst err/bar {r[worst]:.3f} ({worst}); flips {flips}")
    print("    " + " ".join(f"{k}={v:.2f}" for k, v in r.items()))
    missed = {k: round(v, 3) for k, v in r.items() if not v <= 1.0}
    assert not missed, f"{name}: groups over their bar (err / bar): {missed}"
    assert not S["touched"], S["touched"]
    return S, ref


def _inputs(net, M):
    return FC.make_inputs(M, net[3], net[4], net[5])


# ------------------------------------------------------------------------------------------------------------------ row edges
@pytest.mark.parametrize("M", FC.ROW_EDGES)
@pytest.mark.parametrize("net", [FC.DDF_NET, FC.RENI_NET], ids=_id)
def test_row_edges(net, M):
    _parity(f"rows {_id(net)} M={M}", net, M, *_inputs(net, M))


# ------------------------------------------------------------------------------------------------------------------ dimension edges
@pytest.mark.parametrize("net", FC.DIM_NETS, ids=_id)
def test_dimension_edges(net):
    from neusky_amd import hip
    assert hip.film_supported(net[0], *net)
    _parity(f"dims {_id(net)} M={FC.DIM_M}", net, FC.DIM_M, *_inputs(net, FC.DIM_M))


@pytest.mark.parametrize("H", [128, 256])
def test_deepest_supported_network(H):
    from neusky_amd import hip
    accepts = lambda h, m, f: hip.film_supported(h, h, m, f, 36, 8, 2)  # noqa: E731
    net = FC.deepest_net(H, accepts)
    assert net == FC.deepest_net(H), "the CPU suite's restatement of the table limit disagrees with hip.film_supported"
    n_map, n_film = net[1], net[2]
    assert not accepts(H, n_map + 1, n_film) and not accepts(H, n_map, n_film + 1)
    _parity(f"deepest {_id(net)} M={FC.DIM_M}", net, FC.DIM_M, *_inputs(net, FC.DIM_M))


@pytest.mark.parametrize("net", [(128, 2, 2, 321, 8, 2), (128, 2, 2, 36, 17, 2), (128, 2, 2, 36, 8, 5), (128, 2, 2, 0, 8, 2), (64, 2, 2, 36, 8, 2),
                                 (192, 2, 2, 36, 8, 2), (128, 12, 12, 36, 8, 2), (256, 12, 4, 36, 8, 2), (256, 5, 9, 300, 10, 3)], ids=_id)
def test_shapes_past_a_limit_are_refused_not_launched(net):
    """one step past cond_dim 320, x_dim 16, out_dim 4, an empty conditioning, the two widths, and the bias table at each width"""
    from neusky_amd import hip
    H, n_map, n_film, cond_dim, x_dim, out_dim = net
    assert not hip.film_supported(H, *net)
    wb = [torch.zeros_like(w, device=DEV) for w in FC.make_weights(H, n_map, n_film, max(cond_dim, 1), x_dim, min(out_dim, 4))]
    with pytest.raises(hip.NeuSkyHipError):
        hip.film_stream_layout(_desc(net, wb))
    for n_m, n_f in ((hip.FILM_MAX_LAYERS + 1, 1), (1, hip.FILM_MAX_LAYERS + 1)):
        assert not hip.film_supported(128, 128, n_m, n_f, 36, 8, 2)


# ------------------------------------------------------------------------------------------------------------------ gradient scale
SCALE_M = 257


def _scaled_d_res(d_res):
    """rows multiplied by 2^k, k cycling through -30 .. 6, every fifth row exactly zero"""
    M = d_res.shape[0]
    k = torch.arange(M) % 37 - 30
    scale = torch.ldexp(torch.ones(M), k)
    scale[::5] = 0.0
    return d_res * scale[:, None], k, scale


BACKWARD = ("dz", "dfp", "dfp_rowmax", "dpre", "d_cond", "d_x")


def _backward_rows(S):
    out = {}
    for k in BACKWARD:
        for j, t in enumerate(S[k] if isinstance(S[k], list) else [S[k]]):
            out[f"{k}{j}"] = t.reshape(t.shape[0], -1)
    return out


@functools.lru_cache(maxsize=None)
def _unit_scale_run():
    cond, x, d_res = _inputs(FC.DDF_NET, SCALE_M)
    return _parity(f"scale unit {_id(FC.DDF_NET)} M={SCALE_M}", FC.DDF_NET, SCALE_M, cond, x, d_res)[0]


@functools.lru_cache(maxsize=None)
def _row_scaled_run():
    cond, x, d_res = _inputs(FC.DDF_NET, SCALE_M)
    scaled, k, scale = _scaled_d_res(d_res)
    return _parity(f"scale rows 2^-30..2^6 {_id(FC.DDF_NET)} M={SCALE_M}", FC.DDF_NET, SCALE_M, cond, x, scaled, per_row=True)[0], scale


def test_row_scaled_gradient_per_row_parity_and_zero_rows():
    """(a) errors and noise normalised per row; rows of d_res that are exactly zero give exactly zero rows in every backward output"""
    S, scale = _row_scaled_run()
    zero = scale == 0
    for k, t in _backward_rows(S).items():
        assert float(t[zero].abs().max()) == 0.0, f"{k}: rows of a zero d_res row are not zero"
    assert float(S["dfp_rowmax"][zero].abs().max()) == 0.0


def test_row_scaled_gradient_is_the_unit_run_times_the_scale_bit_for_bit():
    """(b) a batch row sits on a lane and every pre-scale is a power of two clamped to 2^+-100: row r of every stored backward matrix of the
    run with d_res row r times 2^k is 2^k times the unscaled run's row, to the bit"""
    S, scale = _row_scaled_run()
    U = _backward_rows(_unit_scale_run())
    for k, t in _backward_rows(S).items():
        want = U[k] * scale[:, None]
        bad = (t != want).any(1)
        assert not bool(bad.any()), f"{k}: {int(bad.sum())} rows differ from 2^k x the unscaled row, first {torch.nonzero(bad).flatten()[:8].tolist()}"


def test_zero_gradient_gives_zeros_and_the_weight_gradient_takes_a_zero_maximum():
    """(c) d_res all zero: every output finite and zero, gmax stays zero; ops.grad_weight with that zero a_scale_max returns finite zeros"""
    from neusky_amd import ops
    net = FC.DDF_NET
    H, n_map, n_film = net[:3]
    cond, x, d_res = _inputs(net, SCALE_M)
    S = _run_kernels(net, SCALE_M, cond, x, torch.zeros_like(d_res))
    for k, t in _backward_rows(S).items():
        assert float(t.abs().max()) == 0.0, k
    assert float(S["gmax"].abs().max()) == 0.0 and not S["touched"], S["touched"]
    N, wb = S["native"], _weights(net)
    o = 2 * n_map + 2
    i = n_film - 1
    dW, db = ops.grad_weight(N["dzs"][i], N["ys"][i - 1], SCALE_M, H, H, wb[o + 2 * i], wb[o + 2 * i + 1], a_native_nt=H // 32, b_native_nt=H // 32,
                             a_scale_max=N["gmax"][i:i + 1])
    assert float(dW.abs().max()) == 0.0 and float(db.abs().max()) == 0.0 and bool(torch.isfinite(dW).all() and torch.isfinite(db).all())
    dW, db = ops.grad_weight(N["dfp"], N["hs"][-1], SCALE_M, 2 * n_film * H, H, wb[2 * n_map], wb[2 * n_map + 1], a_native_nt=2 * n_film * H // 32,
                             b_native_nt=H // 32, a_scale_max=N["gmax"][n_film:n_film + 1])
    assert float(dW.abs().max()) == 0.0 and float(db.abs().max()) == 0.0 and bool(torch.isfinite(dW).all() and torch.isfinite(db).all())


def test_tiny_uniform_gradient_keeps_the_relative_bars():
    """(d) d_res at 1e-7, the size of a mean over ~1e5 rays: the same relative bars as at O(1)"""
    cond, x, d_res = _inputs(FC.DDF_NET, SCALE_M)
    _unit_scale_run()
    _parity(f"scale 1e-7 {_id(FC.DDF_NET)} M={SCALE_M}", FC.DDF_NET, SCALE_M, cond, x, d_res * 1e-7)


# ------------------------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("M", [129, 257])
@pytest.mark.parametrize("net", [FC.DDF_NET, FC.RENI_NET], ids=_id)
def test_film_apply_end_to_end(net, M):
    """ops.film_apply(train_weights=True): d_cond, d_x and every parameter gradient -- now from the streaming weight-gradient kernel and its
    siblings -- against float64.  A weight gradient's bar is its group's plus the 1e-6 |dZ|^T |X| test_gpu_wgrad_native.py allows that kernel"""
    from neusky_amd import hip, ops
    H, n_map, n_film, cond_dim, x_dim, out_dim = net
    cond, x, d_res = _inputs(net, M)
    wb = [w.clone().requires_grad_(True) for w in _weights(net)]
    cd, xd = cond.to(DEV).requires_grad_(True), x.to(DEV).requires_grad_(True)
    ops.begin_step(DEV)
    assert ops._film_fused_ok(xd, cd, n_map, n_film, wb)
    res = ops.film_apply(xd, cd, n_map, n_film, True, True, *wb)
    grads = torch.autograd.grad(res, [cd, xd] + wb, d_res.to(DEV))
    torch.cuda.synchronize()
    # the kernel's LeakyReLU decisions: the same kernels on the same bits (deterministic), through the C ABI
    S = _run_kernels(net, M, cond, x, d_res)
    assert torch.equal(S["res"], res.detach().cpu())
    ref, bar = FC.reference_and_bars([w.detach().cpu() for w in wb], cond, x, d_res, leaky_masks=[h > 0 for h in S["h"]])
    _check_flips(ref)
    g64 = FC.groups(ref)
    names = [f"map_{c}{l}" for l in range(n_map) for c in "wb"] + ["map_wo", "map_bo"] + [f"film_{c}{i}" for i in range(n_film) for c in "wb"] + ["out_w", "out_b"]
    # |dZ|^T |X| of every weight gradient, |dZ| column sums of every bias gradient
    mag = FC.param_grads({k: ([t.abs() for t in v] if isinstance(v, list) else v.abs()) for k, v in ref.items() if k in ("h", "y", "dz", "dpre", "dfp")},
                         cond.abs(), x.abs(), d_res.abs())
    ratio = {}
    for key, got, want, extra in ([("d_cond", grads[0], g64["d_cond"], 0.0), ("d_x", grads[1], g64["d_x"], 0.0)]
                                  + [("grad:" + n, g, g64["grad:" + n], 1e-6 * mag[n]) for n, g in zip(names, grads[2:])]):
        tol = bar[key] * float(want.abs().max()) + extra
        ratio[key] = float(((got.detach().cpu().double() - want).abs() / tol).max())
    worst = max(ratio, key=ratio.get)
    print(f"end to end {_id(net)} M={M}: worst err/bar {ratio[worst]:.3f} ({worst})")
    print("    " + " ".join(f"{k}={v:.2f}" for k, v in ratio.items()))
    missed = {k: round(v, 3) for k, v in ratio.items() if not v <= 1.0}
    assert not missed, f"groups over their bar (err / bar): {missed}"
