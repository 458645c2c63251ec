"""The sdf value chain kernels (csrc/sdf_chain.hip: nsky_sdf_chain_fwd / _bwd, through the C ABI) against the float64 restatement
sdf_chain_cpu.py, per stored quantity, at bars tied to float32 noise, and per class of launch plan.

Every quantity the kernels store is its own group: sdf, a0, a1, dz1, dz0, dE, the batch sums dw2 and db2, and the four parameter gradients
formed in float64 on the host from the stored matrices.  A group's bar is 4 x the float32 restatement's distance from the float64 one (same
inputs, same normaliser), floored at 4 x 2^-24, applied to the group's largest reference entry (sdf_chain_cpu.reference_and_bars, the rule of
film_chain_cpu.py); dw2 and db2, sums of M terms by fp32 atomics, get 1e-6 x the sum of the terms' magnitudes on top.  gmax is held to the
largest stored magnitudes exactly.

The buffers are laid out to show any access outside the ABI: tile-native saves pre-filled with NaN; E and g_sdf with a NaN guard row behind
row M and E with NaN columns beyond in_dim, run at ldE = in_dim and at in_dim + 8 (the same bits are required of both); sdf and dE with 64
sentinel guard rows and dE with sentinel columns beyond in_dim that must come back bit-unchanged.

Launch plans (chain.h tail_plan; sdf_chain_cpu.plan_rows at the device's CU count): a batch row's results depend on that row alone (the
operand scale is the row's, row_scale; an MFMA output element accumulates from its own row and column; the weight tiles and their scales are
the launch's), so every per-row matrix of a launch of any plan must be bit-equal to the same rows run in chunks of <= 8192 rows, whose
workgroups have one live wave.  A mismatch there is a ring race or a leak between rows, never a tolerance.

Measured on an MI355X, 256 CUs (worst err / bar over a case's groups; run with -s for every group of every case): row edges 0.32 .. 0.44 and
0.92 at M = 1 (sdf: one value against the 4 x 2^-24 floor), dimension edges 0.31 .. 0.52, steep weights 0.30, row-scaled gradient 0.52 (per
row), 1e-7 gradient 0.36, end to end 0.23 .. 0.33; by kind of group: sdf 0.92 (0.38 without M = 1), a0 0.44, a1 0.55, dz1 0.71, dz0 0.46, dE
0.40, dw2 0.25, db2 0.04, parameter gradients 0.71.  Launch plans (8187 .. 66 843 rows): every per-row matrix bit-equal to the chunked run and
to a second run in all eight cases, gmax exact, dw2 0.010 .. 0.026 and db2 <= 0.005 of their bars.  The row-scaled run is the unscaled run
times the row's power of two to the bit.  The guards found the dE stores running to min(ldE, 32 ceil(in_dim / 32)): at ldE = in_dim + 8 every
case but in_dim 32 and 64 failed on columns in_dim .. in_dim + 7 before the stores were bounded by in_dim; SdfChainFn.backward handed
autograd a [M, ld(E)] gradient for a [M, in_dim] view of a wider buffer (a shape error), now the view of E's own shape.
With the (weight residual) x (dz hi) term of W1^T dz1 removed from sdf_bwd_kernel in a scratch build, every parity case against float64
fails (25 of the 40 tests; the plan, refusal and zero-gradient tests compare the library with itself): dz0 at 14 .. 143 x its bar, dE 17 ..
177, dW0 36 .. 292, db0 40 .. 249, nothing else over.  The older bars of test_gpu_sdf_chain.py (3e-5 of the largest entry) stand at dE 6.0
.. 8.3, dW0 6.5 .. 7.6, db0 4.5 .. 8.5 with that build (M = 77, 5000, 33000) and fail too: a whole lost term (2^-11 of a product) is too large
a defect to tell the bars apart.  What does: the undamaged kernels sit at 0.012 .. 0.029 of those older bars in the same three groups and at
0.1 .. 0.5 of these, so an error 35 x the kernels' own still passed there and one of 2 .. 8 x fails here."""
import functools

import pytest
import torch

import sdf_chain_cpu as SC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 7.0e37
GUARD_ROWS = 64
H = SC.HIDDEN
PAD = 8
NATIVE = ("a0", "a1", "dz1", "dz0")


@functools.lru_cache(maxsize=None)
def _net(in_dim, steep=False):
    """device weights, descriptor and the packed streams (forward, backward) of a network"""
    from neusky_amd import hip
    ws = tuple(w.to(DEV) for w in SC.make_weights(in_dim, steep))
    desc = hip.sdf_net(*ws, SC.BETA)
    packs = []
    for direction in (0, 1):
        nbytes, _ = hip.sdf_stream_layout(desc, direction)
        stream = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
        table = torch.empty(hip.FILM_TABLE_FLOATS, device=DEV)
        hip.sdf_pack(desc, stream, table, direction)
        packs.append((stream, table))
    return ws, desc, packs


def _guarded_input(t, width):
    """[M, w] (or [M]) -> device view of the first M rows of a buffer with NaN in the columns beyond w and in the row behind"""
    M = t.shape[0]
    if t.dim() == 1:
        buf = torch.full((M + 1,), float("nan"), device=DEV)
        buf[:M] = t.to(DEV)
        return buf[:M]
    buf = torch.full((M + 1, width), float("nan"), device=DEV)
    buf[:M, :t.shape[1]] = t.to(DEV)
    return buf[:M]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _untouched(buf, M, written, what):
    """what of a row-major output's guards was written (asserted empty once the case's figures are printed)"""
    bits = _bits(buf)
    want = torch.full((1,), SENTINEL, device=DEV).view(torch.int32)
    out = []
    if not bool((bits[M:] == want).all()):
        out.append(f"{what}: guard rows behind row {M} were written")
    if buf.dim() == 2 and not bool((bits[:M, written:] == want).all()):
        cols = torch.nonzero((bits[:M, written:] != want).any(0)).flatten() + written
        out.append(f"{what}: columns {cols.tolist()} beyond in_dim = {written} (leading dimension {buf.shape[1]}) were written")
    return out


def _launch(in_dim, M, E_view, g_view, ldE_out, steep=False, sums=True, native=False):
    """both kernels through the C ABI on guarded outputs -> the stored quantities ON THE DEVICE, row-major, rows < M (native: the tile-native
    buffers are kept too)"""
    from neusky_amd import hip
    ws, desc, ((s0, t0), (s1, t1)) = _net(in_dim, steep)
    Mp = hip.film_rows(M)
    nat = {k: torch.full((Mp, H), float("nan"), device=DEV) for k in NATIVE}
    sdf = torch.full((M + GUARD_ROWS,), SENTINEL, device=DEV)
    dE = torch.full((M + GUARD_ROWS, ldE_out), SENTINEL, device=DEV)
    dw2, db2, gmax = torch.zeros(H, device=DEV), torch.zeros(1, device=DEV), torch.zeros(2, device=DEV)
    hip.sdf_chain_fwd(desc, s0, t0, E_view, M, nat["a0"], nat["a1"], sdf[:M])
    hip.sdf_chain_bwd(desc, s1, t1, M, g_view, nat["a0"], nat["a1"], nat["dz1"], nat["dz0"], dE[:M], dw2 if sums else None,
                      db2 if sums else None, gmax)
    torch.cuda.synchronize()
    S = {"native": dict(nat) if native else None}
    for k in NATIVE:
        S[k] = hip.film_native_to_rows(nat.pop(k), M, H)
    S.update(sdf=sdf[:M], dE=dE[:M, :in_dim], dw2=dw2, db2=db2, gmax=gmax)
    S["touched"] = _untouched(sdf, M, 0, "sdf") + _untouched(dE, M, in_dim, "dE")
    for k in SC.ROW_MATRICES + SC.BATCH_SUMS + ("gmax",):
        assert bool(torch.isfinite(S[k]).all()), f"{k}: not finite (a NaN pre-fill or guard was read, or a live row was not stored)"
    return S


def _check_gmax(S):
    """the published maxima are the largest stored magnitudes of the live rows, exactly (maxima of the stored floats themselves)"""
    want = torch.stack([S["dz1"].abs().max(), S["dz0"].abs().max()])
    assert torch.equal(S["gmax"], want), (S["gmax"], want)


def _run_kernels(in_dim, M, E, g, steep=False):
    """the case at ldE = in_dim and at in_dim + PAD (the same bits required) -> CPU dict in sdf_chain_cpu's form"""
    runs = []
    for pad in (0, PAD):
        runs.append(_launch(in_dim, M, _guarded_input(E, in_dim + pad), _guarded_input(g, 0), in_dim + pad, steep, native=True))
    A, B = runs
    touched = A["touched"] + B["touched"]
    for k in SC.ROW_MATRICES:
        assert _same_bits(A[k], B[k]), f"{k}: ldE = in_dim and ldE = in_dim + {PAD} give different bits"
    assert _same_bits(A["gmax"], B["gmax"])
    _check_gmax(B)
    S = {k: B[k].cpu() for k in SC.ROW_MATRICES + SC.BATCH_SUMS + ("gmax",)}
    S["grads"] = SC.param_grads(S, E)
    S["touched"], S["native"], S["dev"] = touched, B["native"], B
    return S


@functools.lru_cache(maxsize=None)
def _case(in_dim, M, steep=False):
    E, g = SC.make_inputs(M, in_dim, steep)
    return SC.make_weights(in_dim, steep), E, g


def _parity(name, in_dim, M, E, g, steep=False, per_row=False):
    S = _run_kernels(in_dim, M, E, g, steep)
    ref, bar = SC.reference_and_bars(SC.make_weights(in_dim, steep), E, g, per_row)
    r = SC.ratios(S, ref, bar, per_row)
    worst = max(r, key=r.get)
    print(f"{name}: worst err/bar {r[worst]:.3f} ({worst})")
    print("    " + " ".join(f"{k}={v:.2f}" for k, v in r.items()))
    missed = {k: round(v, 3) for k, v in r.items() if not v <= 1.0}
    assert not missed, f"{name}: groups over their bar (err / bar): {missed}"
    assert not S["touched"], S["touched"]
    return S, ref, bar


# ------------------------------------------------------------------------------------------------------------------ row and dimension edges
@pytest.mark.parametrize("M", SC.ROW_EDGES)
def test_row_edges(M):
    _, E, g = _case(SC.DDF_DIM, M)
    _parity(f"rows in_dim={SC.DDF_DIM} M={M}", SC.DDF_DIM, M, E, g)


@pytest.mark.parametrize("in_dim", SC.DIM_EDGES)
def test_dimension_edges(in_dim):
    from neusky_amd import hip
    assert hip.sdf_supported(in_dim, H)
    _, E, g = _case(in_dim, SC.DIM_M)
    _parity(f"dims in_dim={in_dim} M={SC.DIM_M}", in_dim, SC.DIM_M, E, g)


def test_steep_weights():
    """beta z far beyond +-20 in both layers (the saved-output sigmoid at both ends of its range): the same bars"""
    _, E, g = _case(SC.DDF_DIM, 257, True)
    _parity(f"steep in_dim={SC.DDF_DIM} M=257", SC.DDF_DIM, 257, E, g, steep=True)


# ------------------------------------------------------------------------------------------------------------------ launch plans
PLAN_NAMES = ("P1", "P2:2", "P2:5", "P2:7", "P3", "P4", "P5:1", "P5:41")


@pytest.mark.parametrize("name", PLAN_NAMES)
def test_launch_plans(name):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rows = SC.plan_rows(cus)
    assert set(rows) == set(PLAN_NAMES), "a device with fewer than 2 CUs has no ragged tail plan"
    cls, M = rows[name]
    in_dim = SC.DDF_DIM
    assert SC.plan_class((M + 31) // 32, cus) == cls
    gen = torch.Generator(device=DEV).manual_seed(M)
    Ebuf = torch.full((M + 1, in_dim + PAD), float("nan"), device=DEV)
    Ebuf[:M, :in_dim] = torch.randn(M, in_dim, generator=gen, device=DEV) * 0.5
    gbuf = torch.full((M + 1,), float("nan"), device=DEV)
    gbuf[:M] = torch.randn(M, generator=gen, device=DEV)
    S = _launch(in_dim, M, Ebuf[:M], gbuf[:M], in_dim + PAD)
    assert not S["touched"], S["touched"]
    _check_gmax(S)
    # the batch sums against float64 sums of the stored a1 and g; the noise behind the bar: the same sums in float32 (torch)
    g64 = gbuf[:M].double()
    terms = g64[:, None] * S["a1"].double()
    for key, got, ref, mag, f32 in (("dw2", S["dw2"], terms.sum(0), terms.abs().sum(0), (gbuf[:M, None] * S["a1"]).sum(0)),
                                    ("db2", S["db2"], g64.sum().reshape(1), g64.abs().sum().reshape(1), gbuf[:M].sum().reshape(1))):
        top = float(ref.abs().max())
        bar = SC.NOISE_FACTOR * max(float((f32.double() - ref).abs().max()) / top, SC.NOISE_FLOOR)
        ratio = float(((got.double() - ref).abs() / (bar * top + SC.SUM_ALLOWANCE * mag)).max())
        print(f"plan {name} M={M} {SC.tail_plan((M + 31) // 32, cus)}: {key} err/bar {ratio:.3f}")
        assert ratio <= 1.0, (key, ratio)
    del terms
    # the same launch again: the same bits
    T = _launch(in_dim, M, Ebuf[:M], gbuf[:M], in_dim + PAD)
    for k in SC.ROW_MATRICES:
        assert _same_bits(S[k], T[k]), f"{k}: two runs of the same launch differ"
    del T
    # every row against the P1 launch of its chunk
    chunk = SC.chunk_rows(cus)
    for r0 in range(0, M, chunk):
        n = min(chunk, M - r0)
        assert SC.plan_class((n + 31) // 32, cus) == "P1"
        C = _launch(in_dim, n, Ebuf[r0:r0 + n], gbuf[r0:r0 + n], in_dim + PAD, sums=False)
        for k in SC.ROW_MATRICES:
            same = _bits(S[k][r0:r0 + n]) == _bits(C[k])
            if not bool(same.all()):
                bad = torch.nonzero(~same.reshape(n, -1).all(1)).flatten() + r0
                raise AssertionError(f"plan {name} M={M}: {k} differs from the chunked run in {bad.numel()} rows, first {bad[:8].tolist()} "
                                     f"(wave tiles {sorted(set((bad[:64] // 32).tolist()))[:8]})")


# ------------------------------------------------------------------------------------------------------------------ gradient scale
SCALE_M = 257
BACKWARD = ("dz1", "dz0", "dE")
TINY = 2.0 ** -120  # a power-of-two scaling is exact in the normal range only: below this (far under any group's resolution) closeness is asked


def _scaled_g(g):
    """rows multiplied by 2^k, k cycling through -30 .. 6, every fifth row exactly zero"""
    M = g.shape[0]
    k = torch.arange(M) % 37 - 30
    scale = torch.ldexp(torch.ones(M), k)
    scale[::5] = 0.0
    return g * scale, scale


@functools.lru_cache(maxsize=None)
def _unit_scale_run():
    _, E, g = _case(SC.DDF_DIM, SCALE_M)
    return _parity(f"scale unit M={SCALE_M}", SC.DDF_DIM, SCALE_M, E, g)[0]


@functools.lru_cache(maxsize=None)
def _row_scaled_run():
    _, E, g = _case(SC.DDF_DIM, SCALE_M)
    scaled, scale = _scaled_g(g)
    return _parity(f"scale rows 2^-30..2^6 M={SCALE_M}", SC.DDF_DIM, SCALE_M, E, scaled, per_row=True)[0], scale


def test_row_scaled_gradient_per_row_parity_and_zero_rows():
    """errors and noise normalised per row; rows of g_sdf that are exactly zero give exactly zero rows in every backward matrix"""
    S, scale = _row_scaled_run()
    zero = scale == 0
    for k in BACKWARD:
        assert float(S[k][zero].abs().max()) == 0.0, f"{k}: rows of a zero g_sdf row are not zero"


def test_row_scaled_gradient_is_the_unit_run_times_the_scale_bit_for_bit():
    """a batch row sits on a lane and its pre-scale is a power of two: row r of every backward matrix of the run with g_sdf[r] x 2^k is 2^k
    x the unscaled run's row, to the bit, wherever neither value is within 2^6 of float32's subnormals (the softplus tails of this case
    reach them; a power of two times a subnormal rounds)"""
    S, scale = _row_scaled_run()
    U = _unit_scale_run()
    for k in BACKWARD:
        want = U[k] * scale[:, None]
        normal = (want.abs() >= TINY) & (U[k].abs() >= TINY) | (want == 0) & (U[k] == 0) | (scale[:, None] == 0)
        bad = ((S[k] != want) & normal | ((S[k] - want).abs() > TINY)).any(1)
        assert not bool(bad.any()), f"{k}: {int(bad.sum())} rows differ from 2^k x the unscaled row, first {torch.nonzero(bad).flatten()[:8].tolist()}"
        assert float(normal.float().mean()) > 0.5, k


def test_zero_gradient_gives_zeros_and_the_weight_gradient_takes_a_zero_maximum():
    """g_sdf all zero: every backward output finite and zero, gmax stays zero; the weight-gradient kernels with that zero maximum return
    finite zeros"""
    from neusky_amd import hip, ops
    ws, E, g = _case(SC.DDF_DIM, SCALE_M)
    S = _run_kernels(SC.DDF_DIM, SCALE_M, E, torch.zeros_like(g))
    for k in BACKWARD + SC.BATCH_SUMS + ("gmax",):
        assert float(S[k].abs().max()) == 0.0, k
    assert not S["touched"], S["touched"]
    N, gmax = S["native"], S["dev"]["gmax"]
    wd = _net(SC.DDF_DIM)[0]
    dW1, db1 = torch.zeros(H, H, device=DEV), torch.zeros(H, device=DEV)
    hip.wgrad_native_batch([hip.wgrad_problem(N["dz1"], H // 32, N["a0"], H // 32, SCALE_M, dW1, db1, gmax[0:1], 8.0)], SCALE_M)
    dW0, db0 = ops.grad_weight(N["dz0"], E.to(DEV), SCALE_M, H, SC.DDF_DIM, wd[0], wd[1], a_native_nt=H // 32, b_native_nt=0, a_scale_max=gmax[1:2])
    torch.cuda.synchronize()
    for t in (dW1, db1, dW0, db0):
        assert float(t.abs().max()) == 0.0 and bool(torch.isfinite(t).all())


def test_tiny_uniform_gradient_keeps_the_relative_bars():
    """g_sdf at 1e-7, the size of a mean over ~1e5 rays: the same relative bars as at O(1)"""
    _, E, g = _case(SC.DDF_DIM, SCALE_M)
    _parity(f"scale 1e-7 M={SCALE_M}", SC.DDF_DIM, SCALE_M, E, g * 1e-7)


# ------------------------------------------------------------------------------------------------------------------ refusals
def _refused(call, *unchanged):
    from neusky_amd import hip
    before = [t.clone() for t in unchanged]
    with pytest.raises(hip.NeuSkyHipError):
        call()
    torch.cuda.synchronize()
    for t, b in zip(unchanged, before):
        assert _same_bits(t, b), "a refused call wrote to an output"


@pytest.mark.parametrize("in_dim,hidden", [(0, 256), (2, 256), (6, 256), (84, 256), (72, 128)])
def test_networks_past_a_limit_are_refused_not_launched(in_dim, hidden):
    from neusky_amd import hip
    assert not hip.sdf_supported(in_dim, hidden)
    M = 33
    W0 = torch.zeros(hidden, 96, device=DEV)[:, :in_dim]
    W1, b, w2, b2 = torch.zeros(hidden, hidden, device=DEV), torch.zeros(hidden, device=DEV), torch.zeros(hidden, device=DEV), torch.zeros(1, device=DEV)
    net = hip.sdf_net(W0, b, W1, b, w2, b2, SC.BETA)
    assert net.in_dim == in_dim and net.hidden == hidden
    stream = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    table = torch.zeros(hip.FILM_TABLE_FLOATS, device=DEV)
    E, g = torch.zeros(M, 96, device=DEV), torch.ones(M, device=DEV)
    nat = [torch.full((hip.film_rows(M), 256), SENTINEL, device=DEV) for _ in range(4)]
    sdf, dE, gmax = torch.full((M,), SENTINEL, device=DEV), torch.full((M, 96), SENTINEL, device=DEV), torch.zeros(2, device=DEV)
    for direction in (0, 1):
        _refused(lambda: hip.sdf_stream_layout(net, direction))
        _refused(lambda: hip.sdf_pack(net, stream, table, direction), stream, table)
    _refused(lambda: hip.sdf_chain_fwd(net, stream, table, E, M, nat[0], nat[1], sdf), sdf, nat[0], nat[1])
    _refused(lambda: hip.sdf_chain_bwd(net, stream, table, M, g, nat[0], nat[1], nat[2], nat[3], dE, None, None, gmax), dE, nat[2], nat[3], gmax)


def test_layouts_outside_the_abi_are_refused_not_launched():
    """ldE < in_dim, ldE % 4 != 0, M = 0, an E / dE / save pointer off 16-byte alignment"""
    from neusky_amd import hip
    in_dim, M = SC.DDF_DIM, 33
    ws, desc, ((s0, t0), (s1, t1)) = _net(in_dim)
    Mp = hip.film_rows(M)
    flat = lambda n: torch.full((n + 4,), SENTINEL, device=DEV)  # noqa: E731
    nat = [torch.full((Mp, H), SENTINEL, device=DEV) for _ in range(4)]
    off = [flat(Mp * H)[1:1 + Mp * H].view(Mp, H) for _ in range(4)]  # 4 bytes off
    E = torch.zeros(M, in_dim, device=DEV)
    g = torch.ones(M, device=DEV)
    sdf, dE, gmax = torch.full((M,), SENTINEL, device=DEV), torch.full((M, in_dim), SENTINEL, device=DEV), torch.zeros(2, device=DEV)
    outs = (sdf, dE, gmax, *nat)
    fwd = lambda E_, M_=M, a0=nat[0], a1=nat[1]: hip.sdf_chain_fwd(desc, s0, t0, E_, M_, a0, a1, sdf)  # noqa: E731
    bwd = lambda dE_, M_=M, a0=nat[0], a1=nat[1], d1=nat[2], d0=nat[3]: hip.sdf_chain_bwd(desc, s1, t1, M_, g, a0, a1, d1, d0, dE_, None, None, gmax)  # noqa: E731
    narrow = torch.zeros(M, in_dim - 4, device=DEV)
    odd = torch.zeros(M, in_dim + 2, device=DEV)[:, :in_dim]
    E_off = flat(M * in_dim)[1:1 + M * in_dim].view(M, in_dim)
    for bad_E in (narrow, odd, E_off):
        _refused(lambda: fwd(bad_E), *outs)
    _refused(lambda: fwd(E, 0), *outs)
    _refused(lambda: fwd(E, M, off[0]), *outs)
    _refused(lambda: fwd(E, M, nat[0], off[1]), *outs)
    dE_narrow = torch.full((M, in_dim - 4), SENTINEL, device=DEV)
    dE_odd = torch.full((M, in_dim + 2), SENTINEL, device=DEV)
    dE_off = flat(M * in_dim)[1:1 + M * in_dim].view(M, in_dim)
    for bad_dE in (dE_narrow, dE_odd[:, :in_dim], dE_off):
        _refused(lambda: bwd(bad_dE), *outs, dE_narrow, dE_odd, dE_off)
    _refused(lambda: bwd(dE, 0), *outs)
    for i in range(4):
        args = list(nat)
        args[i] = off[i]
        _refused(lambda: bwd(dE, M, *args), *outs)


# ------------------------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("wide", [False, True], ids=["ldE=in_dim", "ldE=in_dim+8"])
@pytest.mark.parametrize("M", [129, 257])
def test_sdf_value_apply_end_to_end(M, wide):
    """ops.sdf_value_apply(train_weights=True): dE and all six parameter gradients -- dW1 / db1 from the streaming weight-gradient kernel,
    dW0 / db0 from the split-fp16 GEMM, the sdf row of dW2 / db2 from the chain kernel -- against float64.  A gradient's bar is its group's
    plus its kernel's own allowance: 1e-6 |dZ|^T |X| (test_gpu_wgrad_native.py), 2e-6 of the largest entry (test_gpu_gemm.py
    test_f16_scaled_split_range_and_accuracy), 1e-6 sum |g a1|.  wide: E is a view of a wider buffer; autograd must get E's shape"""
    from neusky_amd import ops
    in_dim, GF = SC.DDF_DIM, 256
    ws, E, g = _case(in_dim, M)
    W0, b0, W1, b1, w2, b2 = _net(in_dim)[0]
    gen = torch.Generator().manual_seed(M)
    W2 = torch.randn(GF + 4, H, generator=gen).to(DEV) / H ** 0.5
    B2 = torch.rand(GF + 4, generator=gen).to(DEV)
    W2[GF], B2[GF] = w2, b2[0]
    wd = [t.clone().requires_grad_(True) for t in (W0, b0, W1, b1, W2, B2)]
    Ebuf = torch.full((M, in_dim + (PAD if wide else 0)), float("nan"), device=DEV)
    Ebuf[:, :in_dim] = E.to(DEV)
    Eg = Ebuf[:, :in_dim].requires_grad_(True)
    ops.begin_step(DEV)
    assert ops.sdf_fused_ok(Eg, wd[0])
    sdf = ops.sdf_value_apply(Eg, *wd, SC.BETA, True)
    grads = torch.autograd.grad(sdf, [Eg] + wd, g.to(DEV))
    torch.cuda.synchronize()
    S = _run_kernels(in_dim, M, E, g)
    assert _same_bits(S["sdf"], sdf.detach().cpu())
    dE, dW0, db0, dW1, db1, dW2, db2 = (t.detach().cpu().double() for t in grads)
    assert dE.shape == (M, in_dim) and bool(torch.isfinite(dE).all())
    sdf_row = torch.arange(GF + 4) == GF
    assert float(dW2[~sdf_row].abs().max()) == 0.0 and float(db2[~sdf_row].abs().max()) == 0.0
    ref, bar = SC.reference_and_bars(ws, E, g)
    g64 = SC.groups(ref)
    top = lambda k: bar[k] * float(g64[k].abs().max())  # noqa: E731
    a = lambda k: ref[k].abs()  # noqa: E731
    checks = [("dE", dE, 0.0), ("grad:dW1", dW1, 1e-6 * a("dz1").t() @ a("a0")), ("grad:db1", db1, 1e-6 * a("dz1").sum(0)),
              ("grad:dW0", dW0, 2e-6 * float(g64["grad:dW0"].abs().max())), ("grad:db0", db0, 2e-6 * float(g64["grad:db0"].abs().max())),
              ("dw2", dW2[GF], SC.SUM_ALLOWANCE * ref["sum_abs"]["dw2"]), ("db2", db2[GF:GF + 1], SC.SUM_ALLOWANCE * ref["sum_abs"]["db2"])]
    ratio = {k: float(((got - g64[k]).abs() / (top(k) + extra)).max()) for k, got, extra in checks}
    worst = max(ratio, key=ratio.get)
    print(f"end to end M={M} wide={wide}: worst err/bar {ratio[worst]:.3f} ({worst})")
    print("    " + " ".join(f"{k}={v:.2f}" for k, v in ratio.items()))
    missed = {k: round(v, 3) for k, v in ratio.items() if not v <= 1.0}
    assert not missed, f"groups over their bar (err / bar): {missed}"
