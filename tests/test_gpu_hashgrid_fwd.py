"""The hash-grid encode forward (encode_fwd_kernel: value rows only, with three tangent rows, with one directional row), the input
gradient of encode_bwd_kernel and the autograd node around them, against the float64 restatement of hashgrid_fwd_cpu.py -- per column
group (x, each PE frequency, each hash level), with the bar of each group taken from the reference alone (4 x its float32-vs-float64
distance over the case's pool, floored at 4 float32 roundings).  Cases: the SDF field's row under both contraction norms, the DDF's,
both proposal geometries (value rows only, no x: feat0 = 0), and grids of 1, 3 and 6 levels (waves of a workgroup that own no level; a
row without a pad column).  Every case runs on prefixes of its pool, edge points first, of 1, 63, 64, 65 and all points.

A (point, level) pair whose corner rows, as the kernel reports them, differ from the reference's is left out of that level's tangent,
directional and dx comparisons (never of the values: the interpolant is continuous across a face); their number is capped at 0 for
modes 0 and 2 and at 1e-4 of the pairs for mode 1.

Measured on an MI355X, worst error / bar over all prefixes and column groups (the run prints every group), and the excluded
(point, level) pairs against their cap:
    case        values   tangent rows   directional row   dx      excluded / cap
    sdf_linf    0.333    0.274          0.300             0.282   1 / 6
    sdf_l2      0.330    0.277          0.308             0.300   0 / 0
    ddf         0.250    -              -                 0.288   0 / 0
    prop64      0.277 (12 and 16 columns)                         0 / 2
    prop256     0.326                                             0 / 2
    small1      0.250                                             0 / 0
    small3      0.262    0.250          -                 -       0 / 1
    small6      0.330                                             0 / 0
Most groups sit at 0.25 exactly: the largest float32-vs-float64 distance of a group is the rounding of the float32 POSITION, scaled by
the level's resolution (or by the PE frequency), and the kernel starts from the same float32 position -- it repeats that error and
adds little of its own.  In particular the origin corner's smoothstep weight, formed as 1 - S(t) here and as S(1 - t) in the scatter
kernels, costs the forward and dx nothing that these bars see: no group of a smoothstep case stands out against the linear ones.
Scratch edits of the kernel (not kept), each run against this module: the dk term of the L-infinity Jacobian dropped -> tangent rows
(sdf_linf, small3), directional row and dx (sdf_linf) fail in every level group, 2e3 .. 3e4 x the bar; the PE exponent step max_exp / F
-> values, tangent rows, directional row and dx of both SDF cases fail in pe1 .. pe5 (and dx `all`), 9e2 .. 3e5 x; level 0's dw
x 1.02 -> tangent rows (sdf_linf, sdf_l2, small3), directional row (both) and dx (both, and ddf) fail in level0 alone, 1e2 .. 6e3 x.
"""
import functools

import pytest
import torch

import hashgrid_fwd_cpu as HF

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
M32 = 0xFFFFFFFF


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _table_dev(n_params):
    return HF.table32(n_params).to(DEV)


@functools.lru_cache(maxsize=None)
def _setup(name):
    from neusky_amd.encoding import HashGridGeometry
    case, cfg = HF.CASES[name], HF.CASES[name].cfg()
    geom = HashGridGeometry(n_levels=case.n_levels, log2_hashmap_size=case.log2T, max_res=case.max_res, smoothstep=case.smooth)
    assert geom.offsets == cfg.offsets and geom.resolutions == cfg.resolutions and geom.scales == cfg.scales
    ref = HF.reference(name)
    return case, geom, _table_dev(geom.n_params), ref, ref["x"].to(DEV)


@functools.lru_cache(maxsize=None)
def _kernel_cells_differ(name):
    """[N,L] bool: where the kernel's corner rows are not the reference's; asserts the cap"""
    from neusky_amd import hip
    case, geom, table, ref, x = _setup(name)
    idx = hip.hash_indices(geom, table, x, case.mode).cpu().to(torch.int64) & M32
    differ = HF.cell_disagreements(idx, ref["cell"][0])
    n, cap = int(differ[ref["values"]].sum()), HF.cell_cap(case, x.shape[0])
    print(f"{name}: {n} (point, level) pairs in another cell than the reference's; cap {cap}")
    assert n <= cap, (name, n, cap)
    return differ


def _value_rows(name, P, ld=None):
    """the value-only kernel on the first P points into a NaN-poisoned buffer with three guard rows -> Y [P, ld] (device)"""
    from neusky_amd import hip
    case, geom, table, ref, x = _setup(name)
    ld = ld or case.ldy
    buf = torch.full((P + 3, ld), NAN, device=DEV)
    hip.encode_fwd(geom, table, x[:P].contiguous(), case.mode, case.include_x, case.pe, case.pe_max_exp, buf[:P])
    torch.cuda.synchronize()
    assert torch.isnan(buf[P:]).all(), "rows past P were written"
    return buf[:P]


def _check_groups(name, quantity, got, want, bars, worst, differ=None, tag=None):
    """got / want [..., P, width] (a leading 3 for tangent rows): every column group inside its bar over the points that take part.
    worst[group] keeps the largest error / bar; worst['misses'] every (group, prefix, ratio) past its bar (_report asserts none)"""
    case, ref = HF.CASES[name], HF.reference(name)
    P = got.shape[-2]
    for g, cols in case.groups():
        keep = HF.point_mask(ref, quantity, g)[:P].clone()
        if differ is not None and g.startswith("level"):
            keep &= ~differ[:P, int(g[5:])]
        err = (got[..., keep, :][..., list(cols)].double() - want[..., :P, :][..., keep, :][..., list(cols)]).abs()
        ratio = err.max().item() / bars[g] if err.numel() else 0.0
        _tally(worst, g, tag or P, ratio)


def _tally(worst, g, tag, ratio):
    worst[g] = max(worst.get(g, 0.0), ratio)
    if not ratio <= 1.0:  # (a NaN is a miss)
        worst.setdefault("misses", []).append((g, tag, round(ratio, 2)))


def _report(name, what, worst):
    misses = worst.pop("misses", [])
    top = max(worst, key=worst.get)
    print(f"{name}: {what}: worst error / bar {worst[top]:.3f} ({top}); per group " + " ".join(f"{g}={r:.2f}" for g, r in worst.items()))
    assert not misses, (name, what, misses[:16])


def _finite_where_compared_for_less(name, got):
    """the points held to finiteness only (the L-infinity tie, the float32-overflow point): x and hash columns; PE columns of far
    points are compared for nothing"""
    case, ref = HF.CASES[name], HF.reference(name)
    P = got.shape[-2]
    pe_cols = [c for g, cols in case.groups() if g.startswith("pe") for c in cols]
    other = [c for c in range(case.width) if c not in pe_cols]
    assert torch.isfinite(got[..., other]).all()
    if pe_cols:
        assert torch.isfinite(got[..., ref["pe"][:P], :][..., pe_cols]).all()


# ---- value rows -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ld", list(zip(HF.CASES, [None] * len(HF.CASES))) + [("prop64", 16)])
def test_value_rows(name, ld):
    """encode_fwd_kernel<false>: what the DDF and both proposal networks call, and the rows the two tangent kernels must repeat bit for
    bit.  ld 16 (prop64): pad columns 10..15 exist"""
    case, geom, table, ref, x = _setup(name)
    _kernel_cells_differ(name)  # (the cap holds for every case; the values themselves leave no pair out)
    worst = {}
    for P in HF.prefix_sizes(name):
        Y = _value_rows(name, P, ld).cpu()
        assert Y.shape == (P, ld or case.ldy)
        assert (Y[:, case.width:] == 0).all(), "pad columns"
        if case.include_x:
            assert torch.equal(_bits(Y[:, :3]), _bits(ref["x"][:P])), "the x columns are a copy"
        _finite_where_compared_for_less(name, Y[:, :case.width])
        _check_groups(name, "value", Y[:, :case.width], ref["Y64"], HF.value_bars(name), worst)
    _report(name, "values", worst)


# ---- three tangent rows -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", HF.TANGENT_CASES)
def test_tangent_rows(name):
    from neusky_amd import hip
    case, geom, table, ref, x = _setup(name)
    differ = _kernel_cells_differ(name)
    ld, W = case.ldy, case.width
    worst = {}
    for P in HF.prefix_sizes(name):
        Y = torch.full((P, ld), NAN, device=DEV)
        flat = torch.full((3 * P * ld + ld,), NAN, device=DEV)
        T = flat[:3 * P * ld].view(3, P, ld)
        hip.encode_fwd(geom, table, x[:P].contiguous(), case.mode, case.include_x, case.pe, case.pe_max_exp, Y, T)
        torch.cuda.synchronize()
        assert torch.isnan(flat[3 * P * ld:]).all(), "the tangent rows ran past their block"
        assert torch.equal(_bits(Y), _bits(_value_rows(name, P))), "value rows differ from the value-only kernel's"
        T = T.cpu()
        assert (T[:, :, W:] == 0).all(), "pad columns of the tangent blocks"
        _finite_where_compared_for_less(name, T[:, :, :W])
        if case.include_x:
            assert torch.equal(T[:, :, :3], torch.eye(3)[:, None, :].expand(3, P, 3)), "the identity tangent"
        _check_groups(name, "tangent", T[:, :, :W], ref["T64"], HF.tangent_bars(name), worst, differ)
    _report(name, "tangent rows", worst)


# ---- the directional row ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", HF.DIR_CASES)
def test_directional_row(name):
    """against sum_k d_k T_k of the FLOAT64 reference (not of the three-row kernel: an error the two kernels share would pass)"""
    from neusky_amd import hip
    case, geom, table, ref, x = _setup(name)
    differ = _kernel_cells_differ(name)
    N, ld, W = x.shape[0], case.ldy, case.width
    worst = {}
    for P, spr in [(1, 1), (63, 1), (64, 1), (64, 32), (65, 1), (65, 13), (N, 1), (N // 32 * 32, 32)]:
        dirs = ref["dirs"][:P // spr].contiguous()
        both = torch.full((2 * P + 1, ld), NAN, device=DEV)
        hip.encode_fwd_dir(geom, table, x[:P].contiguous(), case.mode, case.include_x, case.pe, case.pe_max_exp, dirs.to(DEV), both[:P], both[P:2 * P])
        torch.cuda.synchronize()
        assert torch.isnan(both[2 * P:]).all()
        assert torch.equal(_bits(both[:P]), _bits(_value_rows(name, P))), "value rows differ from the value-only kernel's"
        Td = both[P:2 * P].cpu()
        assert (Td[:, W:] == 0).all()
        _finite_where_compared_for_less(name, Td[:, :W])
        _check_groups(name, "tangent", Td[:, :W], HF.directional_reference(name, spr)[0], HF.directional_bars(name, spr), worst, differ,
                      tag=(P, spr))
    _report(name, "directional row", worst)


# ---- the input gradient -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", HF.DX_CASES)
def test_input_gradient(name):
    """encode_bwd's dx under a row gradient in one column group at a time, then in all: without a table gradient, with one, and with
    a tangent-row gradient beside it (dx is first order by design: unchanged, bit for bit)"""
    from neusky_amd import hip
    case, geom, table, ref, x = _setup(name)
    differ = _kernel_cells_differ(name)
    N, ld = x.shape[0], case.ldy
    dtable = torch.zeros(geom.n_params, 2, device=DEV)
    g32 = torch.Generator().manual_seed(case.seed + 2000)
    dT_all = torch.randn(3, N, ld, generator=g32)
    worst = {}
    for P in HF.prefix_sizes(name):
        xp = x[:P].contiguous()
        dT = dT_all[:, :P].contiguous().to(DEV)
        for g, _ in HF.dx_groups(name):
            dY = HF.group_probe(ref, case, g)[:P].contiguous().to(DEV)
            outs = []
            for dtab, dt in ((None, None), (dtable, None), (dtable, dT)):
                dx = torch.full((P + 1, 3), NAN, device=DEV)
                hip.encode_bwd(geom, table, xp, case.mode, case.include_x, case.pe, case.pe_max_exp, dY, dt, dtab, dx[:P])
                torch.cuda.synchronize()
                assert torch.isnan(dx[P:]).all()
                outs.append(dx[:P].cpu())
            assert torch.equal(_bits(outs[1]), _bits(outs[0])) and torch.equal(_bits(outs[2]), _bits(outs[0])), (g, P)
            dx64, bar = HF.dx_bar(name, g)
            keep = HF.dx_point_mask(ref, g)[:P].clone()
            if g.startswith("level"):
                keep &= ~differ[:P, int(g[5:])]
            elif g == "all":
                keep &= ~differ[:P].any(-1)
            assert torch.isfinite(outs[0][ref["pe_finite"][:P]]).all()
            ratio = ((outs[0].double() - dx64[:P]).abs() / bar[:P])[keep]
            _tally(worst, g, P, ratio.max().item() if ratio.numel() else 0.0)
    _report(name, "dx", worst)


# ---- the autograd node ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tangents,directional", [("prop64", False, False), ("prop256", False, False), ("ddf", False, False),
                                                        ("sdf_linf", False, False), ("sdf_linf", True, False), ("sdf_linf", True, True),
                                                        ("sdf_l2", True, False), ("sdf_l2", True, True)])
def test_autograd_node_is_the_kernel_call(name, tangents, directional):
    """ops.HashEncodeFn.apply as ray_samplers.py (proposal), directional_distance_field.py (DDF) and sdf_albedo_field.py (field)
    call it: [P | 4P | 2P, pad4(width)] rows, bit-equal to the direct kernel calls"""
    from neusky_amd import hip, ops
    case, geom, table, ref, x = _setup(name)
    N, ld = x.shape[0], case.ldy
    for P in (65, N // 32 * 32):
        xp = x[:P].contiguous()
        args = (xp, table, geom, case.mode, case.include_x, case.pe, case.pe_max_exp)
        if directional:
            dirs = ref["dirs"][:P // 32 if P % 32 == 0 else P].contiguous().to(DEV)
            out = ops.HashEncodeFn.apply(*args, True, False, dirs)
            want = torch.full((2 * P, ld), NAN, device=DEV)
            hip.encode_fwd_dir(geom, table, xp, case.mode, case.include_x, case.pe, case.pe_max_exp, dirs, want[:P], want[P:])
        elif tangents:
            out = ops.HashEncodeFn.apply(*args, True, True)
            want = torch.full((4 * P, ld), NAN, device=DEV)
            hip.encode_fwd(geom, table, xp, case.mode, case.include_x, case.pe, case.pe_max_exp, want[:P], want[P:].view(3, P, ld))
        else:
            out = ops.HashEncodeFn.apply(*args, False, False)
            want = _value_rows(name, P)
        torch.cuda.synchronize()
        assert out.shape == ((2 * P if directional else 4 * P if tangents else P), (case.width + 3) // 4 * 4)
        assert torch.equal(_bits(out), _bits(want))


# ---- the cell choice --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("name", list(HF.CASES))
def test_indices_bit_exact_on_every_geometry(name, mode):
    """hip.hash_indices against O.hash_grid_indices of the float32 position, on every geometry and pool, edge points included.  (Mode
    0 feeds x itself to the grid: the far points of a contracted case's pool, whose scale * x leaves the int32 range, are left out.)"""
    from neusky_amd import hip
    case, geom, table, ref, x = _setup(name)
    keep = ref["pe"] if mode == 0 else torch.ones_like(ref["pe"])
    xs = ref["x"][keep].contiguous()
    idx = hip.hash_indices(geom, table, xs.to(DEV), mode).cpu().to(torch.int64) & M32
    want, _ = HF.O.hash_grid_indices(HF.position32(xs, mode), case.cfg())
    differ = HF.cell_disagreements(idx, want)
    assert int(differ.sum()) == 0, (int(differ.sum()), torch.nonzero(differ.any(-1)).flatten().tolist()[:8])
