"""The DDF query rows on the GPU against float64: visibility_rays_kernel (csrc/render.hip), ddf_fit_rows_fwd/bwd_kernel
(csrc/samplers.hip), visibility_finish_fwd/bwd and the two autograd nodes ops.DDFQueryRowsFn / ops.DDFFitRowsFn, on the cases of
ddf_rows_cases.py (whose fitness test_ddf_rows_cases_cpu.py proves), the reference's own recorded outputs (G6) and the statistics
of the multi-view points the forward kernel draws.

No bar is fixed in advance and none comes from the code under test.  For each compared array
    bar = 4 x max |restatement in float32 on the CPU - restatement in float64|, at least 4 * 2^-23 * max |reference|
on the same inputs (ddf_rows_cases.bar); a formula error (an axis, a frequency, a root, a sign, a missing factor) is O(0.1 .. 1) of the
values.  G6: the tolerance of test_g6_ddf_model_plumbing (rtol 2e-5, atol 2e-6) + 4 x the float32 - float64 distance of the oracle
for that output.  d_threshold, a sum by atomics: ddf_rows_cases.threshold_bar.  Every test prints the error and the bar of each
array; the figures of one run on an MI355X are listed at the end of this file's docstring.

Figures of one run on an MI355X (largest |kernel - float64| and bar, smallest .. largest over the cases; n = compared arrays):
    q_pos[fit], q_pos[mv]   n 15  error 0 (copies)           bar 3.6e-07 .. 1.2e-06
    xrow[fit]               n 10  error 1.9e-06 .. 1.1e-05   bar 7.6e-06 .. 4.0e-05   worst error / bar 0.34
    xrow[mv]                n  5  error 1.5e-06 .. 4.8e-06   bar 5.7e-06 .. 2.2e-05   worst error / bar 0.26
    q_pos[sky]              n  7  error 2.1e-08 .. 3.7e-07   bar 3.6e-07 .. 1.7e-06   worst error / bar 0.22
    xrow[sky]               n  7  error 1.1e-06 .. 1.4e-05   bar 2.6e-06 .. 5.5e-05   worst error / bar 0.95 (Ns = 1: one row)
    sky_gt                  n  7  error 3.0e-08 .. 5.0e-07   bar 3.3e-07 .. 2.5e-06   worst error / bar 0.28
    dist_weight (6 modes)   n 22  error 4.4e-09 .. 3.6e-07   bar 2.7e-07 .. 1.5e-06   worst error / bar 0.30
    G6, five outputs        n  5  error 1.8e-07 .. 8.0e-07   bar 2.6e-06 .. 4.1e-05   worst error / bar 0.07
    bwd d_t                 n  6  error 6.8e-08 .. 6.5e-06   bar 5.5e-06 .. 1.7e-03   worst error / bar 0.09
    bwd d_t, one group      n 18  error 1.3e-10 .. 1.7e-06   bar 4.0e-08 .. 6.6e-04   worst error / bar 0.10
    nodes' t.grad           n  2  error 5.3e-07 .. 7.7e-07   bar 1.4e-04 .. 1.7e-04   worst error / bar 0.01
    sphere_points           n  8  error 8.4e-08 .. 6.8e-07   bar 3.5e-07 .. 2.7e-06   worst error / bar 0.32
    termination / surf_dist n 16  error 9.3e-08 .. 9.0e-07   bar 4.8e-07 .. 3.6e-06   worst error / bar 0.29
    visibility xrow         n 16  error 2.0e-06 .. 1.9e-05   bar 1.1e-05 .. 8.2e-05   worst error / bar 0.43
    vis                     n  8  error 2.2e-08 .. 2.1e-07   bar 1.3e-07 .. 8.4e-07   worst error / bar 0.25
    d_t_hat                 n  8  error 1.3e-09 .. 4.2e-07   bar 3.8e-08 .. 2.1e-05   worst error / bar 0.09
    d_threshold             n  8  error 1.3e-09 .. 3.4e-06   bar 3.8e-08 .. 5.8e-04   worst error / bar 0.08
    drawn (x, y) vs Philox  n  2  error 3.9e-07 .. 4.0e-07   bar 1.6e-06              z bit for bit
    drawn points, n = 262 144: mean z 0.49979 (0.5 +- 0.00338), var z 0.083349 (1/12 +- 0.00087), mean cos / sin theta 0.0008 / -0.0014
    (+- 0.0083), largest deviation of a histogram cell 125 (+- 270), corr z call k / k + 1 0.0008, row j / j + 1 -0.0008 (+- 0.0117)

The two backward kernels (ddf_fit_rows_bwd, visibility_finish_bwd) do their arithmetic in double since these tests were written.  In
float they were as accurate as the float32 restatement (row by row at N = 1312: median error 5.1e-06 against 5.8e-06), which is not
enough where ONE number is compared (N = 1: `4 x max |float32 - float64|` is then four times a single draw of float32 noise, and
d_t missed 1.31e-05 by 1.48e-05, the sin1 group 1.54e-06 by 1.69e-06), nor for d_threshold, whose bar allows for the order of a float32
sum of exact terms but not for the float32 rounding of the terms (3.9e-06 .. 4.4e-06 against 3.85e-06 at (5, 51, 2.5), scale 25).
"""
import os

import numpy as np
import pytest
import torch

import ddf_rows_cases as DC
import inputs as gi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64  # rows behind every output, prefilled with NaN: the kernels must leave them alone
NAN = float("nan")
BIG = 1e30  # what column 15 and the columns beyond it of a row gradient hold: they must not reach the result
T = torch.from_numpy


def _ids(cases):
    return ["-".join(str(v) for v in c) for c in cases]


def _names(groups):
    return [name for name, _ in groups]


class Ledger:
    """prints the error and the bar of every compared array, then fails for all that missed theirs"""

    def __init__(self, what):
        self.what, self.missed = what, []

    def check(self, name, got, ref64, ref32=None, bar=None):
        bar = DC.bar(ref32, ref64) if bar is None else bar
        err = DC.max_err(got.cpu(), ref64)
        print(f"{self.what} {name}: error {err:.2e}, bar {bar:.2e}")
        if not err <= bar:
            self.missed.append((name, err, bar))

    def done(self):
        assert not self.missed, (self.what, self.missed)


def _guarded(n, *tail):
    return torch.full((n + GUARD,) + tail, NAN, device=DEV)


def _same_bits(a, b):
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _dev(t):
    return None if t is None else t.to(DEV).contiguous()


def _run_fit(inp, radius, want_mv, ldx, *, mv_given=True, seed=0, counter=None, exp=3.0, include_z=False, want_weight=True,
             want_sky=True):
    """hip.ddf_fit_rows_fwd on views [:E] of guarded buffers -> the outputs on the CPU (None for an absent one)"""
    from neusky_amd import hip
    N = inp["positions"].shape[0]
    Ns = inp["sky_o"].shape[0] if want_sky else 0
    E = DC.fit_launch_rows(N, Ns, want_mv)
    q, x = _guarded(E, 3), _guarded(E, ldx)
    mvo = _guarded(N, 3) if want_mv else None
    sg = _guarded(Ns) if Ns else None
    w = _guarded(N) if want_weight else None
    hip.ddf_fit_rows_fwd(_dev(inp["positions"]), _dev(inp["directions"]), _dev(inp["t"]), _dev(inp["mv"]) if mv_given else None, seed,
                         counter, _dev(inp["sky_o"]) if Ns else None, _dev(inp["sky_d"]) if Ns else None, radius, want_mv, exp, include_z,
                         q[:E], x[:E], None if mvo is None else mvo[:N], None if sg is None else sg[:Ns], None if w is None else w[:N])
    torch.cuda.synchronize()
    for buf, n in ((q, E), (x, E), (mvo, N), (sg, Ns), (w, N)):
        if buf is not None:
            assert torch.isnan(buf[n:]).all(), "a guard row was written"
            assert torch.isfinite(buf[:n]).all()
    cpu = lambda b, n: None if b is None else b[:n].cpu()  # noqa: E731
    return dict(q_pos=cpu(q, E), xrow=cpu(x, E), mv_out=cpu(mvo, N), sky_gt=cpu(sg, Ns), dist_weight=cpu(w, N), N=N, Ns=Ns, E=E)


def _sections(out, want_mv):
    N, Ns = out["N"], out["Ns"]
    s = {"fit": slice(0, N)}
    if want_mv:
        s["mv"] = slice(N, 2 * N)
    s["sky"] = slice(out["E"] - Ns, out["E"])
    return s


# ---- forward -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", DC.FIT_CASES, ids=_ids(DC.FIT_CASES))
def test_fit_rows_forward_against_float64(case):
    N, Ns, want_mv, radius, ldx = case
    inp, ref, ref32 = DC.fit_case(N, Ns, radius)
    out = _run_fit(inp, radius, want_mv, ldx)
    assert out["xrow"].shape == (DC.fit_launch_rows(N, Ns, want_mv), ldx)
    led = Ledger(case)
    for s, rows in _sections(out, want_mv).items():
        led.check(f"q_pos[{s}]", out["q_pos"][rows], ref["pos_" + s], ref32["pos_" + s])
        led.check(f"xrow[{s}]", out["xrow"][rows, :15], ref["rows_" + s], ref32["rows_" + s])
    led.check("sky_gt", out["sky_gt"] if Ns else torch.zeros(0), ref["sky_gt"], ref32["sky_gt"])
    led.check("dist_weight", out["dist_weight"], ref["distance_weight"], ref32["distance_weight"])
    # exact facts
    assert _same_bits(out["q_pos"][:N], inp["positions"])
    assert (out["xrow"][:, 15:] == 0).all() and out["xrow"][:, 15:].shape[1] == ldx - 15
    if want_mv:
        assert _same_bits(out["mv_out"], DC.fold(inp["mv"])) and _same_bits(out["q_pos"][N:2 * N], out["mv_out"])
    else:
        assert out["mv_out"] is None
    led.done()


@pytest.mark.parametrize("include_z,exp", DC.WEIGHT_MODES)
def test_distance_weight_modes(include_z, exp):
    led = Ledger((include_z, exp))
    for N, radius in ((63, 1.0), (257, 2.5)):
        inp = DC.fit_inputs(N, 100, radius)
        out = _run_fit(inp, radius, False, 16, exp=exp, include_z=include_z, want_sky=False)
        led.check(f"dist_weight N {N} radius {radius}", out["dist_weight"],
                  DC.distance_weight(inp["positions"], radius, exp, include_z, torch.float64),
                  DC.distance_weight(inp["positions"], radius, exp, include_z, torch.float32))
    led.done()


def test_an_absent_section_shifts_the_others():
    """E = N + n_mv + Ns: without the multi-view rows the sky rows follow the fit rows; no output depends on which others are asked for"""
    N, Ns, radius = 63, 100, 2.5
    inp = DC.fit_inputs(N, Ns, radius)
    full = _run_fit(inp, radius, True, 16)
    assert full["E"] == 2 * N + Ns
    rows = lambda o, a, b: (o["q_pos"][a:b], o["xrow"][a:b])  # noqa: E731
    same = lambda x, y: all(_same_bits(p, q) for p, q in zip(x, y))  # noqa: E731
    no_w = _run_fit(inp, radius, True, 16, want_weight=False)
    assert no_w["dist_weight"] is None and no_w["E"] == full["E"]
    assert same(rows(no_w, 0, full["E"]), rows(full, 0, full["E"])) and _same_bits(no_w["sky_gt"], full["sky_gt"])
    no_sky = _run_fit(inp, radius, True, 16, want_sky=False)
    assert no_sky["sky_gt"] is None and no_sky["E"] == 2 * N and same(rows(no_sky, 0, 2 * N), rows(full, 0, 2 * N))
    assert _same_bits(no_sky["mv_out"], full["mv_out"]) and _same_bits(no_sky["dist_weight"], full["dist_weight"])
    no_mv = _run_fit(inp, radius, False, 16)
    assert no_mv["E"] == N + Ns and same(rows(no_mv, 0, N), rows(full, 0, N)) and same(rows(no_mv, N, N + Ns), rows(full, 2 * N, 2 * N + Ns))
    assert _same_bits(no_mv["sky_gt"], full["sky_gt"]) and _same_bits(no_mv["dist_weight"], full["dist_weight"])
    only_fit = _run_fit(inp, radius, False, 16, want_sky=False, want_weight=False)
    assert only_fit["E"] == N and same(rows(only_fit, 0, N), rows(full, 0, N))
    wide = _run_fit(inp, radius, True, 20)  # the leading dimension moves nothing but the padding
    assert _same_bits(wide["xrow"][:, :16].contiguous(), full["xrow"]) and (wide["xrow"][:, 15:] == 0).all()


def test_g6_rows_reproduce_the_reference_s_recorded_outputs():
    """the kernel's rows for G6's inputs, through G6's stand-in head in float64 on the CPU, give the outputs the REFERENCE recorded"""
    g = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "g6_ddf.npz")))
    rays = gi.sphere_rays(seed=6, M=40, radius=1.0)
    inp = dict(positions=T(rays["positions"]), directions=T(rays["directions"]), t=T(g["term"][:, 0].copy()), mv=T(g["mv_points"]),
               sky_o=T(g["sky_o"]), sky_d=T(g["sky_d"]))
    out = _run_fit(inp, 1.0, True, 16)
    t_all = DC.g6_head(g, torch.float64)(out["q_pos"].double(), out["xrow"][:, :15].double())
    got = {"expected_termination_dist": t_all[:40], "multi_view_expected_termination_dist": t_all[40:80],
           "sky_ray_expected_termination_dist": t_all[80:], "sky_ray_termination_dist": out["sky_gt"].double(),
           "distance_weight": out["dist_weight"].double()}
    o64, o32 = DC.g6_oracle(g, rays, torch.float64), DC.g6_oracle(g, rays, torch.float32)
    missed = []
    for k in DC.G6_OUTPUTS:
        rec = T(g["out_" + k]).double()
        assert got[k].shape == rec.shape
        bar = DC.G6_RTOL * rec.abs() + DC.G6_ATOL + 4.0 * DC.max_err(o32[k], o64[k])
        over = ((got[k] - rec).abs() - bar).max().item()
        print(f"G6 {k}: error {(got[k] - rec).abs().max().item():.2e}, bar {bar.min().item():.2e} .. {bar.max().item():.2e}")
        if over > 0:
            missed.append((k, over))
    assert not missed, missed


# ---- backward ----------------------------------------------------------------------------------------------------------------------
def _run_bwd(inp, d_rows, ldx):
    """hip.ddf_fit_rows_bwd with d_rows [N,15] in the first 15 of ldx columns and BIG (of both signs) in the others -> d_t [N] (CPU)"""
    from neusky_amd import hip
    N = inp["positions"].shape[0]
    d_xrow = torch.full((N, ldx), BIG)
    d_xrow[:, 16::2] = -BIG
    d_xrow[:, :15] = d_rows
    d_t = _guarded(N)
    hip.ddf_fit_rows_bwd(_dev(inp["positions"]), _dev(inp["directions"]), _dev(inp["t"]), _dev(DC.fold(inp["mv"])), _dev(d_xrow), d_t[:N])
    torch.cuda.synchronize()
    assert torch.isnan(d_t[N:]).all(), "a guard row was written"
    return d_t[:N].cpu()


@pytest.mark.parametrize("case", DC.BWD_CASES, ids=_ids(DC.BWD_CASES))
def test_fit_rows_backward_against_float64_autograd(case):
    N, radius, ldx = case
    inp, ref, ref32 = DC.fit_case(N, 100, radius)
    led = Ledger(case)
    led.check("d_t", _run_bwd(inp, inp["d_xrow"], ldx), ref["d_t"], ref32["d_t"])
    led.done()


GROUP_SHAPES = ((1, 2.5, 16), (257, 2.5, 20))  # (N, radius, ldx): one thread, and two workgroups with one row in the second


@pytest.mark.parametrize("shape", GROUP_SHAPES, ids=_ids(GROUP_SHAPES))
@pytest.mark.parametrize("group", DC.COLUMN_GROUPS, ids=_names(DC.COLUMN_GROUPS))
def test_fit_rows_backward_one_column_group_at_a_time(group, shape):
    """a gradient on the raw, the sin or the shifted-sin columns of ONE local axis: a wrong factor on one group cannot hide under the
    others"""
    (name, cols), (N, radius, ldx) = group, shape
    inp = DC.fit_inputs(N, 100, radius)
    probe = DC.group_probe(inp, cols)
    led = Ledger((name,) + shape)
    led.check("d_t", _run_bwd(inp, probe, ldx), DC.mv_t_gradient(inp, probe, torch.float64), DC.mv_t_gradient(inp, probe, torch.float32))
    led.done()


# ---- visibility rows ---------------------------------------------------------------------------------------------------------------
PREFILL = -7.0  # what vis holds before visibility_finish_fwd: entries outside sel_index keep it


def _run_vis_rays(inp, radius, ldx=16):
    from neusky_amd import hip
    R, Dv = inp["origins"].shape[0], inp["sel_index"].numel()
    M = R * Dv
    sp, xrow, sd, td = _guarded(M, 3), _guarded(M, ldx), _guarded(M), _guarded(M)
    hip.visibility_rays(_dev(inp["origins"]), _dev(inp["ray_dirs"]), _dev(inp["depth"]), _dev(inp["dirs"][inp["sel_index"]]), radius,
                        sp[:M], xrow[:M], sd[:M], td[:M])
    torch.cuda.synchronize()
    for buf in (sp, xrow, sd, td):
        assert torch.isnan(buf[M:]).all(), "a guard row was written"
    return dict(sphere_points=sp[:M].cpu(), xrow=xrow[:M].cpu(), surf_dist=sd[:M].cpu(), termination_dist=td[:M].cpu())


def _run_finish(inp, fin):
    """visibility_finish_fwd / bwd on fin's inputs -> vis [R,D] (prefilled with PREFILL), d_t_hat [M], d_threshold (CPU)"""
    from neusky_amd import hip
    R, Dv, D = inp["origins"].shape[0], inp["sel_index"].numel(), inp["dirs"].shape[0]
    M = R * Dv
    t_hat, sdist = _dev(fin["t_hat"]), _dev(fin["surf_dist"])
    thr, sel32 = torch.tensor([inp["threshold"]], device=DEV), _dev(inp["sel_index"].to(torch.int32))
    vis = torch.full((R + 1, D), PREFILL, device=DEV)
    vis[R:] = NAN
    hip.visibility_finish_fwd(t_hat, sdist, thr, inp["scale"], sel32, R, Dv, D, vis[:R])
    d_t, d_thr = _guarded(M), torch.zeros(1, device=DEV)
    hip.visibility_finish_bwd(t_hat, sdist, thr, inp["scale"], sel32, R, Dv, D, _dev(inp["d_vis"]), d_t[:M], d_thr)
    torch.cuda.synchronize()
    assert torch.isnan(vis[R:]).all() and torch.isnan(d_t[M:]).all(), "a guard row was written"
    return vis[:R].cpu(), d_t[:M].cpu(), d_thr[0].cpu()


@pytest.mark.parametrize("case", DC.vis_cases(), ids=_ids(DC.vis_cases()))
def test_visibility_rows_and_finish_against_float64(case):
    R, Dv, radius = case
    inp, ref, ref32, fin = DC.vis_case(*case)
    M, D, sel = R * Dv, inp["dirs"].shape[0], inp["sel_index"]
    ldx = 20 if (R, Dv) == (37, 7) else 16
    out = _run_vis_rays(inp, radius, ldx)
    led = Ledger(case)
    for k in ("sphere_points", "termination_dist", "surf_dist"):
        led.check(k, out[k], ref[k], ref32[k])
    led.check("xrow", out["xrow"][:, :15], ref["rows"], ref32["rows"])
    led.check("xrow of the ray that ends ON the sphere", out["xrow"][:Dv, :15], ref["rows"][:Dv], ref32["rows"][:Dv])
    assert (out["xrow"][:, 15:] == 0).all() and (out["surf_dist"] <= 2 * radius).all()
    # finish, on inputs of its own (float32 roundings of the reference's read-out and surf_dist)
    r64, r32 = fin["ref"], fin["ref32"]
    vis, d_t, _ = _run_finish(inp, fin)
    rest = torch.ones(D, dtype=torch.bool)
    rest[sel] = False
    assert (vis[:, rest] == PREFILL).all()
    led.check("vis", vis[:, sel], r64["vis"], r32["vis"])
    led.check("d_t_hat", d_t, r64["d_t_hat"], r32["d_t_hat"])
    led.done()


@pytest.mark.parametrize("case", DC.vis_cases(), ids=_ids(DC.vis_cases()))
def test_visibility_finish_threshold_gradient(case):
    """d_threshold, a sum over R Dv rows by float32 atomics, against the float64 sum of the float64 per-row terms"""
    inp, _, _, fin = DC.vis_case(*case)
    _, _, d_thr = _run_finish(inp, fin)
    led = Ledger(case)
    led.check("d_threshold", d_thr, fin["ref"]["d_threshold"], bar=DC.threshold_bar(fin["ref"]["d_threshold_terms"]))
    led.done()


# ---- the two autograd nodes --------------------------------------------------------------------------------------------------------
def _prep(inp, want_mv=True, mv_given=True, counter=None, t=None):
    """as DDFModel.prepare_queries builds it"""
    return {"positions": _dev(inp["positions"]), "directions": _dev(inp["directions"]),
            "term_dist": _dev(inp["t"][:, None]) if t is None else t, "want_mv": want_mv,
            "mv_points_in": _dev(inp["mv"]) if mv_given else None, "seed": 4321, "counter": counter, "sky_o": _dev(inp["sky_o"]),
            "sky_d": _dev(inp["sky_d"]), "want_weight": True, "weight_exp": 2.5, "weight_include_z": True}


def _vis_args(vin):
    return (_dev(vin["origins"]), _dev(vin["ray_dirs"]), _dev(vin["depth"]), _dev(vin["dirs"][vin["sel_index"]]))


def test_nodes_forward_is_the_kernels_bit_for_bit():
    from neusky_amd import hip, ops
    (N, Ns, radius), vin = DC.NODE_FIT, DC.vis_inputs(*DC.NODE_VIS)
    inp = DC.fit_inputs(N, Ns, radius)
    M = vin["origins"].shape[0] * vin["sel_index"].numel()
    E = 2 * N + Ns
    for mv_given in (True, False):
        counter = None if mv_given else torch.zeros(1, dtype=torch.int64, device=DEV)
        prep = _prep(inp, mv_given=mv_given, counter=counter)
        # the raw kernel on the same prep
        q, x, mvo, sg, w = (torch.empty(E, 3, device=DEV), torch.empty(E, 16, device=DEV), torch.empty(N, 3, device=DEV),
                            torch.empty(Ns, device=DEV), torch.empty(N, device=DEV))
        hip.ddf_fit_rows_fwd(prep["positions"], prep["directions"], prep["term_dist"].reshape(-1), prep["mv_points_in"], prep["seed"],
                             counter, prep["sky_o"], prep["sky_d"], radius, True, 2.5, True, q, x, mvo, sg, w)
        if counter is not None:
            assert int(counter) == 1
            counter.zero_()
        fit = ops.DDFFitRowsFn.apply(prep["term_dist"], radius, prep)
        assert len(fit) == 5 and all(_same_bits(a, b) for a, b in zip(fit, (q, x, mvo, sg, w)))
        if counter is not None:
            assert int(counter) == 1
            counter.zero_()
            assert not _same_bits(mvo, DC.fold(inp["mv"]))  # drawn, not handed in
        qry = ops.DDFQueryRowsFn.apply(prep["term_dist"], *_vis_args(vin), radius, prep)
        pts_all, xrow_all, surf, term, mv_points, sky_gt, dist_w = qry
        assert pts_all.shape == (M + E, 3) and xrow_all.shape == (M + E, 16)
        assert _same_bits(pts_all[M:], q) and _same_bits(xrow_all[M:], x)
        assert _same_bits(mv_points, mvo) and _same_bits(sky_gt, sg) and _same_bits(dist_w, w)
        sp, xr, sd, td = (torch.empty(M, 3, device=DEV), torch.empty(M, 16, device=DEV), torch.empty(M, device=DEV), torch.empty(M, device=DEV))
        hip.visibility_rays(*_vis_args(vin), radius, sp, xr, sd, td)
        assert _same_bits(pts_all[:M], sp) and _same_bits(xrow_all[:M], xr) and _same_bits(surf, sd) and _same_bits(term, td)
    # fit = None: the visibility rows alone, no fit outputs
    only = ops.DDFQueryRowsFn.apply(None, *_vis_args(vin), radius, None)
    assert only[0].shape == (M, 3) and _same_bits(only[0], sp) and _same_bits(only[1], xr) and _same_bits(only[2], sd)
    assert _same_bits(only[3], td) and all(o.numel() == 0 for o in only[4:])
    assert not any(o.requires_grad for o in only)


def _node_t_grad(node, section, want_mv=True):
    """t.grad after a backward of the node's rows with a gradient on ONE section (BIG in column 15 there), and that gradient"""
    from neusky_amd import ops
    (N, Ns, radius), vin = DC.NODE_FIT, DC.vis_inputs(*DC.NODE_VIS)
    inp = DC.fit_inputs(N, Ns, radius)
    M = vin["origins"].shape[0] * vin["sel_index"].numel() if node == "query" else 0
    t = _dev(inp["t"][:, None]).requires_grad_(True)
    assert t.is_leaf and t.shape == (N, 1)
    prep = _prep(inp, want_mv=want_mv, t=t)
    if node == "query":
        xrow = ops.DDFQueryRowsFn.apply(t, *_vis_args(vin), radius, prep)[1]
    else:
        xrow = ops.DDFFitRowsFn.apply(t, radius, prep)[1]
    n_mv = N if want_mv else 0
    assert xrow.shape == (M + N + n_mv + Ns, 16)
    a, b = {"vis": (0, M), "fit": (M, M + N), "mv": (M + N, M + N + n_mv), "sky": (M + N + n_mv, M + N + n_mv + Ns)}[section]
    assert b > a
    probe = torch.randn(b - a, 16, generator=torch.Generator().manual_seed(a + b))
    probe[:, 15] = BIG
    g = torch.zeros(xrow.shape)
    g[a:b] = probe
    xrow.backward(g.to(DEV))
    torch.cuda.synchronize()
    return t.grad, probe[:, :15], inp


@pytest.mark.parametrize("node", ("fit", "query"))
def test_nodes_backward_reads_the_multi_view_rows_gradient_and_no_other(node):
    N = DC.NODE_FIT[0]
    for section in ("fit", "sky") + (("vis",) if node == "query" else ()):
        grad, _, _ = _node_t_grad(node, section)
        assert grad is not None and grad.shape == (N, 1) and (grad == 0).all(), (node, section)
    grad, probe, inp = _node_t_grad(node, "mv")
    assert grad.shape == (N, 1)
    led = Ledger(node)
    led.check("t.grad", grad[:, 0], DC.mv_t_gradient(inp, probe, torch.float64), DC.mv_t_gradient(inp, probe, torch.float32))
    led.done()
    for section in ("fit", "sky"):  # without the multi-view rows nothing reaches t
        grad, _, _ = _node_t_grad(node, section, want_mv=False)
        assert grad is None


# ---- the multi-view points the kernel draws ----------------------------------------------------------------------------------------
def test_drawn_multi_view_points_are_uniform_on_the_upper_hemisphere():
    from neusky_amd import hip
    N, calls, seed = DC.DRAW_N, DC.DRAW_CALLS, 1234
    inp = DC.fit_inputs(N, 0, 1.0)
    pos, dirs, t, mv = (_dev(inp[k]) for k in ("positions", "directions", "t", "mv"))
    q, x, mvo = torch.empty(2 * N, 3, device=DEV), torch.empty(2 * N, 16, device=DEV), torch.empty(N, 3, device=DEV)
    counter = torch.zeros(1, dtype=torch.int64, device=DEV)
    draws = torch.empty(calls, N, 3, device=DEV)
    for k in range(calls):
        hip.ddf_fit_rows_fwd(pos, dirs, t, None, seed, counter, None, None, 1.0, True, 3.0, False, q, x, mvo, None, None)
        draws[k] = mvo
    assert int(counter) == calls
    assert torch.isfinite(x).all() and _same_bits(q[N:], mvo)
    # a call that draws nothing leaves the counter alone
    hip.ddf_fit_rows_fwd(pos, dirs, t, mv, seed, counter, None, None, 1.0, True, 3.0, False, q, x, mvo, None, None)
    hip.ddf_fit_rows_fwd(pos, dirs, t, None, seed, counter, None, None, 1.0, False, 3.0, False, q[:N], x[:N], None, None, None)
    assert int(counter) == calls
    counter.zero_()
    hip.ddf_fit_rows_fwd(pos, dirs, t, None, seed, counter, None, None, 1.0, True, 3.0, False, q, x, mvo, None, None)
    assert int(counter) == 1 and _same_bits(mvo, draws[0])  # (seed, call number) fix the draw
    # its stream is not the sampler's: same seed, same call number, other points
    counter.zero_()
    so, sd = torch.empty(N, 3, device=DEV), torch.empty(N, 3, device=DEV)
    hip.ddf_vmf_samples(N, 1, 20.0, 1.0, 1, seed, counter, so, sd)
    assert int(counter) == 1
    shared = int((so == draws[0]).all(dim=1).sum())
    print(f"rows shared with the sampler's positions: {shared} of {N}")
    assert shared == 0
    # ... and it is the generator the kernel file documents: Philox4x32-10 at (row, stream id, call number) under the seed, u strictly
    # inside (0, 1), theta = 2 pi u0, cos(phi) = 2 u1 - 1, fold.  z has no rounding in it: bit for bit
    led = Ledger("draw")
    for call in (0, calls - 1):
        p64, p32 = DC.philox_mv_points(seed, call, N, torch.float64), DC.philox_mv_points(seed, call, N, torch.float32)
        assert _same_bits(draws[call, :, 2], p32[:, 2]), call
        led.check(f"(x, y) of call {call}", draws[call, :, :2], p64[:, :2], p32[:, :2])
    led.done()
    pts = draws.cpu().double()
    assert ((pts.norm(dim=-1) - 1).abs() <= 1e-6).all() and (pts[..., 2] >= 0).all()
    stats = DC.hemisphere_statistics(pts)
    for name, value, expected, bound in stats:
        print(f"{name}: {value:.6g}, expected {expected:.6g} +- {bound:.3g}")
    missed = [s for s in stats if not abs(s[1] - s[2]) <= s[3]]
    assert not missed, missed
