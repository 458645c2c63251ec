"""The cases and bars of hashgrid_fwd_cpu.py are fit to test the encode kernels with: every case has the points and the geometry it
is meant to have, the written-out restatement agrees with the oracle's forward and with its double-backward jvp (two independent
derivations), the reference alone stays inside the cell cap, and a defect injected into the restatement breaks the bar of the column
group it touches at least tenfold and no other."""
import functools

import numpy as np
import pytest
import torch

import hashgrid_bwd_cpu as HB
import hashgrid_fwd_cpu as HF
from oracle import neusky_oracle as O

ALL = tuple(HF.CASES)


@pytest.mark.parametrize("name", ALL)
def test_widths_and_geometry(name):
    case, cfg = HF.CASES[name], HF.CASES[name].cfg()
    want = dict(sdf_linf=(71, 72), sdf_l2=(71, 72), ddf=(35, 36), prop64=(10, 12), prop256=(10, 12), small1=(2, 4), small3=(6, 8),
                small6=(12, 12))[name]
    assert (case.width, case.ldy) == want
    sizes = [cfg.offsets[l + 1] - cfg.offsets[l] for l in range(cfg.n_levels)]
    dense = [r ** 3 <= s for r, s in zip(cfg.resolutions, sizes)]
    assert all(s <= 1 << case.log2T for s in sizes)
    if name in HF.GEOMETRY:
        assert (cfg.resolutions, dense) == HF.GEOMETRY[name]
    elif case.n_levels == 16:
        assert cfg.resolutions[0] == 16 and cfg.resolutions[-1] == 2048 and sizes[-1] == 1 << 19
        assert dense == [True] * 5 + [False] * 11 and cfg.resolutions[4] ** 3 <= 1 << 19 < cfg.resolutions[5] ** 3
    elif name == "small1":
        assert cfg.resolutions == [16] and dense == [True]
    elif name == "small3":
        assert cfg.resolutions == [16, 32, 64] and dense == [True, False, False] and sizes[1:] == [1 << 12] * 2
    else:
        assert cfg.n_levels == 6 and cfg.resolutions[-1] == 128 and dense[0] and not dense[-1]
    # the column groups tile the row
    cols = sorted(c for _, g in case.groups() for c in g)
    assert cols == list(range(case.width))


@pytest.mark.parametrize("name", ALL)
def test_points_are_what_the_case_says(name):
    case, pl = HF.CASES[name], HF.pool(name)
    x, names, ne = pl["x"], pl["names"], pl["n_edges"]
    assert x.dtype == torch.float32 and x.shape == (ne + HF.POOL, 3) and torch.isfinite(x).all()
    at = lambda n: x[names.index(n)].double()  # noqa: E731
    if case.mode == 0:
        assert torch.equal(at("plus_one"), torch.ones(3, dtype=torch.float64)) and torch.equal(at("minus_one"), -torch.ones(3, dtype=torch.float64))
        assert torch.equal(at("origin"), torch.zeros(3, dtype=torch.float64))
        lat = x[[i for i, n in enumerate(names) if n.startswith("lattice")]].double() * HB.LATTICE
        assert lat.shape[0] == 64 and torch.equal(lat, lat.round())
        if case.points == "sphere":
            assert ((x[ne:].double().norm(dim=-1) - 1).abs() < 1e-6).all()
        q = x[[names.index(f"face{j}") for j in (0, 4, 9)]].double() * 15.0 + 0.5
        assert ((q - q.round()).abs() < 2e-6).all()
        return
    m = HF.norm_of(x, case.mode)
    assert (m[ne:] < 1).sum() > 100 and (m[ne:] > 1).sum() > 100  # both sides of the contraction surface, in the seeded pool ...
    assert (m[:ne] < 1).any() and (m[:ne] > 1).any() and (m[:63] > 1).sum() > 5  # ... and in every prefix past the edge points
    assert m[names.index("surface")] == 1.0
    _, J = HB.grid_position(x[names.index("surface")][None], case.mode)
    assert torch.equal(J[0], torch.eye(3, dtype=torch.float64) / 4)  # m == 1 takes the contracted branch: k = 1, dk = 0
    assert m[names.index("step_inside")] == float(np.nextafter(np.float32(1), np.float32(0)))
    assert m[names.index("step_outside")] == float(np.nextafter(np.float32(1), np.float32(2)))
    assert abs(m[names.index("far_1e3")] - 1e3) < 1e-3 and abs(m[names.index("far_1e6")] - 1e6) < 1
    assert at("far_3e38")[0] == float(np.float32(3e38))
    # the point whose position reaches 1.0: on the dense level 0 its +1 corner is cell `res`
    reach = "far_3e38" if case.mode == 1 else "far_1e18"
    assert HF.position32(x, case.mode)[names.index(reach), 0] == 1.0
    _, fl = HF.cells(x[names.index(reach)][None], case)
    assert fl[0, 0, 0] + 1 == case.cfg().resolutions[0]
    assert torch.equal(at("origin"), torch.zeros(3, dtype=torch.float64))
    nz = x[names.index("negative_zero")]
    assert torch.signbit(nz).tolist() == [True, False, True] and nz[0] == 0 and nz[2] == 0
    assert (at("axis_inside") != 0).sum() == 1 and (at("axis_outside") != 0).sum() == 1
    assert at("linf_tie").tolist()[:2] == [1.5, 1.5]
    # what is compared for less (the module docstring's three kinds), and nothing else
    tie = torch.zeros(x.shape[0], dtype=torch.bool)
    over = tie.clone()
    if case.mode == 1:
        tie[names.index("linf_tie")] = True
    else:
        over[names.index("far_3e38")] = True
    assert torch.equal(pl["values"], ~over) and torch.equal(pl["tangents"], ~over & ~tie)
    far = [names.index(n) for n in ("far_1e3", "far_1e6", "far_3e38", "far_1e18")]
    assert sorted(torch.nonzero(~pl["pe"]).flatten().tolist()) == sorted(far)
    assert torch.nonzero(~pl["pe_finite"]).flatten().tolist() == ([names.index("far_3e38")] if case.pe else [])
    q = HF.position32(x, case.mode)[[names.index(f"face{j}") for j in (5, 7, 9)]].double() * 15.0 + 0.5
    assert ((q - q.round()).abs() < 4e-6).all()


def _oracle_row(case, xd, table):
    pos = xd if case.mode == 0 else (O.scene_contraction(xd, float("inf") if case.mode == 1 else 2) + 2.0) / 4.0
    parts = ([xd] if case.include_x else []) + ([O.nerf_encoding(xd, case.pe, 0.0, case.pe_max_exp, False)] if case.pe else [])
    return torch.cat(parts + [O.hash_grid_encode(pos, table, case.cfg())], -1)


@pytest.mark.parametrize("name", ALL)
def test_restatement_equals_the_oracle_and_its_jvp(name):
    """values: O.hash_grid_encode + O.nerf_encoding in float64, wherever the oracle (which rounds ITS float64 position to float32)
    picks the restatement's cell; tangents: the double-backward jvp, on 64 pool points off the contraction surface and off ties"""
    case, ref = HF.CASES[name], HF.reference(name)
    x, ne = ref["x"], ref["n_edges"]
    table = HF.table64(case.cfg().n_params)
    pos64, _ = HB.grid_position(x, case.mode)
    idx64, _ = O.hash_grid_indices(pos64, case.cfg())
    same = ~HF.cell_disagreements(ref["cell"][0], idx64).any(-1)
    ok = same & ref["values"] & ref["pe"]
    assert ok.sum() >= x.shape[0] - 8
    row = _oracle_row(case, x.double(), table)
    for g, cols in case.groups():
        cols = list(cols)
        scale = row[ok][:, cols].abs().max().item()
        err = (ref["Y64"][ok][:, cols] - row[ok][:, cols]).abs().max().item()
        assert scale > 0 and err <= 1e-10 * scale, (g, err, scale)
    m = HF.norm_of(x, case.mode)
    srt = x.abs().sort(-1).values
    smooth_here = torch.ones_like(same)
    if case.mode:
        smooth_here = ((m - 1).abs() > 1e-4) & ((srt[:, 2] - srt[:, 1]) > 1e-5 if case.mode == 1 else smooth_here)
    sub = torch.nonzero(ok & smooth_here & (torch.arange(x.shape[0]) >= ne)).flatten()[:64]
    assert sub.numel() == 64 and (case.mode == 0 or ((m[sub] < 1).any() and (m[sub] > 1).any()))
    xd = x[sub].double().requires_grad_(True)
    row = _oracle_row(case, xd, table)
    v = torch.ones_like(row, requires_grad=True)
    gg = torch.autograd.grad(row, xd, v, create_graph=True)[0]
    for k in range(3):
        ek = torch.zeros_like(xd); ek[:, k] = 1.0
        jvp = torch.autograd.grad(gg, v, ek, retain_graph=True)[0]  # d row / d x_k
        for g, cols in case.groups():
            cols = list(cols)
            scale = ref["T64"][:, sub][:, :, cols].abs().max().item()
            err = (ref["T64"][k, sub][:, cols] - jvp[:, cols]).abs().max().item()
            assert scale > 0 and err <= 1e-10 * scale, (g, k, err, scale)


@pytest.mark.parametrize("name", ALL)
def test_reference_alone_stays_inside_the_cell_cap(name):
    """the cells of the float32 position against those of the float64 position: modes 0 and 2 are pinned to the float32 oracle bit for
    bit, so only mode 1 has a cap -- and plain float32 against float64 uses no more than half of it"""
    case, ref = HF.CASES[name], HF.reference(name)
    N = ref["x"].shape[0]
    pos64, _ = HB.grid_position(ref["x"], case.mode)
    idx64, _ = O.hash_grid_indices(pos64, case.cfg())
    n = int(HF.cell_disagreements(ref["cell"][0], idx64)[ref["values"]].sum())
    print(f"{name}: {n} of {N * case.n_levels} (point, level) pairs in another cell; cap {HF.cell_cap(case, N)}")
    if case.mode == 1:
        assert 2 * n <= HF.CELL_CAP_LINF * N * case.n_levels
    assert HF.cell_cap(case, N) == (int(1e-4 * N * case.n_levels) if case.mode == 1 else 0)


def test_bars_are_finite_and_of_the_size_of_float32():
    for name in ALL:
        ref = HF.reference(name)
        assert torch.isfinite(ref["Y64"][ref["values"]]).all() and torch.isfinite(ref["T64"][:, ref["tangents"]]).all()
        for g, b in HF.value_bars(name).items():
            if g != "x":  # (x: the floor follows the far points' own size; the GPU test holds the copy to equality)
                assert 0 < b < 1e-3, (name, g, b)
        for g, b in HF.tangent_bars(name).items():
            scale = ref["T64"][:, HF.point_mask(ref, "tangent", g)][:, :, list(dict(HF.CASES[name].groups())[g])].abs().max().item()
            assert 0 < b < 1e-2 * scale, (name, g, b, scale)


# ---- injected defects -------------------------------------------------------------------------------------------------------------
SPR = 1


@functools.lru_cache(maxsize=None)
def _defective(name, defect):
    case, ref = HF.CASES[name], HF.reference(name)
    Y, T = HF.encode(case, ref["x"], torch.float64, ref["cell"], HF.table64(case.cfg().n_params), defect=defect)
    Td = HF.directional(T, HF.point_dirs(ref["dirs"], ref["x"].shape[0], SPR), defect=defect)
    return Y, T, Td


def _touched(case, defect):
    """{quantity: set of groups} the defect must break; everything else must stay inside its bar"""
    levels = {f"level{l}" for l in range(case.n_levels)}
    pes = {f"pe{f}" for f in range(case.pe)}
    every = {g for g, _ in case.groups()}
    first_order = lambda gs: dict(value=set(), tangent=gs, directional=gs, dx=gs)  # noqa: E731
    if defect in ("dk", "no_quarter"):
        return first_order(levels)
    if defect == "level0_scale":
        return first_order({"level0"})
    if defect == "smoothstep_derivative":
        return first_order({f"level{HF.SMOOTH_DEFECT_LEVEL}"})
    if defect == "pe_step":
        gs = pes - {"pe0"}
        return dict(value=gs, tangent=gs, directional=gs, dx=gs)
    if defect == "identity_entry":
        return first_order({"x"})
    if defect == "shifted_sin_sign":
        return first_order(pes)
    assert defect == "neighbour_dir"
    return dict(value=set(), tangent=set(), directional=every, dx=set())


@pytest.mark.parametrize("name,defect", list(zip(["sdf_linf"] * len(HF.DEFECTS), HF.DEFECTS)) + [("sdf_l2", "dk"), ("sdf_l2", "no_quarter")])
def test_bars_notice_and_attribute(name, defect):
    """each defect breaks the bar of every group it touches at least tenfold, in every quantity it touches, and no other group's"""
    case, ref = HF.CASES[name], HF.reference(name)
    Y, T, Td = _defective(name, defect)
    Td64, _ = HF.directional_reference(name, SPR)
    ratios = {q: {} for q in ("value", "tangent", "directional", "dx")}
    for g, cols in case.groups():
        cols = list(cols)
        mv, mt = HF.point_mask(ref, "value", g), HF.point_mask(ref, "tangent", g)
        ratios["value"][g] = (Y[mv][:, cols] - ref["Y64"][mv][:, cols]).abs().max().item() / HF.value_bars(name)[g]
        ratios["tangent"][g] = (T[:, mt][:, :, cols] - ref["T64"][:, mt][:, :, cols]).abs().max().item() / HF.tangent_bars(name)[g]
        ratios["directional"][g] = (Td[mt][:, cols] - Td64[mt][:, cols]).abs().max().item() / HF.directional_bars(name, SPR)[g]
        dx64, bar = HF.dx_bar(name, g)
        dxd, _ = HF.input_gradient(T, ref["dY"], cols)
        md = HF.dx_point_mask(ref, g)
        ratios["dx"][g] = ((dxd - dx64).abs() / bar)[md].max().item()
    touched = _touched(case, defect)
    for q, per_group in ratios.items():
        for g, r in per_group.items():
            if g in touched[q]:
                assert r >= 10.0, (defect, q, g, r)
            else:
                assert r <= 1.0, (defect, q, g, r)
