"""The props' three kernels (csrc/props.hip) against the float64 restatement (tests/props_cpu.py) on the drawn cases the CPU test has
checked to hold no margin case: nsky_props_intersect (id equal, t_hit within 1 ulp, normal within 4 * 2^-24, albedo exact),
nsky_props_insert (copies exact, the prop's weight within 2^-24, its starts and ends exact) and nsky_props_occlude (exactly the
restatement's 0 / unchanged pattern under all three addressings).  A case whose margin is below props_cpu.MARGIN is left out of a
comparison; at most 0.1 % of a test's cases may be."""
import numpy as np
import pytest
import torch

import props_cpu as PC
from neusky_amd import hip
from neusky_amd.relight import Prop, props_block
from neusky_amd.relight.props import insert_props, intersect_props, occlude_by_props

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _kept(margin):
    keep = margin >= PC.MARGIN
    assert (~keep).sum() <= 1e-3 * keep.size, f"{(~keep).sum()} of {keep.size} cases are margin cases"
    return keep


def _check_intersect(o, d, block):
    t, who, n, a = (x.cpu().numpy() for x in intersect_props(_dev(o), _dev(d), _dev(block)))
    t0, who0, n0, a0, margin = PC.intersect(o, d, block)
    keep = _kept(margin)
    assert np.array_equal(who[keep], who0[keep])
    hit = keep & (who0 >= 0)
    assert np.array_equal(np.isinf(t[keep]), np.isinf(t0[keep])) and (t[keep & ~hit] == np.inf).all()
    assert (np.abs(t[hit].astype(np.float64) - t0[hit]) <= np.spacing(t0[hit])).all()
    assert np.abs(n[hit].astype(np.float64) - n0[hit]).max(initial=0.0) <= 4 * 2.0 ** -24
    assert np.array_equal(a[keep], a0[keep]) and not n[keep & ~hit].any()
    return who0


@pytest.mark.parametrize("P", PC.INTERSECT_P)
@pytest.mark.parametrize("R", PC.INTERSECT_R)
def test_intersect(R, P):
    block = PC.draw_block(100 + P, P)
    o, d = PC.draw_rays(1000 * P + R, R, block)
    who = _check_intersect(o, d, block)
    if R == 257:
        assert (who >= 0).sum() > R // 4 and (who < 0).sum() > R // 8
        if P == 3:
            assert not (who == 1).any() and (who == 0).any() and (who == 2).any()  # prop 1 is invisible


def test_intersect_the_named_cases():
    ball, box = Prop("sphere", (0, 0, 3), 1.0, (1, 0, 0)), Prop("box", (0, 0, 0), (0.5, 0.25, 1.0), (0, 0, 1), yaw_deg=90)
    near = Prop("sphere", (0, 0, 1.5), 0.3, visible=False)
    block = props_block([near, ball, Prop("sphere", (0, 0, 3), 1.0, (0, 1, 0)), box]).numpy()
    o = F([[0.2, 0.1, 1.2], [0.2, 0.1, 2.5], [0.2, 0.1, 5], [0.2, 0.4, -3], [0.4, 0.2, -3], [0.1, 0.1, 0.1], [-2, -2, -2]])
    d = F([[0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 1], [0.3, 0.4, -0.5], [1, 1, 1]])
    who = _check_intersect(o, d, block)
    # through the invisible prop to the first of two equal balls; from inside the ball; the ball behind; along z through the yawed box's
    # column and beside it (on to the ball); from inside the box; at the box's corner
    assert who.tolist() == [1, -1, -1, 3, 1, -1, 3]


@pytest.mark.parametrize("S", PC.INSERT_S)
@pytest.mark.parametrize("R", PC.INSERT_R)
def test_insert(R, S):
    block = PC.draw_block(103, 3)
    o, d = PC.draw_rays(50 * R + S, R, block)
    hit = PC.intersect(o, d, block)
    w, s, e, a, n = PC.draw_samples(7 * R + S, R, S, hit[0])
    # the kernel's own intersection feeds its insertion; it is compared on the rays whose intersection is no margin case
    keep = _kept(hit[4])
    got = insert_props(_dev(o), _dev(d), _dev(w), _dev(s), _dev(e), _dev(a), _dev(n), _dev(block))
    assert np.array_equal(got.prop_id.cpu().numpy()[keep], hit[1][keep])
    t_hit = intersect_props(_dev(o), _dev(d), _dev(block))[0].cpu().numpy()
    w0, s0, e0, a0, n0, _ = PC.insert(w, s, e, a, n, t_hit, hit[1], hit[2], hit[3])
    gw, gs, ge, ga, gn = (x.cpu().numpy()[keep] for x in got[:5])
    bits = lambda x: np.ascontiguousarray(x).view(np.uint32)  # noqa: E731
    for g, ref in ((gw, w0), (gs, s0), (ge, e0), (ga, a0), (gn, n0)):
        assert g.shape == ref[keep].shape and np.array_equal(bits(g[:, :S]), bits(ref[keep][:, :S]))
    assert np.abs(gw[:, S].astype(np.float64) - w0[keep][:, S]).max() <= 2.0 ** -24
    assert np.array_equal(gs[:, S], s0[keep][:, S]) and np.array_equal(ge[:, S], e0[keep][:, S])
    entered = hit[1][keep] >= 0
    assert np.array_equal(ga[:, S], a0[keep][:, S]) and np.abs(gn[:, S].astype(np.float64) - n0[keep][:, S]).max() <= 4 * 2.0 ** -24
    assert not gw[~entered, S].any() and not ga[~entered, S].any() and not gn[~entered, S].any()
    if R > 1:
        assert entered.any() and (~entered).any() and (gw[entered, S] > 0).any()


def _check_occlude(block, x, normals, bias, layout, **kw):
    """layout: "mn": vis [M, N] row-major; "nm": [N, M], handed over as its transposed view"""
    M, N = x.shape[0], (kw.get("directions") if "directions" in kw else kw["targets"]).shape[0]
    rng = np.random.default_rng(M * 1000 + N)
    before = rng.uniform(0.05, 1.0, (M, N)).astype(F)
    vis = _dev(before) if layout == "mn" else _dev(before.T.copy()).t()
    dk = {k: _dev(v) for k, v in kw.items()}
    if "targets" in dk:  # the lamps' block: position in columns 0..2, clearance in column 9
        lights = torch.zeros(N, hip.LIGHT_FLOATS, device=DEV)
        lights[:, 0:3], lights[:, 9] = dk["targets"], dk["clearance"]
        dk = {"lights": lights}
    occlude_by_props(vis, _dev(x), None if normals is None else _dev(normals), torch.tensor([bias], device=DEV), _dev(block), **dk)
    occ, margin = PC.occlude(x, normals, bias, block, **kw)
    keep = _kept(margin)
    got = vis.cpu().numpy()
    want = np.where(occ, F(0), before)
    assert np.array_equal(got[keep].view(np.uint32), want[keep].view(np.uint32))
    return occ


@pytest.mark.parametrize("N", PC.OCCLUDE_N)
@pytest.mark.parametrize("M", PC.OCCLUDE_M)
@pytest.mark.parametrize("addressing", ("rows", "transposed", "lamps"))
def test_occlude(addressing, M, N):
    block = PC.draw_block(103, 3)
    x, n, d, p, c = PC.draw_points(7 * M + N, M, N, block)
    kw = dict(targets=p, clearance=c) if addressing == "lamps" else dict(directions=d)
    layout = "mn" if addressing == "rows" else "nm"  # (the lamps' [L, R], as the frame holds it)
    for normals in (n, None):
        occ = _check_occlude(block, x, normals, 1e-2, layout, **kw)
        if M * N > 1000:
            assert 0.02 < occ.mean() < 0.98


def test_occlude_64_props():
    block = PC.draw_block(164, 64)
    x, n, d, p, c = PC.draw_points(7 * 65 + 32, 65, 32, block)
    _check_occlude(block, x, n, 1e-2, "mn", directions=d)
    _check_occlude(block, x, n, 1e-2, "nm", targets=p, clearance=c)


def test_occlude_the_named_cases():
    ball = props_block([Prop("sphere", (0, 0, 2), 0.5)]).numpy()
    x = F([[0, 0, 0], [0, 0, 2.1]])  # (the second point is inside the ball)
    lamps, clear = F([[0, 0, 1.0], [0, 0, 4.0], [0, 0, 1.52], [0, 0, 1.52]]), F([0.0, 0.0, 0.0, 0.05])
    occ = _check_occlude(ball, x, None, 0.0, "nm", targets=lamps, clearance=clear)
    assert occ[0].tolist() == [False, True, True, False] and occ[1].all()
    ghost = props_block([Prop("sphere", (0, 0, 2), 0.5, casts_shadows=False), Prop("sphere", (0, 0, -2), 0.5, visible=False)]).numpy()
    occ = _check_occlude(ghost, x[:1], None, 0.0, "mn", directions=F([[0, 0, 1], [0, 0, -1]]))
    assert occ[0].tolist() == [False, True]
    low = props_block([Prop("box", (0, 0, -0.5), (1, 1, 0.505))]).numpy()
    occ = _check_occlude(low, F([[0, 0, 0]] * 4), F([[0, 0, 3], [0, 0, 0], [0, 0, np.inf], [0, 0, -1]]), 0.01, "mn", directions=F([[0, 0, 1]]))
    assert occ[:, 0].tolist() == [False, True, True, True]  # lifted clear of the box; no lift; no lift; pushed deeper


def test_runs_repeat_to_the_bit():
    block = PC.draw_block(103, 3)
    o, d = PC.draw_rays(9, 257, block)
    a, b = intersect_props(_dev(o), _dev(d), _dev(block)), intersect_props(_dev(o), _dev(d), _dev(block))
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))
