"""Props on the CPU: the float64 restatement (tests/props_cpu.py) against closed forms, the insertion's invariants, the drawn cases the GPU
tests share (none of them may be a margin case), and the host side of relight.props: Prop's validation, the block's layout, JSON."""
import json
import math

import numpy as np
import pytest
import torch

import props_cpu as PC
from neusky_amd.relight import MAX_PROPS, Prop, as_props, load_props, props_block, save_props

F = np.float32


def _block(*props):
    return props_block(props).numpy()


# ---------------------------------------------------------------- the restatement against closed forms
def test_sphere_on_axis():
    block = _block(Prop("sphere", (0, 0, 5), 1.5, (0.2, 0.4, 0.6)))
    t, who, n, a, _ = PC.intersect(F([[0, 0, 0]]), F([[0, 0, 1]]), block)
    assert t[0] == F(3.5) and who[0] == 0 and np.array_equal(n[0], F([0, 0, -1])) and np.array_equal(a[0], F([0.2, 0.4, 0.6]))
    # a direction of length 2 halves the parameter; the point of entry and the normal stay
    t2, _, n2, _, _ = PC.intersect(F([[0, 0, 0]]), F([[0, 0, 2]]), block)
    assert t2[0] == F(1.75) and np.array_equal(n2[0], n[0])
    # off axis by b: t_in = 5 - sqrt(r^2 - b^2)
    t3, _, n3, _, _ = PC.intersect(F([[0.9, 0, 0]]), F([[0, 0, 1]]), block)
    assert abs(float(t3[0]) - (5 - math.sqrt(1.5 ** 2 - float(F(0.9)) ** 2))) < 1e-6 and abs(np.linalg.norm(n3[0].astype(np.float64)) - 1) < 1e-7
    # a tangent line (disc == 0) and a miss have no interval
    assert PC.intersect(F([[1.5, 0, 0]]), F([[0, 0, 1]]), block)[1][0] == -1
    assert PC.intersect(F([[2.0, 0, 0]]), F([[0, 0, 1]]), block)[1][0] == -1


def test_yawed_box_is_the_box_turned_back_by_hand():
    rng = np.random.default_rng(5)
    yaw, c, h = 37.0, np.array([0.3, -0.2, 0.1]), (0.2, 0.35, 0.15)
    turned, plain = _block(Prop("box", c, h, yaw_deg=yaw)), _block(Prop("box", (0, 0, 0), h))
    o = rng.uniform(-2, 2, (200, 3))
    d = rng.uniform(-0.3, 0.3, (200, 3)) + c - o
    cy, sy = math.cos(math.radians(yaw)), math.sin(math.radians(yaw))
    back = np.array([[cy, sy, 0], [-sy, cy, 0], [0, 0, 1]])  # a turn by -yaw about z
    t, who, n, _, _ = PC.intersect(F(o), F(d), turned)
    t0, who0, n0, _, _ = PC.intersect(F((o - c) @ back.T), F(d @ back.T), plain)
    assert (who >= 0).sum() > 50 and np.array_equal(who, who0)
    hit = who >= 0
    assert np.allclose(t[hit], t0[hit], rtol=2e-5, atol=0) and np.allclose(n[hit] @ back.T, n0[hit], atol=1e-6)
    # the axis-aligned box's normals are signed unit axes facing the ray
    assert np.all(np.abs(n0[hit]).sum(1) == 1) and np.all((n0[hit] * (d @ back.T)[hit]).sum(1) < 0)


def test_from_inside_a_prop_nothing_is_seen_but_light_is_blocked():
    for prop in (Prop("sphere", (0.1, 0.2, 0.3), 0.5), Prop("box", (0.1, 0.2, 0.3), (0.4, 0.5, 0.6), yaw_deg=20)):
        block = _block(prop)
        o, d = F([[0.15, 0.25, 0.2]]), F([[0.3, -0.5, 0.8]])
        t, who, n, a, _ = PC.intersect(o, d, block)
        assert who[0] == -1 and np.isinf(t[0]) and not n.any() and not a.any()
        occ, _ = PC.occlude(o, None, 0.0, block, directions=d)
        assert occ[0, 0]
        # a lamp inside the prop with the point, nearer than the wall, is not blocked... by t_in < t_max it is: the point is inside
        occ, _ = PC.occlude(o, None, 0.0, block, targets=F([[0.2, 0.2, 0.3]]), clearance=F([0.0]))
        assert occ[0, 0]


def test_prop_behind_the_origin_and_lamps_in_front_of_and_behind_a_prop():
    block = _block(Prop("sphere", (0, 0, 2), 0.5))
    x = F([[0, 0, 0]])
    assert PC.intersect(x, F([[0, 0, -1]]), block)[1][0] == -1
    assert not PC.occlude(x, None, 0.0, block, directions=F([[0, 0, -1]]))[0][0, 0]
    lamps, clear = F([[0, 0, 1.0], [0, 0, 4.0], [0, 0, 1.52], [0, 0, 1.52]]), F([0.0, 0.0, 0.0, 0.05])
    occ, _ = PC.occlude(x, None, 0.0, block, targets=lamps, clearance=clear)
    # in front of the prop; behind it; just inside its near wall; the same lamp with a clearance that ends the ray before the wall
    assert occ[0].tolist() == [False, True, True, False]
    # the lift: the point starts bias along its normal, so a prop within bias below the surface is cleared
    low = _block(Prop("box", (0, 0, -0.5), (1, 1, 0.505)))
    up = F([[0, 0, 1]])
    assert PC.occlude(x, None, 0.01, low, directions=up)[0][0, 0] and PC.occlude(x, F([[0, 0, 0]]), 0.01, low, directions=up)[0][0, 0]
    assert not PC.occlude(x, F([[0, 0, 3]]), 0.01, low, directions=up)[0][0, 0]
    assert PC.occlude(x, F([[0, 0, np.inf]]), 0.01, low, directions=up)[0][0, 0]


def test_ties_go_to_the_lowest_index_and_flags_are_honoured():
    a, b = Prop("sphere", (0, 0, 3), 1.0, (1, 0, 0)), Prop("sphere", (0, 0, 3), 1.0, (0, 1, 0))
    o, d = F([[0.2, 0.1, 0]]), F([[0, 0, 1]])
    t, who, _, alb, margin = PC.intersect(o, d, _block(a, b))
    assert who[0] == 0 and alb[0, 0] == 1 and margin[0] > PC.MARGIN  # (an exact tie is decided, not a margin case)
    assert PC.intersect(o, d, _block(b, a))[3][0, 1] == 1
    # an invisible prop nearer than a visible one is not seen, and shadows; a non-caster is seen and does not shadow
    near = Prop("sphere", (0, 0, 1.5), 0.3, visible=False)
    assert PC.intersect(o, d, _block(near, a))[1][0] == 1
    assert PC.occlude(o, None, 0.0, _block(near), directions=d)[0][0, 0]
    ghost = Prop("sphere", (0, 0, 1.5), 0.3, casts_shadows=False)
    assert PC.intersect(o, d, _block(ghost, a))[1][0] == 0 and not PC.occlude(o, None, 0.0, _block(ghost), directions=d)[0][0, 0]
    # a box's entry axis: ties to the lowest axis (a ray at a corner's diagonal)
    box = _block(Prop("box", (0, 0, 0), (1, 1, 1)))
    n = PC.intersect(F([[-2, -2, -2]]), F([[1, 1, 1]]), box)[2][0]
    assert np.array_equal(n, F([-1, 0, 0]))


def test_a_zero_direction_component_on_and_off_a_slab():
    box = _block(Prop("box", (0, 0, 0), (0.5, 0.25, 1.0)))
    d = F([[0, 0, 1]])
    t, who, n, _, _ = PC.intersect(F([[0.4, 0.2, -3]]), d, box)
    assert who[0] == 0 and t[0] == F(2.0) and np.array_equal(n[0], F([0, 0, -1]))
    assert PC.intersect(F([[0.6, 0.2, -3]]), d, box)[1][0] == -1  # outside the x slab
    assert PC.intersect(F([[0.5, 0.2, -3]]), d, box)[1][0] == -1  # on its face: |o'| < h is strict
    # a yawed box: a ray along z has d'_x = d'_y = 0 whatever the yaw
    yawed = _block(Prop("box", (0, 0, 0), (0.5, 0.25, 1.0), yaw_deg=90))
    assert PC.intersect(F([[0.2, 0.4, -3]]), d, yawed)[1][0] == 0 and PC.intersect(F([[0.4, 0.2, -3]]), d, yawed)[1][0] == -1
    # a zero direction inside a box: a line that never leaves it
    assert PC.occlude(F([[0.1, 0.1, 0.1]]), None, 0.0, box, directions=F([[0, 0, 0]]))[0][0, 0]


# ---------------------------------------------------------------- insert
def _hit_and_samples(seed, R=65, S=24):
    block = PC.draw_block(seed, 3)
    o, d = PC.draw_rays(seed + 1, R, block)
    hit = PC.intersect(o, d, block)
    return hit, PC.draw_samples(seed + 2, R, S, hit[0])


def test_insert_weights_sum_to_one_on_a_ray_that_enters_a_prop():
    hit, (w, s, e, a, n) = _hit_and_samples(11)
    w1, s1, e1, a1, n1, _ = PC.insert(w, s, e, a, n, *hit[:4])
    entered = hit[1] >= 0
    assert entered.sum() > 10 and (~entered).sum() > 10
    assert np.abs(w1[entered].astype(np.float64).sum(1) - 1).max() < 24 * 2.0 ** -24
    assert np.array_equal(s1[entered, -1], hit[0][entered]) and np.array_equal(e1[entered, -1], hit[0][entered])
    assert np.array_equal(a1[entered, -1], hit[3][entered]) and np.array_equal(n1[entered, -1], hit[2][entered])
    # the samples in front keep their weight, those behind lose it, everything else is copied
    front = (s + e) / F(2) < hit[0][:, None]
    assert np.array_equal(w1[:, :-1], np.where(front, w, F(0))) and (front[entered].any() and (~front[entered]).any())
    for new, old in ((s1, s), (e1, e), (a1, a), (n1, n)):
        assert np.array_equal(new[:, :-1], old)


def test_insert_a_prop_behind_an_opaque_ray_gets_no_weight():
    R, S = 4, 8
    w = np.zeros((R, S), F)
    w[:, 2] = 1.0
    s = np.tile(np.arange(S, dtype=F) * F(0.1), (R, 1))
    e = s + F(0.1)
    a, n = np.ones((R, S, 3), F), np.ones((R, S, 3), F)
    t_hit, who = np.full(R, 5.0, F), np.zeros(R, np.int32)
    w1 = PC.insert(w, s, e, a, n, t_hit, who, np.ones((R, 3), F), np.ones((R, 3), F))[0]
    assert np.array_equal(w1[:, :-1], w) and not w1[:, -1].any()


def test_insert_a_miss_returns_the_samples_and_a_zero_sample():
    hit, (w, s, e, a, n) = _hit_and_samples(12)
    miss = np.full(hit[1].shape, -1, np.int32)
    w1, s1, e1, a1, n1, near = PC.insert(w, s, e, a, n, np.full(hit[0].shape, np.inf, F), miss, hit[2], hit[3])
    for new, old in ((w1, w), (s1, s), (e1, e), (a1, a), (n1, n)):
        assert np.array_equal(new[:, :-1].view(np.uint32), old.view(np.uint32))
    assert not w1[:, -1].any() and not a1[:, -1].any() and not n1[:, -1].any() and not near.any()
    assert np.array_equal(s1[:, -1], e[:, -1]) and np.array_equal(e1[:, -1], e[:, -1])


# ---------------------------------------------------------------- the drawn cases: none is a margin case
def test_no_drawn_case_is_left_out():
    left, total = 0, 0
    for P in PC.INTERSECT_P:
        block = PC.draw_block(100 + P, P)
        for R in PC.INTERSECT_R:
            o, d = PC.draw_rays(1000 * P + R, R, block)
            t, who, _, _, margin = PC.intersect(o, d, block)
            left, total = left + int((margin < PC.MARGIN).sum()), total + R
            if R == 257:  # every kind of ray is among them
                assert (who >= 0).sum() > R // 4 and (who < 0).sum() > R // 8, (P, (who >= 0).sum())
    block = PC.draw_block(103, 3)  # the rays of the insertion test, whose own intersection feeds it, and of the repeatability test
    for seed, R in [(50 * R + S, R) for R in PC.INSERT_R for S in PC.INSERT_S] + [(9, 257)]:
        margin = PC.intersect(*PC.draw_rays(seed, R, block), block)[4]
        left, total = left + int((margin < PC.MARGIN).sum()), total + R
    for P in (3, 64):
        block = PC.draw_block(100 + P, P)
        for M in PC.OCCLUDE_M:
            for N in PC.OCCLUDE_N:
                x, n, d, p, c = PC.draw_points(7 * M + N, M, N, block)
                for kw in (dict(directions=d), dict(targets=p, clearance=c)):
                    for normals in (n, None):
                        occ, margin = PC.occlude(x, normals, 1e-2, block, **kw)
                        left, total = left + int((margin < PC.MARGIN).sum()), total + M * N
                        if M * N > 1000:
                            assert 0.02 < occ.mean() < 0.98
    assert left == 0, f"{left} of {total} drawn cases have a margin below {PC.MARGIN}: draw from another seed"


# ---------------------------------------------------------------- Prop, the block, JSON
def test_prop_validation():
    p = Prop("box", [1, 2, 3], [0.1, 0.2, 0.3], yaw_deg=30)
    assert p.position == (1.0, 2.0, 3.0) and p.size == (0.1, 0.2, 0.3) and p.albedo == (0.5, 0.5, 0.5) and p.visible and p.casts_shadows
    with pytest.raises(Exception):
        p.size = 1.0  # frozen
    for bad in (dict(shape="cone", position=(0, 0, 0), size=1.0), dict(shape="sphere", position=(0, 0), size=1.0),
                dict(shape="sphere", position=(0, 0, 0), size=0.0), dict(shape="sphere", position=(0, 0, 0), size=-1.0),
                dict(shape="sphere", position=(0, 0, 0), size=(1, 1, 1)), dict(shape="sphere", position=(0, 0, 0), size=float("nan")),
                dict(shape="box", position=(0, 0, 0), size=1.0), dict(shape="box", position=(0, 0, 0), size=(1, 0, 1)),
                dict(shape="box", position=(0, 0, float("inf")), size=(1, 1, 1)),
                dict(shape="sphere", position=(0, 0, 0), size=1.0, albedo=(0.5, 1.5, 0.5)),
                dict(shape="sphere", position=(0, 0, 0), size=1.0, albedo=(0.5, -0.1, 0.5)),
                dict(shape="box", position=(0, 0, 0), size=(1, 1, 1), yaw_deg=float("nan")),
                dict(shape="sphere", position=(0, 0, 0), size=1.0, visible=False, casts_shadows=False)):
        with pytest.raises(ValueError):
            Prop(**bad)
    assert as_props(None) == () and as_props([]) == () and as_props(p) == (p,)
    with pytest.raises(TypeError):
        as_props([p, "sphere"])


def test_props_block_layout():
    s = Prop("sphere", (1, 2, 3), 0.25, (0.1, 0.2, 0.3), yaw_deg=45, casts_shadows=False)
    b = Prop("box", (-1, -2, -3), (0.5, 0.6, 0.7), (0.9, 0.8, 0.7), yaw_deg=30, visible=False)
    block = props_block([s, b])
    assert block.shape == (2, 16) and block.dtype == torch.float32
    want = [[0, 1, 2, 3, 0.25, 0.25, 0.25, 1, 0, 0.1, 0.2, 0.3, 1, 0, 0, 0],  # (a sphere has no yaw)
            [1, -1, -2, -3, 0.5, 0.6, 0.7, math.cos(math.pi / 6), math.sin(math.pi / 6), 0.9, 0.8, 0.7, 0, 1, 0, 0]]
    assert torch.equal(block, torch.tensor(want, dtype=torch.float64).to(torch.float32))
    with pytest.raises(ValueError):
        props_block([])


def test_json_round_trip_and_max_props(tmp_path):
    props = (Prop("sphere", (1, 2, 3), 0.25, (0.1, 0.2, 0.3)), Prop("box", (0, 0, 0), (0.5, 0.6, 0.7), yaw_deg=-30, visible=False))
    path = tmp_path / "props.json"
    save_props(path, props)
    assert load_props(path) == props
    assert set(json.load(open(path))[0]) == {"shape", "position", "size", "albedo", "yaw_deg", "visible", "casts_shadows"}
    path.write_text(json.dumps([{"shape": "sphere", "position": [0, 0, 0], "size": 0.1}]))
    assert load_props(path) == (Prop("sphere", (0, 0, 0), 0.1),)
    for bad in ({"shape": "sphere"}, [{"shape": "sphere", "position": [0, 0, 0]}],
                [{"shape": "sphere", "position": [0, 0, 0], "size": 0.1, "colour": [1, 1, 1]}]):
        path.write_text(json.dumps(bad))
        with pytest.raises(ValueError):
            load_props(path)
    assert MAX_PROPS == 64
    many = [Prop("sphere", (i, 0, 0), 0.1) for i in range(MAX_PROPS + 1)]
    assert len(as_props(many[:MAX_PROPS])) == MAX_PROPS
    with pytest.raises(ValueError):
        as_props(many)
