"""FilmChainFn with frozen weights (the illumination decoder, the eval-latent fit): the chain kernels then neither store nor allocate
what only the weight gradients read (y_save, dz_save, dpre_save: csrc/film_chain.hip KEEP_Y / KEEP = false).  Skipping a store and
keeping a tile in registers changes no arithmetic, so the frozen run must equal the trained run of the same tensors BIT FOR BIT."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (n_map, n_film, cond_dim, x_dim, out_dim): one and ten d_cond tiles; the second is the product's decoder
NETS = [(2, 2, 36, 16, 1), (5, 9, 300, 10, 3)]
# at H = 256 the decoder's 5 + 3 x 9 bias rows exceed the chain kernels' bias table (hip.film_supported): ops.film_apply runs that case on
# the per-layer node, which must agree with itself just the same; the decoder with five FiLM layers is the widest net the chain takes there
WIDE_256 = (5, 5, 300, 10, 3)
CASES = [(H, net) for H in (128, 256) for net in NETS] + [(256, WIDE_256)]
PER_LAYER = [(256, NETS[1])]
# a single partial tile; two tiles; one full four-wave workgroup plus a tail; two full eight-wave workgroups plus a 70-row tail
ROWS = [1, 33, 133, 582]


def _pad4(n):
    return (n + 3) // 4 * 4


def _padded(rows, cols, real_rows, real_cols, g, scale):
    w = torch.zeros(rows, cols)
    w[:real_rows, :real_cols] = (torch.rand(real_rows, real_cols, generator=g) * 2 - 1) * scale
    return w.to(DEV)


@functools.lru_cache(maxsize=None)
def _weights(H, n_map, n_film, cond_dim, x_dim, out_dim):
    """the padded weight list FilmChainFn takes (map_w0, map_b0, .., map_wo, map_bo, film_w0, film_b0, .., out_w, out_b), seeded"""
    g = torch.Generator().manual_seed(1000 * H + 10 * n_film + n_map)
    wb = []
    for l in range(n_map):
        k = cond_dim if l == 0 else H
        wb += [_padded(H, _pad4(k), H, k, g, (6.0 / k) ** 0.5), _padded(H, 1, H, 1, g, 0.3).reshape(H)]
    wb += [_padded(2 * n_film * H, H, 2 * n_film * H, H, g, 0.25 * (6.0 / H) ** 0.5), _padded(2 * n_film * H, 1, 2 * n_film * H, 1, g, 0.3).reshape(-1)]
    for i in range(n_film):
        k = x_dim if i == 0 else H
        wb += [_padded(H, _pad4(k), H, k, g, (1.0 / k) if i == 0 else (6.0 / k) ** 0.5 / 25.0), _padded(H, 1, H, 1, g, 0.3).reshape(H)]
    wb += [_padded(4, H, out_dim, H, g, (6.0 / H) ** 0.5), _padded(4, 1, out_dim, 1, g, 0.3).reshape(4)]
    return tuple(wb)


@functools.lru_cache(maxsize=None)
def _inputs(M, cond_dim, x_dim):
    g = torch.Generator().manual_seed(7 + M)
    cond = torch.zeros(M, _pad4(cond_dim)); cond[:, :cond_dim] = torch.randn(M, cond_dim, generator=g) * 0.5
    x = torch.zeros(M, _pad4(x_dim)); x[:, :x_dim] = torch.rand(M, x_dim, generator=g) * 2 - 1
    d_res = torch.zeros(M, 4); d_res[:] = torch.randn(M, 4, generator=g)
    return cond.to(DEV), x.to(DEV), d_res.to(DEV)


def _run(H, net, M, trainable):
    """one forward + backward through ops.film_apply -> (res, d_cond, d_x, weight gradients or None)"""
    from neusky_amd import ops
    n_map, n_film, cond_dim, x_dim, out_dim = net
    wb = _weights(H, *net)
    for w in wb:
        w.requires_grad_(trainable)
    cond, x, d_res = _inputs(M, cond_dim, x_dim)
    cond, x = cond.clone().requires_grad_(True), x.clone().requires_grad_(True)
    assert ops._film_fused_ok(x, cond, n_map, n_film, wb) == ((H, net) not in PER_LAYER), "which node the case must reach"
    res = ops.film_apply(x, cond, n_map, n_film, True, True, *wb)
    grads = torch.autograd.grad(res, (cond, x) + (wb if trainable else ()), d_res)
    for w in wb:
        w.requires_grad_(False)
    return res.detach(), grads[0], grads[1], (grads[2:] if trainable else None)


@functools.lru_cache(maxsize=None)
def _reference(H, net, M):
    """(a): the weights take gradients -- today's path; computed once per case and left unchanged"""
    from neusky_amd import ops
    ops.begin_step(DEV)
    return _run(H, net, M, True)


def _same(got, ref, what):
    for name, g, r in zip(("res", "d_cond", "d_x"), got[:3], ref[:3]):
        assert torch.equal(g, r), f"{what}: {name} differs from the trained run, max |diff| {(g - r).abs().max().item():.3e}"


@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("H,net", CASES)
def test_frozen_weights_give_the_trained_run_bit_for_bit(H, net, M):
    from neusky_amd import ops
    ref = _reference(H, net, M)
    ops.begin_step(DEV)
    _same(_run(H, net, M, False), ref, "frozen")


def test_trainable_again_after_a_frozen_backward_still_matches():
    """the packed streams are shared by both runs and the frozen run leaves gmax slots unwritten: neither may leak into a later trained run"""
    from neusky_amd import ops
    H, net, M = 128, NETS[1], 133
    ref = _reference(H, net, M)
    ops.begin_step(DEV)
    _same(_run(H, net, M, False), ref, "frozen")
    again = _run(H, net, M, True)
    _same(again, ref, "trained again")
    # the weight-gradient kernel adds its row blocks' partial sums with float atomics in whatever order they finish: two trained runs
    # agree to a few roundings of the largest entry (2^-24 each), not to the bit.  2^-18 of it leaves room for 64 of them; an operand
    # that was not kept, or a scale off by a power of two, shows at the size of the gradient itself
    for i, (g, r) in enumerate(zip(again[3], ref[3])):
        bound = 2.0 ** -18 * r.abs().max().item()
        assert (g - r).abs().max().item() <= bound, f"weight gradient {i} of the second trained run: {(g - r).abs().max().item():.3e} > {bound:.3e}"


def test_frozen_run_replays_from_a_captured_graph():
    from neusky_amd import ops
    H, net, M = 128, NETS[1], 133
    ops.begin_step(DEV)
    eager = _run(H, net, M, False)
    graph = ops.CapturedGraph(DEV, 2, lambda i: _run(H, net, M, False)[:3])
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        _same(graph.outputs, eager, "replay")
    graph.retire()


@pytest.mark.parametrize("H", [128, 256])
def test_frozen_run_keeps_and_allocates_no_weight_gradient_operands(H, monkeypatch):
    from neusky_amd import hip, ops
    net, M = (NETS[1] if H == 128 else WIDE_256), 133
    n_map, n_film = net[:2]
    seen = {}

    def spy(name, pos):
        orig = getattr(hip, name)

        def wrapper(*a, **kw):
            seen[name] = a[pos]
            return orig(*a, **kw)
        monkeypatch.setattr(hip, name, wrapper)

    spy("film_chain_fwd", 8)       # y_save
    spy("film_chain_bwd_film", 7)  # dz_save
    spy("film_chain_bwd_map", 7)   # dpre_save
    wb = _weights(H, *net)
    cond, x, d_res = _inputs(M, net[2], net[3])
    cond, x = cond.clone().requires_grad_(True), x.clone().requires_grad_(True)
    ops.begin_step(DEV)
    res = ops.film_apply(x, cond, n_map, n_film, True, True, *wb)
    assert len(res.grad_fn.saved_tensors) == 2 + n_map + n_film + len(wb), "x, cond, hs, zs and the weights: no ys"
    torch.autograd.grad(res, (cond, x), d_res)
    distinct = lambda ts: 0 if ts is None else len({t.data_ptr() for t in ts})  # noqa: E731
    assert seen["film_chain_bwd_film"] is None, "no dz buffers"
    if hip.film_keepless(H) == "registers":
        assert H == 128 and seen["film_chain_fwd"] is None and seen["film_chain_bwd_map"] is None
    else:
        assert distinct(seen["film_chain_fwd"]) == 2 and distinct(seen["film_chain_bwd_map"]) == 1, "ping-pong ys, one shared dpre buffer"
