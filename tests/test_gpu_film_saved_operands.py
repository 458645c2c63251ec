"""The FiLM chain on SAVED operands (csrc/film_chain.hip: film_fwd_kernel<.., SAVE_FA>, film_bwd4s_kernel, pack direction 3): the forward
keeps f = 15 F + 30 and the sine argument f z + phase of every FiLM tile, the backward reads them back instead of re-forming F and phase
from the last mapping activation.

The saved values are the ones the re-form rebuilds (same planes, same packed tiles, same k order, same fmaf forms), so
  * the forward's res and every other side output equal the plain forward's BIT FOR BIT, f_save / arg_save meet the float64 restatement
    (film_chain_cpu.py) under the bar that file gives z of the same layer, and
  * the saved backward equals the re-form backward bit for bit in dz_save, dfp, dfp_rowmax, gmax and d_x -- where the head has ONE output.
    The re-form kernel leaves the head gradient's four-term sum  dY = sum_o d_res[o] W_out[o]  to the compiler, which fuses it differently
    from element to element (most as an fma chain, some as plain additions); the saved form states one chain.  With out_dim = 1 three
    terms are exactly zero and every form gives the same bits; with out_dim > 1 the two differ by roundings of dY (measured: see
    profiles/film_saved_operands_ab.txt), and each form is held to the float64 bars of film_chain_cpu.py instead.
Through ops.FilmChainFn the switch (hip.film_saved_operands) therefore changes no bit of res, and none of d_x and d_cond at out_dim = 1;
the weight gradients land by float atomics in no fixed order, so they are held to the spread two switch-off runs of the same inputs show."""
import functools

import pytest
import torch

import film_chain_cpu as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (H, n_map, n_film, cond_dim, x_dim, out_dim): no transposed tile at all / one / the DDF's depth, at both widths and both conditionings
NETS = [(128, 2, 1, 36, 16, 1), (256, 2, 1, 300, 16, 3), (128, 2, 2, 300, 16, 3), (256, 2, 2, 36, 16, 1), (128, 3, 5, 36, 16, 3),
        (256, 3, 5, 300, 16, 1)]
# a partial tile; dead lanes; a workgroup with one full and one one-row wave; one full workgroup and a one-row wave; several workgroups
# with a partial last
ROWS = [1, 31, 33, 129, 582]
CASES = [(net, M) for net in NETS for M in ROWS]


@functools.lru_cache(maxsize=None)
def _weights(net):
    return tuple(w.to(DEV) for w in F.make_weights(*net))


@functools.lru_cache(maxsize=None)
def _inputs(net, M):
    return tuple(t.to(DEV) for t in F.make_inputs(M, net[3], net[4], net[5]))


def _descr(net, direction):
    """(descriptor, packed stream, table) of one direction, packed afresh"""
    from neusky_amd import hip, ops
    H, n_map, n_film = net[:3]
    wb = _weights(net)
    mw, mb, mwo, mbo, fw, fb, ow, ob, _ = ops._film_unpack(wb, n_map, n_film)
    d = hip.film_net(mw[0].shape[1], fw[0].shape[1], ow.shape[0], mw, mb, mwo, mbo, fw, fb, ow, ob)
    nbytes, ntiles = hip.film_stream_layout(d, direction)
    stream = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    table = torch.zeros(hip.FILM_TABLE_FLOATS, device=DEV)
    hip.film_pack(d, stream, table, direction)
    return d, stream, table, ntiles


def _forward(net, M, saved):
    from neusky_amd import hip
    H, n_map, n_film = net[:3]
    cond, x, _ = _inputs(net, M)
    d, stream, table, _ = _descr(net, 0)
    Mp = hip.film_rows(M)
    new = lambda n: [torch.full((Mp, H), float("nan"), device=DEV) for _ in range(n)]  # noqa: E731
    out = dict(h=new(n_map), z=new(n_film), y=new(n_film), f=new(n_film) if saved else None, arg=new(n_film) if saved else None,
               res=torch.empty(M, 4, device=DEV))
    hip.film_chain_fwd(d, stream, table, cond, x, M, out["h"], out["z"], out["y"], out["res"], out["f"], out["arg"])
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def _saved_forward(net, M):
    return _forward(net, M, True)


@functools.lru_cache(maxsize=None)
def _reference(net, M):
    """float64 restatement (differentiating the LeakyReLU branches the kernels took) and its bars, plus f and the sine argument formed in
    float64 from its own h_last and z"""
    cond, x, d_res = (t.cpu() for t in _inputs(net, M))
    wb = [w.cpu() for w in _weights(net)]
    masks = [_live(h, M, net[0]).cpu() > 0 for h in _saved_forward(net, M)["h"]]
    ref, bar = F.reference_and_bars(wb, cond, x, d_res, leaky_masks=masks)
    p = F.unpack_net(wb)
    H, n_film = net[0], net[2]
    fo = ref["h"][-1] @ p["mo_w"].t() + p["mo_b"]
    fs = [15.0 * fo[:, i * H:(i + 1) * H] + 30.0 for i in range(n_film)]
    args = [fs[i] * ref["z"][i] + fo[:, (n_film + i) * H:(n_film + i + 1) * H] for i in range(n_film)]
    return ref, bar, fs, args


def _live(buf, M, H):
    from neusky_amd import hip
    return hip.film_native_to_rows(buf, M, H)


@pytest.mark.parametrize("net,M", CASES)
def test_forward_keeps_f_and_the_sine_argument_and_changes_nothing_else(net, M):
    H, n_map, n_film = net[:3]
    got, plain = _saved_forward(net, M), _forward(net, M, False)
    assert torch.equal(got["res"], plain["res"]), "res differs from the plain forward"
    for name in ("h", "z", "y"):
        for i, (a, b) in enumerate(zip(got[name], plain[name])):
            assert torch.equal(_live(a, M, H), _live(b, M, H)), f"{name}_save[{i}] differs from the plain forward"
    ref, bar, fs, args = _reference(net, M)
    for i in range(n_film):
        for name, mine, want in (("f", got["f"][i], fs[i]), ("arg", got["arg"][i], args[i])):
            err = F.distance(_live(mine, M, H).cpu().double(), want)
            print(f"{name}_save[{i}] H {H} M {M}: err {err:.3e} bar {bar[f'z{i}']:.3e}")
            assert err <= bar[f"z{i}"], f"{name}_save[{i}]: {err:.3e} of the largest entry, bar (z{i}'s) {bar[f'z{i}']:.3e}"


def _backward(net, M, saved, keep, with_dx):
    from neusky_amd import hip
    H, n_map, n_film = net[:3]
    _, _, d_res = _inputs(net, M)
    fwd = _saved_forward(net, M)
    d, stream, table, _ = _descr(net, 3 if saved else 1)
    Mp = hip.film_rows(M)
    dzs = [torch.zeros(Mp, H, device=DEV) for _ in range(n_film)] if keep else None
    dfp = torch.zeros(Mp, 2 * n_film * H, device=DEV)
    rowmax = torch.zeros(Mp, device=DEV)
    gmax = torch.zeros(n_film + 1, device=DEV)
    d_x = torch.zeros(M, 16, device=DEV) if with_dx else None
    hip.film_chain_bwd_film(d, stream, table, M, d_res, None if saved else fwd["h"][-1], fwd["z"], dzs, dfp, rowmax, gmax, d_x,
                            fwd["f"] if saved else None, fwd["arg"] if saved else None)
    torch.cuda.synchronize()
    out = {"dfp": dfp, "dfp_rowmax": rowmax[:M], "gmax": gmax}
    # dead rows of a live tile are stored too (their values follow row M - 1's gradient in both forms): compared whole
    if keep:
        out.update({f"dz{i}": t for i, t in enumerate(dzs)})
    if with_dx:
        out["d_x"] = d_x
    return out


# d_x = NULL changes one store of the last tile: two row counts per network cover it
BWD_CASES = [(net, M, keep, True) for net, M in CASES for keep in (True, False)] + \
            [(net, M, keep, False) for net in NETS for M in (33, 582) for keep in (True, False)]


@pytest.mark.parametrize("net,M,keep,with_dx", BWD_CASES)
def test_saved_backward_equals_the_reform_bit_for_bit(net, M, keep, with_dx):
    from neusky_amd import hip
    H, n_film, out_dim = net[0], net[2], net[5]
    got, ref = _backward(net, M, True, keep, with_dx), _backward(net, M, False, keep, with_dx)
    assert got.keys() == ref.keys()
    assert float(ref["gmax"][-1]) > 0 and float(ref["dfp_rowmax"].min()) > 0, "the comparison saw real gradients"
    # gmax is the largest magnitude among the live rows of what the same launch stored
    dfp_rows = hip.film_native_to_rows(got["dfp"].reshape(-1, 2 * n_film * H), M, 2 * n_film * H)
    assert got["gmax"][n_film].item() == dfp_rows.abs().max().item()
    for i in range(n_film if keep else 0):
        assert got["gmax"][i].item() == _live(got[f"dz{i}"], M, H).abs().max().item()
    if out_dim == 1:
        for k in ref:
            assert torch.equal(got[k].view(torch.int32), ref[k].view(torch.int32)), \
                f"{k}: saved form differs from the re-form, max |diff| {(got[k] - ref[k]).abs().max().item():.3e}"
        return
    # out_dim > 1 (module docstring): each form against float64 under that file's bars; the distance between the two is printed
    r64, bar, _, _ = _reference(net, M)

    def rows(out):
        dfp = hip.film_native_to_rows(out["dfp"].reshape(-1, 2 * n_film * H), M, 2 * n_film * H)
        g = {"dfp_rowmax": (out["dfp_rowmax"], r64["dfp_rowmax"])}
        for i in range(n_film):
            g[f"dF{i}"] = (dfp[:, i * H:(i + 1) * H], r64["dfp"][:, i * H:(i + 1) * H])
            g[f"dphase{i}"] = (dfp[:, (n_film + i) * H:(n_film + i + 1) * H], r64["dfp"][:, (n_film + i) * H:(n_film + i + 1) * H])
            if keep:
                g[f"dz{i}"] = (_live(out[f"dz{i}"], M, H), r64["dz"][i])
        if with_dx:
            g["d_x"] = (out["d_x"][:, :r64["d_x"].shape[1]], r64["d_x"])
        return g
    gs, gr = rows(got), rows(ref)
    for k in gs:
        e_s, e_r = F.distance(gs[k][0].cpu().double(), gs[k][1]), F.distance(gr[k][0].cpu().double(), gr[k][1])
        between = (gs[k][0] - gr[k][0]).abs().max().item() / max(gr[k][0].abs().max().item(), 1e-300)
        print(f"{k} H {H} M {M}: saved {e_s:.3e} re-form {e_r:.3e} bar {bar[k]:.3e}; saved - re-form {between:.3e} = {between * 2 ** 24:.1f} x 2^-24 of the largest entry")
        assert e_s <= bar[k], f"{k}: saved form {e_s:.3e} of the largest entry, bar {bar[k]:.3e} (re-form {e_r:.3e})"


@pytest.mark.parametrize("H,n_film", [(128, 1), (128, 5), (256, 2)])
def test_direction_3_is_direction_1_without_the_f_and_phase_tiles(H, n_film):
    """tile count of the layout, and the packed stream's round trip: every group of direction 3 is, byte for byte, the group of the same
    transposed tile in direction 1 (layers n_film-1 .. 1, then the layer-0 input tile), and so is its reciprocal scale"""
    from neusky_amd import hip
    net = (H, 2, n_film, 36, 16, 1)
    NT, Gh, GROUP = H // 32, (H // 16 + 7) // 8, 16384
    _, s1, t1, n1 = _descr(net, 1)
    _, s3, t3, n3 = _descr(net, 3)
    assert n3 == (n_film - 1) * NT + 1 and n1 == n3 + 2 * n_film * NT
    BIAS = 6144
    idx1 = [(n_film - 1 - i) * 3 * NT + 2 * NT + u for i in range(n_film - 1, 0, -1) for u in range(NT)] + [n1 - 1]
    for j3, j1 in enumerate(idx1):
        assert torch.equal(s3[j3 * Gh * GROUP:(j3 + 1) * Gh * GROUP], s1[j1 * Gh * GROUP:(j1 + 1) * Gh * GROUP]), f"tile {j3} of direction 3"
        assert t3[BIAS + j3].item() == t1[BIAS + j1].item(), f"scale of tile {j3}"
    assert torch.equal(t3[:BIAS], t1[:BIAS]), "bias table"


# ---------------------------------------------------------------------------------------------------------- FilmChainFn, switch off / on
def _chain(net, M, switch, trainable):
    from neusky_amd import hip, ops
    H, n_map, n_film = net[:3]
    wb = _weights(net)
    cond, x, d_res = _inputs(net, M)
    for w in wb:
        w.requires_grad_(trainable)
    cond, x = cond.clone().requires_grad_(True), x.clone().requires_grad_(True)
    old = hip.film_saved_operands
    hip.film_saved_operands = lambda hidden: switch
    try:
        assert ops._film_fused_ok(x, cond, n_map, n_film, wb)
        res = ops.film_apply(x, cond, n_map, n_film, True, True, *wb)
        assert (res.grad_fn.film_fa[0] is not None) == switch
        grads = torch.autograd.grad(res, (cond, x) + (wb if trainable else ()), d_res)
    finally:
        hip.film_saved_operands = old
        for w in wb:
            w.requires_grad_(False)
    return res.detach(), grads[0], grads[1], (grads[2:] if trainable else None)


@pytest.mark.parametrize("trainable", [True, False], ids=["trained", "frozen"])
@pytest.mark.parametrize("net,M", [(NETS[4], 582), (NETS[5], 582), (NETS[2], 33), (NETS[1], 129)])
def test_film_chain_fn_switch_changes_no_bit(net, M, trainable):
    from neusky_amd import ops
    ops.begin_step(DEV)
    off = _chain(net, M, False, trainable)
    on = _chain(net, M, True, trainable)
    exact = ("res", "d_cond", "d_x") if net[5] == 1 else ("res",)
    for name, a, b in zip(("res", "d_cond", "d_x"), on[:3], off[:3]):
        if name in exact:
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{name}: switch on differs, max |diff| {(a - b).abs().max().item():.3e}"
    if net[5] > 1:  # (module docstring) d_cond and d_x of either switch position under the float64 bars
        r64, bar, _, _ = _reference(net, M)
        for name, a, b in zip(("d_cond", "d_x"), on[1:3], off[1:3]):
            w = r64[name].shape[1]
            e_on, e_off = F.distance(a[:, :w].cpu().double(), r64[name]), F.distance(b[:, :w].cpu().double(), r64[name])
            print(f"{name} H {net[0]} M {M}: on {e_on:.3e} off {e_off:.3e} bar {bar[name]:.3e}")
            assert e_on <= bar[name], f"{name}: switch on {e_on:.3e} of the largest entry, bar {bar[name]:.3e} (off {e_off:.3e})"
    if trainable:
        off2 = _chain(net, M, False, True)
        torch.cuda.synchronize()
        for i, (g_on, g_off, g_off2) in enumerate(zip(on[3], off[3], off2[3])):
            # two switch-off runs differ by the order of the float atomics alone, and with dz, dfp and dpre bit-identical so does the
            # switched run: it is held to the spread measured here.  One pair of runs is one draw and may agree exactly, so the spread
            # is floored at the 2^-18 of the largest entry test_gpu_film_frozen.py allows two trained runs (64 roundings of 2^-24)
            spread = (g_off - g_off2).abs().max().item()
            bound = max(spread, 2.0 ** -18 * g_off.abs().max().item())
            d = (g_on - g_off).abs().max().item()
            print(f"weight gradient {i}: on/off {d:.3e}, off/off {spread:.3e}, bound {bound:.3e}")
            assert d <= bound, f"weight gradient {i}: on/off {d:.3e}, off/off spread {spread:.3e}, bound {bound:.3e}"


@pytest.mark.parametrize("net", [NETS[4], NETS[5]], ids=["H128", "H256"])
def test_saved_run_replays_from_a_captured_graph(net):
    from neusky_amd import ops
    M = 129
    ops.begin_step(DEV)
    eager = _chain(net, M, True, False)[:3]
    graph = ops.CapturedGraph(DEV, 2, lambda i: _chain(net, M, True, False)[:3])
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        for name, g, e in zip(("res", "d_cond", "d_x"), graph.outputs, eager):
            assert torch.equal(g, e), f"replay: {name} differs from the eager run"
    graph.retire()
