"""ops.retire_graph (the workaround of the HIP runtime's graph-destroy use-after-free) and ops.role_stream (one stream
per role: pool streams alias after 32 creations), ops.CapturedGraph (the one owner of the capture protocol and of a
graph's retirement), ops._prepared (the one owner of the per-step weight-preparation caches), ops._sink_grads / ops._carve_grads (the
one owner of where a parameter's gradient goes) and the three dispatchers that pick an autograd node per kernel set:
host logic on the CPU, the real thing on the GPU."""
import gc
import time

import pytest
import torch


class _Graph:
    alive = 0

    def __init__(self):
        _Graph.alive += 1

    def __del__(self):
        _Graph.alive -= 1


def test_retire_keeps_a_graph_alive_and_destroys_it_later(monkeypatch):
    from neusky_amd import ops
    calls = []
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: calls.append("sync"))
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    monkeypatch.setattr(ops, "RETIRE_SECONDS", 0.5)
    ops._RETIRED_GRAPHS.clear()
    _Graph.alive = 0
    ops.retire_graph(_Graph())
    gc.collect()
    assert _Graph.alive == 1 and calls == [], "a retired graph must outlive the call that retires it (its last launch may still be in flight)"
    ops.retire_graph(None)  # nothing is old enough yet
    assert _Graph.alive == 1
    time.sleep(0.6)
    ops.retire_graph(_Graph())  # a later retirement: the old one is destroyed HERE, after a device synchronize, on this thread
    gc.collect()
    assert _Graph.alive == 1 and calls == ["sync"] and len(ops._RETIRED_GRAPHS) == 1
    # never from inside a capture (a synchronize would invalidate it): the purge waits for the next call
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    time.sleep(0.6)
    ops.retire_graph(None)
    assert _Graph.alive == 1 and calls == ["sync"]
    ops._RETIRED_GRAPHS.clear()


class _Stream:
    def __init__(self, name, events):
        self.name, self.events = name, events

    def wait_stream(self, other):
        self.events.append(("wait", self.name, other.name))


def _fake_cuda(monkeypatch, events):
    """torch.cuda's capture surface and ops.role_stream replaced by fakes that append to `events`; -> the state the fakes share"""
    from neusky_amd import ops
    state = {"current": _Stream("main", events), "capturing": False, "capture": _Stream("capture", events)}

    class _Current:  # torch.cuda.stream(s) and torch.cuda.graph(g, stream=s): `s` is the current stream inside
        def __init__(self, stream, graph=None, **kw):
            self.stream, self.graph, self.kw = stream, graph, kw

        def __enter__(self):
            if self.graph is not None:
                events.append(("graph", type(self.graph).__name__, self.stream.name, self.kw))
            self.old = state["current"], state["capturing"]
            state["current"], state["capturing"] = self.stream, self.graph is not None

        def __exit__(self, *exc):
            state["current"], state["capturing"] = self.old

    def new_stream(*a, **k):
        events.append(("Stream()",))
        return _Stream("pool", events)

    def role_stream(role, device=None):
        events.append(("role_stream", role))
        return state[role]

    monkeypatch.setattr(torch.cuda, "CUDAGraph", _Graph)
    monkeypatch.setattr(torch.cuda, "graph", lambda graph, stream=None, **kw: _Current(stream, graph, **kw))
    monkeypatch.setattr(torch.cuda, "stream", _Current)
    monkeypatch.setattr(torch.cuda, "Stream", new_stream)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: state["current"])
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: events.append(("sync",)))
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: state["capturing"])
    monkeypatch.setattr(ops, "role_stream", role_stream)
    monkeypatch.setattr(ops, "RETIRE_SECONDS", 1e9)
    return state


def test_captured_graph_follows_the_capture_protocol_in_order(monkeypatch):
    from neusky_amd import ops
    events = []
    state = _fake_cuda(monkeypatch, events)
    monkeypatch.setattr(ops, "CAPTURE_MODE", "a-mode-set-after-import")  # read at capture time (tools/lab.py assigns it)

    def body(i):
        events.append(("body", i, state["current"].name, state["capturing"]))
        return "static outputs" if state["capturing"] else None

    g = ops.CapturedGraph("cuda:0", 2, body)
    assert events == [("role_stream", "capture"),
                      ("wait", "capture", "main"),                       # the capture stream waits for the current stream
                      ("body", 0, "capture", False), ("body", 1, "capture", False),  # eager warm-up on the capture stream
                      ("wait", "main", "capture"),                       # the current stream waits for the warm-up
                      ("sync",),
                      ("graph", "_Graph", "capture", {"capture_error_mode": "a-mode-set-after-import"}),
                      ("body", 2, "capture", True)]                      # the captured run: the body can tell it from the warm-ups
    assert g.outputs == "static outputs"
    assert ("Stream()",) not in events, "a capture must not create a stream: pool streams alias (ops.role_stream)"
    g.retire()
    ops._RETIRED_GRAPHS.clear()


def test_captured_graph_is_retired_exactly_once(monkeypatch):
    from neusky_amd import ops
    _fake_cuda(monkeypatch, [])
    ops._RETIRED_GRAPHS.clear()
    _Graph.alive = 0
    g = ops.CapturedGraph("cuda:0", 1, lambda i: None)
    g.retire()
    del g
    gc.collect()
    assert len(ops._RETIRED_GRAPHS) == 1 and _Graph.alive == 1, "retire() then the destructor: one entry, the graph still alive"
    g = ops.CapturedGraph("cuda:0", 1, lambda i: None)
    del g  # an owner that just drops it
    gc.collect()
    assert len(ops._RETIRED_GRAPHS) == 2 and _Graph.alive == 2 and all(isinstance(o, _Graph) for o, _ in ops._RETIRED_GRAPHS)

    def refused(i):
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("operation not permitted when stream is capturing")
    with pytest.raises(RuntimeError, match="not permitted when stream is capturing"):
        ops.CapturedGraph("cuda:0", 1, refused)
    gc.collect()
    assert len(ops._RETIRED_GRAPHS) == 2, "a graph whose capture was refused was never launched: nothing to retire"
    ops._RETIRED_GRAPHS.clear()


def test_only_ops_constructs_or_captures_a_graph():
    """every capture of the package goes through ops.CapturedGraph: no other module names the two torch entry points in code"""
    import io
    import pathlib
    import tokenize
    import neusky_amd
    root = pathlib.Path(neusky_amd.__file__).parent
    offenders = []
    for path in sorted(root.rglob("*.py")):
        toks = tokenize.generate_tokens(io.StringIO(path.read_text()).readline)
        code = "".join(t.string for t in toks if t.type not in (tokenize.COMMENT, tokenize.STRING, tokenize.NL, tokenize.NEWLINE,
                                                                tokenize.INDENT, tokenize.DEDENT))
        if "CUDAGraph(" in code or "cuda.graph(" in code:
            offenders.append(str(path.relative_to(root)))
    assert offenders == ["ops.py"]


def test_prepared_weights_are_built_once_and_ordered_on_every_hit(monkeypatch):
    from neusky_amd import ops
    calls = []
    marks = iter(["mark-0", "mark-1"])
    monkeypatch.setattr(ops, "_ready_mark", lambda: next(marks))
    monkeypatch.setattr(ops, "_order_after", lambda mark, seq: calls.append(("order_after", mark, seq)))
    ops.begin_step()
    seq0 = ops._STEP_SEQ[0]
    keep = object()

    def build():
        calls.append(("build",))
        return "planes"

    assert ops._prepared(ops._PLANES, "key", keep, build) == "planes"
    assert calls == [("build",)], "a miss builds and has nothing to wait for"
    assert ops._PLANES["key"][0] is keep, "what the key's data pointers belong to is held by the entry"
    assert ops._prepared(ops._PLANES, "key", keep, build) == "planes"
    assert calls == [("build",), ("order_after", "mark-0", seq0)], "a hit orders the current stream after the preparation, and builds nothing"
    ops.begin_step()  # the optimizer has changed the weights: the cache is dropped
    del calls[:]
    assert ops._prepared(ops._PLANES, "key", keep, build) == "planes"
    assert calls == [("build",)] and ops._PLANES["key"][2:] == ("mark-1", seq0 + 1)
    ops._PLANES.clear()


def _slab_param(*shape):
    """a parameter as distributed.GradientSlab leaves it: .grad a view of a zero-filled flat buffer, marked and registered as a sink"""
    from neusky_amd import ops
    p = torch.nn.Parameter(torch.randn(*shape))
    p.grad = torch.zeros((p.numel() + 3) // 4 * 4)[:p.numel()].view_as(p)
    p._nsky_grad_sink = True
    ops.register_grad_sink(p)
    return p


def _strided_grad(p):
    return torch.zeros(*p.shape[:-1], 2 * p.shape[-1])[..., ::2]  # p's shape, not contiguous


def test_sink_helper_finds_the_parameter_behind_a_tensor():
    import weakref
    from neusky_amd import ops
    plain = torch.nn.Parameter(torch.randn(6, 3))
    plain.grad = torch.zeros(6, 3)
    for by in ("object", "pad", "base", "address"):
        assert ops._sink_param(plain, by) is None
        assert ops._sink_grad(plain, by=by, from_first_pass=True) is None and not hasattr(plain, "_nsky_sunk"), "an unregistered tensor never sinks"
    assert ops._sink_param(None) is None and ops._sink_grads((None,), from_first_pass=True) == [None]
    p = _slab_param(6, 3)
    assert ops._sink_param(p) is p and ops._sink_param(p, "base") is p and ops._sink_param(p, "address") is p
    assert ops._sink_param(p.detach(), "address") is p and ops._sink_param(p.detach()) is None, "a saved alias: found by its address only"
    assert ops._sink_param(p.view(-1), "address") is None, "same address, another shape"
    # the padded case: the consumer of the padding copy asks for the parameter behind it
    b = _slab_param(6)
    padded = ops.pad_bias(b)
    assert padded.shape == (8,) and padded._nsky_pad_of is b and ops._sink_param(padded, "pad") is b and ops._sink_param(padded) is None
    assert ops.pad_bias(plain[0])._nsky_pad_of is None
    # the [n, 2] view of a flat parameter (the hash table): found as its base, its gradient view is the same memory
    flat = _slab_param(10)
    table = flat.view(5, 2)
    assert ops._sink_param(table) is None, "not the parameter itself: a wrong shape for every caller that does not ask for the base"
    assert ops._sink_param(table, "base") is flat and ops._sink_param(flat.view(5, 2)[1:], "base") is None
    view = ops._sink_grad(table, by="base", from_first_pass=True)
    assert view is flat.grad and view.view_as(table).data_ptr() == flat.grad.data_ptr() and flat._nsky_sunk
    # a dead weak reference: forgotten; an address reused by another tensor (a dead pipeline's entry): no match, and no mark on the stranger
    t = torch.zeros(4)
    gone = _slab_param(4)
    ops._GRAD_SINKS[t.data_ptr()] = weakref.ref(gone)
    del gone
    gc.collect()
    assert ops._sink_grad(t, by="address", from_first_pass=False) is None and t.data_ptr() not in ops._GRAD_SINKS
    other = _slab_param(4)
    ops._GRAD_SINKS[t.data_ptr()] = weakref.ref(other)
    assert ops._sink_grad(t, by="address", from_first_pass=False) is None and not hasattr(other, "_nsky_sunk")
    del ops._GRAD_SINKS[t.data_ptr()]


# DESIGN section 4, "Where a parameter's gradient goes": per caller, (view taken, parameter marked afterwards) in the four states of a
# slab parameter -- its view as .grad in the first pass (not marked yet) / once marked / .grad None / a .grad that is not contiguous
_TAKES_FROM_FIRST_PASS = {"first": (True, True), "marked": (True, True), "none": (False, True), "strided": (False, False)}
_WAITS_FOR_THE_MARK = {"first": (False, True), "marked": (True, True), "none": (False, True), "strided": (False, True)}
_SINK_SITES = {
    "_PadFn.backward": (dict(from_first_pass=False), _WAITS_FOR_THE_MARK),
    "shared_grad bias": (dict(by="address", from_first_pass=False, bias=True), _WAITS_FOR_THE_MARK),
    "HashEncodeFn.backward": (dict(by="base", from_first_pass=True), _TAKES_FROM_FIRST_PASS),
    "FilmChainFn / FilmLayersFn.backward": (dict(from_first_pass=True), _TAKES_FROM_FIRST_PASS),
    "FilmChainFn.backward, padded weights": (dict(from_first_pass=False, mark=False),
                                             {"first": (False, False), "marked": (True, True), "none": (False, False), "strided": (False, False)}),
    "ProposalMLPFn.backward": (dict(from_first_pass=True, all_or_none=True), _TAKES_FROM_FIRST_PASS),
}


@pytest.mark.parametrize("site", sorted(_SINK_SITES))
@pytest.mark.parametrize("state", ["first", "marked", "none", "strided"])
def test_sink_helper_keeps_every_call_sites_eligibility(site, state):
    from neusky_amd import ops
    how, table = _SINK_SITES[site]
    p = _slab_param(6, 3)
    slab_view = p.grad
    if state == "marked":
        p._nsky_sunk = True
    elif state == "none":
        p.grad = None
    elif state == "strided":
        p.grad = _strided_grad(p)
    ops._SUNK_BIAS.clear()
    view = ops._sink_grad(p, **how)
    taken, marked = table[state]
    assert (view is not None) == taken and getattr(p, "_nsky_sunk", False) == (marked or state == "marked")
    if taken:
        assert view is slab_view, "the accumulator is the slab view itself"
    assert ops._SUNK_BIAS == ({slab_view.data_ptr()} if (taken and how.get("bias")) else set()), "only shared_grad's biases are recorded for first_only"
    ops._SUNK_BIAS.clear()


def test_proposal_parameters_sink_all_four_or_none():
    from neusky_amd import ops
    how = _SINK_SITES["ProposalMLPFn.backward"][0]
    ps = [_slab_param(16, 4), _slab_param(16), _slab_param(1, 16), _slab_param(1)]
    assert [v is p.grad for v, p in zip(ops._sink_grads(ps, **how), ps)] == [True] * 4 and all(p._nsky_sunk for p in ps)
    ps = [_slab_param(16, 4), _slab_param(16), _slab_param(1, 16), _slab_param(1)]
    ps[1].grad = None
    ps[2].grad = _strided_grad(ps[2])
    assert ops._sink_grads(ps, **how) == [None] * 4
    assert [getattr(p, "_nsky_sunk", False) for p in ps] == [False, True, False, False], "nothing taken: only the dropped .grad sinks from the next pass on"
    ps = [_slab_param(16, 4), torch.nn.Parameter(torch.zeros(16)), _slab_param(1, 16), _slab_param(1)]  # (one is no slab parameter)
    assert ops._sink_grads(ps, **how) == [None] * 4 and not any(hasattr(p, "_nsky_sunk") for p in ps)


def test_padded_slab_parameter_sinks_from_its_second_pass_on():
    """_PadFn end to end on the host: the first pass hands the gradient to autograd and marks the parameter, every later one defers the
    add into the slab view to the end of the pass"""
    from neusky_amd import ops
    ops.reset_pass_state()
    b = _slab_param(6)
    slab_view = b.grad
    (ops.pad_bias(b) * torch.arange(8.0)).sum().backward()
    assert b._nsky_sunk and b.grad is slab_view and torch.equal(slab_view, torch.arange(6.0))
    slab_view.zero_()
    (ops.pad_bias(b) * torch.arange(8.0)).sum().backward()
    assert b.grad is slab_view and torch.equal(slab_view, torch.arange(6.0)) and not ops._DEFERRED_PADS and not ops._PASS["queued"]


def test_carved_accumulators_are_aligned_disjoint_and_zero():
    from neusky_amd import ops
    ops.begin_step()
    ts = [torch.empty(5, 3), torch.empty(5), torch.empty(2, 7), torch.empty(1)]
    sink = torch.ones(5)
    grads, sunk = ops._carve_grads(ts, [None, sink, None, None])
    assert sunk == [False, True, False, False] and grads[1] is sink, "a sunk entry is the sink view itself"
    carved = [g for g, s in zip(grads, sunk) if not s]
    assert all(g.shape == t.shape and g.is_contiguous() for g, t in zip(grads, ts))
    assert all(g.data_ptr() % 16 == 0 for g in carved) and all(not g.any() for g in carved)
    base = carved[0].data_ptr()
    assert [(g.data_ptr() - base) // 4 for g in carved] == [0, 16, 32], "pad4(numel) floats apart, in order: 15 -> 16, 14 -> 16"
    assert carved[0]._base is carved[1]._base is carved[2]._base and carved[0]._base.numel() == 16 + 16 + 4, "ONE buffer of the padded sizes"
    grads, sunk = ops._carve_grads(ts[:2], [torch.ones(5, 3), sink])
    assert sunk == [True, True] and grads[1] is sink
    (g,), _ = ops._carve_grads([torch.empty(1)], [None])
    assert g._base.numel() == 4 and g.data_ptr() == g._base.data_ptr()
    # the (dW, db) pair of grad_weight / shared_grad: a bias that sinks takes no room
    like, bias = torch.empty(6, 3), _slab_param(6)
    bias._nsky_sunk = True
    ops.reset_pass_state()
    calls = []
    import unittest.mock as mock
    with mock.patch.object(torch.cuda, "current_stream", lambda *a: mock.Mock(cuda_stream=0)), \
            mock.patch.object(ops, "_queue_end_of_pass", lambda: calls.append("queued")):
        dW, db, first = ops.shared_grad(like, bias)
        assert first and db is bias.grad and dW._base.numel() == 20 and ops.first_only(first, db) is None and ops.first_only(first, dW) is dW
        assert ops.shared_grad(like, bias)[:2] == (dW, db) and ops.shared_grad(like, bias)[2] is False and calls == ["queued"]
    ops.reset_pass_state()


@pytest.mark.parametrize("net", ["film", "field", "sdf"])
def test_dispatchers_pick_the_chain_node_exactly_when_its_predicate_holds(monkeypatch, net):
    from neusky_amd import ops
    picked = []
    for name in ("FilmChainFn", "FilmLayersFn", "FieldChainFn", "SDFAlbedoFn", "SdfChainFn", "SdfLayersFn"):
        monkeypatch.setattr(getattr(ops, name), "apply", staticmethod(lambda *a, _n=name: picked.append(_n)))
    supported = {"v": True}
    for name in ("film_supported", "field_supported", "sdf_supported"):
        monkeypatch.setattr(ops.hip, name, lambda *a: supported["v"])
    z = torch.zeros
    if net == "film":  # x [M, 4], cond [M, 8]; one mapping layer, its head, one FiLM layer, the output layer
        wb = [z(32, 8), z(32), z(64, 32), z(64), z(32, 4), z(32), z(4, 32), z(4)]
        call, nodes = (lambda: ops.film_apply(z(16, 4), z(16, 8), 1, 1, True, False, *wb)), ("FilmChainFn", "FilmLayersFn")
    elif net == "field":
        ws = [z(256, 72), z(256), z(256, 256), z(256), z(260, 256), z(260), z(256, 300), z(256), z(256, 256), z(256), z(4, 256), z(4)]
        call, nodes = (lambda: ops.field_apply(z(16, 72), *ws, 100.0, True)), ("FieldChainFn", "SDFAlbedoFn")
    else:
        ws = [z(256, 72), z(256), z(256, 256), z(256), z(260, 256), z(260)]
        call, nodes = (lambda: ops.sdf_value_apply(z(16, 72), *ws, 100.0, True)), ("SdfChainFn", "SdfLayersFn")
    try:
        call()
        supported["v"] = False
        call()
        supported["v"] = True
        ops.set_precision_policy("f32")
        call()
        assert picked == [nodes[0], nodes[1], nodes[1]], "the chain node when the kernels take the shapes; under the exact-fp32 policy never"
    finally:
        ops.set_precision_policy("splith")


@pytest.mark.gpu
def test_role_streams_are_distinct_and_survive_pool_wraparound():
    from neusky_amd import ops
    roles = {r: ops.role_stream(r) for r in ops.ROLES}
    assert len({s.stream_id for s in roles.values()}) == len(ops.ROLES)
    others = [torch.cuda.Stream() for _ in range(70)]  # the pool (32 per priority) wraps twice: some of these ARE the role streams
    assert any(o == roles["capture"] for o in others), "torch.cuda.Stream() objects alias pool streams: the reason the roles are created once"
    again = {r: ops.role_stream(r) for r in ops.ROLES}
    assert all(again[r] is roles[r] for r in ops.ROLES)


@pytest.mark.gpu
def test_captures_run_on_the_capture_role_stream_after_many_streams():
    """the failing case of the round in small: a process that has created many streams builds a pipeline and captures its step"""
    from util_step import randomise, small_pipeline_config
    from neusky_amd import ops
    from neusky_amd.engine import GraphedTrainStep, Optimizers, neusky_optimizers
    _ = [torch.cuda.Stream() for _ in range(45)]
    torch.manual_seed(0)
    pipe = small_pipeline_config(R=32, S=8, D=24, images=4).setup(device="cuda:0")
    pipe.train()
    randomise(pipe)
    opt = Optimizers(neusky_optimizers(), pipe.get_param_groups())
    rb, batch = pipe.datamanager.next_train(0)
    stepper = GraphedTrainStep(pipe, opt, rb, batch, warmup=1, start_step=10)
    m = pipe.model
    ids = {ops.role_stream("capture").stream_id, m._illumination_stream().stream_id, m._ddf_fit_stream().stream_id, ops.role_stream("wgrad").stream_id}
    assert len(ids) == 4
    loss = stepper.step(11, rb, batch)[0]
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss))
