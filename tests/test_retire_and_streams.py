"""ops.retire_graph (the workaround of the HIP runtime's graph-destroy use-after-free) and ops.role_stream (one stream
per role: pool streams alias after 32 creations), ops.CapturedGraph (the one owner of the capture protocol and of a
graph's retirement) and ops._prepared (the one owner of the per-step weight-preparation caches): host logic on the CPU, the real thing
on the GPU."""
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
