"""moleculesde_amd.capture on the host: the order of the capture protocol, what a failed capture leaves behind, the replay
of a record and the optimiser snapshot -- with recorders in place of the device calls."""
import contextlib
import types

import pytest
import torch

from moleculesde_amd import capture, slabs, wcache


class FakeOpt:
    def __init__(self, log):
        self.log = log

    def new_table_slot(self):
        self.log.append("opt.new_table_slot")

    def use_eager_slot(self):
        self.log.append("opt.use_eager_slot")


@pytest.fixture
def log(monkeypatch):
    calls = []

    def rec(name, ret=None):
        return lambda *a, **k: (calls.append(name), ret)[1]

    @contextlib.contextmanager
    def fake_graph(g, pool=None, capture_error_mode=None):
        calls.append(("graph.enter", pool, capture_error_mode))
        try:
            yield
        finally:
            calls.append("graph.exit")

    @contextlib.contextmanager
    def fake_no_gc():
        calls.append("no_gc.enter")
        try:
            yield
        finally:
            calls.append("no_gc.exit")

    def fake_flush():
        calls.append(("flush", len(slabs._PENDING_UPLOADS)))
        slabs._PENDING_UPLOADS.clear()

    monkeypatch.setattr(slabs, "new_param_grad_slot", rec("slabs.new_param_grad_slot"))
    monkeypatch.setattr(slabs, "use_eager_param_grad_slot", rec("slabs.use_eager_param_grad_slot"))
    monkeypatch.setattr(slabs, "flush_table_uploads", fake_flush)
    monkeypatch.setattr(slabs, "note_capture", rec("slabs.note_capture"))
    monkeypatch.setattr(slabs, "no_gc", fake_no_gc)
    monkeypatch.setattr(slabs, "_PENDING_UPLOADS", [])
    monkeypatch.setattr(torch.cuda, "synchronize", rec("synchronize"))
    monkeypatch.setattr(torch.cuda, "CUDAGraph", lambda: (calls.append("CUDAGraph"), types.SimpleNamespace())[1])
    monkeypatch.setattr(torch.cuda, "graph", fake_graph)
    return calls


@contextlib.contextmanager
def scope(log, name):
    log.append(name + ".enter")
    try:
        yield
    finally:
        log.append(name + ".exit")


HEAD = ["slabs.note_capture", "opt.new_table_slot", "slabs.new_param_grad_slot", "synchronize"]
TAIL = [("flush", 1), "opt.use_eager_slot", "slabs.use_eager_param_grad_slot"]


def one_graph(k, pool):
    return ["CUDAGraph", "no_gc.enter", "bounds.enter", ("graph.enter", pool, "thread_local"), f"body{k}", "graph.exit",
            "bounds.exit", "no_gc.exit"]


@pytest.mark.parametrize("n_graphs", [1, 3])
def test_session_call_order(log, n_graphs):
    graphs = []
    with capture.CaptureSession(FakeOpt(log), "dev", pool="POOL") as s:
        for k in range(n_graphs):
            with s.graph(scope(log, "bounds")) as g:
                log.append(f"body{k}")
                if k == 0:
                    slabs._PENDING_UPLOADS.append(("dev", "host"))       # what upload_table records while capturing
            graphs.append(g)
    assert log == HEAD + [c for k in range(n_graphs) for c in one_graph(k, "POOL")] + TAIL
    assert len({id(g) for g in graphs}) == n_graphs and slabs._PENDING_UPLOADS == []


def test_session_without_optimiser_takes_no_slot(log):
    with capture.CaptureSession(None, "dev") as s, s.graph() as g:
        log.append("body")
    assert g is not None
    assert log == ["slabs.note_capture", "synchronize", "CUDAGraph", "no_gc.enter", ("graph.enter", None, "thread_local"),
                   "body", "graph.exit", "no_gc.exit", ("flush", 0)]


def test_failed_capture_restores_eager_slots_and_drops_uploads(log):
    with pytest.raises(ZeroDivisionError):
        with capture.CaptureSession(FakeOpt(log), "dev") as s, s.graph(scope(log, "bounds")):
            slabs._PENDING_UPLOADS.append(("dev", "host"))
            1 / 0
    assert slabs._PENDING_UPLOADS == []
    assert not any(isinstance(c, tuple) and c[0] == "flush" for c in log)          # nothing was uploaded
    assert log[-5:] == ["graph.exit", "bounds.exit", "no_gc.exit", "opt.use_eager_slot", "slabs.use_eager_param_grad_slot"]


def test_failed_slot_allocation_restores_eager_slots(log, monkeypatch):
    def boom(device):
        log.append("slabs.new_param_grad_slot")
        raise MemoryError("pinned")
    monkeypatch.setattr(slabs, "new_param_grad_slot", boom)
    with pytest.raises(MemoryError):
        with capture.CaptureSession(FakeOpt(log), "dev"):
            log.append("body")                    # never reached
    assert log == ["slabs.note_capture", "opt.new_table_slot", "slabs.new_param_grad_slot", "opt.use_eager_slot",
                   "slabs.use_eager_param_grad_slot"]


def test_session_with_the_weight_gradient_slot_only(log):
    with capture.CaptureSession(None, "dev", grad_slot=True) as s, s.graph():
        log.append("body")
    assert log[:3] == ["slabs.note_capture", "slabs.new_param_grad_slot", "synchronize"]
    assert log[-2:] == [("flush", 0), "slabs.use_eager_param_grad_slot"]


def test_record_replay(monkeypatch):
    calls = []
    monkeypatch.setattr(wcache, "sync_weight_copies", lambda: calls.append("sync"))
    monkeypatch.setattr(wcache, "weight_copies_after_replay", lambda keys: calls.append(("after", keys)))
    g = types.SimpleNamespace(replay=lambda: calls.append("replay"))
    rec = capture.CapturedStep(g, ("k1", "k2"), loss="L", pred="P")
    assert (rec.graph, rec.keys, rec.loss, rec.pred) == (g, ("k1", "k2"), "L", "P")
    rec.replay()
    assert calls == ["sync", "replay", ("after", ("k1", "k2"))]
    del calls[:]
    capture.CapturedStep(g).replay()            # Adam outside the graph: no keys, nothing to mark fresh
    assert calls == ["sync", "replay"]
    del calls[:]
    capture.CapturedStep(g, ()).replay()        # Adam inside, no copy refreshed: the epoch still moves
    assert calls == ["sync", "replay", ("after", ())]


def test_optimizer_snapshot_round_trip(monkeypatch):
    calls = []
    monkeypatch.setattr(wcache, "invalidate_weight_copies", lambda: calls.append("invalidate"))
    gen = torch.Generator().manual_seed(3)
    opt = types.SimpleNamespace(flat_p=torch.randn(17, generator=gen), m=torch.randn(17, generator=gen),
                                v=torch.rand(17, generator=gen), step_dev=torch.tensor([5], dtype=torch.int32))
    loss_acc = torch.tensor([0.1234567890123], dtype=torch.float64)
    live = (opt.flat_p, opt.m, opt.v, opt.step_dev, loss_acc)
    want = [t.clone() for t in live]
    snap = capture.optimizer_snapshot(opt, loss_acc)
    assert len(snap) == 5 and all(s.data_ptr() != t.data_ptr() for s, t in zip(snap, live))
    for t in live:
        t.add_(1)
    assert calls == []
    capture.optimizer_restore(opt, snap, loss_acc)
    assert calls == ["invalidate"]
    assert all(torch.equal(t, w) and t.dtype == w.dtype for t, w in zip(live, want))
    assert all(a is b for a, b in zip((opt.flat_p, opt.m, opt.v, opt.step_dev), live))      # restored in place
