"""Recording a step into a hipGraph and replaying it: the one place that knows the protocol.

    opt.new_table_slot(); slabs.new_param_grad_slot(dev)     own pinned table slots, allocated BEFORE the capture
    torch.cuda.synchronize()
    with slabs.no_gc(), <row-bound scopes>, torch.cuda.graph(g, pool, capture_error_mode="thread_local"): body()
    slabs.flush_table_uploads()                               pointer tables uploaded once, after the capture
    opt.use_eager_slot(); slabs.use_eager_param_grad_slot()   eager steps must never rewrite a graph's host image

and every replay of a step that holds Adam: sync_weight_copies(); g.replay(); weight_copies_after_replay(keys), keys being
what wcache.refresh_weight_t() returned inside the capture.
"""
import contextlib

import torch

from . import slabs, wcache


class CaptureSession:
    """`with CaptureSession(opt, device, pool) as s: with s.graph(scopes...) as g: body()` -- the slot dance once, around
    one or more graphs.  opt None: a capture without Adam (a plan graph, an evaluation), which takes no table slots;
    grad_slot=True with opt None: a backward pass without FlatAdam, which takes the weight-gradient slot only.  When the
    body raises, the eager slots are still restored (or FlatAdam._chunk_table and _SlabBatch._rotate_eager stop rotating
    and every later eager step rewrites one pinned image without waiting on its event) and the uploads the failed capture
    recorded are dropped, not performed."""

    def __init__(self, opt, device, pool=None, grad_slot=None):
        self.opt, self.device, self.pool = opt, device, pool
        self.grad_slot = (opt is not None) if grad_slot is None else grad_slot

    def __enter__(self):
        # outgrown workspaces are parked, not freed, from here on: a graph has their addresses baked in
        slabs.note_capture()
        self._pending = len(slabs._PENDING_UPLOADS)
        try:
            if self.opt is not None:
                self.opt.new_table_slot()       # this session's own (pinned) gradient chunk table
            if self.grad_slot:
                slabs.new_param_grad_slot(self.device)
            torch.cuda.synchronize()
        except BaseException:
            self._use_eager_slots()
            raise
        return self

    def _use_eager_slots(self):
        if self.opt is not None:
            self.opt.use_eager_slot()
        if self.grad_slot:
            slabs.use_eager_param_grad_slot()

    @contextlib.contextmanager
    def graph(self, *scopes):
        """Record one graph: no_gc, the caller's scopes (row bounds), then the capture.  thread_local: other threads of the
        process (the RCCL watchdog under DP) may issue HIP calls while this thread captures; they must not invalidate the
        capture."""
        g = torch.cuda.CUDAGraph()
        with contextlib.ExitStack() as stack:
            stack.enter_context(slabs.no_gc())
            for s in scopes:
                stack.enter_context(s)
            stack.enter_context(torch.cuda.graph(g, pool=self.pool, capture_error_mode="thread_local"))
            yield g

    def __exit__(self, exc_type, exc, tb):
        try:
            if exc_type is None:
                slabs.flush_table_uploads()      # the graphs' pointer tables: uploaded once, not at every replay
            else:
                del slabs._PENDING_UPLOADS[self._pending:]
        finally:
            self._use_eager_slots()
        return False


class CapturedStep:
    """A recorded step: its graph, the weight copies its captured refresh launch re-lays-out at every replay (`keys`; None
    when Adam runs outside the graph) and whatever the caller keeps with it (loss, prediction, the captured batch, ...)."""

    def __init__(self, graph, keys=None, **kept):
        self.graph, self.keys = graph, keys
        self.__dict__.update(kept)

    def replay(self):
        wcache.sync_weight_copies()          # parameters edited from outside since the last step (load_state_dict, ...)
        self.graph.replay()
        if self.keys is not None:
            wcache.weight_copies_after_replay(self.keys)


def optimizer_snapshot(opt, *extra):
    """Clones of the optimiser's state (and `extra` tensors) in front of warm-up steps that must not train."""
    return [t.clone() for t in (opt.flat_p, opt.m, opt.v, opt.step_dev, *extra)]


def optimizer_restore(opt, snap, *extra):
    for t, s in zip((opt.flat_p, opt.m, opt.v, opt.step_dev, *extra), snap):
        t.copy_(s)
    wcache.invalidate_weight_copies()
