"""One training step of a BaseCTRModel on the HIP path, as ONE HIP graph per step.

Step = the body of the reference's ``Trainer._train_epoch`` (trainer.py:212-240):
forward -> BCEWithLogits (+ L2 term) -> backward -> clip -> Adam, with the embedding
tables in row-sparse mode (``RowSparseAdam``).  Layout of one step on the stream:

    [graph A] fused embedding gather, reading the batch from its packed record and refreshing the
              step's static inputs on the way (``dfm_embedding_forward_staged``); row plan,
              interaction layers + DNN forward, loss, backward, row gradients;
              one rank: merge + clip + row-wise Adam + dense Adam as well
    [eager]   data-parallel exchange (RCCL all-gather), world_size > 1 only
    [graph B] merge + clip + row-wise Adam + dense Adam, world_size > 1 only

The batch changes every step and a graph's kernel arguments are frozen at capture, so the gather's
kernel NODE is re-pointed at the next batch record from the host before every launch
(``dfm_embedding_forward_staged`` with a ``dfm_launch`` naming the node -> hipGraphExecKernelNodeSetParams; nothing is
enqueued).  An
exec must not be updated while a launch of it may still be pending, so graph A is instantiated TWICE
and the two execs alternate: while one runs, the other — whose previous launch finished a whole step
ago — is updated and queued.  Measured on one MI355X: 0.216 ms/step against 0.225 with the gather
launched eagerly in front of the graph (two eager <-> graph transitions of ~10 us each disappear).
No host synchronisation inside a step beyond waiting for the launch before the previous one.

Timing the gather kernel: event-record NODES around it inside the graph cost ~5.5 us of device timeline
each and read 3 us more than the kernel runs (measured), so they are not used.  ``capture(timed_variant=
True)`` additionally captures the step WITHOUT its gather; ``run(eager_gather=True)`` then launches the
gather eagerly in front of that copy, where ``dfm_gather_timing_begin`` can attach start/stop events to
the dispatch itself.  bench.py does this on every 8th step of its timed region.
"""

from __future__ import annotations

import atexit
import contextlib
import dataclasses
import gc
import os
import weakref
from typing import List, Optional

import torch

from deepfm_amd import _lib
from deepfm_amd.data.packed import RecordLayout
from deepfm_amd.data.schema import FeatureType
from deepfm_amd.training.losses import bce_with_logits_mean
from deepfm_amd.training.rowsparse import RowSparseOptimizer


@contextlib.contextmanager
def capture_graph(graph: "torch.cuda.CUDAGraph", **kwargs):
    """``torch.cuda.graph(graph, **kwargs)`` with the cyclic garbage collector out of the way.  A dead reference cycle
    that still holds captured graphs (a dropped step object) is destroyed whenever the collector happens to run; inside
    a capture that means hipGraphExecDestroy / hipFree on the capturing thread, which the runtime refuses, and the
    destructor's failed check aborts the process.  torch.cuda.graph no longer collects on entry, so: collect before the
    capture begins and keep the collector off until it has ended."""
    gc.collect()
    was_enabled = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(graph, **kwargs):
            yield
    finally:
        if was_enabled:
            gc.enable()


# Arithmetic of the tower's backward GEMMs that bench.py / the tools select by default (dfm_tower_set_mode): the library
# itself starts in mode 0 and only changes on an explicit call.
TOWER_MODE_DEFAULT = 0

# Every live step, so that one call drops all captured graphs: graphs that hold captured RCCL kernels must be
# destroyed BEFORE the communicator (``destroy_process_group()`` under live graphs does not return — found on
# the one-GPU RCCL run).  Also registered with atexit, for processes that end on an exception.
_LIVE_STEPS: "weakref.WeakSet" = weakref.WeakSet()


def release_all_graphs() -> None:
    for step in list(_LIVE_STEPS):
        try:
            step.release_graphs()
        except Exception:      # teardown: best effort
            pass


atexit.register(release_all_graphs)


class GraphSlot:
    """One instantiated copy of a graph whose nodes are re-pointed before every launch."""

    def __init__(self, graph: "torch.cuda.CUDAGraph", at) -> None:
        self.graph = graph
        self.at = at                       # the launch destinations (``_lib.Launch``) of the nodes ``record`` returned
        self.done: Optional[torch.cuda.Event] = None      # recorded by the caller behind the slot's latest launch


class GraphPair:
    """Two instantiated copies of one graph, used in turn: an exec must not be updated while a launch of it may still
    be pending, so while one copy runs, the other — whose previous launch was enqueued a whole launch earlier — is
    re-pointed and queued.  ``record()`` enqueues the graph's work on the capturing stream and returns the nodes to
    re-point; ``at(graph_exec, nodes)`` turns them into launch destinations once (default: in the shape recorded)."""

    def __init__(self, record, at=_lib.at_nodes, **capture_mode) -> None:
        self.slots: List[GraphSlot] = []
        self._turn = 0
        for _ in range(2):
            # keep_graph: the captured graph stays alive, so the node handles stay valid for
            # hipGraphExecKernelNodeSetParams on the exec instantiated from it
            graph = torch.cuda.CUDAGraph(keep_graph=True)
            with capture_graph(graph, **capture_mode):
                nodes = record()
            graph.instantiate()
            self.slots.append(GraphSlot(graph, at(graph.raw_cuda_graph_exec(), nodes)))

    def next(self) -> GraphSlot:
        """The copy whose turn it is, safe to re-point: its previous launch (two launches ago) has left the device.
        The caller replays it and records ``slot.done`` behind the launch."""
        slot = self.slots[self._turn]
        self._turn ^= 1
        if slot.done is not None:
            slot.done.synchronize()
        else:
            slot.done = torch.cuda.Event()
        return slot


@dataclasses.dataclass
class _Captured:
    """What exists only while a step's graphs are captured.  The step holds one, or None when it runs eagerly."""
    start: GraphPair                       # graph A (per slot and step: (read destinations, apply destination, cur, target))
    cont: Optional[GraphPair]              # its "continuation" flavour: no plan node, the plan is in the hand-off set
    steps_per_graph: int
    plan_sets: Optional[list]              # [H, A, B] row-plan buffer sets of the look-ahead
    body_graph: Optional[torch.cuda.CUDAGraph]            # graph A without the gather (timed variant)
    graph_b: Optional[torch.cuda.CUDAGraph]
    prepared: Optional[GraphSlot] = None   # slot whose nodes prepare_group() has pointed at its records
    handoff_ptr: Optional[int] = None      # record (data_ptr) whose plan the previous launch left in the hand-off set


class RowSparseTrainStep:
    _main = None                  # the step this one is the tail step of (fused_step.py:make_tail_step)
    exchange_in_body = False      # True: the step's collectives are part of _gather / _body_a / _body_b themselves
    rowplan_first_default = True  # row plan + row touch in front of the gather (False: in line behind it, round 2's order)
    plan_lookahead_default = True # steps 2.. of a multi-step graph: the plan is built by the previous step's apply launch

    def __init__(self, model, optimizer: RowSparseOptimizer, batch_size: int, use_graph: bool = True) -> None:
        self.model, self.opt, self.B = model, optimizer, batch_size
        self.emb = model.embedding
        self._check_embedding()
        dev = optimizer.device
        specs = list(model.schema.fields.values())
        # one batch record (data/packed.py: [ids (S,B) int64 | dense (Dn,B) f32 | labels (B) f32]); three buffers of it:
        #   packed : the step's STATIC inputs (read by the row plan, the embedding backward, the loss) —
        #            written by the gather itself from the record it reads
        #   inbox  : where load_batch / load_packed put a batch that is not already a device record
        #   pad    : all-padding batch (id 0 everywhere) used by capture()'s warm-up
        lay = RecordLayout.of(model.schema, batch_size)      # (SEQUENCE bags: the mixed-schema step only)
        self.n_sparse, self.n_dense, self.packed_bytes = lay.n_sparse, lay.n_dense, lay.record_bytes
        self.packed = torch.zeros(self.packed_bytes, dtype=torch.uint8, device=dev)
        self.inbox = torch.zeros(self.packed_bytes, dtype=torch.uint8, device=dev)
        self.pad = torch.zeros(self.packed_bytes, dtype=torch.uint8, device=dev)
        self.ids, self.dense, self.labels, self.bags = lay.views(self.packed)
        self.in_ids, self.in_dense, self.in_labels, self.in_bags = lay.views(self.inbox)
        cols = {FeatureType.SPARSE: iter(self.ids), FeatureType.DENSE: iter(self.dense), FeatureType.SEQUENCE: iter(self.bags)}
        self.inputs: List[torch.Tensor] = [next(cols[s.feature_type]) for s in specs]
        self._rec_offsets = list(lay.field_offsets)   # byte offset of every field's input inside a batch record
        self._rec_labels = lay.labels_offset
        self._rec_id_offsets = [o for o, k in zip(lay.field_offsets, lay.kinds) if k is FeatureType.SPARSE]   # id columns
        # Row plan IN FRONT of the gather, on the batch record itself, with row-touch workgroups (csrc/rowplan.hip):
        # the sort keeps 26 CUs busy for ~13 us either way; here the other CUs use that time to pull the batch's ids
        # and table rows on-die, and the gather that follows no longer pays cold ids + three HBM round trips behind
        # the optimizer's dirty lines.  Same plan, same results; one more graph node re-pointed per step.
        self.rowplan_first = self.n_sparse > 0 and self.rowplan_first_default
        self._plan_done = False
        # Inside a graph of several steps, step k + 1's row plan (+ row touch) rides in step k's last optimizer launch
        # (dfm_step_apply_plan) instead of opening step k + 1: two sets of plan buffers alternate, and a third node per
        # step is re-pointed at launch.  Only the first step of a graph builds its plan in front of its gather.
        self.plan_lookahead = self.rowplan_first and self.plan_lookahead_default
        self._captured: Optional[_Captured] = None   # the graphs and their launch state (``_uncapture`` drops them)
        self._record: torch.Tensor = self.inbox       # batch record the next gather reads
        # The step's OWN row plan + row gradient buffers: the embedding keeps one ``rowsparse`` and replaces it when the
        # batch size changes, which would free buffers a captured graph of another step over the same model (its tail
        # step) still reads.  ``_enter`` installs them at every host entry point that reads ``emb.rowsparse``.
        # (A step whose lists come from another module, the field-sharded one, keeps that module's.)
        from deepfm_amd.models.layers.embedding import RowSparseBuffers
        self._rows = (RowSparseBuffers(self.n_sparse, self.emb.fm_embed_dim, batch_size, dev)
                      if self.n_sparse and self.emb.grad_mode == "rowsparse" and not self.exchange_in_body else None)
        self._tails: list = []                       # this step's tail steps
        F, D = len(specs), self.emb.fm_embed_dim
        self.fo = torch.empty(batch_size, 1, dtype=torch.float32, device=dev)
        self.fe = torch.empty(batch_size, F, D, dtype=torch.float32, device=dev)
        self.loss = torch.zeros((), dtype=torch.float32, device=dev)
        self.use_graph = use_graph
        self.dense_grads = {id(p): p.grad for p in self.emb.non_table_parameters() if p.grad is not None}
        self.emb.pin_plan(dev)             # the step holds raw parameter pointers from here on
        _LIVE_STEPS.add(self)
        for m in model.modules():          # DNN / head backward: accumulate straight into the flat .grad views
            if hasattr(m, "direct_grads"):
                m.direct_grads = True

    def _check_embedding(self) -> None:
        """The gradient mode this step's embedding backward needs (the mixed-schema step keeps ``dense``)."""
        if self.emb.grad_mode != "rowsparse":
            raise ValueError("RowSparseTrainStep needs model.embedding in 'rowsparse' grad mode")

    # the captured state under the names callers read (tools, tests, bench.py), and what an eager step shows instead
    slots = property(lambda self: self._captured.start.slots if self._captured else [])
    cont_slots = property(lambda self: self._captured.cont.slots if self._captured and self._captured.cont else [])
    steps_per_graph = property(lambda self: self._captured.steps_per_graph if self._captured else 1)
    _plan_sets = property(lambda self: self._captured.plan_sets if self._captured else None)
    body_graph = property(lambda self: self._captured.body_graph if self._captured else None)
    graph_b = property(lambda self: self._captured.graph_b if self._captured else None)

    # ------------------------------------------------------------------ inputs
    def load_batch(self, ids: torch.Tensor, dense: torch.Tensor, labels: torch.Tensor) -> None:
        """ids (S,B) int64, dense (Dn,B) float32, labels (B,) — device-to-device copies into the inbox
        record; the next ``run()`` trains on it."""
        if self.n_sparse:
            self.in_ids.copy_(ids, non_blocking=True)
        if self.n_dense:
            self.in_dense.copy_(dense, non_blocking=True)
        self.in_labels.copy_(labels, non_blocking=True)
        self._record = self.inbox

    def pack_batches(self, ids: torch.Tensor, dense: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
        """(n, S, B) int64, (n, Dn, B) f32, (n, B) f32 -> (n, packed_bytes) uint8 records for
        ``run_from`` (done once, outside any timed region)."""
        n = labels.shape[0]
        parts = []
        if self.n_sparse:
            parts.append(ids.contiguous().view(n, -1).view(torch.uint8))
        else:
            parts.append(torch.zeros(n, self.B * 8, dtype=torch.uint8, device=labels.device))
        if self.n_dense:
            parts.append(dense.contiguous().view(n, -1).view(torch.uint8))
        else:
            parts.append(torch.zeros(n, self.B * 4, dtype=torch.uint8, device=labels.device))
        parts.append(labels.contiguous().view(n, -1).view(torch.uint8))
        return torch.cat(parts, dim=1).contiguous()

    def load_packed(self, record: torch.Tensor) -> None:
        """One device-to-device copy of a pack_batches() record into the inbox."""
        self.inbox.copy_(record, non_blocking=True)
        self._record = self.inbox

    # ------------------------------------------------------------------ pieces
    def _gather_args(self) -> dict:
        """Extra outputs of the gather (subclasses: the fused step adds the FM value and S)."""
        return {}

    def _gather_call(self, record: torch.Tensor):
        base = record.data_ptr()
        return ([base + o for o in self._rec_offsets], self.inputs, self.B, self.fo, self.fe), \
            dict(extra_src_ptr=base + self._rec_labels, extra_dst=self.labels, **self._gather_args())

    def _plan_from_record(self, record: torch.Tensor) -> None:
        base = record.data_ptr()
        self.emb.build_rowplan(self.inputs, self.B, ids_ptrs=[base + o for o in self._rec_id_offsets], touch=True)
        self._plan_done = True

    def _siblings(self) -> list:
        """The other steps over this step's optimizer: its tail steps, or its main step and that one's other tails."""
        main = self._main if self._main is not None else self
        return [s for s in [main] + main._tails if s is not self]

    def _enter(self, rows=None) -> None:
        """Every host entry point that enqueues work or re-points a node starts here, before it writes anything.
        Nothing runs between ``prepare_group`` and ``launch_prepared``: while a prepared launch is pending on this
        step or on a sibling, every entry but ``launch_prepared`` (which takes its slot first) is refused, and the
        pending launch is left as it was.  Then this step's row buffers are installed as ``emb.rowsparse`` (``rows``:
        another set of its own, inside the capture of a graph with plan look-ahead), and the siblings' hand-offs are
        dropped: a row-plan hand-off never crosses steps."""
        others = self._siblings()
        for step in [self] + others:
            if step._captured is not None and step._captured.prepared is not None:
                raise RuntimeError("this step or another step over its optimizer has a prepared launch pending: call "
                                   "launch_prepared() on the step that prepared it first")
        if self._rows is not None:
            self.emb.rowsparse = self._rows if rows is None else rows
        for other in others:
            if other._captured is not None:
                other._captured.handoff_ptr = None

    def _gather(self, record: Optional[torch.Tensor] = None) -> None:
        record = self._record if record is None else record
        c = self._captured
        # the previous launch's last apply built this record's plan (hand-off set), or it is built here
        self._plan_done = self.rowplan_first and c is not None and c.handoff_ptr == record.data_ptr()
        if self.rowplan_first and not self._plan_done:
            self._plan_from_record(record)
        if c is not None:
            c.handoff_ptr = None
        a, kw = self._gather_call(record)
        self.emb.forward_staged(*a, **kw)

    def _capture_gather(self, record: torch.Tensor, with_plan: bool = True):
        """``_gather`` while the stream is being captured; returns the graph node(s) that read the batch
        record (``_update_gather`` re-points them before every launch, through the ``_lib.Launch`` built from each
        once the graph is instantiated): (gather node, row-plan node or None).
        ``with_plan`` False: the plan of this step was built by the previous step's apply launch (a step without a
        row plan in front of its gather ignores it)."""
        plan_node = None
        self._plan_done = self.rowplan_first and not with_plan
        if self.rowplan_first and with_plan:
            self._plan_from_record(record)
            plan_node = _lib.last_node()
        a, kw = self._gather_call(record)
        self.emb.forward_staged(*a, **kw)
        return (_lib.last_node(), plan_node)

    def _record_nodes(self, gather_nodes):
        """What ``_update_gather`` re-points, asked once the whole step is captured (mixed schemas: + the backward)."""
        return gather_nodes

    def _update_gather(self, at, record: torch.Tensor) -> None:
        at, plan_at = at
        if plan_at is not None:
            base = record.data_ptr()
            self.emb.build_rowplan(self.inputs, self.B, ids_ptrs=[base + o for o in self._rec_id_offsets], touch=True,
                                   at=plan_at)
        a, kw = self._gather_call(record)
        self.emb.forward_staged(*a, **kw, at=at)

    def _build_rowplan(self) -> None:
        """Row plan of the step's ids (sort / unique / segments per SPARSE field) — unless ``_gather`` already
        built it from the batch record (``rowplan_first``)."""
        if self._plan_done:
            self._plan_done = False
            return
        self.emb.build_rowplan(self.inputs, self.B)

    def _embedding_backward(self, g_fo: torch.Tensor, g_fe: torch.Tensor) -> None:
        """d first_order (B, 1), d field_embeddings (B, F, D) -> DENSE-field Linear gradients and one
        gradient row per distinct id (into the row buffers the step's entry point installed)."""
        self.emb.backward_rowsparse(self.inputs, g_fo, g_fe, self.dense_grads, dense_slices=self._dense_slices())

    def _dense_slices(self):
        """Batch-sliced DENSE-field gradients (see FeatureEmbedding.backward_rowsparse), or None."""
        return None

    def _body_a(self) -> None:
        self.opt.zero_grad()
        self._build_rowplan()              # in line (fused_step.py: a side stream measured slower, twice)
        fo = self.fo.detach().requires_grad_()
        fe = self.fe.detach().requires_grad_()
        logits = self.model._forward_components(fo, fe, fe.view(self.B, -1))
        # plain BCE: the L2 term (base.py:78-83) is applied as g += 2*l2*p by the optimizer
        loss = bce_with_logits_mean(logits.view(-1), self.labels)
        loss.backward()
        self.loss.copy_(loss.detach())
        self._embedding_backward(fo.grad, fe.grad)

    def _body_b(self) -> None:
        self.opt.apply()

    # ------------------------------------------------------------------ capture / run
    def _mutable_state(self) -> List[torch.Tensor]:
        """Everything a training step writes besides the table rows of the ids it is given: the flat dense
        parameter / moment / gradient buffers, step count, norm scalars, dropout seed, every module buffer
        (BatchNorm running statistics) and the static inputs."""
        opt = self.opt
        ts = [opt.flat_param, opt.flat_m, opt.flat_v, opt.flat_grad, opt.step_count, opt.sq_norm, opt.clip_coef,
              self.loss, self.packed]
        if opt.seed_tick is not None:
            ts.append(opt.seed_tick)
        seed = getattr(getattr(self.model, "dnn", None), "_seed", None)
        if seed is not None:
            ts.append(seed)
        ts += list(self.model.buffers())
        return ts

    def capture(self, warmup_iters: int = 1, timed_variant: bool = False, steps_per_graph: int = 1) -> None:
        """Capture the step's graphs after ``warmup_iters`` eager steps (``timed_variant``: also a copy of
        graph A without the gather, for ``run(eager_gather=True)``; ``steps_per_graph`` > 1: that many
        consecutive steps in one graph, launched with ``run_group`` — back-to-back graph launches are
        ~14 us apart on the device, whatever they contain).  Side-effect free: the warm-up
        steps run on an all-padding batch (id 0 everywhere: no table row receives a gradient, so the
        row-wise Adam touches nothing) and every other piece of state a step writes — dense parameters,
        Adam moments, step count, dropout seed, BatchNorm running statistics, the static inputs — is
        restored afterwards, bit for bit."""
        if not self.use_graph:
            return
        self._enter()
        self.release_graphs()              # a second capture starts from a step without captured launches
        state = self._mutable_state()
        saved = [t.clone() for t in state]
        try:
            self._captured = self._capture(warmup_iters, timed_variant, steps_per_graph)
        except BaseException:
            # a refused capture (e.g. a runtime that will not capture the collectives) built its graphs into locals,
            # but left the optimizer and the embedding mid-step: the caller may go on eagerly (bench.py does)
            self._uncapture()
            raise
        finally:
            # whatever happened, the warm-up steps' writes are undone, bit for bit
            torch.cuda.synchronize()
            with torch.no_grad():
                for t, v in zip(state, saved):
                    t.copy_(v)
            torch.cuda.synchronize()

    def _uncapture(self) -> None:
        """The one place that returns the step to "no captured launches": drops the graphs with their launch state,
        disarms the optimizer's plan look-ahead and puts the step's own row buffers back."""
        self._captured = None
        self.opt.next_plan = self.opt.plan_node = None
        if self._rows is not None:
            self.emb.rowsparse = self._rows
        self._plan_done = False

    def _capture(self, warmup_iters: int, timed_variant: bool, steps_per_graph: int) -> _Captured:
        """Builds every graph into locals: the caller publishes the result, so a capture that raises leaves nothing
        half-built in the step."""
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warmup_iters):
                self._gather(self.pad)
                self._body_a()
                self.opt.exchange()
                self._body_b()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        single = not self.opt.split
        # opt-in (DFM_DP_GRAPH_COLLECTIVE=1): capture the exchange inside the graph — one graph launch
        # per step under data parallelism.  Verified with a single-rank RCCL communicator only
        # (DFM_FORCE_DP_PATH=1); not validated on a multi-GPU box, hence not the default.
        # A step whose collectives sit inside its body (exchange_in_body: the field-sharded step) has no
        # split form: it is captured whole.
        fused_exchange = self.exchange_in_body or (
            (not single) and os.environ.get("DFM_DP_GRAPH_COLLECTIVE") == "1"
            and torch.distributed.is_initialized() and torch.distributed.get_backend() == "nccl")
        # thread_local capture mode: another thread (the RCCL watchdog polling its events under
        # data parallelism) must not invalidate the capture
        mode = dict(capture_error_mode="thread_local")
        def body():
            self._body_a()
            if single or fused_exchange:
                self.opt.exchange()          # one rank: no device work, selects the local row lists
                self._body_b()
        if steps_per_graph < 1 or (steps_per_graph > 1 and not single and not fused_exchange):
            raise ValueError("steps_per_graph > 1 needs the whole step inside one graph (one rank, or the in-graph exchange)")
        # plan look-ahead: whole steps in one graph, several of them, plan built from the batch record
        look = self.plan_lookahead and steps_per_graph > 1 and (single or fused_exchange) and self._rows is not None
        sets = None
        if look:
            # three sets of plan buffers: H ("hand-off": the plan a launch starts from — built by its own first node or
            # by the LAST apply of the previous launch) and A / B alternating inside the graph
            from deepfm_amd.models.layers.embedding import RowSparseBuffers
            rs = self._rows                                    # (the step's own: installed by capture()'s _enter)
            mk = lambda: RowSparseBuffers(rs.num_sparse, rs.dim, rs.batch, rs.row_g2.device)
            sets = [rs, mk(), mk()]                            # [H, A, B]
        ids0 = self.pad.data_ptr() + (self._rec_id_offsets[0] if self._rec_id_offsets else 0)

        def record_steps(cont: bool) -> list:
            steps = []
            for k in range(steps_per_graph):
                self._enter((sets[0] if k == 0 else sets[1 + (k - 1) % 2]) if look else None)
                gather_nodes = self._capture_gather(self.pad, with_plan=not (look and (k > 0 or cont)))
                apply_node = cur = target = None
                if look:
                    # this step's apply launch also builds the NEXT step's plan: the following step of the graph
                    # (other set), or — last step — the first step of the next launch (hand-off set)
                    target = sets[1 + k % 2] if k + 1 < steps_per_graph else sets[0]
                    self.opt.next_plan = (ids0, target)
                body()
                if target is not None:
                    apply_node = self.opt.plan_node        # (launches may follow it: the optimizer names the node)
                    cur = self.opt._cur
                steps.append((self._record_nodes(gather_nodes), apply_node, cur, target))
            return steps

        def at(ex, steps):
            return [(_lib.at_nodes(ex, read), _lib.at_nodes(ex, apply), cur, target) for read, apply, cur, target in steps]

        start = GraphPair(lambda: record_steps(False), at, **mode)
        # "continuation" flavour: no plan node, the plan is already in the hand-off set
        cont = GraphPair(lambda: record_steps(True), at, **mode) if look else None
        self._enter()                          # H: single steps (eager, timed variant) and every launch's first step
        body_graph = graph_b = None
        if timed_variant:
            body_graph = torch.cuda.CUDAGraph()
            with capture_graph(body_graph, **mode):
                self._plan_done = self.rowplan_first      # run(eager_gather=True) launches plan + gather eagerly in front
                body()
        if not single and not fused_exchange:
            self.opt.exchange()
            torch.cuda.synchronize()
            graph_b = torch.cuda.CUDAGraph()
            with capture_graph(graph_b, **mode):
                self._body_b()
        return _Captured(start, cont, steps_per_graph, sets, body_graph, graph_b)

    def release_graphs(self) -> None:
        """Drop every captured graph (the step runs eagerly afterwards).  Call before
        ``torch.distributed.destroy_process_group()`` when collectives were captured: the graphs hold the
        communicator's kernels, and tearing the communicator down under them does not return."""
        if self._captured is None:
            return
        torch.cuda.synchronize()
        self._uncapture()
        gc.collect()
        torch.cuda.synchronize()

    def run_from(self, record: torch.Tensor, eager_gather: bool = False) -> None:
        """One step on a ``pack_batches()`` record: the gather reads its inputs from the record and
        refreshes the static input buffers — ids, dense values, labels — the rest of the step reads.
        (A record that the previous ``run_group(..., next_record=record)`` planned for starts at its gather.)"""
        if record.numel() != self.packed_bytes or record.dtype != torch.uint8 or not record.is_contiguous():
            raise ValueError("run_from expects one contiguous pack_batches() record")
        if record.data_ptr() % 16:
            raise ValueError("batch records must be 16-byte aligned")
        self._enter()
        self._record = record
        self._run(eager_gather)

    def run(self, eager_gather: bool = False) -> None:
        self._enter()
        self._run(eager_gather)

    def _run(self, eager_gather: bool) -> None:
        c = self._captured
        if c is None:
            self._gather()
            self._body_a()
            self.opt.exchange()
            self._body_b()
            return
        if eager_gather:
            if c.body_graph is None:
                raise RuntimeError("run(eager_gather=True) needs capture(timed_variant=True)")
            self._gather()                 # eager: dfm_gather_timing_begin may attach events to this dispatch
            c.body_graph.replay()          # (its apply plans for nobody: the next launch builds its own plan)
            self._after_graph_a(None)
            return
        if c.steps_per_graph != 1:
            raise RuntimeError(f"the graphs hold {c.steps_per_graph} steps each: use run_group()")
        self._launch([self._record])

    def run_group(self, records, next_record: Optional[torch.Tensor] = None) -> None:
        """``steps_per_graph`` consecutive steps, one graph launch: ``records[k]`` is step k's batch record.
        ``next_record`` (optional): the record the NEXT launch (``run_group`` or ``run_from``) starts with — this
        launch's last optimizer kernel then builds its row plan, and the next launch starts at its gather.  The
        hand-off is keyed by the record's address: a record announced here must not be rewritten in place until the
        launch that consumes it has been issued, or that launch starts from the plan of the ids it held before."""
        if len(records) != self.steps_per_graph:
            raise ValueError(f"run_group expects {self.steps_per_graph} records")
        if self._captured is None:
            for r in records:
                self.run_from(r)
            return
        for r in records:
            if r.numel() != self.packed_bytes or r.dtype != torch.uint8 or not r.is_contiguous() or r.data_ptr() % 16:
                raise ValueError("run_group expects contiguous, 16-byte aligned pack_batches() records")
        self._launch(list(records), next_record)

    def prepare_group(self, records, next_record: Optional[torch.Tensor] = None) -> None:
        """The host half of ``run_group``: picks the graph copy, waits for its last launch and points its nodes at
        ``records`` — everything but the launch itself, which ``launch_prepared()`` does.  A training loop calls this
        for launch k + 1 while launch k is on the device (two copies of the graph alternate for that); ``run_group``
        is the two calls back to back.  Until ``launch_prepared()`` every other entry of this step and of its
        siblings raises ``RuntimeError`` (``_enter``)."""
        if len(records) != self.steps_per_graph or self._captured is None:
            raise ValueError(f"prepare_group needs captured graphs of {len(records)} steps")
        self._captured.prepared = self._prepare(list(records), next_record)

    def launch_prepared(self) -> None:
        c = self._captured
        if c is None or c.prepared is None:
            raise RuntimeError("nothing prepared")
        slot, c.prepared = c.prepared, None
        self._enter()
        slot.graph.replay()
        self._after_graph_a(slot.done)

    def _launch(self, records, next_record: Optional[torch.Tensor] = None) -> None:
        slot = self._prepare(records, next_record)
        slot.graph.replay()
        self._after_graph_a(slot.done)

    def _prepare(self, records, next_record: Optional[torch.Tensor] = None) -> GraphSlot:
        self._enter()
        c = self._captured
        cont = c.cont is not None and c.handoff_ptr == records[0].data_ptr()
        slot = (c.cont if cont else c.start).next()
        for k, ((read_at, apply_at, cur, target), rec) in enumerate(zip(slot.at, records)):
            self._update_gather(read_at, rec)
            if apply_at is not None:         # step k's apply launch sorts the next step's ids: point it at that record
                nxt = records[k + 1] if k + 1 < len(records) else (next_record if next_record is not None else records[0])
                self.opt.apply_plan(cur, nxt.data_ptr() + self._rec_id_offsets[0], target, apply_at)
        c.handoff_ptr = next_record.data_ptr() if (next_record is not None and c.cont is not None) else None
        return slot

    def _after_graph_a(self, done) -> None:
        if self.graph_b is not None:
            # the replay produced the row gradients; the Python-side flag was only set while
            # the graph was being captured
            self.emb.rowsparse.has_grad = True
            self.opt.exchange()
            self.graph_b.replay()
        if done is not None:
            done.record()
