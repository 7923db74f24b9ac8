"""RowSparseAdam / RowSparseAdamW / RowSparseSGD: the optimizer half of the row-sparse fast mode.

Reference step (``deepfm/training/trainer.py:212-240``): BCE + ``get_l2_reg_loss`` ->
backward -> ``clip_grad_norm_`` over all parameters -> dense ``Adam``.  At the Criteo
shape 98 % of that step is dense full-table traffic.  Here the (V, d)
tables are updated only on the rows the (global) batch touched:

    g_row = grad_scale * sum(contributions) + 2*l2*w_row        (lazy L2, base.py:78-83)
    clip  = min(1, max_norm / (||all grads|| + 1e-6))            (trainer.py:232-235)
    Adam(w_row, m_row, v_row, clip * g_row)                      (trainer.py:67-70,237)

All other parameters (DENSE-field Linears, DNN, heads, CIN, attention) live in ONE flat
buffer (each ``nn.Parameter`` becomes a view of it) and take a dense Adam step from one
kernel; the L2 term of the embedding's dense parameters is added to their gradient there
(``g += 2*l2*p``), so the training loss passed to ``backward`` is the plain BCE.
This is NOT trajectory-identical to the reference's dense Adam (untouched rows do not
move); DESIGN.md states the delta.  Everything runs on the current stream with no host
synchronisation, so a whole step can be captured in a HIP graph.

The update rule is the optimizer's kind (``training.optimizer``, trainer.py:67-78): ``adam``, ``adamw``
(``p *= 1 - lr*wd`` before the Adam update) or ``sgd`` (momentum buffer ``buf = mu*buf + g``, ``p -= lr*buf``,
kept where Adam's first moment lives; no second moment).  Row-wise updates are lazy for every kind: only touched
rows decay or move.  The learning rate lives on the device (one fp32 scalar read by every apply launch), so a
change of ``opt.lr`` reaches captured graphs too.

Data parallel (one process per GPU, tables replicated): the flat dense gradient is
all-reduced, the row lists (ids + gradient rows) are all-gathered, and every rank runs
the same deterministic merge (``csrc/tail_bodies.h``) so replicas stay bit-identical.
"""

from __future__ import annotations

import ctypes as C
from typing import Optional

import torch
import torch.distributed as dist

from deepfm_amd import _lib
from deepfm_amd.data.schema import FeatureType
from deepfm_amd.training import exchange
from deepfm_amd.models.layers.embedding import FeatureEmbedding


_KIND_CODE = {"adam": _lib.OPT_ADAM, "adamw": _lib.OPT_ADAMW, "sgd": _lib.OPT_SGD}


class RowSparseOptimizer:
    """Shared body of the row-sparse optimizers; the subclasses fix the update rule (``kind``).

    Learning rate: ``opt.lr`` (and ``opt.param_groups[0]["lr"]``, for code written against torch) reads a host
    mirror; setting it writes the device scalar every apply launch reads, with a stream-ordered fill on the current
    stream.  A change takes effect at the next ``run`` or graph launch, eager or captured, look-ahead or not; all
    steps inside one multi-step graph launch share the learning rate.  It may not be set while the current stream
    is capturing."""
    kind = "adam"
    row_tables = True        # False (training/dense_table.py): the tables are dense parameters of the flat buffer too

    def __init__(self, model: torch.nn.Module, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 l2: float = 0.0, max_grad_norm: Optional[float] = None,
                 process_group: Optional[dist.ProcessGroup] = None,
                 row_embedding: Optional[FeatureEmbedding] = None, weight_decay: float = 0.0,
                 momentum: float = 0.0) -> None:
        emb = model.embedding
        if not isinstance(emb, FeatureEmbedding):
            raise ValueError("model.embedding must be a FeatureEmbedding")
        if self.row_tables and emb.grad_mode != "rowsparse":
            raise ValueError("model.embedding must be a FeatureEmbedding in 'rowsparse' grad mode")
        self.model, self.emb = model, emb
        self.row_emb = row_embedding if row_embedding is not None else emb
        self.betas, self.eps, self.l2 = tuple(betas), eps, l2
        self.weight_decay, self.momentum = float(weight_decay), float(momentum)
        self.max_grad_norm = max_grad_norm
        self.group = process_group
        self.world = exchange.world_size(process_group)
        # DFM_FORCE_DP_PATH=1 with an initialised (even single-rank) process group: take the N > 1 code
        # path — two graphs around eager collectives — so that RCCL and its interplay with graph capture
        # can be exercised on a one-GPU box
        import os
        self.split = self.world > 1 or (os.environ.get("DFM_FORCE_DP_PATH") == "1" and dist.is_available()
                                        and dist.is_initialized())

        tables = self.row_emb.table_parameters() if self.row_tables else []
        if self.row_tables and not tables:
            raise ValueError("no SPARSE tables to optimise")
        anchor = tables[0] if tables else next(emb.parameters())
        dev = anchor.device
        _lib.require_device(anchor, "embedding tables")
        self.device = dev
        # [clip coefficient | learning rate] in one 64-byte line: the apply launch reads both, and the clip
        # coefficient is rewritten every step (dfm_grad_norm_finalize), so the learning rate's line is never cold
        self._scalars = torch.zeros(16, dtype=torch.float32, device=dev)
        self._lr_dev = self._scalars[1:2]      # read by every apply launch
        self.lr = lr
        self.num_sparse = len(tables) // 2
        self.dim = emb.fm_embed_dim
        # Adam moments (SGD: the momentum buffer in exp_avg, no exp_avg_sq): inside the packed row records when
        # the embedding was packed (FeatureEmbedding.pack_tables_), else separate contiguous tensors
        second = self.kind != "sgd"
        self.exp_avg, self.exp_avg_sq = [], []
        sparse_names = [n for n, spec in self.row_emb.schema.fields.items() if spec.feature_type is FeatureType.SPARSE]
        for name, w2, w1 in zip(sparse_names, tables[0::2], tables[1::2]):
            rec = self.row_emb.packed.get(name) if getattr(self.row_emb, "packed", None) else None
            if rec is not None and rec["buffer"].data_ptr() == w2.data_ptr():
                self.exp_avg += [rec["m2"], rec["m1"]]
                self.exp_avg_sq += [rec["v2"], rec["v1"]] if second else [None, None]
            else:
                self.exp_avg += [torch.zeros_like(w2, memory_format=torch.contiguous_format),
                                 torch.zeros_like(w1, memory_format=torch.contiguous_format)]
                self.exp_avg_sq += ([torch.zeros_like(w2, memory_format=torch.contiguous_format),
                                     torch.zeros_like(w1, memory_format=torch.contiguous_format)] if second
                                    else [None, None])
        self._tables = tables
        self.step_count = torch.zeros(1, dtype=torch.int32, device=dev)
        self.sq_norm = torch.zeros(1, dtype=torch.float32, device=dev)
        self.clip_coef = self._scalars[0:1]
        self.clip_coef.fill_(1.0)

        # dense parameters: ONE flat parameter buffer and ONE flat gradient buffer; every
        # parameter / .grad becomes a view (embedding parameters first: they take the L2 term)
        table_ids = {id(p) for p in tables} | ({id(p) for p in emb.table_parameters()} if self.row_tables else set())
        emb_dense = [p for p in (emb.non_table_parameters() if self.row_tables else emb.parameters()) if p.requires_grad]
        emb_ids = {id(p) for p in emb_dense}
        others = [p for p in model.parameters()
                  if id(p) not in table_ids and id(p) not in emb_ids and p.requires_grad]
        # modules may ask for groups of parameters to lie back to back (attention: W_q | W_k | W_v as one
        # stacked weight without a copy): each group moves, in its order, to where its first member is
        groups = [g for m in model.modules() if hasattr(m, "adjacent_parameters") for g in m.adjacent_parameters()]
        for g in groups:
            ids = {id(p) for p in g}
            if all(any(p is q for q in others) for p in g):
                first = min(i for i, q in enumerate(others) if id(q) in ids)
                rest = [q for q in others if id(q) not in ids]
                first -= sum(1 for q in others[:first] if id(q) in ids)
                others = rest[:first] + list(g) + rest[first:]
        self.dense_params = emb_dense + others
        # every parameter starts on a 64-byte boundary (16 floats) so kernels can use 16-byte
        # vector loads on the views; the padding stays 0 (zero grad -> zero Adam update)
        def padded(n):
            return (n + 15) // 16 * 16
        self.n_l2 = sum(padded(p.numel()) for p in emb_dense)
        total = sum(padded(p.numel()) for p in self.dense_params)
        self.flat_param = torch.zeros(total, dtype=torch.float32, device=dev)
        self.flat_grad = torch.zeros(total, dtype=torch.float32, device=dev)
        self.flat_m = torch.zeros(total, dtype=torch.float32, device=dev)
        self.flat_v = torch.zeros(total if second else 16, dtype=torch.float32, device=dev)   # (SGD: unused)
        off = 0
        for p in self.dense_params:
            n = p.numel()
            self.flat_param[off:off + n].copy_(p.data.reshape(-1))
            p.data = self.flat_param[off:off + n].view_as(p)
            p.grad = self.flat_grad[off:off + n].view_as(p)
            off += padded(n)
        self._owner = None
        self._workspaces: dict = {}      # per list shape: (_owner, _partials, _match), see _workspace()
        self.plan_node = None            # graph node of the last apply launch captured with a plan (dfm_step_apply_plan)
        self.next_plan = None            # (next batch's ids pointer, target RowSparseBuffers): set by the step, see apply()
        self._vocab_dev, self._max_vocab = None, 0
        specs = list(self.row_emb.schema.fields.values())
        vocab = [specs[i].vocabulary_size for i in self.row_emb._sparse_pos] if self.row_tables else []
        if vocab:                            # vocabulary sizes on the device, for dfm_step_apply_plan (not creatable under capture)
            self._vocab_dev = torch.tensor(vocab, dtype=torch.int32, device=self.device)
            self._max_vocab = max(vocab)
        self._gathered = None
        self._partials = None
        self._match = None
        self._cur = None
        self.seed_tick: Optional[torch.Tensor] = None    # int64 device counter advanced once per apply()
        # (dfm_slab_ref[], count): d-weight slabs of dfm_linear_backward that apply() folds into the flat
        # gradient (single rank only: under data parallelism they must be in before the all-reduce)
        self.slab_refs = None

    # ------------------------------------------------------------------ learning rate
    @property
    def lr(self) -> float:
        return self._lr

    @lr.setter
    def lr(self, value: float) -> None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("the learning rate cannot be changed inside a graph capture (set it between launches)")
        self._lr = float(value)
        self._lr_dev.fill_(self._lr)         # stream-ordered: steps enqueued after this see the new value

    @property
    def param_groups(self):
        """``[{"lr": ...}]``: a view for code that reads / sets ``optimizer.param_groups[0]["lr"]``."""
        return [_LrGroup(self)]

    def _optim_struct(self) -> "_lib.Optim":
        o = _lib.Optim()
        o.kind = _KIND_CODE[self.kind]
        o.beta1, o.beta2, o.eps = self.betas[0], self.betas[1], self.eps
        o.weight_decay, o.momentum = self.weight_decay, self.momentum
        o.d_lr = self._lr_dev.data_ptr()
        return o

    # ------------------------------------------------------------------ helpers
    def zero_grad(self, force: bool = False) -> None:
        """``optimizer.zero_grad()`` (trainer.py:219).  The buffer starts zeroed and ``apply()``
        leaves it zeroed (the Adam kernel clears what it consumed), so no fill is launched; pass
        ``force=True`` to discard gradients accumulated by a backward pass that was not applied."""
        if force:
            self.flat_grad.zero_()
        if self.row_emb.rowsparse is not None:
            self.row_emb.rowsparse.has_grad = False

    def _table_struct(self):
        arr = (_lib.Table * self.num_sparse)()
        for s in range(self.num_sparse):
            t = arr[s]
            t.w2, t.w1 = self._tables[2 * s].data_ptr(), self._tables[2 * s + 1].data_ptr()
            t.m2, t.m1 = self.exp_avg[2 * s].data_ptr(), self.exp_avg[2 * s + 1].data_ptr()
            t.v2, t.v1 = _lib.ptr(self.exp_avg_sq[2 * s]), _lib.ptr(self.exp_avg_sq[2 * s + 1])
            t.stride2, t.stride1 = self._tables[2 * s].stride(0), self._tables[2 * s + 1].stride(0)
            for a, b in ((self.exp_avg[2 * s], t.stride2), (self.exp_avg_sq[2 * s], t.stride2),
                         (self.exp_avg[2 * s + 1], t.stride1), (self.exp_avg_sq[2 * s + 1], t.stride1)):
                if a is not None and a.stride(0) != b:
                    raise RuntimeError("Adam state and table row strides differ (re-create the optimizer after "
                                       "pack_tables_() / .to())")
        return arr

    # ------------------------------------------------------------------ step
    @torch.no_grad()
    def exchange(self) -> None:
        """Data-parallel gradient exchange (no-op for one rank): all-reduce of the flat dense
        gradient, all-gather of the row lists.  Plain RCCL collectives on the current stream."""
        rs = self.row_emb.rowsparse
        if rs is None or not rs.has_grad:
            raise RuntimeError(f"{type(self).__name__}: no row gradients (run a backward pass first)")
        local = (rs.uniq_rows, rs.num_uniq, rs.row_g2, rs.row_g1)
        if not self.split:
            self._cur = local + (rs.chunks,)
            return
        # one grouped all-gather: [dense gradient buffer | row lists]; the dense mean over ranks is formed
        # by the optimizer's prepare launch in rank order (no all-reduce, no scaling launch)
        world = max(self.world, 1)
        full = (self.flat_grad.view(1, -1),) + local
        if self._gathered is None or self._gathered[1].shape[0] != world * rs.chunks:
            self._gathered = exchange.alloc_gathered(full, world)
        exchange.allgather_step(full, self._gathered, self.group)
        self._cur = self._gathered[1:] + (world * rs.chunks,)

    @torch.no_grad()
    def apply(self, row_sq=None) -> None:
        """Merge lists, L2 + global norm + clip, the update rule row-wise on the tables and on the flat
        dense buffer: three kernel launches, no host synchronisation.  ``row_sq`` (a step that tracks the epoch's
        loss): (old, new) float64 partial buffers that take the sum of squares of the rows this step owns, before and
        after their update (``dfm_rows_sqnorm``: two more launches)."""
        lib = _lib.load()
        stream = _lib.stream_handle()
        grad_scale = 1.0 / self.world
        uniq, num, g2, g1, lists = self._cur
        n_dense = self.flat_param.numel()
        n_partials = lib.dfm_step_prepare_num_partials(self.num_sparse, self.dim, lists, n_dense)
        self._owner, self._partials, self._match = self._workspace(uniq, lists, n_partials)
        dense_gathered, gathered_stride = self._dense_source()
        tabs = self._table_struct()
        refs, n_refs = self.slab_refs if (self.slab_refs is not None and not self.split) else (None, 0)
        # three launches: [row-list merge | dense L2 (+ d-weight slabs) + norm partials] -> clip coefficient
        # (+ step / seed tick) -> [row-wise Adam | dense Adam (+ clears the gradient buffer)]
        _lib.check(lib.dfm_step_prepare(tabs, self.num_sparse, self.dim, lists, uniq.data_ptr(), num.data_ptr(),
                                        g2.data_ptr(), g1.data_ptr(), self._owner.data_ptr(), grad_scale, self.l2,
                                        self.flat_grad.data_ptr(), self.flat_param.data_ptr(), n_dense, self.n_l2,
                                        refs, n_refs, _lib.ptr(dense_gathered), max(self.world, 1), gathered_stride,
                                        self._partials.data_ptr(), self._dense_partial_offset(lists),
                                        _lib.ptr(self._match), stream))
        norm_ptr, n_norm = self._norm_partials(n_partials, lists)
        _lib.check(lib.dfm_grad_norm_finalize(norm_ptr, n_norm,
                                              self.max_grad_norm or 0.0, self.sq_norm.data_ptr(),
                                              self.clip_coef.data_ptr(), self.step_count.data_ptr(),
                                              _lib.ptr(self.seed_tick), stream))
        if row_sq is not None:
            self._rows_sqnorm(tabs, row_sq[0])       # behind the prepare launch (owner flags), in front of the update
        if self.next_plan is not None:
            # the row plan (+ row touch) of the NEXT step rides in this launch (csrc/step_tail.hip)
            ids_ptr, target = self.next_plan
            self.next_plan = None
            self.apply_plan(self._cur, ids_ptr, target)
            if torch.cuda.is_current_stream_capturing():
                self.plan_node = _lib.last_node()
        else:
            _lib.check(lib.dfm_step_apply(*self._apply_args(tabs, self._cur), stream))
        if row_sq is not None:
            self._rows_sqnorm(tabs, row_sq[1])
        self.row_emb.rowsparse.has_grad = False

    def _workspace(self, uniq: torch.Tensor, lists: int, n_partials: int):
        """The per-launch workspaces (owner flags, norm partials, match bytes) of lists shaped like ``uniq``: kept per
        shape, because two steps of different batch sizes over this optimizer (a step and its tail step) alternate,
        and captured graphs of either hold the addresses."""
        ws = self._workspaces.get(uniq.shape)
        if ws is None:
            lib = _lib.load()
            mbytes = lib.dfm_step_match_bytes(self.num_sparse, lists)
            ws = self._workspaces[uniq.shape] = (
                torch.empty_like(uniq),
                torch.zeros(n_partials + self._extra_partial_count(lists), dtype=torch.float32, device=self.device),
                torch.empty(mbytes, dtype=torch.uint8, device=self.device) if mbytes else None)
        return ws

    def _rows_sqnorm(self, tabs, partials: torch.Tensor) -> None:
        uniq, num, _, _, lists = self._cur
        _lib.check(_lib.load().dfm_rows_sqnorm(tabs, self.num_sparse, self.dim, lists, uniq.data_ptr(), num.data_ptr(),
                                               self._owner.data_ptr(), partials.data_ptr(), partials.numel(),
                                               _lib.stream_handle()))

    def _apply_args(self, tabs, cur):
        """The arguments every apply entry point takes, ``tables`` ... ``zero_grad``: ``tabs`` = this optimizer's
        ``_table_struct()``, ``cur`` = this step's lists (``_cur``)."""
        uniq, num, g2, g1, lists = cur
        return (tabs, self.num_sparse, self.dim, lists, uniq.data_ptr(), num.data_ptr(), g2.data_ptr(), g1.data_ptr(),
                self._workspaces[uniq.shape][0].data_ptr(), self.clip_coef.data_ptr(), C.byref(self._optim_struct()),
                self.step_count.data_ptr(), self.flat_param.data_ptr(), self.flat_m.data_ptr(), self._flat_v_ptr(),
                self.flat_grad.data_ptr(), self.flat_param.numel(), 1)

    def apply_plan(self, cur, ids_ptr: int, target, at: Optional[_lib.Launch] = None) -> None:
        """dfm_step_apply_plan: ``cur`` = this step's lists (``_cur``), ``ids_ptr`` = device address of the next
        batch's (S, B) int64 id columns, ``target`` = the RowSparseBuffers the next step's plan goes to.  ``at``: None
        enqueues on the current stream; ``_lib.at_node(graph_exec, node)`` re-points the captured launch at the next
        launch's record (host-side only; refused by the library when the node was captured for another update
        rule)."""
        if self._vocab_dev is None:
            raise RuntimeError(f"{type(self).__name__}: no SPARSE fields to plan for")
        tabs = self._table_struct()
        B = target.batch
        _lib.check(_lib.load().dfm_step_apply_plan(
            *self._apply_args(tabs, cur), ids_ptr, B, self._vocab_dev.data_ptr(), self._max_vocab, B,
            target.sorted_pos.data_ptr(), target.uniq_rows.data_ptr(), target.seg_start.data_ptr(),
            target.num_uniq.data_ptr(), self.row_emb._err.data_ptr(), at or _lib.stream_handle()))

    def _flat_v_ptr(self) -> int:
        return self.flat_v.data_ptr() if self.kind != "sgd" else 0

    def _dense_source(self):
        """(every rank's dense gradient buffer, floats between ranks) for the prepare launch's rank-ordered
        mean, or (None, 0): the local flat gradient is the whole gradient."""
        if (self.split and self._gathered is not None and self._cur is not None
                and self._cur[0] is self._gathered[1]):
            return self._gathered[0], 0
        return None, 0

    def _extra_partial_count(self, lists: int) -> int:
        """Floats kept free behind the norm partials (subclasses that exchange partial norms)."""
        return 0

    def _dense_partial_offset(self, lists: int) -> int:
        """Where the dense buffer's norm partials start in ``_partials`` (0: right behind the row partials)."""
        return 0

    def _norm_partials(self, n_partials: int, lists: int):
        """(address, count) of the floats whose sum is the squared global gradient norm."""
        return self._partials.data_ptr(), n_partials

    def step(self) -> None:
        self.exchange()
        self.apply()

    # ------------------------------------------------------------------ checkpointing
    def _table_state(self):
        """[(table parameter, exp_avg, exp_avg_sq)] of every table a checkpoint covers."""
        return list(zip(self._tables, self.exp_avg, self.exp_avg_sq))

    def _named(self):
        names = {id(p): n for n, p in self.model.named_parameters()}
        return ([(names[id(p)], m, v) for p, m, v in self._table_state()],
                [(names[id(p)], p) for p in self.dense_params])

    def _slots(self):
        """Names of the per-parameter state tensors, as torch's optimizer of this kind names them."""
        return ("momentum_buffer",) if self.kind == "sgd" else ("exp_avg", "exp_avg_sq")

    def state_dict(self) -> dict:
        """Optimizer state keyed by parameter NAME, each entry shaped like the parameter and named like
        torch's per-parameter state (Adam / AdamW: ``exp_avg`` / ``exp_avg_sq``; SGD: ``momentum_buffer``),
        the shared step count, and the hyper-parameters (``hyper["kind"]`` names the update rule)."""
        tables, dense = self._named()
        slots = self._slots()
        state = {}
        for name, m, v in tables:
            arrays = (m,) if self.kind == "sgd" else (m, v)
            state[name] = {k: a.detach().clone().contiguous() for k, a in zip(slots, arrays)}
        off = 0
        for name, p in dense:
            n = p.numel()
            arrays = (self.flat_m,) if self.kind == "sgd" else (self.flat_m, self.flat_v)
            state[name] = {k: a[off:off + n].view_as(p).clone() for k, a in zip(slots, arrays)}
            off += (n + 15) // 16 * 16
        return {"step": int(self.step_count.item()), "state": state,
                "hyper": {"kind": self.kind, "lr": self.lr, "betas": list(self.betas), "eps": self.eps,
                          "weight_decay": self.weight_decay, "momentum": self.momentum, "l2": self.l2,
                          "max_grad_norm": self.max_grad_norm}}

    @staticmethod
    def _torch_kind(group: dict) -> str:
        """The update rule of a torch optimizer's param group: SGD has ``momentum`` and no ``betas``; AdamW is Adam
        with ``decoupled_weight_decay`` (torch >= 2.6 writes the flag; older AdamW groups are told by their
        non-zero weight decay, which the reference's Adam(lr) never sets)."""
        if "betas" not in group:
            return "sgd"
        if "decoupled_weight_decay" in group:
            return "adamw" if group["decoupled_weight_decay"] else "adam"
        return "adamw" if group.get("weight_decay", 0.0) else "adam"

    def load_state_dict(self, sd: dict) -> None:
        """This optimizer's own ``state_dict()``, or the ``state_dict()`` of the torch optimizer of the same kind
        (``torch.optim.Adam`` / ``AdamW`` / ``SGD``) over ``model.parameters()`` — what the reference's trainer
        writes as ``optimizer_state_dict`` (trainer.py:140-148; position-keyed ``state`` + ``param_groups``):
        state is matched to parameters by position in ``model.named_parameters()``; parameters torch never stepped
        get zeros (SGD state has no ``step``).  A state dict of another kind is refused (ValueError).  The
        learning rate is restored when the state dict carries one (``param_groups[0]["lr"]`` / ``hyper["lr"]``)."""
        slots = self._slots()
        lr = None
        if "param_groups" in sd:
            kinds = {self._torch_kind(g) for g in sd["param_groups"]}
            if kinds != {self.kind}:
                raise ValueError(f"{type(self).__name__} cannot load the state of a torch {'/'.join(sorted(kinds))} "
                                 f"optimizer")
            lr = sd["param_groups"][0].get("lr")
            names = [n for n, _ in self.model.named_parameters()]
            order = [i for g in sd["param_groups"] for i in g["params"]]
            if len(order) != len(names):
                raise KeyError(f"torch optimizer state covers {len(order)} parameters, the model has {len(names)}")
            shapes = dict(self.model.named_parameters())
            state, step = {}, 0
            for i, name in zip(order, names):
                st = sd["state"].get(i)
                if st is None or any(k not in st for k in slots):
                    state[name] = {k: torch.zeros_like(shapes[name], memory_format=torch.contiguous_format)
                                   for k in slots}
                else:
                    state[name] = {k: st[k] for k in slots}
                if st is not None and "step" in st:
                    step = max(step, int(st["step"]))
            sd = {"step": step, "state": state}
        else:
            hyper = sd.get("hyper", {})
            kind = hyper.get("kind", "adam")         # (state dicts written before the kinds existed are Adam's)
            if kind != self.kind:
                raise ValueError(f"{type(self).__name__} cannot load the state of a row-sparse {kind} optimizer")
            lr = hyper.get("lr")
        tables, dense = self._named()
        want = {n for n, _, _ in tables} | {n for n, _ in dense}
        if set(sd["state"]) != want:
            raise KeyError(f"optimizer state keys differ: {sorted(set(sd['state']) ^ want)[:5]} ...")
        with torch.no_grad():
            for name, m, v in tables:
                m.copy_(sd["state"][name][slots[0]])
                if self.kind != "sgd":
                    v.copy_(sd["state"][name][slots[1]])
            off = 0
            for name, p in dense:
                n = p.numel()
                self.flat_m[off:off + n].copy_(sd["state"][name][slots[0]].reshape(-1))
                if self.kind != "sgd":
                    self.flat_v[off:off + n].copy_(sd["state"][name][slots[1]].reshape(-1))
                off += (n + 15) // 16 * 16
            self.step_count.fill_(int(sd["step"]))
        if lr is not None:
            self.lr = float(lr)


class _LrGroup(dict):
    """``param_groups[0]`` of a row-sparse optimizer: ``["lr"]`` reads and sets ``opt.lr``."""

    def __init__(self, opt: RowSparseOptimizer) -> None:
        super().__init__(lr=opt.lr)
        self._opt = opt

    def __getitem__(self, key):
        return self._opt.lr if key == "lr" else super().__getitem__(key)

    def __setitem__(self, key, value) -> None:
        if key == "lr":
            self._opt.lr = value
        super().__setitem__(key, value)


class RowSparseAdam(RowSparseOptimizer):
    """torch.optim.Adam semantics (trainer.py:67-70) on the row-sparse step."""
    kind = "adam"

    def __init__(self, model: torch.nn.Module, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 l2: float = 0.0, max_grad_norm: Optional[float] = None,
                 process_group: Optional[dist.ProcessGroup] = None,
                 row_embedding: Optional[FeatureEmbedding] = None) -> None:
        """``row_embedding``: the module whose SPARSE tables take the row-wise updates and whose row
        lists (``.rowsparse``) feed them — ``model.embedding`` unless the tables are field-sharded
        (training/sharded.py passes this rank's shard, whose tables are the model's own Parameters)."""
        super().__init__(model, lr=lr, betas=betas, eps=eps, l2=l2, max_grad_norm=max_grad_norm,
                         process_group=process_group, row_embedding=row_embedding)


class RowSparseAdamW(RowSparseOptimizer):
    """torch.optim.AdamW semantics (trainer.py:71-72; torch's default ``weight_decay=0.01``): ``p *= 1 - lr*wd``,
    then the Adam update.  The decay is not part of the gradient norm; tables decay on touched rows only."""
    kind = "adamw"

    def __init__(self, model: torch.nn.Module, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2, l2: float = 0.0, max_grad_norm: Optional[float] = None,
                 process_group: Optional[dist.ProcessGroup] = None,
                 row_embedding: Optional[FeatureEmbedding] = None) -> None:
        super().__init__(model, lr=lr, betas=betas, eps=eps, l2=l2, max_grad_norm=max_grad_norm,
                         process_group=process_group, row_embedding=row_embedding, weight_decay=weight_decay)


class RowSparseSGD(RowSparseOptimizer):
    """torch.optim.SGD(momentum=0.9) semantics (trainer.py:73-76; dampening 0, no Nesterov): ``buf = mu*buf + g``,
    ``p -= lr*buf``.  The buffer starts at zero, which gives torch's first-step ``buf = g`` exactly; it lives in
    ``exp_avg`` / ``flat_m``; there is no second moment."""
    kind = "sgd"

    def __init__(self, model: torch.nn.Module, lr: float = 1e-3, momentum: float = 0.9, l2: float = 0.0,
                 max_grad_norm: Optional[float] = None, process_group: Optional[dist.ProcessGroup] = None,
                 row_embedding: Optional[FeatureEmbedding] = None) -> None:
        super().__init__(model, lr=lr, l2=l2, max_grad_norm=max_grad_norm, process_group=process_group,
                         row_embedding=row_embedding, momentum=momentum)


OPTIMIZERS = {"adam": RowSparseAdam, "adamw": RowSparseAdamW, "sgd": RowSparseSGD}


def build_optimizer(model: torch.nn.Module, cfg) -> RowSparseOptimizer:
    """The row-sparse optimizer ``Trainer._build_optimizer`` (trainer.py:67-78) would build for ``cfg``
    (an ``ExperimentConfig``): ``training.optimizer`` picks the kind with torch's defaults (AdamW: weight decay
    0.01; SGD: momentum 0.9), ``training.lr`` the learning rate; the step's L2 term and clip come from
    ``feature.embedding_l2_reg`` and ``training.gradient_clip_norm`` (0: no clipping)."""
    tc = cfg.training
    cls = OPTIMIZERS.get(tc.optimizer)
    if cls is None:
        raise ValueError(f"Unknown optimizer: {tc.optimizer}")
    clip = tc.gradient_clip_norm
    return cls(model, lr=tc.lr, l2=cfg.feature.embedding_l2_reg, max_grad_norm=clip if clip else None)
