"""``mkb_amd.optim.Adam`` -- dense Adam with the element-wise semantics of ``torch.optim.Adam`` (the optimizer
the reference's training loops construct, README.md:123-126; stepped at compose/pipeline.py:238-240), running as
one HBM-streaming HIP kernel per parameter (``mkb_adam_step``) with ``optimizer.zero_grad()`` fused into it.

Opt-in: ``torch.optim.Adam`` keeps working with ``mkb_amd`` models (gradients are ordinary dense ``.grad``
tensors).  Dense means dense: every row of the tables moves every step through its moments, exactly like the
reference -- rows with a zero gradient still decay ``exp_avg`` / ``exp_avg_sq`` and step along the stale
momentum.

``Adam(..., lazy_rows=True)`` keeps those semantics bit for bit but defers the zero-gradient steps of the rows a
step does not touch (``mkb_adam_rows_advance`` / ``mkb_adam_rows_step``, see mkb_amd/csrc/adam.hip): the fused
training step tells the optimizer which entity rows it reads (candidate pool + heads + tails); those rows are
brought up to date before the forward pass and take the real step afterwards; everything else is replayed when
it is next needed or at ``flush()`` (``compose.Pipeline`` / ``evaluation`` / ``model(...)`` outside the fused
step / ``model.embeddings`` / ``model.save`` flush automatically; flush by hand before reading
``model.entity_embedding`` directly).

``defer_step=True`` (``compose.Pipeline`` turns it on for its fused loop) defers the REAL step of the touched rows as
well: after backward such a row is "current through t-1, gradient of step t in its ``.grad`` row", and the next
catch-up / flush that visits it replays step t WITH that gradient (then clears it) -- ``step()`` launches nothing, and
the second pass over p / m / v of every touched row (``mkb_adam_rows_step``) disappears.  Same arithmetic in the same
order: still bit-identical to dense Adam after ``flush()``.  The small dense parameters that rode the step launch (the
relation table) ride the next catch-up launch instead, so with ``defer_step`` they too are only current after
``flush()``.  Contract: clear gradients through ``optimizer.zero_grad()`` only (``model.zero_grad()`` /
``p.grad.zero_()`` would erase a step that has not been applied yet), and let every step that reads a row-lazy table keep to
"the protocol" below (the step classes and ``model(...)`` do): rows current before the forward pass, then their gradient, then the report.

``mkb_amd.optim.Adagrad`` -- ``torch.optim.Adagrad`` (``weight_decay=0``) stepped ROW-SPARSELY, one ``mkb_adagrad_step`` launch per
step with ``zero_grad()`` fused into it (mkb_amd/csrc/adagrad.hip).  A zero gradient moves neither Adagrad's accumulator nor the
parameter, so stepping only the rows a batch wrote is dense Adagrad bit for bit: the rows of its tables are ALWAYS current, and
the protocol's catch-up, flush and replay are no launches at all.
"""
import torch

from . import _hip, _links

__all__ = ["Adam", "Adagrad"]


def _draw_ahead_handle(sampler, device):
    """The device handle of the sampler an optimizer carries the next draw of, or None: no sampler, none on ``device``, or one that
    has not generated yet (the sampler creates its device state on its first ``generate()``)."""
    if sampler is None or getattr(sampler, "_handle", None) is None or sampler._device != device:
        return None
    return sampler._handle


class Adam:
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, lazy_rows=False, draw_ahead=None, defer_step=None):
        """``draw_ahead``: a ``mkb_amd.sampling.NegativeSampling`` whose NEXT pool draw should ride the row catch-up
        launch of each step (one kernel launch and ~13 us of serial latency fewer per training step; the negatives are
        the same, bit for bit).  Only meaningful with ``lazy_rows=True`` and a sampler on the same device / stream."""
        self.params = [p for p in params]
        self.draw_ahead = draw_ahead
        self.lr, self.betas, self.eps = lr, betas, eps
        self.state = {}
        self.step_count = 0
        self.lazy_rows = lazy_rows
        self.defer_step = defer_step  # None: off until compose.Pipeline (or the caller) turns it on; False: never
        self._pending_dense = None    # (parameter, AdamDense, lr, gradient tensor kept alive) of a deferred step
        self._zeroed = False
        # the backward functions of model(...) add their rows straight into .grad of a row-lazily stepped table (no dense buffer
        # goes through autograd: _gradshare.direct); False: they hand autograd a dense gradient as for any other optimizer
        self.direct_grads = True
        if lazy_rows:
            for p in self.params:
                if p.dim() == 2 and p.shape[0] >= 4096:  # big tables only; small ones stay on the dense kernel
                    _links.attach(p, self)
                    if p.grad is None and p.is_cuda:
                        p.grad = torch.zeros_like(p)  # (where the row gradients land; all-zero outside pending rows from now on)

    # ------------------------------------------------------------------ state
    def _state(self, p):
        st = self.state.get(p)
        if st is None:
            st = self.state[p] = {"m": torch.zeros_like(p), "v": torch.zeros_like(p), "n": 0}
            if _links.owner(p) is self:
                st["last"] = torch.zeros(p.shape[0], dtype=torch.int32, device=p.device)
                st["consts"] = torch.zeros((1 << 16, 2), dtype=torch.float32, device=p.device)
        return st

    def _consts(self, st, step):
        c = st["consts"]
        if step >= c.shape[0]:
            new = torch.zeros((max(2 * c.shape[0], step + 1), 2), dtype=torch.float32, device=c.device)
            new[: c.shape[0]] = c
            st["consts"] = c = new
        return c

    # ------------------------------------------------------------------ lazy rows
    def _take_dense(self):
        """The dense rider of the last deferred step (or None): it joins the launch that is about to be made."""
        pend, self._pending_dense = self._pending_dense, None
        return None if pend is None else pend[1]

    def _lr_of(self, st, step):
        return st.get("lrs", {}).get(step, self.lr)

    def _advance(self, p, st, upto, rows, sampler_tail=None, draw_ahead=None):
        """One ``mkb_adam_rows_advance`` launch (``mkb_adam_rows_advance_generate`` when ``sampler_tail``, that call's sampler
        arguments, is given) that makes ``rows`` -- the call's row-listing arguments -- of ``p`` current through ``upto``.  With a
        deferred step pending (``st["defer"]``) it is the advance form: it carries the gradient, that step's learning rate and
        the dense rider of the step; otherwise it is the plain catch-up."""
        c, defer, lib = self._consts(st, max(upto, 1)), st.get("defer"), _hip.lib()
        with _hip.on_device(p.device):
            table = (_hip.ptr(p.data), _hip.ptr(st["g"]) if defer else None, _hip.ptr(st["m"]), _hip.ptr(st["v"]),
                     _hip.ptr(st["last"]), _hip.ptr(c), p.shape[0], p.shape[1])
            step = (upto, self._lr_of(st, upto) if defer else 0.0, self.betas[0], self.betas[1], self.eps,
                    self._take_dense() if defer else None)
            if sampler_tail is None:
                _hip.check(lib.mkb_adam_rows_advance(*table, *rows, *step, draw_ahead, _hip.stream_ptr()), "mkb_adam_rows_advance")
            else:
                _hip.check(lib.mkb_adam_rows_advance_generate(*table, *rows, *step, *sampler_tail, _hip.stream_ptr()),
                           "mkb_adam_rows_advance_generate")

    def catch_up(self, p, ids, upto=None):
        """Make the rows ``ids`` of ``p`` current through step ``upto`` (default: every step taken so far)."""
        st = self._state(p)
        upto = st["n"] if upto is None else upto
        if upto <= 0:
            return
        ids = _hip.contiguous(ids, torch.int64)
        st["caught_up"] = (ids, upto)
        self._advance(p, st, upto, (None, 0, 0, 0, _hip.ptr(ids), ids.numel()), draw_ahead=self._sampler_handle(p.device))

    @staticmethod
    def _shard_rows(world, rank, local_ids):
        n_loc = 0 if local_ids is None else local_ids.numel()
        return world, rank, _hip.ptr(local_ids) if n_loc else None, n_loc

    def catch_up_sharded(self, p, global_ids, world, rank, local_ids, listed_as=None):
        """``catch_up`` for a ROW SHARD of a table (``mkb_amd.table_rows``): the rows to make current are the entries of
        ``global_ids`` this rank owns (``e % world == rank``, shard index ``e // world``) plus the shard indices
        ``local_ids``; one launch, no id list.  ``listed_as``: the tensor the caller will report them with, recorded as what
        was caught up -- also when no step has been taken yet and nothing is launched."""
        st = self._state(p)
        upto = st["n"]
        st["caught_up"] = (listed_as, upto)
        if upto <= 0:
            return
        self._advance(p, st, upto, (_hip.ptr(global_ids), global_ids.numel(), *self._shard_rows(world, rank, local_ids)),
                      draw_ahead=self._sampler_handle(p.device))

    def catch_up_with_sampler(self, p, shard, sampler_handle, sample, mode_id, outputs, listed_as=None):
        """``catch_up(p, rows of this batch)`` (``shard = (world, rank, local_ids)``: ``catch_up_sharded(p, the pool, *shard)``) in ONE
        launch with the sampler's filter and next draw (``mkb_adam_rows_advance_generate``; ``NegativeSampling.generate_with_catch_up``)."""
        st = self._state(p)
        st["caught_up"] = (listed_as, st["n"])
        self._advance(p, st, st["n"], (0, 0, None, 0) if shard is None else self._shard_rows(*shard),
                      (sampler_handle, _hip.ptr(sample), sample.shape[0], mode_id, *[_hip.ptr(t) for t in outputs]))

    # --------------------------------------------- the protocol; only it touches caught_up, fwd_n, defer, g, lrs, flushed
    @staticmethod
    def _caught_up(st, ids, n):  # the last catch-up recorded was of this very tensor (identity: no device sync) through n
        done = st.get("caught_up")
        return done is not None and done[0] is ids and done[1] == n

    def ensure_current(self, p, ids):
        """``catch_up(p, ids)`` unless the last catch-up at this step count did that (e.g. folded into the sampler's launch)."""
        st = self._state(p)
        if not self._caught_up(st, ids, st["n"]):
            self.catch_up(p, ids)

    def begin_step_on(self, p, ids):
        """In front of a fused step that reads the rows ``ids`` of ``p`` and adds to their rows of ``p.grad``: they become current
        and are marked as written.  -> ``mkb_grads_t.rows_clear``: those gradient rows are all-zero, the kernels may store."""
        st, rec = self._state(p), _links.record(p)
        if not self._caught_up(st, ids, st["n"]):
            self.catch_up(p, ids)
        # Deferred real step: that launch consumed AND cleared the gradient row of every row this step writes, so unless an earlier
        # backward of this optimizer step has written since (marked rows, or autograd, which marks none) they are all-zero.  Read BEFORE the mark.
        clear = bool(st.get("defer") and st["n"] >= 1 and rec.touched is None and not rec.wrote
                     and st.get("g") is not None and st["g"].data_ptr() == p.grad.data_ptr())
        rec.mark(ids)  # accumulates when several steps share one optimizer.step()
        return clear

    def before_forward(self, p, ids):
        """In front of a forward pass that reads the rows ``ids`` of ``p`` (``None`` = too many to list: the whole table is flushed)."""
        st = self._state(p)
        st["fwd_n"] = st["n"]  # (the rows read at this step count are current from here on: rows_written(after_forward=True))
        if st["n"] <= 0 or st.get("flushed") == st["n"]:
            return  # nothing pending
        if ids is None:
            self.flush(p)
        else:
            self.catch_up(p, ids)

    def rows_written(self, p, ids, after_forward=False, replace=False):
        """Report the rows a backward pass wrote into ``p.grad`` (``_links.Link.mark``).  ``after_forward``: behind autograd's back
        (``_gradshare.direct``); if ``before_forward`` ran at this step count, ``step()`` need not make the rows current first."""
        rec = _links.record(p)
        st = self._state(p) if after_forward else None
        rec.mark(ids, replace, after_forward and st.get("fwd_n") == st["n"])
        if after_forward:
            rec.rebase(p)

    def flush(self, p=None):
        """Replay everything that is pending: afterwards the tables equal what dense Adam would hold."""
        for q in ([p] if p is not None else self.params):
            if _links.owner(q) is not self:
                continue
            st = self._state(q)
            if st["n"] <= 0 or st.get("flushed") == st["n"]:
                continue
            self._advance(q, st, st["n"], (None, 0, 0, 0, None, 0))  # no row list: the whole table
            st["flushed"] = st["n"]
        pend, self._pending_dense = self._pending_dense, None
        if pend is not None:  # no launch above carried it (its table was already flushed): step it on its own
            q, d, lr, _ = pend
            with _hip.on_device(q.device):
                _hip.check(_hip.lib().mkb_adam_step(d.param, d.grad, d.exp_avg, d.exp_avg_sq, d.n, d.step, lr, self.betas[0],
                                                    self.betas[1], self.eps, 1, _hip.stream_ptr()), "mkb_adam_step")

    def stop_deferring(self):
        """Apply whatever ``defer_step`` left pending and switch it off for good (callers whose gradient rows are not
        preceded by a catch-up, e.g. ``parallel.SparseGradExchange``)."""
        self.flush()
        self.defer_step = False
        for st in self.state.values():
            st.pop("defer", None)

    # ------------------------------------------------------------------ torch.optim-like API
    def _link(self, p):  # p's _links record when this optimizer steps it row-lazily, else None (one lookup, then attribute reads)
        rec = _links.record(p)
        return rec if rec is not None and rec.owner is self else None

    def _rider(self):
        """The dense tensor that steps inside the row-lazy launch (one fewer kernel per step): the first dense,
        16-byte aligned float32 parameter with a gradient, when some table steps row-lazily this time."""
        links = [self._link(p) for p in self.params]
        lazy = [p for p, rec in zip(self.params, links) if p.grad is not None and rec is not None and rec.touched is not None
                and not rec.wrote]  # (autograd wrote as well: that table takes the dense route this time)
        if len(lazy) != 1:
            return None, None
        for q, rec in zip(self.params, links):
            if (q.grad is not None and rec is None and q.is_cuda and q.device == lazy[0].device
                    and q.dtype == torch.float32 and q.is_contiguous() and q.grad.is_contiguous() and q.numel() >= 4
                    and "last" not in self._state(q)):
                st = self._state(q)
                ptrs = (q.data_ptr(), q.grad.data_ptr(), st["m"].data_ptr(), st["v"].data_ptr())
                if all(x % 16 == 0 for x in ptrs):
                    return q, _hip.AdamDense(*ptrs, q.numel(), st["n"] + 1)
        return None, None

    def _sampler_handle(self, device):
        return _draw_ahead_handle(self.draw_ahead, device)

    def step(self):
        self.step_count += 1
        lib = _hip.lib()
        rider_p, rider = self._rider()
        dense_todo = []
        for p in self.params:
            if p.grad is None:
                continue
            if p is rider_p:  # stepped by the row-lazy launch below / above
                self._state(p)["n"] += 1
                continue
            _hip.require_device(p)
            st = self._state(p)
            g = p.grad
            if not g.is_contiguous():
                g = p.grad = g.contiguous()
            touched, rec = None, self._link(p)
            if rec is not None:
                current = rec.all_marks_current()  # (every row was made current by the forward pass that read it)
                wrote, touched = rec.wrote, rec.take_touched()
                if wrote:  # autograd accumulated into .grad in this step as well: which rows is unknown -> the dense route below
                    touched = None
            with _hip.on_device(p.device):
                if touched is not None:
                    done = st.get("caught_up")
                    caught = done is not None and done[1] == st["n"]  # a catch-up at this step count preceded the gradient
                    if self.defer_step and st["n"] >= 1 and caught:
                        # deferred: the rows were current through n before their gradient was written; the next catch-up /
                        # flush that visits a row replays this step with its gradient row (nothing is launched here)
                        st["n"] += 1
                        st["defer"], st["g"] = True, g
                        lrs = st.setdefault("lrs", {})
                        lrs[st["n"]] = self.lr
                        lrs.pop(st["n"] - 4, None)
                        if rider_p is not None:
                            self._pending_dense = (rider_p, rider, self.lr, rider_p.grad)
                        continue
                    if st.get("defer") and not caught:
                        raise RuntimeError("mkb_amd.optim.Adam(defer_step=True): gradient rows were written without a catch-up of "
                                           "those rows in this step, so they cannot be told from a step that is still pending; "
                                           "call optimizer.stop_deferring() before training this way")
                    st["n"] += 1
                    ids = _hip.contiguous(touched, torch.int64)
                    c = self._consts(st, st["n"])
                    if not current and not self._caught_up(st, touched, st["n"] - 1):
                        self.catch_up(p, ids, upto=st["n"] - 1)  # e.g. rows only OTHER data-parallel ranks touched
                    _hip.check(lib.mkb_adam_rows_step(_hip.ptr(p.data), _hip.ptr(g), _hip.ptr(st["m"]), _hip.ptr(st["v"]),
                                                      _hip.ptr(st["last"]), _hip.ptr(c), p.shape[0], p.shape[1],
                                                      _hip.ptr(ids), ids.numel(), st["n"], self.lr, self.betas[0],
                                                      self.betas[1], self.eps, rider, _hip.stream_ptr()), "mkb_adam_rows_step")
                else:
                    if "last" in st:  # a step whose touched rows are unknown: fall back to dense for good
                        self.flush(p)
                        st.pop("last"), st.pop("consts")
                        _links.detach(p)
                    st["n"] += 1
                    dense_todo.append((p, g, st))
        # the dense tensors of a device step in ONE launch (mkb_adam_step_multi: the same arithmetic per element; small models
        # are bound by launches -- Umls TransE-64 spends 9 launches of ~5 us per step)
        while dense_todo:
            dev = dense_todo[0][0].device
            group = [t for t in dense_todo if t[0].device == dev][:8]
            dense_todo = [t for t in dense_todo if not any(t is u for u in group)]
            aligned = all(x.data_ptr() % 16 == 0 for p, g, st in group for x in (p.data, g, st["m"], st["v"]))
            sampler = self._sampler_handle(dev)  # (its next pool is drawn by one more workgroup of this launch)
            with _hip.on_device(dev):
                if (len(group) > 1 or sampler is not None) and aligned:
                    arr = (_hip.AdamDense * len(group))(*[_hip.AdamDense(p.data_ptr(), g.data_ptr(), st["m"].data_ptr(), st["v"].data_ptr(),
                                                                          p.numel(), st["n"]) for p, g, st in group])
                    _hip.check(lib.mkb_adam_step_multi(arr, len(group), self.lr, self.betas[0], self.betas[1], self.eps, 1,
                                                       sampler, _hip.stream_ptr()), "mkb_adam_step_multi")
                else:
                    for p, g, st in group:
                        _hip.check(lib.mkb_adam_step(_hip.ptr(p.data), _hip.ptr(g), _hip.ptr(st["m"]), _hip.ptr(st["v"]),
                                                     p.numel(), st["n"], self.lr, self.betas[0], self.betas[1], self.eps, 1,
                                                     _hip.stream_ptr()), "mkb_adam_step")
        self._zeroed = True

    def zero_grad(self, set_to_none=False):
        """Gradients were already cleared inside ``step`` (fused); they stay allocated so the next backward
        accumulates in place."""
        if self._zeroed and not set_to_none:
            self._zeroed = False
            return
        if any(st.get("defer") for st in self.state.values()):
            self.flush()  # a deferred step lives in the gradient rows: apply it before they are really cleared
        for p in self.params:
            rec = _links.record(p)
            if rec is not None:
                rec.wrote = False
            if p.grad is not None:
                if set_to_none:
                    p.grad = None
                else:
                    p.grad.zero_()
        self._zeroed = False

    # ------------------------------------------------------------------ checkpointing (torch.optim-style)
    def state_dict(self):
        """Like ``torch.optim.Adam.state_dict()``: per-parameter ``step`` / ``exp_avg`` / ``exp_avg_sq`` (clones) keyed by
        the parameter's position, plus the hyper-parameters.  Pending row-lazy steps are flushed first, so the tables and
        the moments the caller saves next to each other are the dense-Adam state of this step."""
        self.flush()
        state = {}
        for i, p in enumerate(self.params):
            st = self.state.get(p)
            if st is not None:
                state[i] = {"step": st["n"], "exp_avg": st["m"].clone(), "exp_avg_sq": st["v"].clone()}
        return {"state": state, "param_groups": [{"lr": self.lr, "betas": tuple(self.betas), "eps": self.eps,
                                                  "params": list(range(len(self.params)))}],
                "step_count": self.step_count}

    def load_state_dict(self, sd):
        """Restore ``state_dict()`` onto an optimizer built over the same parameters (their tables must be restored by the
        caller, e.g. ``model.load_state_dict``): every row is then current through the saved step."""
        g = sd["param_groups"][0]
        self.lr, self.betas, self.eps = g["lr"], tuple(g["betas"]), g["eps"]
        self.step_count = sd.get("step_count", 0)
        for i, p in enumerate(self.params):
            saved = sd["state"].get(i, sd["state"].get(str(i)))
            if saved is None:
                self.state.pop(p, None)
                continue
            st = self._state(p)
            st["m"].copy_(saved["exp_avg"])
            st["v"].copy_(saved["exp_avg_sq"])
            st["n"] = int(saved["step"])
            st.pop("caught_up", None)
            st["flushed"] = st["n"]
            if st.pop("defer", None):  # nothing is pending in a restored state
                st["g"].zero_()
            if "last" in st:  # row-lazy: nothing is pending, the replay constants of earlier steps are not needed again
                st["last"].fill_(st["n"])
        self._pending_dense = None
        self._zeroed = False


class Adagrad:
    """``torch.optim.Adagrad(params, lr, lr_decay, 0, initial_accumulator_value, eps)`` with the big tables (two dimensions, 4,096
    rows or more: the rule of ``Adam(lazy_rows=True)``) stepped row-sparsely and everything else as dense riders of the same
    launch: ``step()`` is one ``mkb_adagrad_step`` per device, gradient clearing included.

    It speaks the protocol of the steps that read a row-lazily stepped table (``_links.owner(p)``) on the fact that its
    rows are always current: making rows current launches nothing, the marks say which rows ``step()`` visits.  A step into which
    autograd wrote as well (which rows is unknown) visits every row of that table, once: nothing is pending that could be lost, so
    the next step is row-sparse again.  The same holds for a table with a gradient whose rows nobody reported: a writer that does
    not report (the fused steps report entity rows only, so a relation table of 4,096 rows or more) cannot be told from no writer,
    and the all-rows form only reads where the gradient is zero.  Like torch's, a parameter's step count advances with every
    ``step()`` that finds a gradient on it.

    ``draw_ahead``: a ``mkb_amd.sampling.NegativeSampling`` whose NEXT pool draw rides the step's launch (``compose.Pipeline``
    lends its sampler for the length of ``learn()``); the negatives are the same, bit for bit."""

    lazy_rows = True            # (compose.Pipeline lends such an optimizer its sampler; there is no defer_step to borrow)
    rows_always_current = True  # fused.sampled_step: nothing to fold into the sampler's launch, plain generate() it is
    direct_grads = True         # the backward functions of model(...) add their rows straight into .grad (_gradshare.direct)

    def __init__(self, params, lr=1e-2, lr_decay=0.0, weight_decay=0.0, initial_accumulator_value=0.0, eps=1e-10, draw_ahead=None):
        for name, value in (("learning rate", lr), ("lr_decay value", lr_decay), ("weight_decay value", weight_decay),
                            ("initial_accumulator_value value", initial_accumulator_value), ("epsilon value", eps)):
            if not 0.0 <= value:
                raise ValueError(f"Invalid {name}: {value}")
        if weight_decay != 0:
            raise ValueError("mkb_amd.optim.Adagrad steps only the rows a batch wrote; a weight decay moves every row every step. "
                             "The row-sparse way to get it is mkb_amd.regularizers.L2 on the batch's rows")
        self.params = [p for p in params]
        self.lr, self.lr_decay, self.eps = lr, lr_decay, eps
        self.weight_decay, self.initial_accumulator_value = weight_decay, initial_accumulator_value
        self.draw_ahead = draw_ahead
        self.state = {}
        self.step_count = 0
        self._zeroed = False
        for p in self.params:
            if p.dim() == 2 and p.shape[0] >= 4096:
                _links.attach(p, self)
            st = self._state(p)
            if "last" in st and p.grad is None and p.is_cuda:
                p.grad = st["clean"] = torch.zeros_like(p)  # (where the row gradients land; all-zero between steps)

    # ------------------------------------------------------------------ state
    def _state(self, p):
        # sum / n: torch's state_sum / step.  Row-sparse tables also: last [rows] int32 = the last step that visited a row (the
        # kernel's ownership stamp), fwd_n = the step count at the last before_forward, clean = the .grad TENSOR known to be
        # all-zero between steps (held, so that its address cannot come back as another tensor's)
        st = self.state.get(p)
        if st is None:
            st = self.state[p] = {"sum": torch.full_like(p, self.initial_accumulator_value), "n": 0}
            if _links.owner(p) is self:
                st["last"] = torch.zeros(p.shape[0], dtype=torch.int32, device=p.device)
        return st

    def _link(self, p):
        rec = _links.record(p)
        return rec if rec is not None and rec.owner is self else None

    # ------------------------------------------------------------------ the protocol: rows are always current
    def ensure_current(self, p, ids):
        pass

    def catch_up(self, p, ids, upto=None):
        pass

    def flush(self, p=None):
        pass

    def before_forward(self, p, ids):
        st = self._state(p)
        st["fwd_n"] = st["n"]  # (rows_written(after_forward=True) at this step count marks its rows as current)

    def begin_step_on(self, p, ids):
        """In front of a fused step that adds to the rows ``ids`` of ``p.grad``: they are marked as written.  -> ``mkb_grads_t.
        rows_clear``: EVERY row of ``p.grad`` is zero, the kernels may store.  That is known when the tensor is the one this
        optimizer created or last cleared in full, every step since cleared the rows it was told about (each did), and nothing has
        been marked and autograd has written nothing since the last step.  Read BEFORE the mark."""
        st, rec = self._state(p), _links.record(p)
        clean, g = st.get("clean"), p.grad
        clear = bool(clean is not None and g is not None and clean.data_ptr() == g.data_ptr() and rec.touched is None and not rec.wrote)
        rec.mark(ids)  # accumulates when several steps share one optimizer.step()
        return clear

    def rows_written(self, p, ids, after_forward=False, replace=False):
        """Report the rows a backward pass wrote into ``p.grad`` (``_links.Link.mark``); ``after_forward``: behind autograd's back
        (``_gradshare.direct``)."""
        rec = _links.record(p)
        st = self._state(p) if after_forward else None
        rec.mark(ids, replace, after_forward and st.get("fwd_n") == st["n"])
        if after_forward:
            rec.rebase(p)

    def catch_up_with_sampler(self, *args, **kwargs):
        raise NotImplementedError("mkb_amd.optim.Adagrad steps single-device tables only and has no catch-up for the sampler's launch "
                                  "to carry: use sampler.generate (fused.sampled_step does)")

    def catch_up_sharded(self, *args, **kwargs):
        raise NotImplementedError("mkb_amd.optim.Adagrad steps single-device tables only: row-sharded (mkb_amd.table_rows) and "
                                  "data-parallel (mkb_amd.parallel) tables need mkb_amd.optim.Adam(lazy_rows=True)")

    # ------------------------------------------------------------------ torch.optim-like API
    def step(self):
        self.step_count += 1
        work = {}  # (device, clr) -> (tables, dense tensors): one launch carries one table, up to 8 dense tensors and ONE rate
        for p in self.params:
            g = p.grad
            if g is None:
                continue
            _hip.require_device(p)
            st = self._state(p)
            if g.dtype != torch.float32 or p.dtype != torch.float32 or not p.is_contiguous():
                raise TypeError("mkb_amd.optim.Adagrad steps contiguous float32 parameters")
            if st["sum"].device != p.device:  # the model moved after the optimizer was built: the state follows it
                st.update({k: v.to(p.device) for k, v in st.items() if k in ("sum", "last")})
            if not g.is_contiguous():
                g = p.grad = g.contiguous()
                st.pop("clean", None)
            ids, rec = None, self._link(p)
            if rec is not None:
                wrote, ids = rec.wrote, rec.take_touched()
                if wrote or ids is None or ids.numel() == 0:
                    # autograd accumulated into .grad in this step as well, or nobody reported a row: a writer that keeps no protocol
                    # for this table (the fused steps report the ENTITY rows only; a relation table of 4,096 rows takes their
                    # gradient unreported) cannot be told from no writer.  Which rows is unknown -> every row, this once: the
                    # all-rows form reads the gradient and writes only where it is not zero.  (optim.Adam steps such a table densely.)
                    ids = None
                else:
                    ids = _hip.contiguous(ids, torch.int64)
            st["n"] += 1
            clr = self.lr / (1.0 + (st["n"] - 1) * self.lr_decay)
            tables, dense = work.setdefault((p.device, clr), ([], []))
            (tables if rec is not None else dense).append((p, g, st, ids))
        lib = _hip.lib()
        for (dev, clr), (tables, dense) in work.items():
            sampler = _draw_ahead_handle(self.draw_ahead, dev)  # (its next pool is drawn by one more workgroup of the first launch it meets)
            with _hip.on_device(dev):
                while tables or dense:
                    group, dense = dense[:8], dense[8:]
                    arr = None
                    if group:
                        arr = (_hip.AdagradDense * len(group))(*[_hip.AdagradDense(q.data_ptr(), h.data_ptr(), s["sum"].data_ptr(), q.numel())
                                                                 for q, h, s, _ in group])
                    if tables:
                        p, g, st, ids = tables.pop(0)
                        table = (_hip.ptr(p.data), _hip.ptr(g), _hip.ptr(st["sum"]), _hip.ptr(st["last"]), p.shape[0], p.shape[1],
                                 _hip.ptr(ids), 0 if ids is None else ids.numel(), st["n"])
                        if ids is None:
                            st["clean"] = g  # every row was cleared
                    else:
                        table = (None, None, None, None, 0, 0, None, 0, group[0][2]["n"])
                    _hip.check(lib.mkb_adagrad_step(*table, clr, self.eps, arr, len(group), sampler, _hip.stream_ptr()), "mkb_adagrad_step")
        self._zeroed = True

    def zero_grad(self, set_to_none=False):
        """Gradients were already cleared inside ``step`` (fused); they stay allocated so the next backward accumulates in place."""
        if self._zeroed and not set_to_none:
            self._zeroed = False
            return
        for p in self.params:
            rec, st = self._link(p), self._state(p)
            if rec is not None:
                rec.take_touched()  # the rows that were marked are cleared with everything else
                st.pop("clean", None)
            if p.grad is not None:
                if set_to_none:
                    p.grad = None
                else:
                    p.grad.zero_()
                    if rec is not None:
                        st["clean"] = p.grad
        self._zeroed = False

    # ------------------------------------------------------------------ checkpointing (torch.optim-style)
    def state_dict(self):
        """Like ``torch.optim.Adagrad.state_dict()``: per-parameter ``step`` / ``sum`` (a clone) keyed by the parameter's position,
        and one param group with the hyper-parameters.  Nothing is ever pending, so nothing is flushed."""
        state = {i: {"step": torch.tensor(float(self.state[p]["n"])), "sum": self.state[p]["sum"].clone()}  # (torch keeps `step` as a tensor)
                 for i, p in enumerate(self.params)}
        return {"state": state, "param_groups": [{"lr": self.lr, "lr_decay": self.lr_decay, "eps": self.eps, "weight_decay": self.weight_decay,
                                                  "initial_accumulator_value": self.initial_accumulator_value,
                                                  "params": list(range(len(self.params)))}]}

    def load_state_dict(self, sd):
        """Restore ``state_dict()`` onto an optimizer built over the same parameters (the caller restores their tables)."""
        g = sd["param_groups"][0]
        self.lr, self.lr_decay, self.eps = g["lr"], g["lr_decay"], g["eps"]
        self.initial_accumulator_value = g.get("initial_accumulator_value", self.initial_accumulator_value)
        for i, p in enumerate(self.params):
            saved = sd["state"].get(i, sd["state"].get(str(i)))
            st = self._state(p)
            if saved is None:
                st["sum"].fill_(self.initial_accumulator_value)
                st["n"] = 0
            else:
                st["sum"].copy_(saved["sum"])
                st["n"] = int(saved["step"])
            st.pop("fwd_n", None)
            if "last" in st:
                st["last"].fill_(st["n"])  # every stamp is below the next step: no row of it looks claimed
        self.step_count = max([self.state[p]["n"] for p in self.params], default=0)  # (torch's layout has no optimizer-wide count)
        self._zeroed = False
