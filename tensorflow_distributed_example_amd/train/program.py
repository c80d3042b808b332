"""Per-replica execution plans and the multi-step training program.

A *plan* executes one replica's work for one step on one device:

* ``ConvNetPlan`` (GPU): the DWK/TF2M small CNN as five
  fused gfx950 HIP kernels —
      conv+bias+ReLU+maxpool (VALU)  → Dense split-K MFMA (atomic f32)
      → head: bias+ReLU, Dense, softmax-CE, accuracy, and the whole head backward
      → dW of the big Dense (MFMA) → conv backward with the Dense input-gradient
        computed in-kernel (MFMA) and routed through pool argmax / ReLU mask;
  followed by the RCCL all-reduce of the flat gradient bucket and ONE
  multi-tensor optimizer kernel.
* ``LayerwisePlan`` (GPU): any Sequential model built from the supported layers,
  one HIP kernel family per layer (ops/layerwise.py) — Model B, ResNet-18.
* ``ReferencePlan`` (CPU, or GPU when explicitly requested for testing): torch
  ops + autograd — the CPU backend's kernel library and the numerics oracle.

``TrainProgram`` strings ``steps_per_execution`` steps (Keras
``compile(steps_per_execution=N)``) of every local replica together with the
gradient all-reduce and optimizer, and on a single-local-replica GPU captures the
whole N-step sequence — RCCL collective included — into one hipGraph replayed
per execution, so the host issues one launch per N steps.
"""
from __future__ import annotations

import math
import os

import numpy as np
import torch

from .. import backend as Kb
from ..models import layers as L
from . import params as P


def _round8(n):
    return (n + 7) // 8 * 8


class ReplicaPlan:
    kind = "base"

    def __init__(self, model, store, device, batch, global_batch, optimizer):
        self.model = model
        self.store = store
        self.device = torch.device(device)
        self.B = int(batch)
        self.global_batch = int(global_batch)
        self.scale = 1.0 / float(global_batch)
        self.optimizer = optimizer
        self.metrics = torch.zeros(4, dtype=torch.float32, device=self.device)
        self.iterations = torch.zeros(1, dtype=torch.int64, device=self.device)
        for s in optimizer.slot_names() if optimizer is not None else []:
            store.slot(s)
        # step mode "xgmi" with the fused exchange (set_push): the step stores its big weight gradient straight
        # into the xGMI owners' contribution areas; _pushed marks that the step's launch did so (xg_apply_spec)
        self._push = None
        self._pushed = False
        self._opt_key_set = None   # optimizer.key() the descriptors of the current step mode were built at
        self._zl = None
        # weight regularizers (regularizers.py): [(offset, numel, l1, l2)] of the regularized variables
        from .. import regularizers as RG
        self.reg_segs = RG.segments(model, store)
        # rows of the running step (train_step sets it): the regularizers' penalty enters the loss sum once
        # per row, as the per-sample losses do
        self.step_rows = self.B
        self._reg_eval = None      # eval programs: the penalty launches (GPU), made on first use
        self._reg_stale = True     # the penalty partials are older than the weights
        if optimizer is not None:
            optimizer._plan_built = True   # the per-variable decay is settled: exclude_from_weight_decay raises
        # the loss head's spec (losses.py): label smoothing by value, and -- in a program built for
        # fit(class_weight=) -- the table of row weights by class, which ``set_class_weight`` rewrites in place
        self.smooth = 0.0
        self.class_w = None
        # metrics beyond the accuracy (metrics.py): their layout, the ctypes MetricSpec of the launches and the
        # second accumulator the layout describes; None for a model compiled without them
        self.metric_layout = getattr(getattr(model, "_metric_names", None), "layout", None)
        self.metrics_ext = None
        if self.metric_layout is not None:
            self.metrics_ext = torch.zeros(self.metric_layout.words, dtype=torch.float32, device=self.device)

    @property
    def metric_spec(self):
        """The ``MetricSpec`` (csrc/include/tde_metric.h) of a plan built for extra metrics, else None."""
        return self.metric_layout.struct() if self.metric_layout is not None else None

    def _init_loss_spec(self, loss, classes):
        """Take the spec of ``loss`` (a plan that runs a non-trivial one calls this from its constructor)."""
        from .. import losses as LS
        self.smooth = LS.smoothing(loss)
        if LS.class_weighted(loss):
            self.class_w = torch.ones(int(classes), dtype=torch.float32, device=self.device)

    @property
    def loss_spec(self):
        """A non-trivial spec: the plan launches the loss-head variants (csrc/include/tde_loss.h)."""
        return self.smooth != 0.0 or self.class_w is not None

    def set_class_weight(self, table):
        """``fit(class_weight=)``: the float32 [classes] table into the plan's own, in place -- a captured step
        reads the new weights at its next replay."""
        if self.class_w is None:
            raise RuntimeError(f"the {self.kind} plan was not built for class weights")
        t = torch.as_tensor(table, dtype=torch.float32)
        if t.numel() != self.class_w.numel():
            raise ValueError(f"class-weight table of {t.numel()} entries, plan has {self.class_w.numel()} classes")
        self.class_w.copy_(t.reshape(-1))

    def reset_metrics(self):
        self.metrics.zero_()
        if self.metrics_ext is not None:
            self.metrics_ext.zero_()

    def all_metrics(self):
        """``metrics`` with ``metrics_ext`` behind it: what ``metrics.logs_from`` reads."""
        return self.metrics if self.metrics_ext is None else torch.cat([self.metrics, self.metrics_ext])

    def set_iterations(self, step):
        """Assign the device step counter from the host (checkpoint restore)."""
        self.iterations.fill_(int(step))

    def train_step(self, x, y, B=None):
        raise NotImplementedError

    def apply(self):
        raise NotImplementedError

    def eval_step(self, x, y, B=None):
        raise NotImplementedError

    def predict(self, x, B=None):
        raise NotImplementedError

    def on_weights_loaded(self):
        pass

    # How the optimizer runs (set by the Program): "plain" — gradients land in the flat bucket and
    # ``apply()`` runs the multi-tensor optimizer; fused plans may also support "local" (the update
    # happens inside the step's own kernels; ``finish()`` flushes what is deferred) and "xgmi" (the
    # communicator's fused all-reduce applies it).
    step_mode = "plain"
    input_dtype = torch.float32   # dtype of the Program's input ring for this plan
    compute_dtype = "fp32"        # what the plan's kernels compute in ("fp32" | "bf16"; bench / logs)
    parity = 0   # step parity of plans that double-buffer across steps (one hipGraph per start parity)

    # step modes whose launch descriptors carry the optimizer's hyper-parameters by value (``refresh``)
    hyper_by_value = ()

    def supports_step_mode(self, mode):
        return mode == "plain"

    def _opt_fused(self):
        """The optimizer is one the fused step kernels and the xGMI all-reduce apply themselves (kinds 0..3,
        ``opt_step``).  RMSprop is not: such a plan runs "plain", the multi-tensor launch applies it."""
        from ..optimizers import FUSED_KINDS
        # a learning-rate schedule takes the same route: those kernels carry the rate by value, the
        # multi-tensor launch reads it from the device word the schedule launch wrote (OptimizerKernel)
        # gradient clipping too: a norm needs every gradient before any update, a grid-wide dependency the
        # fused steps do not have; the norm launches run in front of the multi-tensor launch
        # weight regularizers and decoupled weight decay as well: the penalty's gradient is added to the
        # aggregated gradient in front of the clip, and the decay is a variant of the multi-tensor launch alone
        return (self.optimizer is not None and self.optimizer.kind_id in FUSED_KINDS
                and self.optimizer.schedule is None and self.optimizer.clip is None
                and not self.reg_segs and self.optimizer.decay is None)

    def decay_segments(self):
        """(offset, numel) of the trainable variables the optimizer's weight decay applies to."""
        st, opt = self.store, self.optimizer
        return [(st.segments[n].offset, st.segments[n].numel) for n in st.names(trainable=True) if opt.decays(n)]

    def add_eval_penalty(self, rows):
        """After an ``eval_step`` of ``rows`` rows: metrics[0] += rows * (the regularizers' penalty of the
        weights).  The partials are computed once per evaluation (``_reg_stale``: the Program marks them when
        the weights may have changed), the finish launch runs per batch."""
        if not self.reg_segs or rows <= 0:
            return
        if self._reg_eval is None:
            self._reg_eval = WeightRegKernel(self.store, self.reg_segs)
        if self._reg_stale:
            self._reg_eval.grad(None)
            self._reg_stale = False
        self._reg_eval.finish(self.metrics, rows)

    def set_step_mode(self, mode):
        if not self.supports_step_mode(mode):
            raise ValueError(f"{self.kind} plan does not support step mode {mode!r}")
        self.step_mode = mode
        if mode != "xgmi":
            self._push = None
        self._opt_key_set = self._opt_key()

    def _opt_key(self):
        return self.optimizer.key() if self.optimizer is not None else None

    def push_range(self):
        """Bucket range the step can push into the xGMI owners itself, or None when this plan cannot."""
        return None

    def set_push(self, spec):
        """Fused data-parallel exchange (step mode "xgmi"): ``spec`` is the communicator's ``XgPush`` for
        this replica (None: the whole bucket stays local, the all-reduce pushes it)."""
        if spec is not None and (self.step_mode != "xgmi" or self.push_range() is None):
            raise ValueError("the fused exchange needs step mode 'xgmi' and the float32 plan")
        self._push = spec

    def xg_apply_spec(self):
        """``XgApply`` for the communicator's fused all-reduce (step mode "xgmi") of a plan whose weights are
        the f32 master store only (no bf16 shadows): it applies the optimizer to ``store.w`` / slots."""
        from ..ops import kernels as K
        st, opt = self.store, self.optimizer
        m, v = K.opt_slots(st, opt)
        # the plan's step pushed part of the bucket into the owners itself (a replica without data this step
        # pushed nothing)
        lo, hi = self.push_range() if (self._push is not None and self._pushed) else (0, 0)
        self._pushed = False
        return K.XgApply(K.opt_hyper(opt), K._P(st.w), K._P(m), K._P(v), K._P(self.iterations), None, 0, 0, None,
                         0, 0, lo, hi)

    def _dummy_labels(self, B):
        """int32 zeros for launches that take labels they do not use (predict)."""
        if self._zl is None or self._zl.shape[0] < B:
            self._zl = torch.zeros(max(B, self.B), dtype=torch.int32, device=self.device)
        return self._zl

    @property
    def applies_in_step(self):
        return self.step_mode == "local"

    def finish(self):
        """End of an execution (a run of steps): commit deferred updates."""

    def trace_tensors(self):
        """State recorded per step by ``Program.enable_trace`` (diagnostics)."""
        return [self.store.w, self.metrics]

    def refresh(self):
        """Before an execution is launched or captured: pick up optimizer hyper-parameter changes."""
        if self.step_mode in self.hyper_by_value and self._opt_key_set != self._opt_key():
            self.set_step_mode(self.step_mode)
        if getattr(self, "opt", None) is not None:
            self.opt.refresh()


# ---------------------------------------------------------------------------------------
def _last_softmax(model, loss):
    last = model.layers[-1]
    act = getattr(last, "activation", None)
    if act == "softmax" and not getattr(loss, "from_logits", False):
        return True
    return False


class ReferencePlan(ReplicaPlan):
    kind = "reference"

    def __init__(self, model, store, device, batch, global_batch, optimizer, loss):
        super().__init__(model, store, device, batch, global_batch, optimizer)
        self.loss = loss
        self.strip_softmax = _last_softmax(model, loss)
        self.rng = Kb.make_generator(1234)
        from .. import losses as LS
        if LS.nontrivial(loss):
            self._init_loss_spec(loss, model.output_shape[-1])

    def _weights(self, wl):
        W = {}
        st = self.store
        for layer in self.model.layers:
            d = {}
            for s in layer.weight_specs:
                seg = st.segments[s.full_name]
                if seg.trainable and wl is not None:
                    d[s.name] = wl[seg.offset: seg.offset + seg.numel].view(seg.shape)
                else:
                    d[s.name] = st.view(s.full_name)
            W[layer.name] = d
        return W

    def _forward(self, x, W, training, updates=None):
        t = {0: x.float()}
        nodes = self.model._nodes()
        for i, (layer, ins, out) in enumerate(nodes):
            h = [t[j] for j in ins] if layer.multi_input else t[ins[0]]
            if i == len(nodes) - 1 and self.strip_softmax:
                act = layer.activation
                layer.activation = None
                try:
                    t[out] = layer.ref_call(h, W[layer.name], training, self.rng, updates)
                finally:
                    layer.activation = act
            else:
                t[out] = layer.ref_call(h, W[layer.name], training, self.rng, updates)
        return t[nodes[-1][2]]

    def train_step(self, x, y, B=None):
        B = x.shape[0] if B is None else B
        self.step_rows = B
        x, y = x[:B], y[:B]
        wl = self.store.w.detach().requires_grad_(True)
        W = self._weights(wl)
        updates = []
        out = self._forward(x, W, True, updates)
        if self.class_w is not None:   # the training loss and gradient only
            ls = self.loss.per_sample(y, out, pred_is_logits=self.strip_softmax, class_weight=self.class_w)
        else:
            ls = self.loss.per_sample(y, out, pred_is_logits=self.strip_softmax)
        (ls.sum() * self.scale).backward()
        with torch.no_grad():
            self.store.g.add_(wl.grad)
            for name, val in updates:
                self.store.view(name).copy_(val)
            self._acc(out, y, ls)

    def _acc(self, out, y, ls):
        yy = torch.as_tensor(y, device=out.device).reshape(-1).long()
        correct = (out.argmax(dim=1) == yy).sum().float()
        loss_sum = ls.sum().float()
        if self.reg_segs:   # the penalty of the weights this forward used, once per row
            from .. import regularizers as RG
            loss_sum = loss_sum + float(ls.shape[0]) * RG.penalty(self.store.w.detach(), self.reg_segs).float()
        self.metrics += torch.stack([loss_sum, correct, torch.tensor(float(ls.shape[0]), device=out.device),
                                     torch.zeros((), device=out.device)])
        if self.metric_layout is not None:
            self._acc_ext(out, yy)

    def _acc_ext(self, out, yy):
        """The words of ``metrics_ext`` with torch (the layout of csrc/include/tde_metric.h)."""
        from .. import losses as LS
        lay, ext = self.metric_layout, self.metrics_ext
        z = out.detach().float()
        if getattr(self.model.layers[-1], "activation", None) == "softmax" and not self.strip_softmax:
            z = z.clamp_min(torch.finfo(torch.float32).tiny).log()   # probabilities: log p is the logits up to lse
        C = z.shape[1]
        valid = (yy >= 0) & (yy < C)
        yc = yy.clamp(0, C - 1)
        zy = torch.where(valid, z.gather(1, yc[:, None]).squeeze(1), z.max(dim=1).values)
        if lay.k:
            rank = (z > zy[:, None]).sum(dim=1)
            for i, k in enumerate(lay.k):
                ext[lay.off_topk + i] += ((rank < k) & torch.isfinite(zy) & valid).sum().float()
        for i, e in enumerate(lay.smooth):
            ext[lay.off_ce + i] += LS.softmax_ce(z, yy, e).sum().float()
        if lay.cm:
            am = z.argmax(dim=1)[valid]
            cm = ext[lay.off_cm: lay.off_cm + C * C].view(C, C)
            cm.index_put_((yy[valid], am), torch.ones(am.shape[0], dtype=torch.float32, device=z.device),
                          accumulate=True)

    def add_eval_penalty(self, rows):
        """``_acc`` has added it already."""

    @torch.no_grad()
    def apply(self):
        st = self.store
        slots = {n: st.slot(n) for n in self.optimizer.slot_names()}
        step = int(self.iterations.item())
        if self.reg_segs:   # on the aggregated gradient, in front of the clip: Keras clips the total loss's gradient
            from .. import regularizers as RG
            RG.reg_reference(st.w, st.g, self.reg_segs)
        if self.optimizer.clip is not None:   # st.g is the aggregated gradient by now: clipped after the all-reduce
            segs = [(st.segments[n].offset, st.segments[n].numel) for n in st.names(trainable=True)]
            self.optimizer.clip_reference(st.g, segs)
        if self.optimizer.decay is not None:   # the step starts from the decayed weight
            self.optimizer.decay_reference(st.w, self.decay_segments(), step)
        self.optimizer.apply_reference(st.w, st.g, slots, step)
        st.g.zero_()
        self.iterations += 1

    @torch.no_grad()
    def eval_step(self, x, y, B=None):
        B = x.shape[0] if B is None else B
        out = self._forward(x[:B], self._weights(None), False)
        ls = self.loss.per_sample(y[:B], out, pred_is_logits=self.strip_softmax)
        self._acc(out, y[:B], ls)

    @torch.no_grad()
    def predict(self, x, B=None):
        B = x.shape[0] if B is None else B
        out = self._forward(x[:B], self._weights(None), False)
        if self.strip_softmax:
            out = torch.softmax(out, dim=-1)
        return out


# ---------------------------------------------------------------------------------------
_OPTSEG = np.dtype([("off", "<i8"), ("rows", "<i4"), ("cols", "<i4"), ("sh", "<i8"), ("sht", "<i8")])


class WeightRegKernel:
    """Device-side state of the weight-regularizer launches of one replica (csrc/include/tde_reg.h,
    csrc/kernels/weightreg.hip): the table over the regularized segments, the penalty partials and the penalty
    word.  ``grad(g)`` adds the penalty's gradient to ``g`` (None: partials only) and ``finish(metrics, rows)``
    sums the partials into ``penalty`` and adds ``rows * penalty`` to ``metrics[0]``; both on the current stream."""

    def __init__(self, store, reg_segs):
        from .. import _native as N
        self.N = N
        self.store = store
        segs = np.array([(o, 1, n, -1, -1) for o, n, _, _ in reg_segs], dtype=_OPTSEG)
        coef = np.ascontiguousarray(np.array([(c1, c2) for _, _, c1, c2 in reg_segs], dtype=np.float32).reshape(-1, 2))
        lib = N.hip()
        ne = lib.tde_reg_table_size(segs.ctypes.data, coef.ctypes.data, len(segs))
        N.check(min(ne, 0), "tde_reg_table_size")
        ents = np.zeros((max(ne, 1), 2), dtype=np.int32)
        N.check(min(lib.tde_reg_build_table(segs.ctypes.data, coef.ctypes.data, len(segs), ents.ctypes.data), 0),
                "tde_reg_build_table")
        dev = store.device
        self.nent = ne
        self.segs_dev = torch.from_numpy(segs.view(np.uint8).copy()).to(dev)
        self.coef_dev = torch.from_numpy(coef).to(dev)
        self.ents_dev = torch.from_numpy(ents).to(dev)
        self.partials = torch.zeros(max(ne, 1), dtype=torch.float32, device=dev)
        self.penalty = torch.zeros(1, dtype=torch.float32, device=dev)

    def grad(self, g):
        N = self.N
        rc = N.hip().tde_reg_grad(self.store.w.data_ptr(), N.ptr(g), self.segs_dev.data_ptr(), self.coef_dev.data_ptr(),
                                  self.ents_dev.data_ptr(), self.nent, self.partials.data_ptr(), N.stream_ptr())
        N.check(rc, "tde_reg_grad")

    def finish(self, metrics, rows):
        N = self.N
        rc = N.hip().tde_reg_finish(self.partials.data_ptr(), self.nent, self.penalty.data_ptr(), N.ptr(metrics),
                                    int(rows), N.stream_ptr())
        N.check(rc, "tde_reg_finish")


class OptimizerKernel:
    """Device-side state for the multi-tensor optimizer kernel of one replica.  Under a learning-rate schedule
    it owns the device word ``lr_word``: ``apply()`` first launches the schedule at ``iterations + sched_bias``
    into it, and the optimizer launch reads the rate from there, both on the step's stream (inside its capture)."""

    # the step kernels have advanced ``iterations`` by the time ``apply()`` runs: the update is number
    # iterations - 1 (csrc/include/tde_sched.h)
    sched_bias = -1

    def __init__(self, store: P.ParamStore, optimizer, shadows: dict, iterations, plan=None):
        from .. import _native as N
        self.N = N
        # the plan this kernel updates for: its regularized segments, its metrics (the penalty joins the loss
        # sum there) and the rows of its running step
        self.plan = plan
        self.store = store
        self.optimizer = optimizer
        self.iterations = iterations
        segs = []
        sh_total = 0
        self.shadow_views = {}
        layout = []
        for name in store.names(trainable=True):
            seg = store.segments[name]
            # 2-D view [prod(shape[:-1]), shape[-1]]: Dense [in, out] and conv HWIO as [KH*KW*Cin, Cout],
            # so the transposed ("col") shadow is the K-contiguous [out, K] operand of the forward GEMM
            rows, cols = (int(np.prod(seg.shape[:-1])), seg.shape[-1]) if len(seg.shape) >= 2 else (1, seg.numel)
            sh = sht = -1
            if name in shadows:
                want = shadows[name]
                if "row" in want:
                    sh = sh_total
                    sh_total += _round8(seg.numel)
                if "col" in want:
                    sht = sh_total
                    sh_total += _round8(seg.numel)
            segs.append((seg.offset, rows, cols, sh, sht))
            layout.append((name, rows, cols, sh, sht))
        self.shadow = torch.zeros(max(sh_total, 8), dtype=torch.bfloat16, device=store.device)
        for name, rows, cols, sh, sht in layout:
            if sh >= 0:
                self.shadow_views[(name, "row")] = self.shadow[sh: sh + rows * cols].view(rows, cols)
            if sht >= 0:
                self.shadow_views[(name, "col")] = self.shadow[sht: sht + rows * cols].view(cols, rows)
        arr = np.array(segs, dtype=_OPTSEG)
        self._segs_host = arr
        lib = N.hip()
        nb = lib.tde_optim_table_size(arr.ctypes.data, len(arr))
        table = np.zeros((max(nb, 1), 4), dtype=np.int32)
        lib.tde_optim_build_table(arr.ctypes.data, len(arr), table.ctypes.data)
        self.nblocks = nb
        self.segs_dev = torch.from_numpy(arr.view(np.uint8).copy()).to(store.device)
        self.table_dev = torch.from_numpy(table).to(store.device)
        self.lr_word = None
        if optimizer.schedule is not None:
            self.lr_word = torch.full((1,), float(optimizer.lr_at(0)), dtype=torch.float32, device=store.device)
        self._sched = self._sched_key = None
        # gradient clipping (csrc/include/tde_clip.h): the sum-of-squares table and the words the norm launches
        # write; clipvalue travels by value and needs none of them
        self.clip_nent = 0
        self.clip_ents_dev = self.clip_ranges_dev = self.clip_partials = self.clip_norm = self.clip_scale = None
        if optimizer.clip is not None and optimizer.clip[0] != "clipvalue":
            ne = lib.tde_clip_table_size(arr.ctypes.data, len(arr))
            ents = np.zeros((max(ne, 1), 2), dtype=np.int32)
            ranges = np.zeros((max(len(arr), 1), 2), dtype=np.int32)
            lib.tde_clip_build_table(arr.ctypes.data, len(arr), ents.ctypes.data, ranges.ctypes.data)
            self.clip_nent = ne
            self.clip_ents_dev = torch.from_numpy(ents).to(store.device)
            self.clip_ranges_dev = torch.from_numpy(ranges).to(store.device)
            nw = len(arr) if optimizer.clip[0] == "clipnorm" else 1
            self.clip_partials = torch.zeros(max(ne, 1), dtype=torch.float32, device=store.device)
            self.clip_norm = torch.zeros(max(nw, 1), dtype=torch.float32, device=store.device)
            self.clip_scale = torch.ones(max(nw, 1), dtype=torch.float32, device=store.device)
        # weight regularizers and decoupled weight decay (csrc/include/tde_reg.h): the regularizer launches'
        # state and the per-segment decay, only when the model or the optimizer has them
        self.reg = WeightRegKernel(store, plan.reg_segs) if plan is not None and plan.reg_segs else None
        self.wd_dev = self._wd_key = None
        self.refresh()
        self.refresh_shadows()

    def _decay_key(self):
        return (self.optimizer.decay, self.optimizer._wd_exclude)

    def refresh(self):
        """Before an execution is launched or captured: the per-segment decay follows the optimizer."""
        if self._wd_key == self._decay_key():
            return
        opt, names = self.optimizer, self.store.names(trainable=True)
        self._wd_key = self._decay_key()
        if opt.decay is None:
            self.wd_dev = None
            return
        wd = np.array([opt.decay if opt.decays(n) else 0.0 for n in names] or [0.0], dtype=np.float32)
        self.wd_dev = torch.from_numpy(wd).to(self.store.device)

    def refresh_shadows(self):
        if not self.shadow_views:   # f32 plans read the master weights: nothing to refresh
            return
        N = self.N
        with torch.cuda.device(self.store.device):
            rc = N.hip().tde_shadow_refresh(self.store.w.data_ptr(), self.shadow.data_ptr(),
                                            self.segs_dev.data_ptr(), self.table_dev.data_ptr(), self.nblocks,
                                            N.stream_ptr())
        N.check(rc, "tde_shadow_refresh")

    def apply(self, zero_grad=True, rows=None):
        """schedule -> regularizers (gradient, penalty) -> clip norms -> the (WD / CLIP) apply.  ``rows``: the
        rows of the step (default: the plan's ``step_rows``), what the step's loss head was given."""
        N = self.N
        st = self.store
        from ..ops.kernels import opt_hyper, opt_slots
        h = opt_hyper(self.optimizer)
        m, v = opt_slots(st, self.optimizer)
        sch = self.optimizer.schedule
        if sch is not None:
            from ..ops import kernels as K
            if self.lr_word is None:   # the optimizer was given a schedule after this plan was built
                self.lr_word = torch.zeros(1, dtype=torch.float32, device=st.device)
            if self._sched_key != sch.key():
                self._sched, self._sched_key = K.lr_sched(sch), sch.key()
            K.lr_schedule(self._sched, self.iterations, self.sched_bias, self.lr_word)
        lr_ptr = N.ptr(self.lr_word) if sch is not None else None
        if self.reg is not None:
            self.reg.grad(st.g)
            self.reg.finish(self.plan.metrics, self.plan.step_rows if rows is None else rows)
        if self.optimizer.decay is not None and self.wd_dev is None:
            self.refresh()
        if self.optimizer.clip is not None or self.optimizer.decay is not None:
            from ..optimizers import CLIP_MODE
            mode, c = (CLIP_MODE[self.optimizer.clip[0]], float(self.optimizer.clip[1])) \
                if self.optimizer.clip is not None else (0, 0.0)
            lib = N.hip()
            if self.clip_scale is not None:   # a norm mode: partials, then norm and scale, on the step's stream
                rc = lib.tde_clip_sumsq(st.g.data_ptr(), self.segs_dev.data_ptr(), self.clip_ents_dev.data_ptr(),
                                        self.clip_nent, self.clip_partials.data_ptr(), N.stream_ptr())
                N.check(rc, "tde_clip_sumsq")
                rc = lib.tde_clip_scale(self.clip_partials.data_ptr(), self.clip_ranges_dev.data_ptr(),
                                        len(self._segs_host), self.clip_nent, mode, c, self.clip_norm.data_ptr(),
                                        self.clip_scale.data_ptr(), N.stream_ptr())
                N.check(rc, "tde_clip_scale")
            if self.optimizer.decay is not None:
                rc = lib.tde_optim_apply_wd(st.w.data_ptr(), st.g.data_ptr(), N.ptr(m), N.ptr(v),
                                            self.shadow.data_ptr(), self.segs_dev.data_ptr(),
                                            self.table_dev.data_ptr(), self.nblocks, self.iterations.data_ptr(),
                                            h.kind, h.lr, h.mom, h.b1, h.b2, h.eps, 1.0, int(zero_grad), lr_ptr, mode,
                                            c, N.ptr(self.clip_scale), self.wd_dev.data_ptr(), N.stream_ptr())
                N.check(rc, "tde_optim_apply_wd")
                return
            rc = lib.tde_optim_apply_clip(st.w.data_ptr(), st.g.data_ptr(), N.ptr(m), N.ptr(v),
                                          self.shadow.data_ptr(), self.segs_dev.data_ptr(),
                                          self.table_dev.data_ptr(), self.nblocks, self.iterations.data_ptr(), h.kind,
                                          h.lr, h.mom, h.b1, h.b2, h.eps, 1.0, int(zero_grad), lr_ptr, mode, c,
                                          N.ptr(self.clip_scale), N.stream_ptr())
            N.check(rc, "tde_optim_apply_clip")
            return
        rc = N.hip().tde_optim_apply(st.w.data_ptr(), st.g.data_ptr(), N.ptr(m), N.ptr(v), self.shadow.data_ptr(),
                                     self.segs_dev.data_ptr(), self.table_dev.data_ptr(), self.nblocks,
                                     self.iterations.data_ptr(), h.kind, h.lr, h.mom, h.b1, h.b2, h.eps, 1.0,
                                     int(zero_grad), N.ptr(self.lr_word) if sch is not None else None,
                                     N.stream_ptr())
        N.check(rc, "tde_optim_apply")


def extra_metrics(model):
    """The names of the model's compiled metrics beyond the accuracy ("" without any), for a plan's warning that
    it declines them."""
    lay = getattr(getattr(model, "_metric_names", None), "layout", None)
    return lay.describe() if lay is not None else ""


def match_convnet(model, loss):
    """Pattern of the DWK/TF2M small CNN: Conv2D(3x3,relu,bias) on 1 channel ·
    MaxPooling2D(2) · Flatten · Dense(bias[,relu]) · Dense(bias[,softmax]) + softmax-CE with a trivial spec
    (the sparse loss, or the categorical one without label smoothing; no class weights)."""
    from .. import losses as LS
    ls = [l for l in model.body_layers if not isinstance(l, L.InputLayer)]   # (without the input stage)
    if ls and isinstance(ls[0], L.Reshape) and len(ls[0].target_shape) == 3:
        ls = ls[1:]
    if len(ls) != 5 or not LS.is_softmax_ce(loss):
        return None
    c, p, f, d1, d2 = ls
    ok = (isinstance(c, L.Conv2D) and c.kernel_size == (3, 3) and c.strides == (1, 1) and c.padding == "valid"
          and c.activation == "relu" and c.use_bias and c.input_shape[-1] == 1
          and c.input_shape[1] % 2 == 0
          and isinstance(p, L.MaxPooling2D) and p.pool_size == (2, 2) and p.strides == (2, 2) and p.padding == "valid"
          and isinstance(f, L.Flatten)
          and isinstance(d1, L.Dense) and d1.activation in (None, "relu")
          and isinstance(d2, L.Dense) and d2.use_bias and d2.activation in (None, "softmax"))
    if not ok:
        return None
    if (d2.activation == "softmax") == bool(loss.from_logits):
        return None  # probabilities fed to from_logits=True (or logits w/o from_logits): not fusable
    if LS.nontrivial(loss):
        import warnings
        warnings.warn(f"model {model.name!r}: the fused small-CNN step has no loss head for "
                      f"{LS.spec_reason(loss)}; running the per-layer kernel plan")
        return None
    extra = extra_metrics(model)
    if extra:
        import warnings
        warnings.warn(f"model {model.name!r}: the fused small-CNN step has no metric head for {extra}; running "
                      "the per-layer kernel plan")
        return None
    force_gen = os.environ.get("TDE_CONVNET_GENERIC", "0") == "1"   # A/B: the generic kernels at any width
    if c.filters != 32 or d1.units != 64 or force_gen:
        # the hand-tuned step is the reference's Conv2D(32)/Dense(64) (distributed_with_keras.py:34,37);
        # other widths run the generic fused kernels (float32 policy, ConvNetGenPlan) when they fit them,
        # and say so instead of silently dropping to the slower per-layer plan otherwise
        H, W = c.input_shape[0], c.input_shape[1]
        why = None
        if Kb.global_policy().compute_dtype != torch.float32:
            why = "the generic widths are implemented for the float32 policy"
        elif not gen_fits(c.filters, d1.units):
            why = (f"Conv2D filters must be one of {GEN_FILTERS} and Dense units a multiple of 32 up to 256 whose "
                   "backward fits a CU's LDS (Conv2D(48): up to 192 units, Conv2D(64): up to 160)")
        elif d2.units > 16 or W % 4 or W > 32 or H % 2:
            why = "at most 16 classes and an even height, width a multiple of 4 up to 32"
        if why is None:
            return dict(conv=c, pool=p, dense1=d1, dense2=d2, generic=True)
        import warnings
        warnings.warn(f"model {model.name!r}: no fused small-CNN step for Conv2D({c.filters}) + Dense({d1.units}) "
                      f"({why}); running the per-layer kernel plan")
        return None
    if d2.units > 16:
        import warnings
        warnings.warn(f"model {model.name!r}: the fused small-CNN step takes at most 16 classes (got {d2.units}); "
                      "running the per-layer kernel plan")
        return None
    return dict(conv=c, pool=p, dense1=d1, dense2=d2)


GEN_FILTERS = (16, 32, 48, 64)      # csrc/kernels/convnet_gen.hip instantiations
GEN_UNITS = tuple(range(32, 257, 32))


def gen_fits(filters, units):
    """Whether the generic fused kernels are instantiated for Conv2D(filters) / Dense(units): the backward's
    LDS carve at 8 waves (csrc/kernels/convnet_gen.hip BwdCfg) within a CU's 160 KB."""
    if filters not in GEN_FILTERS or units not in GEN_UNITS:
        return False
    cc, hd = filters, units
    rg = hd + 4
    lds = (64 * rg * 4 + cc * rg * 4 + cc * 68 * 4 + 64 * 16 * 4 + 64 * cc + 64 * (cc + 4) * 4
           + max(4096 + 64 * 17 * 4, 8 * 10 * cc * 4) + hd * 17 * 4 + 16 * 4 + 64 * 4)
    return lds <= 160 * 1024


def _env_count(name, default):
    """A replica count from the environment, 1..8."""
    return max(1, min(8, int(os.environ.get(name, str(default)))))


class SmallCnnPlan(ReplicaPlan):
    """What the two fused small-CNN plans share: the variables by role, the geometry, and the state of the
    two-launch step around the launches themselves —

      hpre2   the big Dense's pre-activation by step parity, ``hrep`` split-K replicas each (the forward's
              adders per address spread out, the consumers sum them; TDE_CONVNET_HREP), and ``hpre`` for
              eval / predict
      gconv   the conv gradients by step parity, ``crep`` replicas of the conv segments' span each (backward
              workgroup x adds into replica x % crep: same-address float atomics from every workgroup
              serialise at the memory side; TDE_CONVNET_GREP).  Step mode "local": the deferred update of
              step t (``pend`` flags it, ``iter_prev`` is its step count) is applied on the fly by forward
              t+1, committed by backward t+1 and flushed by ``finish()``; "xgmi": the all-reduce sums the
              replicas of set 0 (``_xg_rep``); "plain" adds into the gradient bucket
      hsnap   the head variables as of the step's forward ([b1 | W2 | b2], written by the forward): the
              backward's trunk reads them while its head workgroup updates the originals

    A subclass supplies the launches and their descriptors (``set_step_mode``, ``train_step``,
    ``_infer_forward``) and, where it differs, ``_size_replicas`` and ``_conv_ranges``."""
    _commit_count = None   # device counter of committed conv updates, where the plan keeps one

    def __init__(self, model, store, device, batch, global_batch, optimizer, pattern):
        super().__init__(model, store, device, batch, global_batch, optimizer)
        from ..ops import kernels as K
        self.K = K
        c, d1, d2 = pattern["conv"], pattern["dense1"], pattern["dense2"]
        self.H, self.W, self.C = c.input_shape[0], c.input_shape[1], c.filters
        self.P = ((self.H - 2) // 2) * ((self.W - 2) // 2)
        self.Hd, self.Cls = d1.units, d2.units
        self.pre_relu = d1.activation == "relu"
        self.logits_out = d2.activation is None
        n = lambda l, w: f"{l.name}/{w}"  # noqa: E731
        self.names = dict(wc=n(c, "kernel"), bc=n(c, "bias"), w1=n(d1, "kernel"),
                          b1=n(d1, "bias") if d1.use_bias else None, w2=n(d2, "kernel"), b2=n(d2, "bias"))
        seg = store.segments
        sw, sb = seg[self.names["wc"]], seg[self.names["bc"]]
        self._conv_lo = min(sw.offset, sb.offset)
        self._conv_span = max(sw.offset + sw.numel, sb.offset + sb.numel) - self._conv_lo
        foreign = any(nm not in (self.names["wc"], self.names["bc"]) and
                      self._conv_lo <= seg[nm].offset < self._conv_lo + self._conv_span for nm in store.order)
        self.hrep, self.crep = _env_count("TDE_CONVNET_HREP", 4), _env_count("TDE_CONVNET_GREP", 8)
        self._size_replicas(foreign)
        B, dev, Hd, C_ = self.B, self.device, self.Hd, self.Cls
        f32 = dict(dtype=torch.float32, device=dev)
        self.hpre2 = torch.zeros(2, self.hrep, B, Hd, **f32)
        self.hpre = torch.zeros(B, Hd, **f32)
        self.probs = torch.zeros(B, C_, **f32)
        self.parity = 0
        self.gconv = torch.zeros(2, self.crep, self._conv_span, **f32)
        self.pend = torch.zeros(2, dtype=torch.int32, device=dev)
        self.iter_prev = torch.zeros(1, dtype=torch.int64, device=dev)
        self.hsnap = torch.zeros(Hd + Hd * C_ + C_, **f32)
        self._hs_b1 = self.hsnap[:Hd]
        self._hs_w2 = self.hsnap[Hd: Hd + Hd * C_].view(Hd, C_)
        self._hs_b2 = self.hsnap[Hd + Hd * C_:]
        self._flush = None

    def _size_replicas(self, foreign):
        """Settle ``hrep`` / ``crep`` (preset from the environment) and ``_xg_rep``: whether the xGMI all-reduce
        takes the conv gradients from the replicas of set 0.  ``foreign``: another variable's segment lies
        inside the conv span, so a range over the span would cover it too."""
        raise NotImplementedError

    def supports_step_mode(self, mode):
        if mode == "plain":
            return True
        return self._opt_fused() and self.device.type == "cuda" and mode in ("local", "xgmi")

    def _v(self, key):
        nm = self.names[key]
        return None if nm is None else self.store.view(nm)

    def _g(self, key):
        nm = self.names[key]
        return None if nm is None else self.store.grad(nm)

    # ------------------------------------------------------------------ the conv-gradient sets
    def _gset(self, q, key):
        """Replica 0 of conv variable ``key``'s gradient in parity set q."""
        sg = self.store.segments[self.names[key]]
        lo = sg.offset - self._conv_lo
        return self.gconv[q, 0, lo: lo + sg.numel].view(sg.shape)

    def _gbase(self, q):
        """Pointer that indexes parity set q's replica 0 with the flat-buffer offsets."""
        return self.gconv[q].data_ptr() - 4 * self._conv_lo

    def _reads_set(self, spec, q):
        """Point an update descriptor (``g`` / ``grep`` / ``grep_stride``) at the replicas of parity set q."""
        spec.g = self._gbase(q)
        spec.grep, spec.grep_stride = self.crep, self._conv_span
        return spec

    def _conv_ranges(self):
        """[(lo, n), ...] of the flat buffers that the commit / flush launches update."""
        return [(self._conv_lo, self._conv_span)]

    def _conv_apply(self, q, m, v):
        """``FlatApply`` of the deferred conv update waiting in parity set q (the commit and the flush)."""
        f = self.K.flat_apply_spec(self.optimizer, self.store.w, None, m, v, self.iterations, self.pend[q],
                                   self._conv_ranges())
        f.count = self.K._P(self._commit_count)
        return self._reads_set(f, q)

    def _conv_grads(self, q):
        """(dwc, dbc, sets) the backward of parity q adds the conv gradients into; ``sets``: replica 0 of a
        parity set (the launch spreads its workgroups over the ``crep`` replicas), not the gradient bucket."""
        if self.step_mode == "local":
            return self._gset(q, "wc"), self._gset(q, "bc"), True
        if self.step_mode == "xgmi" and self._xg_rep:
            return self._gset(0, "wc"), self._gset(0, "bc"), True
        return self._g("wc"), self._g("bc"), False

    def _head_vars(self):
        """(b1, W2, b2) the backward's trunk reads: in the fused step the forward's snapshot (the head workgroup
        updates the originals)."""
        if self.step_mode == "local":
            return (self._hs_b1 if self.names["b1"] is not None else None), self._hs_w2, self._hs_b2
        return self._v("b1"), self._v("w2"), self._v("b2")

    # ------------------------------------------------------------------ plan interface
    def push_range(self):
        """Bucket range the backward can push into the xGMI owners itself: the big Dense kernel's gradient
        (the reference's Dense(64): 99.7 % of the gradient bytes)."""
        seg = self.store.segments[self.names["w1"]]
        return seg.offset, seg.offset + seg.numel

    def xg_apply_spec(self):
        spec = super().xg_apply_spec()
        if self._xg_rep:   # the conv gradients wait in the replicas of set 0: the all-reduce sums (and zeroes) them
            spec.rep, spec.nrep = self.gconv[0].data_ptr(), self.crep
            spec.rep_lo, spec.rep_hi = self._conv_lo, self._conv_lo + self._conv_span
            spec.rep_stride = self._conv_span
        return spec

    def finish(self):
        if self.step_mode == "local":
            # only the last step's conv update can be pending (each backward commits the previous one)
            self.K.flat_apply(self._flush[1 - self.parity])

    def step_invariants(self):
        """The deferred conv update's state between executions (step mode "local"; synchronises): nothing
        pending, every gradient replica consumed."""
        torch.cuda.synchronize(self.device)
        return dict(pending=[int(v) for v in self.pend.cpu()], gconv_abs_max=float(self.gconv.abs().max()))

    def on_weights_loaded(self):
        # loaded weights replace whatever update was outstanding
        self.pend.zero_()
        self.gconv.zero_()
        self.store.g.zero_()

    def apply(self):
        # step mode "plain": multi-tensor optimizer (+ grad zeroing + bf16 shadow refresh)
        self.opt.apply()

    def _infer_forward(self, x, B):
        """The forward outside training: the Dense pre-activation of x[:B] into ``hpre``."""
        raise NotImplementedError

    def _infer_head(self, B, labels, scale, **kw):
        self.K.head_xent(self.hpre, self._v("w2"), self._v("b2"), labels, B=B, scale=scale, pre_bias=self._v("b1"),
                         pre_relu=self.pre_relu, compute_grad=False, zero_hin=True, **kw)

    def eval_step(self, x, y, B=None):
        B = self.B if B is None else B
        self._infer_forward(x, B)
        self._infer_head(B, y, self.scale, metrics=self.metrics)

    def predict(self, x, B=None):
        B = self.B if B is None else B
        self._infer_forward(x, B)
        self._infer_head(B, self._dummy_labels(B), 1.0, probs=self.probs, probs_are_logits=self.logits_out)
        return self.probs[:B]


class ConvNetPlan(SmallCnnPlan):
    """The DWK/TF2M small CNN as two HIP launches per training step, in the precision of the global
    policy: float32 (the reference's; csrc/kernels/convnet_f32.hip, exact-f32 MFMA over the f32 master
    weights) or mixed_bfloat16 (csrc/kernels/convnet.hip, bf16 MFMA over bf16 weight shadows):

      forward   conv+bias+ReLU+pool fused with the Dense(64) matmul (split-K atomics into hpre[p])
      backward  the head recomputed from hpre[p] in every workgroup (softmax-CE, dlogits, Dense(64)
                input gradient), Dense(64) weight / input gradients, pool / ReLU routing and conv
                gradients; one extra workgroup makes the head's own gradients and the metrics; the
                other parity buffer hpre[1-p] is zeroed for the next forward

    followed, by step mode, by the multi-tensor optimizer ("plain"), nothing ("local": the update
    runs inside the two launches, the conv update deferred to the next step and flushed by
    ``finish()``), or the xGMI all-reduce that applies it ("xgmi").  ``parity`` alternates per step;
    the Program captures one hipGraph per starting parity."""
    kind = "fused_convnet"

    hyper_by_value = ("local", "xgmi")   # "xgmi": set_step_mode also caches ``_slots`` for xg_apply_spec
    _mode_set = None

    def __init__(self, model, store, device, batch, global_batch, optimizer, loss, pattern):
        # read by _size_replicas, which the base constructor calls
        self.f32 = Kb.global_policy().compute_dtype == torch.float32
        # TDE_DETERMINISTIC=1 (debugging): one pre-activation replica per forward workgroup (each address
        # receives exactly one add, into zeros; the consumer sums the replicas in order) and the conv
        # gradients as per-workgroup partials summed in order by an extra launch: bitwise-reproducible
        # training steps at the cost of 2.8 MB of replicas and one launch per step
        self.det = os.environ.get("TDE_DETERMINISTIC", "0") not in ("", "0")
        super().__init__(model, store, device, batch, global_batch, optimizer, pattern)
        self.loss = loss
        self.compute_dtype = "fp32" if self.f32 else "bf16"
        Kf, Bp, dev = self.P * self.C, _round8(self.B), self.device
        self.Pt = torch.zeros(Kf, Bp, dtype=torch.float32 if self.f32 else torch.bfloat16, device=dev)
        self.amax = torch.zeros(Kf // 32, 4, Bp, dtype=torch.int64, device=dev)  # [P][C/8][B] argmax bytes
        self.cpart = torch.zeros((self.P + 1) * 320, dtype=torch.float32, device=dev) if self.det else None
        # bf16: the forward reads the Dense(64) kernel from the row-major bf16 shadow (the one the
        # backward reads and the fused updates rewrite); TDE_CONVNET_W1=col keeps a transposed [64, K]
        # copy for it.  f32: both read the f32 master kernel itself (no shadow exists).
        self.w1_rows = self.f32 or os.environ.get("TDE_CONVNET_W1", "rows") != "col"
        if self.f32:
            shadows = {}
        else:
            shadows = {self.names["w1"]: ("row",) if self.w1_rows else ("row", "col")}
        self.opt = OptimizerKernel(store, optimizer, shadows, self.iterations, self) if optimizer is not None else None
        self._shadow_only = None
        if self.opt is None and shadows:
            # eval/predict-only plan still needs the bf16 weight copies
            from ..optimizers import SGD
            self._shadow_only = OptimizerKernel(store, SGD(0.0), shadows, self.iterations)
        if self.f32:
            self.W1row = store.view(self.names["w1"])
            self.W1col = None
        else:
            ok = self.opt or self._shadow_only
            self.W1row = ok.shadow_views[(self.names["w1"], "row")]
            self.W1col = None if self.w1_rows else ok.shadow_views[(self.names["w1"], "col")]
        self.W1fwd = self.W1row if self.w1_rows else self.W1col
        # device counters of the deferred conv update (the local step's invariants, ``step_invariants``):
        # [0] updates committed (by the next backward's head workgroup or the flush), [1] forwards that
        # applied a pending update on the fly
        self.ucount = torch.zeros(2, dtype=torch.int64, device=dev)
        self._commit_count = self.ucount[0]
        self._fopt = self._bopt = None
        self._slots = (None, None)

    def _size_replicas(self, foreign):
        if self.det:   # one split-K replica per forward workgroup, the conv partials in ``cpart``
            self.hrep, self.crep = self.P, 1
        # the all-reduce sums the replicas over the whole span: float32 form, nothing else inside it; the
        # fused step's ranges name the two segments, so it keeps its replicas either way
        self._xg_rep = self.f32 and self.crep > 1 and not foreign

    def _conv_ranges(self):
        seg = self.store.segments
        return [(seg[self.names[k]].offset, seg[self.names[k]].numel) for k in ("wc", "bc")]

    def set_step_mode(self, mode):
        super().set_step_mode(mode)
        if mode != self._mode_set:
            self.gconv.zero_()   # the replicas change roles between the step modes
            self.pend.zero_()
        self._mode_set = mode
        self._fopt = self._bopt = self._flush = None
        self._slots = (None, None)
        if mode == "plain":
            return
        K, st, opt = self.K, self.store, self.optimizer
        self._slots = m, v = K.opt_slots(st, opt)
        if mode != "local":
            return
        seg = st.segments
        P_ = K._P
        self._fopt, self._bopt, self._flush = [], [], []
        for q in (0, 1):
            # forward of parity q: the deferred update of the previous step (parity 1-q), t = iter_prev
            f = self._reads_set(K.step_opt(opt, st.w, None, m, v, self.iter_prev, self.pend[1 - q]), 1 - q)
            f.fly_count = self.ucount[1].data_ptr()
            f.hsrc_w2, f.hsrc_b2 = self._v("w2").data_ptr(), self._v("b2").data_ptr()
            f.hsrc_b1 = self._v("b1").data_ptr() if self.names["b1"] is not None else None
            f.hsnap, f.hC = self.hsnap.data_ptr(), self.Cls
            self._fopt.append(f)
            b1 = self.names["b1"]
            self._bopt.append(K.BwdOpt(
                K.opt_hyper(opt), P_(st.w), P_(m), P_(v),
                seg[self.names["w1"]].offset, seg[self.names["w2"]].offset, seg[self.names["b2"]].offset,
                seg[b1].offset if b1 is not None else -1, P_(self.W1col),
                self.W1col.stride(0) if self.W1col is not None else 0, P_(self.iterations), P_(self.iter_prev),
                self._conv_apply(1 - q, m, v), self.pend[q].data_ptr(), self.crep, self._conv_span))
            self._flush.append(self._conv_apply(q, m, v))

    def push_range(self):
        return super().push_range() if self.f32 else None   # the bf16 backward cannot push

    def xg_apply_spec(self):
        if self.f32:   # no shadow: the all-reduce updates the f32 master weights only
            return super().xg_apply_spec()
        st, K = self.store, self.K
        m, v = self._slots
        seg = st.segments[self.names["w1"]]
        return K.XgApply(K.opt_hyper(self.optimizer), K._P(st.w), K._P(m), K._P(v), K._P(self.iterations),
                         K._P(self.W1row), seg.offset, seg.offset + seg.numel, K._P(self.W1col), self.Hd,
                         self.W1col.stride(0) if self.W1col is not None else 0)

    def step_invariants(self):
        """The base's, and every step's update committed exactly once."""
        iv = super().step_invariants()
        return dict(commits=int(self.ucount[0]), applied_on_the_fly=int(self.ucount[1]), **iv)

    def trace_tensors(self):
        """Per-step state recorded by ``Program.enable_trace`` (diagnostics)."""
        return [self.store.w, self.gconv.view(-1), self.pend.float(), self.metrics]

    def effective_weights(self, trace):
        """From ``Program.enable_trace`` rows of this plan ([S, n]): the weights each step left for the next
        forward, [S, store.w.numel()] — in step mode "local" the stored conv weights lag by the pending
        (deferred) update, which the next forward applies on the fly (SGD: w - lr * sum of the pending
        parity's gradient replicas)."""
        nw, ng = self.store.w.numel(), self.gconv.numel()
        w = trace[:, :nw].clone()
        if self.step_mode != "local":
            return w
        if self.optimizer.kind_id != 0:
            raise NotImplementedError("effective_weights: the deferred update is reconstructed for SGD only")
        g = trace[:, nw: nw + ng].reshape(len(trace), 2, self.crep, self._conv_span).sum(dim=2)
        pend = trace[:, nw + ng: nw + ng + 2]
        lo, span = self._conv_lo, self._conv_span
        lr = float(self.optimizer.learning_rate)
        for q in (0, 1):
            w[:, lo: lo + span] -= lr * g[:, q] * (pend[:, q:q + 1] != 0)
        return w

    def on_weights_loaded(self):
        if not self.f32:
            (self.opt or self._shadow_only).refresh_shadows()
        super().on_weights_loaded()

    def _forward(self, x, B, hpre, with_pt, opt=None, train=False, hrep=1):
        # launch 1: conv+bias+ReLU+pool fused with the Dense(Hd) matmul (split-K atomics into hpre,
        # which the previous backward / head launch left zeroed)
        seg = self.store.segments
        self.K.convnet_fwd(x[:B], self._v("wc"), self._v("bc"), self.W1fwd, hpre,
                           self.Pt if with_pt else None, self.amax, opt=opt,
                           off_wc=seg[self.names["wc"]].offset, off_bc=seg[self.names["bc"]].offset,
                           inc_iter=self.iterations if train else None, hrep=hrep)

    def _infer_forward(self, x, B):
        self._forward(x, B, self.hpre, False)

    def train_step(self, x, y, B=None):
        K = self.K
        B = self.B if B is None else B
        self.step_rows = B
        q = self.parity
        local = self.step_mode == "local"
        self._forward(x, B, self.hpre2[q], True, self._fopt[q] if local else None, train=True, hrep=self.hrep)
        # launch 2: head + trunk backward (fused step: the updates too, and its descriptor carries crep)
        dwc, dbc, sets = self._conv_grads(q)
        push = self._push if self.step_mode == "xgmi" else None
        b1, w2, b2 = self._head_vars()
        K.convnet_bwd(x, self.amax, self.hpre2[q], self.hpre2[1 - q], b1, w2, b2, y,
                      scale=self.scale, pre_relu=self.pre_relu, metrics=self.metrics, W1row=self.W1row, Pt=self.Pt,
                      dW1=self._g("w1"), dwc=dwc, dbc=dbc, dW2=self._g("w2"), db2=self._g("b2"), db1=self._g("b1"),
                      B=B, opt=self._bopt[q] if local else None, cpart=self.cpart, push=push,
                      crep=self.crep if sets and not local else 1, crep_stride=self._conv_span)
        self._pushed = push is not None
        if self.det:
            K.convnet_cgrad_reduce(self.cpart, self.P, dwc, dbc)
        self.parity = 1 - q


class ConvNetGenPlan(SmallCnnPlan):
    """The DWK/TF2M small CNN at the user's own widths — Conv2D(F in 16/32/48/64) · MaxPool(2) · Flatten ·
    Dense(U in 32/64/96/128) · Dense(<= 16) (distributed_with_keras.py:33-43 and tf2_mnist_distributed.py:66-72
    with other filter / unit counts) — as two fused float32 HIP launches per step (csrc/kernels/convnet_gen.hip):

      forward   conv+bias+ReLU+pool fused with the Dense(U) matmul (split-K atomics into hpre replicas)
      backward  every workgroup recomputes the head from hpre, then the Dense(U) weight / input gradients
                of its pooled position, the pool / ReLU routing MFMA and the conv gradients; one extra
                workgroup makes the head's own gradients, the metrics and the step count

    followed, by step mode, by the multi-tensor optimizer ("plain"), nothing ("local": two launches per step —
    each backward workgroup applies the optimizer to the Dense(U) rows it owns in place, no other workgroup of
    the launch reading them; the head workgroup updates the head in place while the trunk reads the forward's
    snapshot of it; the conv update is deferred: the next forward applies it on the fly, the next backward's
    head workgroup commits it, ``finish()`` flushes the last one), or the xGMI all-reduce that applies it
    ("xgmi"; the backward pushes the Dense(U) gradient rows straight into the owners' windows).  The
    reference's own Conv2D(32)/Dense(64) keeps the hand-tuned ``ConvNetPlan``."""
    kind = "fused_convnet_generic"

    hyper_by_value = ("local",)

    def __init__(self, model, store, device, batch, global_batch, optimizer, loss, pattern):
        from ..ops import kernels as K
        c, d1 = pattern["conv"], pattern["dense1"]
        if not K.cgen_supported(c.filters, d1.units):
            raise NotImplementedError(f"convnet_gen: Conv2D({c.filters}) + Dense({d1.units}) not instantiated")
        if os.environ.get("TDE_DETERMINISTIC", "0") not in ("", "0"):
            import warnings
            warnings.warn("TDE_DETERMINISTIC: the generic-width fused CNN step adds its split-K and conv-gradient "
                          "partials with float atomics; its steps are not bitwise reproducible")
        super().__init__(model, store, device, batch, global_batch, optimizer, pattern)
        Bp, dev = _round8(self.B), self.device
        self.Pt = torch.zeros(self.P * self.C, Bp, dtype=torch.float32, device=dev)
        self.amax = torch.zeros(self.P, self.C // 8, Bp, dtype=torch.int64, device=dev)
        self.W1 = store.view(self.names["w1"])
        self.opt = OptimizerKernel(store, optimizer, {}, self.iterations, self) if optimizer is not None else None
        self._copt = self._fly = self._hopt = self._commit = None

    def _size_replicas(self, foreign):
        if foreign:   # every consumer here walks one range over the whole span
            self.crep = 1
        self._xg_rep = self.crep > 1

    def set_step_mode(self, mode):
        super().set_step_mode(mode)
        self._copt = self._fly = self._hopt = self._commit = self._flush = None
        self.gconv.zero_()
        self.pend.zero_()
        if mode != "local":
            return
        K, st, o = self.K, self.store, self.optimizer
        m, v = K.opt_slots(st, o)
        h = K.opt_hyper(o)
        seg = st.segments
        at = lambda t, name: None if t is None or name is None else t.data_ptr() + 4 * seg[self.names[name]].offset  # noqa: E731
        self._copt = K.CgenOpt(h, at(st.w, "w1"), at(m, "w1"), at(v, "w1"), self.iterations.data_ptr())
        self._fly, self._hopt, self._commit, self._flush = [], [], [], []
        for q in (0, 1):
            # forward of parity q: the update of the previous step (set 1-q) on the fly, the head snapshot
            self._fly.append(K.CgenFly(
                h, self.pend[1 - q].data_ptr(), self._gset(1 - q, "wc").data_ptr(),
                self._gset(1 - q, "bc").data_ptr(), self.crep, self._conv_span, at(m, "wc"), at(m, "bc"), at(v, "wc"),
                at(v, "bc"), self.iter_prev.data_ptr(), at(st.w, "b1"), at(st.w, "w2"), at(st.w, "b2"), self.hsnap.data_ptr(), self.Cls))
            # backward of parity q: the head in place, the previous step's conv update committed, set q flagged
            b1 = self.names["b1"]
            self._hopt.append(K.CgenHead(
                h, st.w.data_ptr(), K._P(m), K._P(v), seg[self.names["w2"]].offset, seg[self.names["b2"]].offset,
                seg[b1].offset if b1 is not None else -1, self.iterations.data_ptr(), self.pend[q].data_ptr(),
                self.iter_prev.data_ptr()))
            self._commit.append(self._conv_apply(1 - q, m, v))
            self._flush.append(self._conv_apply(q, m, v))

    def _infer_forward(self, x, B):
        self.K.cgen_fwd(x, self._v("wc"), self._v("bc"), self.W1, self.hpre, self.Pt, self.amax, B=B)

    def train_step(self, x, y, B=None):
        K = self.K
        B = self.B if B is None else B
        self.step_rows = B
        q = self.parity
        local = self.step_mode == "local"
        # the fused step's Adam t is read by every backward workgroup: the forward advances the counter
        K.cgen_fwd(x, self._v("wc"), self._v("bc"), self.W1, self.hpre2[q], self.Pt, self.amax, B=B,
                   inc_iter=self.iterations if local else None, fly=self._fly[q] if local else None)
        dwc, dbc, sets = self._conv_grads(q)
        push = self._push if self.step_mode == "xgmi" else None
        b1, w2, b2 = self._head_vars()
        K.cgen_bwd(x, self.amax, self.hpre2[q], self.hpre2[1 - q], b1, w2, b2, y,
                   scale=self.scale, pre_relu=self.pre_relu, metrics=self.metrics, W1=self.W1, Pt=self.Pt,
                   dW1=None if local else self._g("w1"), dwc=dwc, dbc=dbc, dW2=self._g("w2"),
                   db2=self._g("b2"), db1=self._g("b1"), B=B, iterations=None if local else self.iterations,
                   opt=self._copt if local else None, crep=self.crep if sets else 1,
                   crep_stride=self._conv_span if sets else 0,
                   hopt=self._hopt[q] if local else None, fcommit=self._commit[q] if local else None, push=push)
        self._pushed = push is not None
        self.parity = 1 - q


# ---------------------------------------------------------------------------------------
def make_plan(model, store, device, batch, global_batch, optimizer, loss, prefer=None, class_weight=False):
    """``class_weight``: the program is built for ``fit(class_weight=)`` -- the plan keeps a table of row weights
    by class (a non-trivial loss spec: the small-net, layer-wise and reference plans)."""
    device = torch.device(device)
    if class_weight:
        from .. import losses as LS
        loss = LS.with_class_weight(loss)
    prefer = prefer or os.environ.get("TDE_EXECUTOR")
    if device.type == "cuda" and prefer != "reference":
        pat = match_convnet(model, loss)
        if pat is not None and prefer in (None, "fused"):
            cls = ConvNetGenPlan if pat.get("generic") else ConvNetPlan
            return cls(model, store, device, batch, global_batch, optimizer, loss, pat)
        if prefer in (None, "fused", "bncnn"):
            from . import bncnn
            plan = bncnn.try_make(model, store, device, batch, global_batch, optimizer, loss)
            if plan is not None:
                return plan
        if prefer in (None, "fused", "smallnet"):
            from . import smallnet
            plan = smallnet.try_make(model, store, device, batch, global_batch, optimizer, loss)
            if plan is not None:
                return plan
        from . import layerwise
        plan = layerwise.try_make(model, store, device, batch, global_batch, optimizer, loss)
        if plan is not None:
            return plan
        raise NotImplementedError(
            f"model {model.name!r} has layers without a HIP kernel path; set TDE_EXECUTOR=reference to run it "
            "with torch reference ops")
    return ReferencePlan(model, store, device, batch, global_batch, optimizer, loss)
