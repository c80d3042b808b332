"""Losses: SparseCategoricalCrossentropy, CategoricalCrossentropy (one-hot labels, label
smoothing) and their string aliases; ``fit(class_weight=)``'s per-row weight.

Keras semantics (distributed_with_keras.py:41, mnist_keras_distributed.py:114,
tf2_mnist_distributed.py:81-83):
  * ``from_logits=True``: softmax-CE on logits.
  * ``from_logits=False`` on the output of a softmax activation: computed from the
    pre-softmax logits (stable; quirk Q5).  On other probabilities: clip to
    [eps, 1-eps] and take -log p.
  * reduction AUTO/SUM_OVER_BATCH_SIZE: under a distribution strategy the
    per-replica loss is sum / GLOBAL batch, so SUM-all-reduced gradients equal
    the mean gradient.  NONE returns per-sample losses.

The softmax-CE head (every plan's loss) for an integer label y over C classes, label smoothing e and the row
weight w = class_weight.get(y, 1.0) of ``fit``:

    t_c      = (1 - e) [c == y] + e / C
    loss     = w ((1 - e) (lse - l_y) + e (lse - mean_c l_c))
    dlogit_c = w (p_c - t_c) scale

``CategoricalCrossentropy`` takes exactly one-hot rows, converted to int32 class indices where the labels are
staged (``onehot_to_index``); soft targets are not supported, ``label_smoothing`` is the supported form.  The
weight applies to the training loss and gradient only, and the reported loss is ``sum w_i l_i / rows``.  A spec
with e == 0 and no class weights is *trivial*: the sparse loss after label conversion, on every plan.
"""
from __future__ import annotations

import copy
import math

import numpy as np
import torch
import torch.nn.functional as F

EPSILON = 1e-7


class Reduction:
    AUTO = "auto"
    NONE = "none"
    SUM = "sum"
    SUM_OVER_BATCH_SIZE = "sum_over_batch_size"


class Loss:
    def __init__(self, reduction=Reduction.AUTO, name=None):
        self.reduction = reduction
        self.name = name

    def per_sample(self, y_true, y_pred, *, pred_is_logits=False):
        raise NotImplementedError

    def __call__(self, y_true, y_pred, sample_weight=None):
        ls = self.per_sample(y_true, y_pred)
        if sample_weight is not None:
            ls = ls * torch.as_tensor(sample_weight, dtype=ls.dtype, device=ls.device)
        if self.reduction == Reduction.NONE:
            return ls
        if self.reduction == Reduction.SUM:
            return ls.sum()
        return ls.sum() / max(ls.shape[0], 1)


class SparseCategoricalCrossentropy(Loss):
    def __init__(self, from_logits=False, reduction=Reduction.AUTO, name="sparse_categorical_crossentropy"):
        super().__init__(reduction, name)
        self.from_logits = from_logits

    def per_sample(self, y_true, y_pred, *, pred_is_logits=False, class_weight=None):
        y = torch.as_tensor(y_true, device=y_pred.device).reshape(-1).long()
        if self.from_logits or pred_is_logits:
            if class_weight is not None:
                return softmax_ce(y_pred, y, 0.0, class_weight)
            return F.cross_entropy(y_pred.float(), y, reduction="none")
        p = y_pred.float().clamp(EPSILON, 1 - EPSILON)
        ls = -torch.log(p.gather(1, y[:, None]).squeeze(1))
        if class_weight is not None:
            ls = ls * torch.as_tensor(class_weight, dtype=ls.dtype, device=ls.device)[y]
        return ls

    def get_config(self):
        return {"from_logits": self.from_logits, "reduction": self.reduction, "name": self.name}


def softmax_ce(logits, y, smooth=0.0, class_weight=None):
    """Per-row softmax cross-entropy of float32 ``logits`` [N, C] against integer labels ``y`` [N] with label
    smoothing and a [C] table of row weights by class (None: 1), the formula at the top written out from
    ``log_softmax`` (``F.cross_entropy(weight=, label_smoothing=)`` weights the smoothing term per class and
    normalises by the weights' sum: not these semantics).  A label outside [0, C) has weight 1 and l_y := max."""
    z = logits.float()
    C = z.shape[1]
    lsm = F.log_softmax(z, dim=1)
    ok = (y >= 0) & (y < C)
    yc = y.clamp(0, C - 1)
    nll = -lsm.gather(1, yc[:, None]).squeeze(1)
    if not bool(ok.all()):
        # lse - max, the max a constant: the gradient keeps no one-hot term
        nll = torch.where(ok, nll, torch.logsumexp(z, dim=1) - z.max(dim=1).values.detach())
    ls = (1.0 - smooth) * nll + smooth * (-lsm.mean(dim=1)) if smooth else nll
    if class_weight is not None:
        w = torch.as_tensor(class_weight, dtype=ls.dtype, device=ls.device)
        ls = ls * torch.where(ok, w[yc], torch.ones((), dtype=ls.dtype, device=ls.device))
    return ls


class CategoricalCrossentropy(Loss):
    """Keras ``CategoricalCrossentropy``: one-hot ``y`` [N, C] (or the int32 class indices the plans are fed
    after ``onehot_to_index``), ``label_smoothing`` in [0, 1)."""

    def __init__(self, from_logits=False, label_smoothing=0.0, reduction=Reduction.AUTO,
                 name="categorical_crossentropy"):
        super().__init__(reduction, name)
        self.from_logits = from_logits
        try:
            e = float(label_smoothing)
        except (TypeError, ValueError):
            raise ValueError(f"label_smoothing must be a number in [0, 1), got {label_smoothing!r}") from None
        if not math.isfinite(e) or not 0.0 <= e < 1.0:
            raise ValueError(f"label_smoothing must be finite and in [0, 1), got {label_smoothing!r}")
        self.label_smoothing = e

    def per_sample(self, y_true, y_pred, *, pred_is_logits=False, class_weight=None):
        C = y_pred.shape[1]
        if not torch.is_tensor(y_true) or (y_true.dim() == 2 and y_true.shape[1] != 1):
            yt = y_true.detach().cpu().numpy() if torch.is_tensor(y_true) else np.asarray(y_true)
            if yt.ndim == 2 and yt.shape[1] != 1:
                y_true = onehot_to_index(yt, C)
        y = torch.as_tensor(y_true, device=y_pred.device).reshape(-1).long()
        e = self.label_smoothing
        if self.from_logits or pred_is_logits:
            if not e and class_weight is None:   # the trivial spec: the sparse loss, to the bit
                return F.cross_entropy(y_pred.float(), y, reduction="none")
            return softmax_ce(y_pred, y, e, class_weight)
        # probabilities that are not a softmax layer's: normalise, clip, -sum t log p (Keras)
        p = y_pred.float()
        p = (p / p.sum(dim=1, keepdim=True)).clamp(EPSILON, 1 - EPSILON)
        t = F.one_hot(y, C).to(p.dtype) * (1.0 - e) + e / C
        ls = -(t * torch.log(p)).sum(dim=1)
        if class_weight is not None:
            ls = ls * torch.as_tensor(class_weight, dtype=ls.dtype, device=ls.device)[y]
        return ls

    def get_config(self):
        return {"from_logits": self.from_logits, "label_smoothing": self.label_smoothing,
                "reduction": self.reduction, "name": self.name}

    @classmethod
    def from_config(cls, config):
        return cls(**config)


# ---------------------------------------------------------------------------------------
# what the plans ask of a loss
def is_softmax_ce(loss):
    return isinstance(loss, (SparseCategoricalCrossentropy, CategoricalCrossentropy))


def smoothing(loss):
    return float(getattr(loss, "label_smoothing", 0.0))


def class_weighted(loss):
    """The program was built for ``fit(class_weight=)``: the plan owns a table of row weights by class."""
    return bool(getattr(loss, "_class_weighted", False))


def with_class_weight(loss):
    """A copy of ``loss`` that tells a plan to keep a class-weight table (``fit`` fills it in place)."""
    out = copy.copy(loss)
    out._class_weighted = True
    return out


def nontrivial(loss):
    """Label smoothing or class weights: the spec the small-net, layer-wise and reference plans run."""
    return smoothing(loss) != 0.0 or class_weighted(loss)


def spec_reason(loss):
    """The non-trivial part of the spec, for a plan's warning that it declines it."""
    why = []
    if smoothing(loss):
        why.append(f"{type(loss).__name__}(label_smoothing={smoothing(loss):g})")
    if class_weighted(loss):
        why.append("fit(class_weight=)")
    return " with ".join(why)


def onehot_to_index(y, num_classes):
    """int32 class indices of exactly one-hot rows ``y`` [N, num_classes] (any numeric dtype: one entry == 1,
    the rest == 0)."""
    y = np.asarray(y)
    if y.ndim != 2 or y.shape[1] != int(num_classes):
        raise ValueError(f"categorical_crossentropy takes one-hot labels of shape [N, {int(num_classes)}] "
                         f"(the model's classes), got {tuple(y.shape)}")
    if y.dtype.kind not in "biuf":
        raise ValueError(f"one-hot labels must be numeric, got dtype {y.dtype}")
    ones = y == 1
    if not bool((ones | (y == 0)).all()) or not bool((ones.sum(axis=1) == 1).all()):
        raise ValueError("categorical_crossentropy: every label row must be exactly one-hot (one entry 1, the "
                         "rest 0); soft targets are not supported -- label_smoothing= is the supported form")
    return ones.argmax(axis=1).astype(np.int32)


def labels_for(loss, y, num_classes):
    """The flat class indices a plan is fed, from what the user's dataset yields for ``loss``: one-hot rows
    for the categorical loss, [N] / [N, 1] indices for the sparse one (as they are)."""
    if isinstance(loss, CategoricalCrossentropy):
        if torch.is_tensor(y):
            y = y.detach().cpu().numpy()
        return onehot_to_index(y, num_classes)
    return y.reshape(-1) if torch.is_tensor(y) else np.asarray(y).reshape(-1)


def class_weight_table(class_weight, num_classes):
    """float32 [num_classes] of ``class_weight.get(c, 1.0)`` (Keras 3), validated: int keys in [0, C), finite
    values >= 0."""
    if not isinstance(class_weight, dict):
        raise ValueError(f"class_weight must be a dict of class index -> weight, got {type(class_weight).__name__}")
    C = int(num_classes)
    table = np.ones(C, dtype=np.float32)
    for k, v in class_weight.items():
        if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or not 0 <= int(k) < C:
            raise ValueError(f"class_weight keys must be ints in [0, {C}), got {k!r}")
        try:
            f = float(v)
        except (TypeError, ValueError):
            raise ValueError(f"class_weight[{k!r}] must be a number, got {v!r}") from None
        if not math.isfinite(f) or f < 0 or f > float(np.finfo(np.float32).max):
            raise ValueError(f"class_weight[{k!r}] must be finite and >= 0, got {v!r}")
        table[int(k)] = f
    return table


def get(identifier):
    if isinstance(identifier, Loss):
        return identifier
    if identifier in ("sparse_categorical_crossentropy", "SparseCategoricalCrossentropy"):
        return SparseCategoricalCrossentropy()
    if identifier in ("categorical_crossentropy", "CategoricalCrossentropy"):
        return CategoricalCrossentropy()
    raise ValueError(f"unsupported loss {identifier!r}")
