"""Metrics: ``'accuracy'`` (sparse categorical accuracy), the running loss mean, and the
classification metrics beyond them: top-k accuracy, crossentropy as a metric and the F-score.

Accumulators are device-resident.  Every plan owns ``metrics = [loss_sum, correct, count, 0]`` (f32), updated
inside the fused head kernel (no host sync per step).  A model compiled with any metric beyond the accuracy
runs plans that own a second f32 vector, ``metrics_ext``, laid out by ``metric_spec`` (``MetricSpec`` of
csrc/include/tde_metric.h): top-k hit counts, crossentropy sums and a ``C x C`` confusion block
``cm[label][argmax]``.  Across replicas both are SyncOnRead/SUM: ``read()`` all-reduces them only when a value
is read (progbar refresh, epoch end, evaluation end -- SURVEY §2.6 C3/C5); ``logs_from`` turns the concatenated
sums into the logged values in float64 on the host.

For a row with label ``y`` and logits ``l`` over ``C`` classes:

  * top-k: a hit iff ``0 <= y < C``, ``l_y`` is finite and ``#{c : l_c > l_y} < k`` (``tf.math.in_top_k``:
    classes tied across the boundary all count).  The logits are ranked even when the head is a softmax layer
    (quirk Q5): the ranking is monotone in them and has no saturation ties.
  * crossentropy: ``(1 - e)(lse - l_y) + e (lse - mean l)``, unweighted and without the regularizers' penalty
    -- the plain crossentropy beside a ``loss`` that carries class weights and penalties.
  * F-score: from the confusion counts of the lowest-index argmax against the label (below).

The non-sparse forms go with ``CategoricalCrossentropy`` (whose one-hot labels are class indices by the time a
plan sees them), the sparse forms with the sparse loss; both F-scores go with either (an extension of Keras,
whose F-scores take one-hot labels only).
"""
from __future__ import annotations

import math

import numpy as np
import torch

EPSILON = 1e-7
MAX_TOPK = 4            # MetricSpec.k
MAX_CE = 2              # MetricSpec.smooth
MAX_CM_CLASSES = 1024   # the confusion block is C x C words


class Metric:
    """A compiled metric: ``name`` is its key in the logs.  Compares equal to its name, so a resolved list reads
    as the list of log names."""
    kind = None
    sparse = None      # True: goes with the sparse loss, False: with the categorical one, None: with either

    def __init__(self, name):
        if not isinstance(name, str) or not name:
            raise ValueError(f"a metric's name must be a non-empty string, got {name!r}")
        self.name = name

    def __eq__(self, other):
        if isinstance(other, str):
            return self.name == other
        return type(other) is type(self) and other.get_config() == self.get_config()

    def __hash__(self):
        return hash(self.name)

    def __repr__(self):
        return f"{type(self).__name__}({', '.join(f'{k}={v!r}' for k, v in self.get_config().items())})"

    def get_config(self):
        return {"name": self.name}

    @classmethod
    def from_config(cls, config):
        return cls(**config)


class SparseCategoricalAccuracy(Metric):
    kind = "accuracy"
    name = "accuracy"

    def __init__(self, name="accuracy"):
        super().__init__(name)


class Mean:
    name = "loss"


class SparseTopKCategoricalAccuracy(Metric):
    """``k`` >= 1 (an int); ``k >= C`` is allowed: every row with a valid label and a finite ``l_y`` hits."""
    kind = "topk"
    sparse = True

    def __init__(self, k=5, name="sparse_top_k_categorical_accuracy"):
        super().__init__(name)
        if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or int(k) < 1:
            raise ValueError(f"{type(self).__name__}: k must be an int >= 1, got {k!r}")
        self.k = int(k)

    def get_config(self):
        return {"k": self.k, "name": self.name}


class TopKCategoricalAccuracy(SparseTopKCategoricalAccuracy):
    sparse = False

    def __init__(self, k=5, name="top_k_categorical_accuracy"):
        super().__init__(k, name)


class SparseCategoricalCrossentropy(Metric):
    """``from_logits`` must agree with the model's head (True: a linear ``Dense``, False: ``Dense(softmax)``, as
    for the loss); the string form takes the head's."""
    kind = "ce"
    sparse = True
    label_smoothing = 0.0

    def __init__(self, name="sparse_categorical_crossentropy", from_logits=False):
        super().__init__(name)
        self.from_logits = None if from_logits is None else bool(from_logits)

    def get_config(self):
        return {"name": self.name, "from_logits": self.from_logits}


class CategoricalCrossentropy(SparseCategoricalCrossentropy):
    sparse = False

    def __init__(self, name="categorical_crossentropy", from_logits=False, label_smoothing=0.0):
        super().__init__(name, from_logits)
        try:
            e = float(label_smoothing)
        except (TypeError, ValueError):
            raise ValueError(f"label_smoothing must be a number in [0, 1), got {label_smoothing!r}") from None
        if not math.isfinite(e) or not 0.0 <= e < 1.0:
            raise ValueError(f"label_smoothing must be finite and in [0, 1), got {label_smoothing!r}")
        self.label_smoothing = e

    def get_config(self):
        return {"name": self.name, "from_logits": self.from_logits, "label_smoothing": self.label_smoothing}


class FBetaScore(Metric):
    """Keras 3's formula over the confusion counts ``cm[label][argmax]``:
    ``p_c = tp / (tp + fp + eps)``, ``r_c = tp / (tp + fn + eps)``,
    ``f_c = (1 + beta^2) p_c r_c / (beta^2 p_c + r_c + eps)``, ``eps = 1e-7``; ``average="micro"`` sums the
    counts over the classes first, ``"macro"`` is the mean of ``f_c`` and ``"weighted"`` weighs ``f_c`` by the
    class's share of the labels.  ``threshold=None`` only: the prediction is the argmax, and ties at the maximum
    go to the lowest index, the accuracy's rule here (Keras marks every tied class as predicted).  Rows whose
    label is outside ``[0, C)`` do not enter the counts.  Accepted under the sparse loss too (class indices in
    place of one-hot rows): an extension of Keras.  ``average=None`` (a vector of per-class scores) is not
    supported: the logs are scalars."""
    kind = "fbeta"

    def __init__(self, average=None, beta=1.0, threshold=None, name="fbeta_score"):
        super().__init__(name)
        if average is None:
            raise NotImplementedError(f"{type(self).__name__}(average=None) logs a vector of per-class scores; "
                                      "only 'micro', 'macro' and 'weighted' are supported")
        if average not in ("micro", "macro", "weighted"):
            raise ValueError(f"{type(self).__name__}: average must be 'micro', 'macro' or 'weighted', "
                             f"got {average!r}")
        if threshold is not None:
            raise NotImplementedError(f"{type(self).__name__}(threshold={threshold!r}) is not supported: the "
                                      "prediction is the argmax (threshold=None)")
        if isinstance(beta, (bool, np.bool_)) or not isinstance(beta, (int, float, np.integer, np.floating)) \
                or not math.isfinite(float(beta)) or float(beta) <= 0.0:
            raise ValueError(f"{type(self).__name__}: beta must be a finite number > 0, got {beta!r}")
        self.average = average
        self.beta = float(beta)
        self.threshold = None

    def get_config(self):
        return {"average": self.average, "beta": self.beta, "threshold": None, "name": self.name}


class F1Score(FBetaScore):
    def __init__(self, average=None, threshold=None, name="f1_score"):
        super().__init__(average=average, beta=1.0, threshold=threshold, name=name)

    def get_config(self):
        return {"average": self.average, "threshold": None, "name": self.name}


_STRINGS = {
    "sparse_top_k_categorical_accuracy": SparseTopKCategoricalAccuracy,
    "top_k_categorical_accuracy": TopKCategoricalAccuracy,
    "sparse_categorical_crossentropy": lambda: SparseCategoricalCrossentropy(from_logits=None),
    "categorical_crossentropy": lambda: CategoricalCrossentropy(from_logits=None),
}


class MetricList(list):
    """The compiled metrics in compile order (the accuracy's aliases once); ``layout``: the ``MetricLayout`` of
    the entries beyond the accuracy, set by ``Model.compile`` (None: there are none)."""
    layout = None

    @property
    def extra(self):
        return [m for m in self if isinstance(m, Metric) and m.kind != "accuracy"]


def resolve(metrics, loss=None):
    """The metric objects of ``compile(metrics=)``.  ``"categorical_accuracy"`` is ``"accuracy"``'s alias under
    the categorical loss: the one-hot labels are class indices by the time a plan sees them, and the accuracy is
    argmax against the index either way.  With ``loss`` given, a sparse metric under the categorical loss (or
    the reverse) raises."""
    from .losses import CategoricalCrossentropy as CatLoss
    out = MetricList()
    for m in metrics or []:
        if m in ("accuracy", "acc", "sparse_categorical_accuracy") or isinstance(m, SparseCategoricalAccuracy):
            obj = m if isinstance(m, SparseCategoricalAccuracy) else SparseCategoricalAccuracy()
            obj.name = "accuracy"
        elif isinstance(m, str) and m == "categorical_accuracy" and isinstance(loss, CatLoss):
            obj = SparseCategoricalAccuracy()
        elif isinstance(m, str) and m in _STRINGS:
            obj = _STRINGS[m]()
        elif isinstance(m, Metric) and m.kind in ("topk", "ce", "fbeta"):
            obj = m
        else:
            raise ValueError(f"unsupported metric {m!r}")
        if obj.sparse is not None and loss is not None and obj.sparse == isinstance(loss, CatLoss):
            raise ValueError(f"metric {obj.name!r} ({type(obj).__name__}) does not go with the loss "
                             f"{type(loss).__name__}: the sparse forms go with SparseCategoricalCrossentropy, the "
                             "others with CategoricalCrossentropy")
        if obj.kind == "accuracy":
            if "accuracy" not in out:
                out.append(obj)
            continue
        if obj.name in out or obj.name == "loss":
            raise ValueError(f"duplicate metric name {obj.name!r}: give the second instance its own name=")
        out.append(obj)
    return out


def check_head(metrics, model):
    """``from_logits`` of every crossentropy metric against the model's head, by the rule the plans' matchers
    apply to the loss: True with a linear ``Dense`` head, False with ``Dense(softmax)``."""
    head = model.layers[-1]
    act = getattr(head, "activation", None)
    for m in metrics:
        if getattr(m, "kind", None) != "ce":
            continue
        if act not in (None, "softmax"):
            raise ValueError(f"metric {m.name!r}: the crossentropy metric needs a Dense head that is linear or a "
                             f"softmax, got activation {act!r}")
        if m.from_logits is None:
            m.from_logits = act != "softmax"
        elif (act == "softmax") == bool(m.from_logits):
            raise ValueError(f"metric {m.name!r}: from_logits={m.from_logits} contradicts the model's head "
                             f"({'a softmax layer' if act == 'softmax' else 'a linear layer: logits'})")


class MetricLayout:
    """Where each extra metric lives in ``metrics_ext`` (the fields of csrc/include/tde_metric.h's ``MetricSpec``):
    ``k`` / ``smooth``: the top-k and crossentropy entries, ``cm``: the confusion block is kept, ``off_*`` the
    word offset of each part, ``words`` the buffer's length; ``entries``: ``(metric, index)`` in compile order,
    index into ``k`` / ``smooth`` (None for an F-score)."""

    def __init__(self, classes, k, smooth, cm, entries):
        self.classes = int(classes)
        self.k, self.smooth, self.cm = list(k), list(smooth), int(bool(cm))
        self.off_topk = 0
        self.off_ce = len(self.k)
        self.off_cm = self.off_ce + len(self.smooth)
        self.words = self.off_cm + (self.classes ** 2 if self.cm else 0)
        self.entries = entries
        self._struct = None

    def fields(self):
        return dict(n_topk=len(self.k), k=self.k, n_ce=len(self.smooth), smooth=self.smooth, cm=self.cm,
                    off_topk=self.off_topk, off_ce=self.off_ce, off_cm=self.off_cm, words=self.words)

    def struct(self):
        """The ctypes ``MetricSpec`` the launches take (ops/metric_ops.py)."""
        if self._struct is None:
            from .ops import metric_ops
            self._struct = metric_ops.spec_struct(self)
        return self._struct

    def describe(self):
        return ", ".join(m.name for m, _ in self.entries)


def metric_spec(metrics, loss, classes):
    """The ``MetricLayout`` of the metrics beyond the accuracy for a model of ``classes`` classes under ``loss``,
    or None when there are none.  Top-k entries with the same ``k`` (and crossentropy entries with the same
    smoothing) share a word."""
    classes = int(classes)
    k, smooth, cm, entries = [], [], False, []
    for m in metrics or []:
        kind = getattr(m, "kind", None)
        if kind == "topk":
            if m.k not in k:
                k.append(m.k)
            entries.append((m, k.index(m.k)))
        elif kind == "ce":
            e = float(m.label_smoothing)
            if e not in smooth:
                smooth.append(e)
            entries.append((m, smooth.index(e)))
        elif kind == "fbeta":
            if classes > MAX_CM_CLASSES:
                raise ValueError(f"metric {m.name!r} ({type(m).__name__}) keeps a classes x classes confusion block "
                                 f"on the device: at most {MAX_CM_CLASSES} classes, the model has {classes}")
            cm = True
            entries.append((m, None))
    if not entries:
        return None
    if len(k) > MAX_TOPK:
        raise ValueError(f"at most {MAX_TOPK} different k among the top-k metrics, got {sorted(k)}")
    if len(smooth) > MAX_CE:
        raise ValueError(f"at most {MAX_CE} different label_smoothing values among the crossentropy metrics, "
                         f"got {sorted(smooth)}")
    return MetricLayout(classes, k, smooth, cm, entries)


def fbeta_from_confusion(cm, beta, average):
    """The F-score of a float64 ``[C, C]`` count matrix ``cm[label][prediction]`` (Keras 3's formula)."""
    cm = np.asarray(cm, dtype=np.float64)
    tp = np.diag(cm)
    fp = cm.sum(axis=0) - tp
    fn = cm.sum(axis=1) - tp
    support = cm.sum(axis=1)
    if average == "micro":
        tp, fp, fn = tp.sum(), fp.sum(), fn.sum()
    p = tp / (tp + fp + EPSILON)
    r = tp / (tp + fn + EPSILON)
    b2 = beta * beta
    f = (1.0 + b2) * (p * r) / (b2 * p + r + EPSILON)
    if average == "weighted":
        total = support.sum()
        return float((f * support / total).sum()) if total else float("nan")
    return float(np.mean(f))


def logs_from(acc: torch.Tensor, names):
    """The logged values of the concatenated accumulator ``[4 + layout.words]`` (``[4]`` without extra
    metrics), in compile order behind ``loss``, computed in float64."""
    a = acc.detach().double().cpu()
    cnt = float(a[2])
    nan = float("nan")
    logs = {"loss": float(a[0]) / cnt if cnt else nan}
    layout = getattr(names, "layout", None)
    ext = a[4:].numpy() if layout is not None else None
    if layout is not None and ext.shape[0] != layout.words:
        raise ValueError(f"accumulator of {a.numel()} words, the metrics' layout expects {4 + layout.words}")
    where = {m.name: (m, i) for m, i in layout.entries} if layout is not None else {}
    for n in names:
        if n == "accuracy":
            logs["accuracy"] = float(a[1]) / cnt if cnt else nan
        elif isinstance(n, Metric) and n.name in where:
            m, i = where[n.name]
            if m.kind == "topk":
                logs[m.name] = float(ext[layout.off_topk + i]) / cnt if cnt else nan
            elif m.kind == "ce":
                logs[m.name] = float(ext[layout.off_ce + i]) / cnt if cnt else nan
            else:
                C = layout.classes
                cm = ext[layout.off_cm: layout.off_cm + C * C].reshape(C, C)
                logs[m.name] = fbeta_from_confusion(cm, m.beta, m.average) if cnt else nan
    return logs
