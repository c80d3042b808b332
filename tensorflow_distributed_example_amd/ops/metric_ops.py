"""Host side of the metric launch (csrc/kernels/metrichead.hip, csrc/include/tde_metric.h): the ctypes
``MetricSpec`` and ``metric_rows``, what the layer-wise plan's head launches behind its softmax-CE launch when the
model was compiled with metrics beyond the accuracy.  The operands are checked here: the kernel indexes ``ext``
by the spec, and the spec's layout must be that of ``Cc`` classes."""
from __future__ import annotations

import ctypes as _ct

import torch

from .. import _native as N

_P = N.ptr

MAX_TOPK, MAX_CE, MAX_CM_CLASSES = 4, 2, 1024


class MetricSpec(_ct.Structure):
    """``MetricSpec`` (csrc/include/tde_metric.h)."""
    _fields_ = [("n_topk", _ct.c_int), ("k", _ct.c_int * MAX_TOPK), ("n_ce", _ct.c_int),
                ("smooth", _ct.c_float * MAX_CE), ("cm", _ct.c_int), ("off_topk", _ct.c_int), ("off_ce", _ct.c_int),
                ("off_cm", _ct.c_int), ("words", _ct.c_int)]


def _req(cond, msg):
    if not cond:
        raise ValueError(msg)


def spec_struct(layout):
    """The struct of a ``metrics.MetricLayout``."""
    f = layout.fields()
    _req(len(f["k"]) <= MAX_TOPK and len(f["smooth"]) <= MAX_CE, "metric spec: too many entries")
    s = MetricSpec(n_topk=f["n_topk"], n_ce=f["n_ce"], cm=f["cm"], off_topk=f["off_topk"], off_ce=f["off_ce"],
                   off_cm=f["off_cm"], words=f["words"])
    for i, k in enumerate(f["k"]):
        s.k[i] = int(k)
    for i, e in enumerate(f["smooth"]):
        s.smooth[i] = float(e)
    return s


def words_for(spec: MetricSpec, Cc):
    """The length of ``ext`` the spec's layout needs for ``Cc`` classes."""
    return spec.n_topk + spec.n_ce + (int(Cc) ** 2 if spec.cm else 0)


def metric_rows(logits, labels, B, Cc, spec: MetricSpec, ext, *, ldl=None):
    """``ext`` += the top-k hits, crossentropy sums and confusion counts of ``logits`` [B][ldl] (f32, ``ldl`` >=
    ``Cc``, default ``Cc``) against ``labels`` [B] (int32), on the current stream."""
    B, Cc = int(B), int(Cc)
    ldl = Cc if ldl is None else int(ldl)
    _req(B >= 0 and Cc >= 1 and ldl >= Cc, "metric_rows shape")
    _req(logits.dtype == torch.float32 and logits.is_contiguous() and logits.numel() >= (B - 1) * ldl + Cc,
         f"metric_rows logits: f32 [{B}][{ldl}] expected")
    _req(labels.dtype == torch.int32 and labels.is_contiguous() and labels.numel() >= B, "metric_rows labels")
    _req(isinstance(spec, MetricSpec), "metric_rows: a MetricSpec expected")
    _req(ext is not None and ext.dtype == torch.float32 and ext.is_contiguous()
         and ext.numel() >= max(spec.words, words_for(spec, Cc)), "metric_rows ext: f32 [spec.words] expected")
    _req(labels.device == logits.device and ext.device == logits.device, "metric_rows: operands on one device expected")
    rc = N.hip().tde_metric_rows(_P(logits), ldl, _P(labels), B, Cc, _ct.byref(spec), _P(ext), N.stream_ptr())
    N.check(rc, "tde_metric_rows")
