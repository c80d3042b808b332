"""Host wrapper for the softmax-CE launch with label smoothing and per-class row weights
(csrc/kernels/losshead.hip, csrc/include/tde_loss.h): what the layer-wise plan's head launches in place of
``layer_ops32.xent`` / ``layer_ops.xent`` when the loss has a non-trivial spec.  Same arguments and the same checks;
``dlogits`` is float32 or bfloat16, and the kernel keeps the arithmetic of the plain kernel of that type, so
``smooth=0`` with all-ones weights reproduces it bit for bit."""
from __future__ import annotations

import math

import torch

from .. import _native as N

_P = N.ptr


def _req(cond, msg):
    if not cond:
        raise ValueError(msg)


def _f32(t, n, what):
    _req(t is not None and t.dtype == torch.float32 and t.is_contiguous() and t.numel() >= n,
         f"{what}: f32 [{n}] expected")


def xent_spec(logits, labels, B, Cc, *, smooth=0.0, class_w=None, scale=1.0, dlogits=None, metrics=None, probs=None,
              probs_are_logits=False, iterations=None, bf16=None):
    """``bf16``: the arithmetic of the bf16 plain kernel (default: by the type of ``dlogits``, float32 without)."""
    B, Cc = int(B), int(Cc)
    _req(B >= 0 and Cc >= 1, "xent_spec shape")
    _f32(logits, B * Cc, "xent_spec logits")
    _req(labels.dtype == torch.int32 and labels.is_contiguous() and labels.numel() >= B, "xent_spec labels")
    _req(math.isfinite(smooth) and 0.0 <= smooth < 1.0, "xent_spec smooth: a float in [0, 1) expected")
    if class_w is not None:
        _f32(class_w, Cc, "xent_spec class_w")
    bf = bool(bf16)
    if dlogits is not None:
        _req(dlogits.dtype in (torch.float32, torch.bfloat16) and dlogits.is_contiguous()
             and dlogits.numel() >= B * Cc, f"xent_spec dlogits: f32 or bf16 [{B * Cc}] expected")
        _req(bf16 is None or bool(bf16) == (dlogits.dtype == torch.bfloat16), "xent_spec: bf16 contradicts dlogits")
        bf = dlogits.dtype == torch.bfloat16
    if probs is not None:
        _f32(probs, B * Cc, "xent_spec probs")
    if metrics is not None:
        _f32(metrics, 3, "xent_spec metrics")
    if iterations is not None:
        _req(iterations.dtype == torch.int64 and iterations.numel() >= 1, "xent_spec iterations")
    for t in (labels, class_w, dlogits, metrics, probs, iterations):
        _req(t is None or t.device == logits.device, "xent_spec: operands on one device expected")
    rc = N.hip().tde_xent_spec(_P(logits), Cc, _P(labels), B, Cc, float(scale), _P(dlogits), Cc, int(bf), _P(metrics),
                               _P(probs), int(probs_are_logits), _P(iterations), float(smooth), _P(class_w),
                               N.stream_ptr())
    N.check(rc, "tde_xent_spec")
