"""Weight regularizers (``tf.keras.regularizers``): ``L1``, ``L2``, ``L1L2`` for ``kernel_regularizer`` /
``bias_regularizer`` (Conv2D, Dense) and ``gamma_regularizer`` / ``beta_regularizer`` (BatchNormalization).

A regularized variable adds ``P = l1 * sum|w| + l2 * sum w^2`` to the loss: the ``loss`` that ``fit`` logs and
``evaluate`` returns is the mean per-sample loss plus every P, and ``2 l2 w + l1 sgn(w)`` (``sgn(+-0) = 0``) is
added to the aggregated gradient, after the all-reduce and before a clip.  On the GPU both run inside the
captured step (csrc/include/tde_reg.h); ``reg_reference`` and ``penalty`` are the torch forms the reference
plan uses.
"""
from __future__ import annotations

import math

import torch


def _coef(name, v):
    try:
        c = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a finite float >= 0 (got {v!r})") from None
    if not (c >= 0.0 and math.isfinite(c)):
        raise ValueError(f"{name} must be a finite float >= 0 (got {v!r})")
    return c


class Regularizer:
    l1 = 0.0
    l2 = 0.0

    def __call__(self, x):
        """The penalty of tensor ``x`` (torch, in x's dtype)."""
        x = torch.as_tensor(x)
        p = torch.zeros((), dtype=x.dtype, device=x.device)
        if self.l1:
            p = p + self.l1 * x.abs().sum()
        if self.l2:
            p = p + self.l2 * x.square().sum()
        return p

    @property
    def coefficients(self):
        return (self.l1, self.l2)

    def __eq__(self, other):
        return isinstance(other, Regularizer) and self.coefficients == other.coefficients

    def __hash__(self):
        return hash(self.coefficients)

    def __repr__(self):
        return f"<{type(self).__name__} {self.get_config()}>"


class L1L2(Regularizer):
    def __init__(self, l1=0.0, l2=0.0):
        self.l1 = _coef("l1", 0.0 if l1 is None else l1)
        self.l2 = _coef("l2", 0.0 if l2 is None else l2)

    def get_config(self):
        return {"l1": self.l1, "l2": self.l2}


class L1(Regularizer):
    def __init__(self, l1=0.01):
        self.l1 = _coef("l1", l1)

    def get_config(self):
        return {"l1": self.l1}


class L2(Regularizer):
    def __init__(self, l2=0.01):
        self.l2 = _coef("l2", l2)

    def get_config(self):
        return {"l2": self.l2}


def l1_l2(l1=0.01, l2=0.01):
    return L1L2(l1=l1, l2=l2)


l1 = L1
l2 = L2

_CLASSES = {"L1": L1, "L2": L2, "L1L2": L1L2}
_STRINGS = {"l1": L1, "l2": L2, "l1_l2": l1_l2}


def serialize(reg):
    return None if reg is None else {"class_name": type(reg).__name__, "config": reg.get_config()}


def deserialize(cfg):
    if cfg is None:
        return None
    if cfg.get("class_name") not in _CLASSES:
        raise ValueError(f"unknown regularizer {cfg!r}")
    return _CLASSES[cfg["class_name"]](**cfg.get("config", {}))


def get(identifier):
    """None, a ``Regularizer``, ``get_config()``'s serialized form, or one of the strings "l1", "l2", "l1_l2"
    (Keras's default coefficient 0.01)."""
    if identifier is None or isinstance(identifier, Regularizer):
        return identifier
    if isinstance(identifier, dict):
        return deserialize(identifier)
    if isinstance(identifier, str):
        if identifier in _STRINGS:
            return _STRINGS[identifier]()
        if identifier in _CLASSES:
            return _CLASSES[identifier]()
    raise ValueError(f"unsupported regularizer {identifier!r}")


# ---------------------------------------------------------------------------------------
def coefficients(model):
    """{variable full name: (l1, l2)} of the model's regularized trainable variables (non-zero ones only)."""
    out = {}
    for layer in getattr(model, "layers", None) or ():
        for s in getattr(layer, "weight_specs", ()):
            c1, c2 = getattr(s, "l1", 0.0), getattr(s, "l2", 0.0)   # a spec from before the regularizers: none
            if s.trainable and (c1 or c2):
                out[s.full_name] = (float(c1), float(c2))
    return out


def segments(model, store):
    """[(offset, numel, l1, l2)] of the regularized variables in ``store``'s flat buffers, in store order."""
    co = coefficients(model)
    return [(store.segments[n].offset, store.segments[n].numel) + co[n]
            for n in store.names(trainable=True) if n in co]


@torch.no_grad()
def reg_reference(w, g, segs):
    """The kernels' gradient in torch: g += 2 l2 w + l1 sgn(w) over ``segs`` (``segments()``), in place."""
    for off, n, c1, c2 in segs:
        x = w[off: off + n]
        g[off: off + n].add_(2.0 * c2 * x + c1 * torch.sign(x))
    return g


def penalty(w, segs):
    """Sum of the penalties of the flat weights ``w`` over ``segs``; differentiable, in w's dtype."""
    p = torch.zeros((), dtype=w.dtype, device=w.device)
    for off, n, c1, c2 in segs:
        x = w[off: off + n]
        p = p + c1 * x.abs().sum() + c2 * x.square().sum()
    return p
