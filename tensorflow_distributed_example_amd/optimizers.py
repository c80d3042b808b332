"""Optimizers: Keras SGD (v2: distributed_with_keras.py:42,
tf2_mnist_distributed.py:137), TF1 GradientDescentOptimizer
(mnist_keras_distributed.py:111), Adam (BASELINE north star) and RMSprop (the
default of Keras's ``compile()``).

On the GPU the update runs as ONE multi-tensor HIP kernel over the flat
parameter buffer (csrc/kernels/optim.hip) that also zeroes gradients, refreshes
bf16 weight shadows and advances the device-resident ``iterations`` counter.
``apply_reference`` is the torch implementation of the same math (CPU backend
and numerics oracle).

``learning_rate`` is a float or a ``schedules.LearningRateSchedule`` (``schedules.py``): the update that
is the k-th ever applied uses ``lr_at(k)``.  On the GPU a schedule is evaluated from the device counter
inside the captured step (csrc/include/tde_sched.h), so ``key()`` holds its configuration, not a rate.

``clipvalue`` / ``clipnorm`` / ``global_clipnorm`` (at most one, as in Keras 3) clip the aggregated gradient
before the update (TF 2.4+ order: after the all-reduce): ``clip_reference`` is the torch form, on the GPU two
norm launches and a clipped variant of the multi-tensor launch run inside the captured step
(csrc/include/tde_clip.h).

``weight_decay`` (Keras 2.11+; ``AdamW``) is decoupled weight decay: before the gradient step of a variable,
``w <- w - (w * weight_decay) * lr`` with the rate this step uses (the schedule's value, never Adam's
bias-corrected step size); the step then starts from the decayed weight.  Every trainable variable decays unless
``exclude_from_weight_decay`` names it; ``0`` and ``None`` mean off.  ``decay_reference`` is the torch form, on
the GPU the WD variants of the multi-tensor launch read a per-variable decay (csrc/include/tde_reg.h).  The
layers' weight regularizers (``regularizers.py``) are applied to the aggregated gradient before a clip.
"""
from __future__ import annotations

import math

import torch

from . import schedules
from .schedules import LearningRateSchedule

KIND = {"sgd": 0, "momentum": 1, "nesterov": 2, "adam": 3, "rmsprop": 4, "rmsprop_momentum": 5}
# kinds the fused step kernels, the xGMI all-reduce and the parameter server apply themselves (opt_step in
# csrc/include/tde_optim.h); the others run through the multi-tensor launch or the small-net commit only
FUSED_KINDS = (0, 1, 2, 3)
# optimizer.clip[0] -> the kernels' mode (csrc/include/tde_clip.h)
CLIP_MODE = {"clipvalue": 1, "clipnorm": 2, "global_clipnorm": 3}


def _clip_of(clipnorm, clipvalue, global_clipnorm):
    given = [(k, v) for k, v in (("clipnorm", clipnorm), ("clipvalue", clipvalue),
                                 ("global_clipnorm", global_clipnorm)) if v is not None]
    if len(given) > 1:
        raise ValueError("only one of clipnorm, clipvalue and global_clipnorm can be set (got "
                         + ", ".join(f"{k}={v!r}" for k, v in given) + ")")
    if not given:
        return None
    mode, c = given[0]
    try:
        c = float(c)
    except (TypeError, ValueError):
        raise ValueError(f"{mode} must be a positive finite float (got {given[0][1]!r})") from None
    if not (c > 0.0 and math.isfinite(c)):
        raise ValueError(f"{mode} must be a positive finite float (got {c!r})")
    return mode, c


def _decay_of(weight_decay):
    if weight_decay is None:
        return None
    try:
        wd = float(weight_decay)
    except (TypeError, ValueError):
        raise ValueError(f"weight_decay must be a finite float >= 0 (got {weight_decay!r})") from None
    if not (wd >= 0.0 and math.isfinite(wd)):
        raise ValueError(f"weight_decay must be a finite float >= 0 (got {weight_decay!r})")
    return wd


class Optimizer:
    kind = "sgd"

    def __init__(self, learning_rate=0.01, name=None, clipnorm=None, clipvalue=None, global_clipnorm=None,
                 weight_decay=None, **kw):
        if "lr" in kw:   # the Keras 2 spelling
            learning_rate = kw.pop("lr")
        if kw:
            raise TypeError(f"{type(self).__name__}() got unexpected keyword argument(s) "
                            + ", ".join(repr(k) for k in sorted(kw)))
        self.learning_rate = learning_rate
        self.name = name or type(self).__name__
        self.iterations = 0  # host mirror; device counter lives in the program
        self._clip = _clip_of(clipnorm, clipvalue, global_clipnorm)
        self.weight_decay = _decay_of(weight_decay)
        self._wd_exclude = (frozenset(), ())   # (full names, substrings of full names)
        self._plan_built = False               # a plan holds the per-variable decay: exclusions are closed

    @property
    def decay(self):
        """The decoupled weight decay in effect: a positive float, or None (``weight_decay`` None or 0)."""
        return self.weight_decay if self.weight_decay else None

    def exclude_from_weight_decay(self, var_list=None, var_names=None):
        """Keras's: the variables of ``var_list`` (full names, or objects with a ``full_name``) and every
        variable whose full name contains one of ``var_names`` do not decay.  Before the first plan is built."""
        if self._plan_built:
            raise ValueError("exclude_from_weight_decay() must be called before the optimizer has built a plan "
                             "(before fit / the first training step)")
        names = set(self._wd_exclude[0])
        for v in var_list or []:
            n = v if isinstance(v, str) else getattr(v, "full_name", None)
            if not isinstance(n, str):
                raise TypeError(f"exclude_from_weight_decay: {v!r} is neither a variable name nor has a full_name")
            names.add(n)
        subs = tuple(self._wd_exclude[1]) + tuple(str(n) for n in (var_names or []))
        self._wd_exclude = (frozenset(names), subs)

    def decays(self, full_name):
        """Whether the variable ``full_name`` decays under this optimizer."""
        if self.decay is None or full_name in self._wd_exclude[0]:
            return False
        return not any(sub in full_name for sub in self._wd_exclude[1])

    @torch.no_grad()
    def decay_reference(self, w, segments, step):
        """Decoupled weight decay of the flat weights ``w`` in place, the kernels' order of operations:
        ``w - (w * wd) * lr`` over ``segments``, the (offset, numel) of the variables that decay."""
        if self.decay is None:
            return w
        lr = self.lr_at(step)
        for o, n in segments:
            x = w[o: o + n]
            x.sub_((x * self.decay) * lr)
        return w

    @property
    def clip(self):
        """None, or (mode, c) with mode "clipvalue", "clipnorm" or "global_clipnorm" (constructor-only)."""
        return self._clip

    @property
    def clipvalue(self):
        return self._clip[1] if self._clip and self._clip[0] == "clipvalue" else None

    @property
    def clipnorm(self):
        return self._clip[1] if self._clip and self._clip[0] == "clipnorm" else None

    @property
    def global_clipnorm(self):
        return self._clip[1] if self._clip and self._clip[0] == "global_clipnorm" else None

    @torch.no_grad()
    def clip_reference(self, g, segments):
        """Clips the flat (aggregated) gradient ``g`` in place: ``segments`` are the (offset, numel) of the
        trainable variables; what lies between them is left alone.  The kernels' order: each element times
        the scale c / max(norm, c), a zero gradient scaled by exactly 1."""
        if self._clip is None:
            return g
        mode, c = self._clip
        views = [g[o: o + n] for o, n in segments]
        if mode == "clipvalue":
            for x in views:
                x.clamp_(-c, c)
            return g
        sq = [x.double().square().sum() for x in views]
        if mode == "global_clipnorm":
            sq = [torch.stack(sq).sum()] * len(views) if views else []
        for x, s in zip(views, sq):
            norm = s.sqrt().to(g.dtype)
            x.mul_(c / torch.clamp(norm, min=c))
        return g

    @property
    def learning_rate(self):
        """A float, or the ``schedules.LearningRateSchedule`` object it was given (as in Keras)."""
        return self._lr

    @learning_rate.setter
    def learning_rate(self, value):
        if isinstance(value, dict) and "class_name" in value:   # get_config()'s form of a schedule
            value = schedules.deserialize(value)
        self._lr = value if isinstance(value, LearningRateSchedule) else float(value)

    @property
    def lr(self):
        return self.learning_rate

    @property
    def schedule(self):
        """The learning-rate schedule, or None under a constant rate."""
        return self._lr if isinstance(self._lr, LearningRateSchedule) else None

    def lr_at(self, step):
        """The rate of the update that is the ``step``-th ever applied (0 for the first)."""
        return self._lr(step) if isinstance(self._lr, LearningRateSchedule) else self._lr

    def current_lr(self):
        """``lr_at`` at the host mirror of the step counter: the rate the next update uses."""
        return self.lr_at(self.iterations)

    @property
    def kind_id(self):
        return KIND[self.kind]

    def slot_names(self):
        return []

    def hparams(self):
        return dict(mom=0.0, b1=0.9, b2=0.999, eps=1e-7)

    def key(self):
        """Everything a kernel argument struct holds of this optimizer: a plan that built its structs at one
        key rebuilds them when the key has changed (compared for equality only, never stored)."""
        sch = self.schedule
        # a schedule's key is its configuration: constant over the run, so nothing is captured again
        return (self.kind_id, sch.key() if sch is not None else self._lr, tuple(sorted(self.hparams().items())),
                self._clip, self.decay, (tuple(sorted(self._wd_exclude[0])), self._wd_exclude[1]))

    def apply_reference(self, w, g, slots, step):
        raise NotImplementedError

    def get_config(self):
        sch = self.schedule
        cfg = {"name": self.name, "learning_rate": schedules.serialize(sch) if sch is not None else self._lr}
        if self._clip is not None:   # the one that is set: ``type(opt)(**config)`` rebuilds the optimizer
            cfg[self._clip[0]] = self._clip[1]
        if self.weight_decay is not None:   # like the clip: only when given, so an optimizer without it keeps its config
            cfg["weight_decay"] = self.weight_decay
        return cfg


class SGD(Optimizer):
    def __init__(self, learning_rate=0.01, momentum=0.0, nesterov=False, name="SGD", **kw):
        super().__init__(learning_rate, name, **kw)
        self.momentum = float(momentum)
        self.nesterov = bool(nesterov)
        if self.momentum < 0:
            raise ValueError("momentum must be >= 0")

    @property
    def kind(self):
        if self.momentum == 0.0:
            return "sgd"
        return "nesterov" if self.nesterov else "momentum"

    def slot_names(self):
        return ["momentum"] if self.momentum else []

    def hparams(self):
        return dict(mom=self.momentum, b1=0.9, b2=0.999, eps=1e-7)

    @torch.no_grad()
    def apply_reference(self, w, g, slots, step):
        lr = self.lr_at(step)
        if self.momentum == 0.0:
            w.sub_(lr * g)
            return
        v = slots["momentum"]
        v.mul_(self.momentum).sub_(lr * g)
        if self.nesterov:
            w.add_(self.momentum * v - lr * g)
        else:
            w.add_(v)

    def get_config(self):
        return {**super().get_config(), "momentum": self.momentum, "nesterov": self.nesterov}


class GradientDescentOptimizer(SGD):
    """TF1 ``tf.train.GradientDescentOptimizer(learning_rate)`` (mnist_keras_distributed.py:111)."""

    def __init__(self, learning_rate, use_locking=False, name="GradientDescent"):
        super().__init__(learning_rate, 0.0, False, name)

    def get_config(self):
        cfg = super().get_config()
        cfg.pop("weight_decay", None)   # not an argument of the TF1 optimizer
        return cfg


class Adam(Optimizer):
    kind = "adam"

    def __init__(self, learning_rate=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7, name="Adam", **kw):
        super().__init__(learning_rate, name, **kw)
        self.beta_1, self.beta_2, self.epsilon = float(beta_1), float(beta_2), float(epsilon)

    def slot_names(self):
        return ["m", "v"]

    def hparams(self):
        return dict(mom=0.0, b1=self.beta_1, b2=self.beta_2, eps=self.epsilon)

    @torch.no_grad()
    def apply_reference(self, w, g, slots, step):
        t = step + 1
        m, v = slots["m"], slots["v"]
        m.mul_(self.beta_1).add_((1 - self.beta_1) * g)
        v.mul_(self.beta_2).add_((1 - self.beta_2) * g * g)
        lr_t = self.lr_at(step) * math.sqrt(1 - self.beta_2 ** t) / (1 - self.beta_1 ** t)
        w.sub_(lr_t * m / (v.sqrt() + self.epsilon))

    def get_config(self):
        return {**super().get_config(), "beta_1": self.beta_1, "beta_2": self.beta_2, "epsilon": self.epsilon}


class AdamW(Adam):
    """Keras ``AdamW``: Adam with decoupled weight decay (Loshchilov & Hutter), Keras's defaults."""

    def __init__(self, learning_rate=0.001, weight_decay=0.004, beta_1=0.9, beta_2=0.999, epsilon=1e-7, name="AdamW",
                 **kw):
        if weight_decay is None:
            raise ValueError("AdamW needs a weight_decay (got None); Adam is the optimizer without one")
        super().__init__(learning_rate, beta_1, beta_2, epsilon, name, weight_decay=weight_decay, **kw)


class RMSprop(Optimizer):
    """Keras ``RMSprop`` in the TF 2.x form.  Slots are TensorFlow's: ``rms`` and, with momentum,
    ``momentum`` -- in that order, so ``rms`` travels as the kernels' first slot pointer.  Epsilon sits
    outside the square root without momentum and inside it with momentum: TF's own inconsistency, kept."""

    def __init__(self, learning_rate=0.001, rho=0.9, momentum=0.0, epsilon=1e-7, centered=False, name="RMSprop",
                 **kw):
        super().__init__(learning_rate, name, **kw)
        self.rho, self.momentum, self.epsilon = float(rho), float(momentum), float(epsilon)
        self.centered = bool(centered)
        if self.centered:
            raise ValueError("RMSprop(centered=True) needs a third slot (the mean gradient); the flat store "
                             "and the kernel interfaces carry two slots")
        if not 0.0 <= self.rho < 1.0:
            raise ValueError("rho must be in [0, 1)")
        if self.momentum < 0:
            raise ValueError("momentum must be >= 0")

    @property
    def kind(self):
        return "rmsprop_momentum" if self.momentum > 0 else "rmsprop"

    def slot_names(self):
        return ["rms", "momentum"] if self.momentum > 0 else ["rms"]

    def hparams(self):
        return dict(mom=self.momentum, b1=0.0, b2=self.rho, eps=self.epsilon)

    @torch.no_grad()
    def apply_reference(self, w, g, slots, step):
        lr, r = self.lr_at(step), slots["rms"]
        r.mul_(self.rho).add_((1 - self.rho) * g * g)
        if self.momentum > 0:
            q = slots["momentum"]
            q.mul_(self.momentum).add_(lr * g / (r + self.epsilon).sqrt())   # epsilon inside the root (TF)
            w.sub_(q)
        else:
            w.sub_(lr * g / (r.sqrt() + self.epsilon))                        # epsilon outside the root (TF)

    def get_config(self):
        return {**super().get_config(), "rho": self.rho, "momentum": self.momentum, "epsilon": self.epsilon,
                "centered": self.centered}


def get(identifier):
    if isinstance(identifier, Optimizer):
        return identifier
    if isinstance(identifier, str):
        k = identifier.lower()
        if k == "sgd":
            return SGD()
        if k == "adam":
            return Adam()
        if k == "adamw":
            return AdamW()
        if k == "rmsprop":
            return RMSprop()
    raise ValueError(f"unsupported optimizer {identifier!r}")
