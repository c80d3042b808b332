"""Learning-rate schedules (``tde.optimizers.schedules``, ``tde.keras.optimizers.schedules``): the five
``tf.keras.optimizers.schedules`` classes of TF 2.x under their Keras argument names and defaults.

A schedule is a pure function of the optimizer's step counter.  ``__call__`` is the host twin (float64, a
Python float; the CPU backend and the tests use it); on the GPU the same function is evaluated from the
device-resident ``iterations`` word inside the captured step (``sched_lr`` in csrc/include/tde_sched.h, from
the ``LrSched`` descriptor that ``ops.kernels.lr_sched`` builds out of ``descriptor()``), so one captured
hipGraph serves the whole run and the rate may change between two steps of one replay.

Step convention (Keras): the update that is the k-th ever applied (k = 0 for the first) uses ``schedule(k)``.
"""
from __future__ import annotations

import math

KIND = {"none": 0, "exponential": 1, "inverse_time": 2, "polynomial": 3, "cosine": 4, "piecewise": 5}
STAIRCASE, CYCLE = 1, 2          # LrSched.flags
MAX_BOUNDARIES = 8               # LrSched is passed to the kernels by value


class LearningRateSchedule:
    """Base class: ``__call__(step) -> float``, ``get_config`` / ``from_config``."""

    def __call__(self, step):
        raise NotImplementedError

    def get_config(self):
        raise NotImplementedError

    @classmethod
    def from_config(cls, config):
        return cls(**config)

    def descriptor(self):
        """What the device evaluates: dict(kind, flags, lr0, p=(p0, p1, p2), decay_steps, bounds, values)."""
        raise NotImplementedError

    def key(self):
        """Hashable, constant over a run: part of ``Optimizer.key()``."""
        return (type(self).__name__,) + tuple((k, tuple(v) if isinstance(v, list) else v)
                                              for k, v in sorted(self.get_config().items()))


def _step(step):
    return max(int(step), 0)   # a negative step is treated as 0, on the host as on the device


class _Decay(LearningRateSchedule):
    def __init__(self, initial_learning_rate, decay_steps, name=None):
        self.initial_learning_rate = float(initial_learning_rate)
        self.decay_steps = int(decay_steps)
        self.name = name
        if self.decay_steps <= 0:
            raise ValueError(f"decay_steps must be positive (got {decay_steps})")


class ExponentialDecay(_Decay):
    """``lr0 * decay_rate ** (step / decay_steps)``; the exponent floored when ``staircase``."""

    def __init__(self, initial_learning_rate, decay_steps, decay_rate, staircase=False, name=None):
        super().__init__(initial_learning_rate, decay_steps, name)
        self.decay_rate, self.staircase = float(decay_rate), bool(staircase)

    def __call__(self, step):
        p = _step(step) / self.decay_steps
        if self.staircase:
            p = math.floor(p)
        return self.initial_learning_rate * self.decay_rate ** p

    def get_config(self):
        return dict(initial_learning_rate=self.initial_learning_rate, decay_steps=self.decay_steps,
                    decay_rate=self.decay_rate, staircase=self.staircase, name=self.name)

    def descriptor(self):
        return dict(kind=KIND["exponential"], flags=STAIRCASE * self.staircase, lr0=self.initial_learning_rate,
                    p=(self.decay_rate, 0.0, 0.0), decay_steps=self.decay_steps, bounds=(), values=())


class InverseTimeDecay(_Decay):
    """``lr0 / (1 + decay_rate * step / decay_steps)``; the quotient floored when ``staircase``."""

    def __init__(self, initial_learning_rate, decay_steps, decay_rate, staircase=False, name=None):
        super().__init__(initial_learning_rate, decay_steps, name)
        self.decay_rate, self.staircase = float(decay_rate), bool(staircase)

    def __call__(self, step):
        p = _step(step) / self.decay_steps
        if self.staircase:
            p = math.floor(p)
        return self.initial_learning_rate / (1.0 + self.decay_rate * p)

    def get_config(self):
        return dict(initial_learning_rate=self.initial_learning_rate, decay_steps=self.decay_steps,
                    decay_rate=self.decay_rate, staircase=self.staircase, name=self.name)

    def descriptor(self):
        return dict(kind=KIND["inverse_time"], flags=STAIRCASE * self.staircase, lr0=self.initial_learning_rate,
                    p=(self.decay_rate, 0.0, 0.0), decay_steps=self.decay_steps, bounds=(), values=())


class PolynomialDecay(_Decay):
    """``(lr0 - end) * (1 - s / D) ** power + end``.  Without ``cycle`` s = min(step, decay_steps) and
    D = decay_steps; with it s = step and D = decay_steps * max(1, ceil(step / decay_steps))."""

    def __init__(self, initial_learning_rate, decay_steps, end_learning_rate=1e-4, power=1.0, cycle=False,
                 name=None):
        super().__init__(initial_learning_rate, decay_steps, name)
        self.end_learning_rate, self.power, self.cycle = float(end_learning_rate), float(power), bool(cycle)

    def __call__(self, step):
        s, D = _step(step), self.decay_steps
        if self.cycle:
            D = D * max(1, -(-s // D))
        else:
            s = min(s, D)
        return ((self.initial_learning_rate - self.end_learning_rate) * (1.0 - s / D) ** self.power
                + self.end_learning_rate)

    def get_config(self):
        return dict(initial_learning_rate=self.initial_learning_rate, decay_steps=self.decay_steps,
                    end_learning_rate=self.end_learning_rate, power=self.power, cycle=self.cycle, name=self.name)

    def descriptor(self):
        return dict(kind=KIND["polynomial"], flags=CYCLE * self.cycle, lr0=self.initial_learning_rate,
                    p=(self.end_learning_rate, self.power, 0.0), decay_steps=self.decay_steps, bounds=(), values=())


class CosineDecay(_Decay):
    """``lr0 * ((1 - alpha) * 0.5 * (1 + cos(pi * s / decay_steps)) + alpha)``, s = min(step, decay_steps).
    (The warm-up arguments of newer Keras versions are not taken.)"""

    def __init__(self, initial_learning_rate, decay_steps, alpha=0.0, name=None):
        super().__init__(initial_learning_rate, decay_steps, name)
        self.alpha = float(alpha)

    def __call__(self, step):
        s = min(_step(step), self.decay_steps)
        c = 0.5 * (1.0 + math.cos(math.pi * s / self.decay_steps))
        return self.initial_learning_rate * ((1.0 - self.alpha) * c + self.alpha)

    def get_config(self):
        return dict(initial_learning_rate=self.initial_learning_rate, decay_steps=self.decay_steps,
                    alpha=self.alpha, name=self.name)

    def descriptor(self):
        return dict(kind=KIND["cosine"], flags=0, lr0=self.initial_learning_rate, p=(self.alpha, 0.0, 0.0),
                    decay_steps=self.decay_steps, bounds=(), values=())


class PiecewiseConstantDecay(LearningRateSchedule):
    """``values[0]`` while step <= boundaries[0], ``values[i]`` while boundaries[i-1] < step <= boundaries[i],
    ``values[-1]`` beyond the last boundary; the compares are integer (64-bit on the device)."""

    def __init__(self, boundaries, values, name=None):
        self.boundaries = [int(b) for b in boundaries]
        self.values = [float(v) for v in values]
        self.name = name
        if len(self.boundaries) > MAX_BOUNDARIES:
            raise ValueError(f"PiecewiseConstantDecay takes at most {MAX_BOUNDARIES} boundaries (got "
                             f"{len(self.boundaries)}): the schedule descriptor is passed to the kernels by value")
        if len(self.values) != len(self.boundaries) + 1:
            raise ValueError(f"PiecewiseConstantDecay: len(values) must be len(boundaries) + 1 (got "
                             f"{len(self.values)} values for {len(self.boundaries)} boundaries)")
        if any(b <= a for a, b in zip(self.boundaries, self.boundaries[1:])):
            raise ValueError("PiecewiseConstantDecay: boundaries must be strictly increasing")

    def __call__(self, step):
        s = _step(step)
        for b, v in zip(self.boundaries, self.values):
            if s <= b:
                return v
        return self.values[-1]

    def get_config(self):
        return dict(boundaries=list(self.boundaries), values=list(self.values), name=self.name)

    def descriptor(self):
        return dict(kind=KIND["piecewise"], flags=0, lr0=self.values[0], p=(0.0, 0.0, 0.0), decay_steps=1,
                    bounds=tuple(self.boundaries), values=tuple(self.values))


_CLASSES = {c.__name__: c for c in (ExponentialDecay, InverseTimeDecay, PolynomialDecay, CosineDecay,
                                    PiecewiseConstantDecay)}


def serialize(schedule):
    """Keras form: ``{"class_name", "config"}``."""
    return {"class_name": type(schedule).__name__, "config": schedule.get_config()}


def deserialize(config):
    try:
        cls = _CLASSES[config["class_name"]]
    except KeyError:
        raise ValueError(f"unknown learning-rate schedule {config.get('class_name')!r}") from None
    return cls.from_config(config["config"])
