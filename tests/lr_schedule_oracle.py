"""Oracle and case table of the learning-rate schedule tests (tests/test_lr_schedule.py on the CPU,
tests/test_lr_schedule_gpu.py on the GPU).

``eval64`` is the issue's formula of each schedule in float64 from exact integers, written here from the
formulas and not through the package's ``__call__``.  ``eval32`` is ``sched_lr`` (csrc/include/tde_sched.h)
operation by operation in numpy float32, no contraction: the fp32 twin, one sample of what float32 arithmetic
loses.  The device is held to

    |device - eval64| <= max(2^-22 lr0, 4 |eval32 - eval64|)                                     (``bound``)

the project's rule (tests/smallnet_oracle.py: a derived tolerance, or four times the fp32 reference's own
error).  The derived part: the division step / decay_steps, powf / cosf and the last multiply each lose a few
half-ulps of a value no larger than lr0, and the rounding of the exponent p is amplified by |p ln(rate)|
(|power ln(1 - s/D)| for the polynomial); the table keeps that amplification <= 4 (``amplification``, asserted
on the CPU), so the sum stays below 4 ulps of lr0, 2^-22 lr0.

Every parameter of the table is a float32 value (``F``), so the device, which receives floats, and the
float64 oracle are asked the same question.  ``EXACT`` marks what has to come out bit for bit: piecewise
values, step 0 of every kind (in the step-0 rows lr0, end_learning_rate and alpha are dyadic, so
(lr0 - end) + end and (1 - alpha) + alpha are exact in float32 too) and staircase forms with a dyadic rate.
"""
from __future__ import annotations

import math

import numpy as np


def F(x) -> float:
    """x rounded to float32, as a Python float."""
    return float(np.float32(x))


BIG = 2 ** 33            # a step past 2^31 and 2^32: the piecewise compares are 64-bit
KINDS = ("ExponentialDecay", "InverseTimeDecay", "PolynomialDecay", "CosineDecay", "PiecewiseConstantDecay")


def _steps(D, far):
    return [0, 1, D - 1, D, D + 1, far]


# (class name, kwargs, steps, exact): exact "all" | "step0" | None
TABLE = [
    ("ExponentialDecay", dict(initial_learning_rate=F(0.1), decay_steps=16, decay_rate=F(0.96)), _steps(16, 1500), "step0"),
    ("ExponentialDecay", dict(initial_learning_rate=F(1e-3), decay_steps=16, decay_rate=0.5), _steps(16, 91), "step0"),
    ("ExponentialDecay", dict(initial_learning_rate=F(0.1), decay_steps=7, decay_rate=0.5, staircase=True), _steps(7, 40), "all"),
    ("ExponentialDecay", dict(initial_learning_rate=0.25, decay_steps=1000, decay_rate=F(0.9)), [0, 999, 1000, 1001, 37000], "step0"),
    ("InverseTimeDecay", dict(initial_learning_rate=F(0.1), decay_steps=10, decay_rate=F(0.3)), _steps(10, 100000), "step0"),
    ("InverseTimeDecay", dict(initial_learning_rate=0.5, decay_steps=3, decay_rate=0.5, staircase=True), _steps(3, 3001), "all"),
    ("InverseTimeDecay", dict(initial_learning_rate=F(0.01), decay_steps=3, decay_rate=F(0.7), staircase=True), _steps(3, 100), "step0"),
    ("PolynomialDecay", dict(initial_learning_rate=0.5, decay_steps=50, end_learning_rate=0.125), _steps(50, 10 ** 6), "step0"),
    ("PolynomialDecay", dict(initial_learning_rate=F(0.1), decay_steps=20, end_learning_rate=F(1e-4), power=0.5), _steps(20, 10 ** 6)[1:], None),
    ("PolynomialDecay", dict(initial_learning_rate=0.25, decay_steps=7, end_learning_rate=0.0625, power=2.0, cycle=True),
     [0, 1, 6, 7, 8, 12, 14, 15], "step0"),
    ("PolynomialDecay", dict(initial_learning_rate=F(0.1), decay_steps=7, end_learning_rate=F(0.01), power=F(1.5), cycle=True),
     [1, 6, 7, 8, 13, 14, 15, 19], None),
    # a later cycle: D = decay_steps * ceil(step / decay_steps) (the base 1 - s/D is at most 1 / cycles there, so
    # the amplification limit keeps the table to the first few cycles)
    ("PolynomialDecay", dict(initial_learning_rate=F(0.05), decay_steps=1000, end_learning_rate=F(1e-3), cycle=True),
     [900, 1000, 1001, 2500, 5100], None),
    ("CosineDecay", dict(initial_learning_rate=0.5, decay_steps=16), _steps(16, 10 ** 5), "step0"),
    ("CosineDecay", dict(initial_learning_rate=0.125, decay_steps=9, alpha=0.25), _steps(9, 10 ** 5), "step0"),
    ("CosineDecay", dict(initial_learning_rate=F(0.003), decay_steps=1000, alpha=F(0.1)), [1, 333, 500, 999, 1000, 1001], None),
    ("PiecewiseConstantDecay", dict(boundaries=[1], values=[0.125, 0.25]), [0, 1, 2, 3, BIG + 7], "all"),
    ("PiecewiseConstantDecay", dict(boundaries=[3, 10, 11], values=[F(0.1), F(0.03), F(0.007), F(1e-4)]),
     [0, 2, 3, 4, 9, 10, 11, 12, 1000], "all"),
    ("PiecewiseConstantDecay", dict(boundaries=[7, BIG + 6], values=[F(0.1), F(0.02), F(0.003)]),
     [7, 8, BIG + 6, BIG + 7, 2 ** 32 + 7, 2 ** 31, 2 ** 40], "all"),
    ("PiecewiseConstantDecay", dict(boundaries=[1, 2, 3, 5, 8, 13, 21, 34], values=[F(0.5 ** i) for i in range(9)]),
     [0, 1, 2, 3, 4, 5, 6, 8, 9, 13, 14, 21, 22, 34, 35, BIG], "all"),
    ("PiecewiseConstantDecay", dict(boundaries=[], values=[F(0.3)]), [0, 5], "all"),
]


def rows():
    """[(case index, class name, kwargs, iterations, bias, exact)]: every step of the table as the pair the
    kernel receives -- bias 0, and, for the steps the step kernels produce, bias -1 on iterations = step + 1;
    plus iterations = 0 with bias -1 (a negative step is treated as 0)."""
    out = []
    for ci, (name, kw, steps, exact) in enumerate(TABLE):
        for s in steps:
            ex = exact == "all" or (exact == "step0" and s == 0)
            out.append((ci, name, kw, s, 0, ex))
            out.append((ci, name, kw, s + 1, -1, ex))
        out.append((ci, name, kw, 0, -1, exact in ("all", "step0")))
    return out


def make(tde, name, kw):
    return getattr(tde.optimizers.schedules, name)(**kw)


def eval64(name, kw, step) -> float:
    s = max(int(step), 0)
    if name == "PiecewiseConstantDecay":
        for b, v in zip(kw["boundaries"], kw["values"]):
            if s <= b:
                return float(v)
        return float(kw["values"][-1])
    lr0, D = float(kw["initial_learning_rate"]), int(kw["decay_steps"])
    if name in ("ExponentialDecay", "InverseTimeDecay"):
        p = float(s // D) if kw.get("staircase") else s / D
        rate = float(kw["decay_rate"])
        return lr0 * rate ** p if name == "ExponentialDecay" else lr0 / (1.0 + rate * p)
    if name == "PolynomialDecay":
        end, power = float(kw.get("end_learning_rate", 1e-4)), float(kw.get("power", 1.0))
        if kw.get("cycle"):
            DD = D * max(1, -(-s // D))
        else:
            s, DD = min(s, D), D
        return (lr0 - end) * (1.0 - s / DD) ** power + end
    assert name == "CosineDecay"
    alpha = float(kw.get("alpha", 0.0))
    s = min(s, D)
    return lr0 * ((1.0 - alpha) * 0.5 * (1.0 + math.cos(math.pi * s / D)) + alpha)


def eval32(name, kw, step) -> float:
    f = np.float32
    s = max(int(step), 0)
    if name == "PiecewiseConstantDecay":
        return eval64(name, kw, s)
    lr0, ds, st = f(kw["initial_learning_rate"]), f(kw["decay_steps"]), f(s)
    one = f(1.0)
    with np.errstate(all="ignore"):
        if name in ("ExponentialDecay", "InverseTimeDecay"):
            p = st / ds
            if kw.get("staircase"):
                p = np.floor(p)
            rate = f(kw["decay_rate"])
            return float(lr0 * np.power(rate, p) if name == "ExponentialDecay" else lr0 / (one + rate * p))
        if name == "PolynomialDecay":
            end, power = f(kw.get("end_learning_rate", 1e-4)), f(kw.get("power", 1.0))
            if kw.get("cycle"):
                d = ds * np.maximum(one, np.ceil(st / ds))
            else:
                st, d = np.minimum(st, ds), ds
            return float((lr0 - end) * np.power(one - st / d, power) + end)
        alpha = f(kw.get("alpha", 0.0))
        c = f(0.5) * (one + np.cos(f(math.pi) * (np.minimum(st, ds) / ds)))
        return float(lr0 * ((one - alpha) * c + alpha))


def lr0_of(name, kw) -> float:
    return float(max(kw["values"])) if name == "PiecewiseConstantDecay" else float(kw["initial_learning_rate"])


def bound(name, kw, step) -> float:
    return max(2.0 ** -22 * lr0_of(name, kw), 4.0 * abs(eval32(name, kw, step) - eval64(name, kw, step)))


def amplification(name, kw, step) -> float:
    """How much a relative rounding error of the exponent's argument grows in the result (0 where the
    argument is exact or there is no power)."""
    s, D = max(int(step), 0), int(kw.get("decay_steps", 1))
    if name == "ExponentialDecay":
        p = s // D if kw.get("staircase") else s / D
        return abs(p * math.log(float(kw["decay_rate"])))
    if name == "PolynomialDecay":
        if kw.get("cycle"):
            DD = D * max(1, -(-s // D))
        else:
            s, DD = min(s, D), D
        base = 1.0 - s / DD
        return abs(float(kw.get("power", 1.0)) * math.log(base)) if 0.0 < base < 1.0 else 0.0
    return 0.0


# ------------------------------------------------------------------------- optimizer steps under a schedule
def rho_bound(t, hyper, K=4):
    """Relative error allowed to the kernel's Adam lr_t at step t (tests/test_optim_gpu.py ``rho_bound``)."""
    b1, b2 = F(hyper["b1"]), F(hyper["b2"])
    t = max(int(t), 1)
    p1, p2 = b1 ** t, b2 ** t
    return 2.0 ** -24 * (K * (p2 / (2.0 * (1.0 - p2)) + p1 / (1.0 - p1)) + 8.0)
