"""Float64 oracle of weight regularizers and decoupled weight decay (csrc/include/tde_reg.h), and the fixtures
of tests/test_weight_reg.py (CPU) and tests/test_weight_reg_gpu.py (GPU).

``trajectory`` is independent of the package's reference plan: it differentiates ``mean CE + sum P`` directly
with torch autograd in float64 (the penalty is part of the differentiated scalar, not a term added to the
gradient afterwards), clips that gradient, decays the weights (``w - (w * wd) * lr``) and steps the optimizer by
the formulas of Keras, written out here.  The forward is the layers' ``ref_call`` on float64 tensors.

Error bounds of the device's regularizer launches, from the summation order stated in
csrc/kernels/weightreg.hip: a penalty partial has 16 x (l2 * w, fmaf, fmaf) = 48 float32 roundings on its longest
path, + 6 wave levels + 3 adds = 57; the float64 sum of the partials adds nothing at that scale; the cast to
float32: PENALTY_ROUNDINGS = 58.  Every term is >= 0, so the relative error is at most half a unit of 2^-24 per
rounding; the tests allow twice the count (the convention of grad_clip_oracle.NORM_TOL).  The gradient has two
roundings per element, the fmaf and the add.
"""
from __future__ import annotations

import math

import numpy as np
import torch

CHUNK = 4096                 # kRegChunk
PENALTY_ROUNDINGS = 58
PENALTY_TOL = 2 * PENALTY_ROUNDINGS * 2.0 ** -24 / 2      # relative
GRAD_ROUNDINGS = 2
GRAD_TOL = 2 * GRAD_ROUNDINGS * 2.0 ** -24 / 2            # relative to |g| + |2 l2 w| + l1


def sgn(w):
    return torch.sign(w)     # sign(+-0) = 0


def penalty(w, l1, l2):
    """float64 scalar: l1 * sum|w| + l2 * sum w^2."""
    w = w.detach().double()
    return l1 * w.abs().sum() + l2 * w.square().sum()


def reg_grad(w, l1, l2):
    w = w.detach().double()
    return 2.0 * l2 * w + l1 * sgn(w)


def chunks(numel):
    return (numel + CHUNK - 1) // CHUNK


def table(numels, coefs):
    """What tde_reg_build_table has to produce: [(seg, chunk)] over the segments with a non-zero coefficient."""
    return [(i, c) for i, (n, (a, b)) in enumerate(zip(numels, coefs)) if a or b for c in range(chunks(n))]


# ------------------------------------------------------------------------------------- trajectories
def _named_weights(model, dtype=torch.float64):
    st = model._store
    return {n: st.view(n).detach().cpu().to(dtype).clone() for n in st.order}


def _forward(model, W, x):
    t = {0: x}
    nodes = model._nodes()
    for layer, ins, out in nodes:
        d = {s.name: W[s.full_name] for s in layer.weight_specs}
        h = [t[j] for j in ins] if layer.multi_input else t[ins[0]]
        t[out] = layer.ref_call(h, d, True, None, [])
    return t[nodes[-1][2]]


def coefficients(model):
    return {s.full_name: (float(s.l1), float(s.l2)) for l in model.layers for s in l.weight_specs
            if s.trainable and (s.l1 or s.l2)}


def total_loss(model, W, x, y, global_batch=None):
    """(mean CE + sum P, mean CE, sum P) in W's dtype; logits models (from_logits=True)."""
    logits = _forward(model, W, x)
    ce = torch.nn.functional.cross_entropy(logits, y.long(), reduction="sum") / float(global_batch or len(y))
    pen = torch.zeros((), dtype=logits.dtype)
    for n, (a, b) in coefficients(model).items():
        pen = pen + a * W[n].abs().sum() + b * W[n].square().sum()
    return ce + pen, ce, pen


def _clip(g, clip):
    if clip is None:
        return g
    mode, c = clip
    if mode == "clipvalue":
        return {n: t.clamp(-c, c) for n, t in g.items()}
    if mode == "clipnorm":
        return {n: t * (c / max(float(t.square().sum().sqrt()), c)) for n, t in g.items()}
    norm = math.sqrt(sum(float(t.square().sum()) for t in g.values()))
    return {n: t * (c / max(norm, c)) for n, t in g.items()}


def global_norm(g):
    return math.sqrt(sum(float(t.double().square().sum()) for t in g.values()))


def trajectory(model, batches, opt, decays=lambda name: True):
    """Float64 trajectory of ``model``'s trainable variables from its current weights over ``batches``
    [(x, y)], under the hyper-parameters of the package optimizer ``opt`` (kind, rate or schedule, clip,
    weight_decay) but none of its code paths that apply them.  -> (weights {name: float64}, [logged loss per step:
    mean CE + sum P of the weights the step's forward used], [global norm of the total gradient per step])."""
    W = _named_weights(model)
    names = [n for n in model._store.names(trainable=True)]
    hp = {k: float(np.float32(v)) for k, v in opt.hparams().items()}
    s0 = {n: torch.zeros_like(W[n]) for n in names}
    s1 = {n: torch.zeros_like(W[n]) for n in names}
    wd = opt.weight_decay or 0.0
    losses, norms = [], []
    for k, (x, y) in enumerate(batches):
        leaves = {n: (W[n].clone().requires_grad_(True) if n in names else W[n]) for n in W}
        tot, ce, pen = total_loss(model, leaves, x.double(), y)
        tot.backward()
        losses.append(float(tot.detach()))
        g = {n: leaves[n].grad.detach() for n in names}
        norms.append(global_norm(g))
        g = _clip(g, opt.clip)
        lr = float(opt.lr_at(k))
        t = k + 1
        for n in names:
            w = W[n]
            if wd and decays(n):
                w = w - (w * wd) * lr
            if opt.kind == "sgd":
                w = w - lr * g[n]
            elif opt.kind in ("momentum", "nesterov"):
                s0[n] = hp["mom"] * s0[n] - lr * g[n]
                w = w + hp["mom"] * s0[n] - lr * g[n] if opt.kind == "nesterov" else w + s0[n]
            elif opt.kind == "adam":
                s0[n] = hp["b1"] * s0[n] + (1.0 - hp["b1"]) * g[n]
                s1[n] = hp["b2"] * s1[n] + (1.0 - hp["b2"]) * g[n] * g[n]
                lr_t = lr * math.sqrt(1.0 - hp["b2"] ** t) / (1.0 - hp["b1"] ** t)
                w = w - lr_t * s0[n] / (s1[n].sqrt() + hp["eps"])
            else:
                raise NotImplementedError(opt.kind)
            W[n] = w
    return {n: W[n] for n in names}, losses, norms


def batches(model, n, steps, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(steps):
        x = torch.from_numpy(rng.standard_normal((n,) + tuple(model.input_shape[1:])).astype(np.float32))
        y = torch.from_numpy(rng.integers(0, 10, n).astype(np.int32))
        out.append((x, y))
    return out
