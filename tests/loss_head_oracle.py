"""Float64 oracle of the softmax-CE head with label smoothing and class weights (csrc/include/tde_loss.h), and
the cases of tests/test_loss_head.py (CPU) and tests/test_loss_head_gpu.py (GPU).

For a row with integer label y over C classes, smoothing e and weight w = class_weight.get(y, 1.0):

    t_c      = (1 - e) [c == y] + e / C
    loss     = w ((1 - e) (lse - l_y) + e (lse - mean_c l_c))
    dlogit_c = w (p_c - t_c) scale

written out from ``log_softmax`` in float64 (``torch.nn.functional.cross_entropy(weight=, label_smoothing=)``
weights the smoothing term per class and divides by the weights' sum: other semantics).  A label outside [0, C)
has weight 1, l_y := max and no one-hot term.  ``trajectory`` is independent of the package's reference plan: it
differentiates ``sum(loss) / rows`` with autograd and steps SGD / momentum by the formulas of Keras.
"""
from __future__ import annotations

import numpy as np
import torch

import weight_reg_oracle as W

# the specs of the plan tests: (label smoothing, class_weight of fit)
CASES = {
    "smooth": (0.1, None),
    "class_weight": (0.0, {0: 2.0, 2: 0.0, 7: 0.5}),
    "both": (0.1, {0: 2.0, 2: 0.0, 7: 0.5}),
}

# the kernel cases: (B, C) -- one row of two classes; a row tail in one workgroup; one lane past a full wave;
# a row tail (B % 4 != 0) over 18 workgroups with 16 trips of the class loop
SHAPES = [(1, 2), (5, 10), (3, 65), (70, 1000)]
SMOOTH = [0.0, 0.1]
WEIGHTS = ["none", "random", "zero"]


def table(class_weight, C, dtype=np.float64):
    t = np.ones(C, dtype=dtype)
    for k, v in (class_weight or {}).items():
        t[k] = v
    return t


def kernel_weights(kind, C, rng, zero_at=0):
    """The weight table of a kernel case as float32 (None: no table): uniform in [0.5, 2], "zero": with a zero at
    class ``zero_at``."""
    if kind == "none":
        return None
    w = rng.uniform(0.5, 2.0, C).astype(np.float32)
    if kind == "zero":
        w[zero_at] = 0.0
    return w


def rows(logits, y, smooth, tab):
    """Per-row loss, differentiable: float64 ``logits`` [N, C], int64 ``y`` [N], ``tab`` float64 [C] or None."""
    C = logits.shape[1]
    lsm = torch.log_softmax(logits, dim=1)
    ok = (y >= 0) & (y < C)
    yc = y.clamp(0, C - 1)
    lse = torch.logsumexp(logits, dim=1)
    nll = torch.where(ok, -lsm.gather(1, yc[:, None]).squeeze(1), lse - logits.max(dim=1).values.detach())
    sm = -lsm.mean(dim=1)
    w = torch.ones_like(nll) if tab is None else torch.where(ok, torch.as_tensor(tab, dtype=nll.dtype)[yc],
                                                              torch.ones_like(nll))
    return w * ((1.0 - smooth) * nll + smooth * sm)


def head(logits, y, smooth, tab, scale=1.0):
    """-> dict(loss [N] float64, dlogits [N, C] float64 = w (p - t) scale by the formula, probs, correct: the
    number of rows whose lowest-index argmax is the label)."""
    z = torch.as_tensor(logits).double()
    y = torch.as_tensor(y).long()
    C = z.shape[1]
    ok = (y >= 0) & (y < C)
    p = torch.softmax(z, dim=1)
    onehot = torch.zeros_like(z)
    onehot[ok, y[ok]] = 1.0
    t = (1.0 - smooth) * onehot + smooth / C
    w = torch.ones(len(y), dtype=torch.float64)
    if tab is not None:
        w[ok] = torch.as_tensor(tab).double()[y[ok]]
    am = torch.tensor([int(np.flatnonzero(r == r.max())[0]) for r in z.numpy()])
    return dict(loss=rows(z, y, smooth, None if tab is None else torch.as_tensor(tab).double()),
                dlogits=w[:, None] * (p - t) * scale, probs=p, correct=int((am == y).sum()), w=w)


def trajectory(model, batches, opt, smooth, class_weight):
    """Float64 trajectory of ``model``'s trainable variables over ``batches`` [(x, int labels)] under SGD /
    momentum: -> (weights {name: float64}, [the logged loss per step: sum w_i l_i / rows])."""
    Wt = W._named_weights(model)
    names = list(model._store.names(trainable=True))
    C = model.output_shape[-1]
    tab = None if class_weight is None else torch.from_numpy(table(class_weight, C))
    hp = {k: float(np.float32(v)) for k, v in opt.hparams().items()}
    vel = {n: torch.zeros_like(Wt[n]) for n in names}
    losses = []
    for k, (x, y) in enumerate(batches):
        leaves = {n: (Wt[n].clone().requires_grad_(True) if n in names else Wt[n]) for n in Wt}
        logits = W._forward(model, leaves, x.double())
        tot = rows(logits, y.long(), smooth, tab).sum() / float(len(y))
        tot.backward()
        losses.append(float(tot.detach()))
        lr = float(opt.lr_at(k))
        for n in names:
            g = leaves[n].grad.detach()
            if opt.kind == "sgd":
                Wt[n] = Wt[n] - lr * g
            elif opt.kind == "momentum":
                vel[n] = hp["mom"] * vel[n] - lr * g
                Wt[n] = Wt[n] + vel[n]
            else:
                raise NotImplementedError(opt.kind)
    return {n: Wt[n] for n in names}, losses


def eval_loss(model, x, y, smooth):
    """What ``evaluate`` reports: the smoothing, no class weights."""
    logits = W._forward(model, W._named_weights(model), x.double())
    return float(rows(logits, y.long(), smooth, None).mean())


def batches(model, n, steps, seed, classes=None):
    """[(x float32, int32 labels)]: every class of ``CASES``' weights occurs."""
    rng = np.random.default_rng(seed)
    C = classes or model.output_shape[-1]
    out = []
    for _ in range(steps):
        x = torch.from_numpy(rng.standard_normal((n,) + tuple(model.input_shape[1:])).astype(np.float32))
        y = rng.integers(0, C, n).astype(np.int32)
        y[:3] = (0, 2, 7)[: min(3, n)] if C > 7 else y[:3]
        out.append((x, torch.from_numpy(y)))
    return out


def onehot(y, C, dtype=np.float32):
    return np.eye(C, dtype=dtype)[np.asarray(y)]
