"""Autograd oracle of the BN-CNN family (train/bncnn.py, csrc/kernels/bncnn.hip) in plain torch:
``(Conv2D(no bias) · BatchNormalization · ReLU) x L · Flatten · Dense(no bias) · BatchNormalization · ReLU ·
[Dropout] · Dense(+bias)[softmax]`` with sparse categorical cross-entropy, for any geometry the plan holds
(kernel size, strides, ``same`` / ``valid`` padding from ``conv.pads``), BatchNormalization with or without
gamma (``scale``) and beta (``center``), each layer's own epsilon / momentum, a softmax or a logits head.

The ReLU decisions are an INPUT (``masks``): a pre-activation within one f32 ulp of zero may be decided
differently in f64, and a flipped ReLU moves a whole gradient element.  ``plan_masks`` rebuilds them from the
plan's own f32 pre-activations (its stored raw conv / dense outputs and saved batch statistics) after a
training step; ``host_masks`` takes them from a float32 forward on the host (CPU-side conditioning checks).
Everything else runs in ``dtype``: float64 is the oracle, float32 with the same masks is one sample of what
a second f32 implementation loses (``bound``).

No GPU marker: importable and runnable on the CPU (tests/test_bncnn_oracle.py)."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def spec_of(plan):
    """The layers of a BnCnnPlan in the form ``match_bncnn`` returns."""
    return dict(convs=[(b["conv"], b["bn"]) for b in plan.blocks], dense=(plan.dense, plan.bnd["layer"], plan.drop),
                head=plan.head)


def _f32(v):
    """A layer's hyper-parameter as the kernels receive it: rounded to float32 (momentum 0.99 -> 1 - momentum
    9.5e-7 away from 0.01, which is the whole moving-statistics tolerance)."""
    return float(np.float32(v))


def _bn_vars(W, bn):
    gamma = W[f"{bn.name}/gamma"] if bn.scale else None
    beta = W[f"{bn.name}/beta"] if bn.center else None
    return gamma, beta


def _affine(xhat, gamma, beta):
    y = xhat if gamma is None else xhat * gamma
    return y if beta is None else y + beta


def plan_masks(plan, B):
    """ReLU decisions of the plan's last training step over B rows: ((z32 - mean) * rstd * gamma + beta) > 0
    from the stored raw outputs and the saved statistics, per conv block [B, Ho, Wo, Co] and the dense BN
    [B, D]."""
    st = plan.store
    out = []
    for blk in plan.blocks:
        g, bn = blk["geo"], blk["bn"]
        z32 = blk["z"][: B * g.Ho * g.Wo * g.Co].view(B, g.Ho, g.Wo, g.Co)
        s = blk["saved"]
        pre = (z32 - s[: g.Co]) * s[g.Co:]
        if bn.scale:
            pre = pre * st.view(f"{bn.name}/gamma")
        if bn.center:
            pre = pre + st.view(f"{bn.name}/beta")
        out.append(pre > 0)
    bnl = plan.bnd["layer"]
    h32 = plan.h[: B * plan.Dp].view(B, plan.Dp)[:, : plan.D]
    sv = plan.bnd["saved"]
    pre = (h32 - sv[: plan.D]) * sv[plan.D:]
    if bnl.scale:
        pre = pre * st.view(f"{bnl.name}/gamma")
    if bnl.center:
        pre = pre + st.view(f"{bnl.name}/beta")
    out.append(pre > 0)
    return out


def _conv(a, w, conv):
    (pt, pb), (pl, pr) = conv.pads(conv.input_shape)
    return F.conv2d(F.pad(a.permute(0, 3, 1, 2), (pl, pr, pt, pb)), w.permute(3, 2, 0, 1),
                    stride=tuple(conv.strides)).permute(0, 2, 3, 1)


def oracle(store, spec, x, y, B, masks, scale, drop_mask=None, dtype=torch.float64, device=None):
    """Autograd of the model ``spec`` at the store's weights over the first B rows of x / y, in ``dtype``.
    ``masks``: the ReLU decisions (``plan_masks`` / ``host_masks``), or None to decide them from this
    forward's own pre-activations; ``drop_mask`` [B, D] (keep scales) is applied after the dense BN's ReLU;
    ``scale`` multiplies the summed loss (the plan's 1 / global batch); ``device``: where it runs (default: the
    store's device).
    Returns ({trainable var: grad}, {moving var: new value}, mean loss, logits)."""
    st = store
    dd = dtype
    dev = torch.device(device) if device is not None else st.view(st.order[0]).device
    W = {n: st.view(n).detach().to(dev, dd).clone().requires_grad_(st.segments[n].trainable) for n in st.order}
    H, W_, C = spec["convs"][0][0].input_shape
    a = x[:B].to(dev, dd).reshape(B, H, W_, C)
    moving = {}
    used = []
    for li, (conv, bn) in enumerate(spec["convs"]):
        z = _conv(a, W[f"{conv.name}/kernel"], conv)
        mean, var = z.mean((0, 1, 2)), z.var((0, 1, 2), unbiased=False)
        gamma, beta = _bn_vars(W, bn)
        pre = _affine((z - mean) / torch.sqrt(var + _f32(bn.epsilon)), gamma, beta)
        mask = (pre.detach() > 0) if masks is None else masks[li].to(dev)
        used.append(mask)
        a = pre * mask
        R = z.numel() // z.shape[-1]
        mom = _f32(bn.momentum)
        moving[f"{bn.name}/moving_mean"] = W[f"{bn.name}/moving_mean"] * mom + mean.detach() * (1 - mom)
        # TF's fused batch norm (4-D input): the moving variance takes the Bessel-corrected batch variance
        moving[f"{bn.name}/moving_variance"] = (W[f"{bn.name}/moving_variance"] * mom
                                                + var.detach() * R / max(R - 1, 1) * (1 - mom))
    dense, bnl, _ = spec["dense"]
    head = spec["head"]
    h = a.reshape(B, -1) @ W[f"{dense.name}/kernel"]
    mean, var = h.mean(0), h.var(0, unbiased=False)
    gamma, beta = _bn_vars(W, bnl)
    pre = _affine((h - mean) / torch.sqrt(var + _f32(bnl.epsilon)), gamma, beta)
    mask = (pre.detach() > 0) if masks is None else masks[-1].to(dev)
    used.append(mask)
    a = pre * mask
    if drop_mask is not None:
        a = a * drop_mask[:B].to(dev, dd)
    mom = _f32(bnl.momentum)
    moving[f"{bnl.name}/moving_mean"] = W[f"{bnl.name}/moving_mean"] * mom + mean.detach() * (1 - mom)
    moving[f"{bnl.name}/moving_variance"] = W[f"{bnl.name}/moving_variance"] * mom + var.detach() * (1 - mom)
    logits = a @ W[f"{head.name}/kernel"] + W[f"{head.name}/bias"]
    loss = F.cross_entropy(logits, y[:B].to(dev).long(), reduction="sum") * scale
    loss.backward()
    grads = {n: W[n].grad for n in st.names(trainable=True)}
    oracle.last_masks = used
    return grads, moving, loss.item() / scale / B, logits.detach()


def host_masks(store, spec, x, y, B):
    """The ReLU decisions of a float32 forward on the host (a stand-in for the plan's, to check a case's
    conditioning without a GPU)."""
    oracle(store, spec, x, y, B, None, 1.0, dtype=torch.float32)
    return oracle.last_masks


def plan_oracle(plan, x, y, B, drop_mask=None, dtype=torch.float64, device=None):
    """``oracle`` of a BnCnnPlan after ``plan.train_step(x, y, B)`` (the store holding the pre-step weights):
    ReLU decisions from the plan's f32 pre-activations."""
    return oracle(plan.store, spec_of(plan), x, y, B, plan_masks(plan, B), plan.scale, drop_mask, dtype, device)


def inference(store, spec, x, B, dtype=torch.float64):
    """Forward with the moving statistics and no dropout: (logits, probabilities)."""
    dd = dtype
    dev = store.view(store.order[0]).device
    W = {n: store.view(n).detach().to(dd) for n in store.order}
    H, W_, C = spec["convs"][0][0].input_shape
    a = x[:B].to(dev, dd).reshape(B, H, W_, C)

    def bn_relu(z, bn):
        xh = (z - W[f"{bn.name}/moving_mean"]) / torch.sqrt(W[f"{bn.name}/moving_variance"] + _f32(bn.epsilon))
        return torch.relu(_affine(xh, *_bn_vars(W, bn)))

    for conv, bn in spec["convs"]:
        a = bn_relu(_conv(a, W[f"{conv.name}/kernel"], conv), bn)
    dense, bnl, _ = spec["dense"]
    head = spec["head"]
    a = bn_relu(a.reshape(B, -1) @ W[f"{dense.name}/kernel"], bnl)
    logits = a @ W[f"{head.name}/kernel"] + W[f"{head.name}/bias"]
    return logits, torch.softmax(logits, 1)


def bound(g64, g32):
    """Allowed error norm of an f32 kernel's gradient against the float64 oracle g64, given the float32
    oracle g32 (same ReLU masks): the project's 1e-5 relative, or 4x the error of the f32 reference (a
    second f32 implementation with another summation order) where few values per BN statistic amplify f32
    rounding through rstd and cancellation."""
    g64 = g64.double()
    return max(1e-5 * g64.norm().item(), 4 * (g32.double() - g64).norm().item())
