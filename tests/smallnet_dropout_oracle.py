"""Float64 oracle and test models for Dropout on the fused small-net plan (train/smallnet.py,
csrc/kernels/smallnet.hip).  A plain helper module: tests/test_smallnet_dropout.py (CPU) and
tests/test_smallnet_dropout_gpu.py (GPU) import it; the quantizer, the weights, ``rel`` and ``bound`` are
those of tests/smallnet_oracle.py.

The oracle is smallnet_oracle's forward with one extra multiplication per Dropout: the activation of D
values per image (NHWC order) times ``ops.philox.keep_scales(rate, seed, step, lid, B D).reshape(B, D)``,
the host twin of the device mask.  ``seed`` and ``lid`` come from ``train/elementwise_ids.dropout_ids``
(the CPU test pins that helper to what the layer-wise plan holds), ``step`` is the number of training
steps completed before the one computed.  The same function in torch fp32 on the CPU, with the same
masks, is the reference whose own error sets the bound per variable: max(1e-5, 4 err_fp32).

Quantizer.  As in smallnet_oracle: inputs and conv weights on dyadic grids make every conv
pre-activation exact in fp32 under any summation order while the sum of |terms| stays below 2^24 grid
steps.  A Dropout in front of a conv keeps that only when its scale is a power of two, so ``conv_drop``
drops at rate 0.5 (scale 2: one bit of headroom); ``pool_drop`` and LeNet-5 drop behind the last conv,
where the scale may be anything.  ``trunk_check`` evaluates both conditions on the data at hand.

Seeds.  SEEDS lists, per (model, B), the data seed for which the near-tie (every dense ReLU
pre-activation further than 1e-4 rms from 0) and top-2 margin conditions hold at every step index the
tests use; found by trying 0, 1, 2, ... on the oracle alone (``find_seed``), on the CPU.
"""
import numpy as np
import torch
import torch.nn.functional as F

import smallnet_oracle as O

MODEL_SEED = 11      # backend seed under which unseeded Dropout layers draw their Philox keys


# ------------------------------------------------------------------------------------------ models
def _mask_probe(tde, K):
    return tde.Sequential([
        K.Dense(10, activation="relu", input_shape=(6,)),
        K.Dropout(0.5, seed=1234),
        K.Dense(3),
    ], name="mask_probe")


def _pool_drop(tde, K):
    return tde.Sequential([
        K.Conv2D(4, 3, activation="relu", input_shape=(6, 6, 2)),
        K.MaxPooling2D(),
        K.Dropout(0.25),
        K.Flatten(),
        K.Dense(9, activation="relu"),
        K.Dropout(0.5, seed=77),
        K.Dense(5),
    ], name="pool_drop")


def _conv_drop(tde, K):
    return tde.Sequential([
        K.Conv2D(4, 3, padding="same", activation="relu", input_shape=(7, 6, 2)),
        K.Dropout(0.5),
        K.Conv2D(5, 3),
        K.Flatten(),
        K.Dense(5),
    ], name="conv_drop")


def _linear(tde, K, rate, drop=True):
    layers = [K.Flatten(input_shape=(4, 4, 1)), K.Dense(12)]
    if drop:
        layers.append(K.Dropout(rate, seed=5))
    layers += [K.Dense(7, activation="relu", use_bias=False), K.Dense(4, activation="softmax")]
    return tde.Sequential(layers, name="linear_drop")


def _linear_drop(tde, K):
    return _linear(tde, K, 0.5)


def _linear_rate0(tde, K):
    return _linear(tde, K, 0.0)


def _linear_plain(tde, K):
    return _linear(tde, K, 0.0, drop=False)


def _lenet5_drop(tde, K):
    """LeNet-5 (zoo.lenet5) with Dropout(0.5) after Dense(120) and after Dense(84)."""
    return tde.Sequential([
        K.Conv2D(6, 5, padding="same", activation="relu", input_shape=(28, 28, 1)),
        K.MaxPooling2D(),
        K.Conv2D(16, 5, activation="relu"),
        K.MaxPooling2D(),
        K.Flatten(),
        K.Dense(120, activation="relu"),
        K.Dropout(0.5),
        K.Dense(84, activation="relu"),
        K.Dropout(0.5),
        K.Dense(10),
    ], name="lenet5_drop")


# name -> (builder, head gives logits, input bits, conv weight bits)
MODELS = {
    "mask_probe": (_mask_probe, True, 4, 6),
    "pool_drop": (_pool_drop, True, 4, 6),
    "conv_drop": (_conv_drop, True, 2, 4),
    "linear_drop": (_linear_drop, False, 4, 6),
    "linear_rate0": (_linear_rate0, False, 4, 6),
    "linear_plain": (_linear_plain, False, 4, 6),
    "lenet5_drop": (_lenet5_drop, True, 4, 6),
}
SMALL = ("pool_drop", "conv_drop", "linear_drop")
SMALL_BATCHES = O.SMALL_BATCHES            # (5, 8), (67, 67)
FAST_BATCH = O.FAST_BATCH                  # (37, 64)
CASES = [(n, B, Bp) for n in SMALL for B, Bp in SMALL_BATCHES] + [("lenet5_drop",) + FAST_BATCH]
TRAJ = ("pool_drop", 5, 8)                 # the three-step SGD trajectory
TRAJ_STEPS = 3

# data seeds for which near-tie and margin hold (at step 0; TRAJ: along the three steps); see find_seed
SEEDS = {("lenet5_drop", 37): 1}           # every other case: 0


def seed_of(name, B):
    return SEEDS.get((name, B), 0)


def make_case(tde, name, B, Bplan):
    """-> (compiled model with grid weights loaded, x, y) on the CPU."""
    fn, logits, in_bits, w_bits = MODELS[name]
    tde.backend.set_random_seed(MODEL_SEED)
    m = fn(tde, tde.keras.layers)
    m.compile(loss=tde.losses.SparseCategoricalCrossentropy(from_logits=logits), optimizer=tde.optimizers.SGD(0.01),
              metrics=["accuracy"])
    m.build()
    rng = np.random.default_rng(2000 + seed_of(name, B))
    m._store.load_dict(O.make_weights(m, rng, w_bits), strict=True)
    x, y = O.make_batch(m, rng, Bplan, in_bits)
    return m, x, y


# ------------------------------------------------------------------------------------------ masks
def drop_table(model):
    """{Dropout layer name: (rate, seed, lid)} -- seed and lid as every plan derives them."""
    from tensorflow_distributed_example_amd.models import layers as L
    from tensorflow_distributed_example_amd.train.elementwise_ids import dropout_ids
    ids = dropout_ids(model)
    return {l.name: (l.rate,) + tuple(reversed(ids[l.name])) for l in model.layers if isinstance(l, L.Dropout)}


def mask(rate, seed, step, lid, B, D):
    """[B, D] float32 keep scales of a dropped activation of D values per image."""
    from tensorflow_distributed_example_amd.ops.philox import keep_scales
    return torch.from_numpy(keep_scales(rate, seed, step, lid, B * D).reshape(B, D).copy())


# ------------------------------------------------------------------------------------------ oracle
def forward(model, W, x, step, drops, absW=None):
    """smallnet_oracle._forward with Dropout.  ``step`` None: no masks (eval / predict).  -> (head
    pre-activation, records, dropped): records as in smallnet_oracle plus ("terms", conv name, largest sum
    of |terms| of one output) when ``absW`` is given; dropped {Dropout name: activation after the mask}."""
    from tensorflow_distributed_example_amd.models import layers as L
    h = x
    rec, dropped = [], {}
    last = None
    layers = [l for l in model.layers if not isinstance(l, L.InputLayer)]
    for i, layer in enumerate(layers):
        if isinstance(layer, L.Conv2D):
            assert layer.strides == (1, 1)
            (pt, pb), (pl, pr) = layer.pads(tuple(h.shape[1:]))
            xc = F.pad(h.permute(0, 3, 1, 2), (pl, pr, pt, pb))
            b = W[f"{layer.name}/bias"] if layer.use_bias else None
            z = F.conv2d(xc, W[f"{layer.name}/kernel"].permute(3, 2, 0, 1), b).permute(0, 2, 3, 1)
            if absW is not None:
                ab = absW[f"{layer.name}/bias"] if layer.use_bias else None
                tot = F.conv2d(xc.detach().abs(), absW[f"{layer.name}/kernel"].permute(3, 2, 0, 1), ab)
                rec.append(("terms", layer.name, tot.max()))
            rec.append(("conv", layer.name, z))
            last = "conv"
            if layer.activation == "relu":
                rec.append(("relu_conv", layer.name, z))
                z = F.relu(z)
            else:
                assert layer.activation is None
            h = z
        elif isinstance(layer, L.Activation):
            assert layer.activation == "relu" and last is not None
            rec.append(("relu_" + last, layer.name, h))
            h = F.relu(h)
        elif isinstance(layer, L.MaxPooling2D):
            assert layer.pool_size == (2, 2) and layer.strides == (2, 2) and layer.padding == "valid"
            h = F.max_pool2d(h.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
        elif isinstance(layer, L.Flatten):
            h = h.reshape(h.shape[0], -1)
        elif isinstance(layer, L.Reshape):
            h = h.reshape((h.shape[0],) + tuple(layer.target_shape))
        elif isinstance(layer, L.Dropout):
            if step is not None and layer.rate > 0:
                rate, seed, lid = drops[layer.name]
                B, D = h.shape[0], int(np.prod(h.shape[1:]))
                h = h * mask(rate, seed, step, lid, B, D).to(h.dtype).reshape(h.shape)
            dropped[layer.name] = h
        elif isinstance(layer, L.Dense):
            z = h @ W[f"{layer.name}/kernel"]
            if layer.use_bias:
                z = z + W[f"{layer.name}/bias"]
            last = "dense"
            if i == len(layers) - 1:
                assert layer.activation in (None, "softmax")
                return z, rec, dropped
            if layer.activation == "relu":
                rec.append(("relu_dense", layer.name, z))
                z = F.relu(z)
            else:
                assert layer.activation is None
            h = z
        else:
            raise NotImplementedError(type(layer).__name__)
    raise AssertionError("no Dense head")


def oracle(model, store, x, y, B, global_batch, step, dtype=torch.float64, weights=None):
    """Forward + autograd in ``dtype`` with the masks of step index ``step`` (None: no masks).  -> dict(grads,
    loss (sum of CE), correct, out (what predict returns), near_tie, margin, dropped).  ``weights``
    ({name: tensor}) replaces the store's values (the trajectory)."""
    W = O._weights(model, store, dtype, True)
    if weights is not None:
        W = {n: weights[n].detach().to(dtype).clone().requires_grad_(w.requires_grad) for n, w in W.items()}
    xd = x[:B].detach().cpu().to(dtype)
    yl = y[:B].detach().cpu().long()
    z, rec, dropped = forward(model, W, xd, step, drop_table(model))
    ls = -torch.log_softmax(z, dim=1).gather(1, yl[:, None]).squeeze(1)
    (ls.sum() / float(global_batch)).backward()
    zd = z.detach()
    top = zd.topk(2, dim=1).values
    near = 1.0
    for kind, _, t in rec:
        if kind == "relu_dense":
            t = t.detach()
            near = min(near, (t.abs().min() / t.pow(2).mean().sqrt()).item())
    softmax = model.layers[-1].activation == "softmax"
    return dict(grads={n: w.grad.detach() for n, w in W.items() if w.requires_grad}, loss=ls.sum().item(),
                correct=int((zd.argmax(1) == yl).sum()), out=torch.softmax(zd, 1) if softmax else zd,
                near_tie=near, margin=((top[:, 0] - top[:, 1]).min() / zd.pow(2).mean().sqrt()).item(),
                dropped={n: t.detach() for n, t in dropped.items()})


def trunk_check(model, store, x, B, in_bits, w_bits, step):
    """-> (exact, headroom): every conv pre-activation of the fp32 CPU forward (masks of ``step``) equals
    the float64 one bit for bit; headroom = smallest 2^24 step_k / largest sum of |terms| (must be > 1).
    A power-of-two dropout scale s in front of the k-th conv moves its values to the grid step_k itself at
    most (s >= 1 only coarsens), so step_k = 2^-(in_bits + k w_bits) still divides every term."""
    W64 = O._weights(model, store, torch.float64, False)
    W32 = {n: w.float() for n, w in W64.items()}
    xd = x[:B].detach().cpu()
    drops = drop_table(model)
    _, r64, _ = forward(model, W64, xd.double(), step, drops, absW={n: w.abs() for n, w in W64.items()})
    _, r32, _ = forward(model, W32, xd.float(), step, drops)
    c64 = [t for k, _, t in r64 if k == "conv"]
    c32 = [t for k, _, t in r32 if k == "conv"]
    exact = len(c64) == len(c32) and all(torch.equal(a.double(), b) for a, b in zip(c32, c64))
    headroom = float("inf")
    for k, tot in enumerate([t for kk, _, t in r64 if kk == "terms"], start=1):
        headroom = min(headroom, 2.0 ** 24 * 2.0 ** -(in_bits + k * w_bits) / max(tot.item(), 1e-30))
    return exact, headroom


def conditions(tde, name, B, Bplan, steps=(0,)):
    """The conditions on the inputs, on the oracle alone: dict(exact, headroom, near_tie, margin), the worst
    over ``steps`` (each evaluated at the case's initial weights)."""
    m, x, y = make_case(tde, name, B, Bplan)
    in_bits, w_bits = MODELS[name][2:]
    out = dict(exact=True, headroom=float("inf"), near_tie=1.0, margin=float("inf"))
    for s in steps:
        ex, hr = trunk_check(m, m._store, x, B, in_bits, w_bits, s)
        orc = oracle(m, m._store, x, y, B, Bplan, s)
        out = dict(exact=out["exact"] and ex, headroom=min(out["headroom"], hr),
                   near_tie=min(out["near_tie"], orc["near_tie"]), margin=min(out["margin"], orc["margin"]))
    return out


def trajectory(model, store, x, y, B, global_batch, lr, steps, dtype=torch.float64, mask_steps=None):
    """Plain SGD from the store's weights: step k uses the masks of index ``mask_steps[k]`` (default k).
    -> (weights after the last step {name: tensor}, [oracle dict of every step])."""
    W = {n: w.detach().clone() for n, w in O._weights(model, store, dtype, False).items()}
    figs = []
    for k in range(steps):
        orc = oracle(model, store, x, y, B, global_batch, k if mask_steps is None else mask_steps[k], dtype, weights=W)
        figs.append(orc)
        W = {n: (w - lr * orc["grads"][n].to(dtype)) if n in orc["grads"] else w for n, w in W.items()}
    return W, figs


def find_seed(tde, name, B, Bplan, steps=(0,), tries=20):
    """The first data seed for which the conditions hold (how SEEDS was filled)."""
    for s in range(tries):
        SEEDS[(name, B)] = s
        c = conditions(tde, name, B, Bplan, steps)
        if c["exact"] and c["headroom"] > 1 and c["near_tie"] > O.TIE and c["margin"] > O.TIE:
            return s
    raise AssertionError((name, B))
