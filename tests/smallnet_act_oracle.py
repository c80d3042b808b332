"""Float64 oracle and test models for the tanh / sigmoid activations and the 2x2 average pool of the fused
small-net plan (train/smallnet.py, csrc/kernels/smallnet.hip).  A plain helper module in the style of
tests/smallnet_oracle.py, whose bound, data makers and reference comparison it uses:
tests/test_smallnet_act_oracle.py (CPU), tests/test_smallnet_act_gpu.py and tests/_smallnet_act_child.py
(GPU) import it.

The oracle walks ``model.layers`` with torch double ops on the CPU: Conv2D (stride 1, explicit ``F.pad``
from ``layer.pads``), ``Activation``, MaxPooling2D(2) and AveragePooling2D(2) (both floor), Flatten /
Reshape, Dense, with relu / tanh / sigmoid on the layer or as a standalone ``Activation``, a logits or a
softmax head, loss = sum(CE) / global_batch.

Bound (unchanged): every gradient norm-wise within max(TOL = 1e-5, REF_FACTOR = 4 x the error of the fp32
CPU reference plan against the same oracle).

Tanh, sigmoid and the average pool are smooth: fp32 and float64 take no different decision in them, so the
inputs need no quantization grid here (data is randn, weights Glorot).  Conditions on the inputs remain
only where a decision remains, all evaluated on the oracle alone:
  relu_near   smallest |pre-activation| / rms over every ReLU (conv or dense) >= TIE
  pool_gap    smallest top-2 gap / rms over the windows of every max pool behind a tanh / sigmoid conv >= TIE
              (the kernel recomputes the argmax in fp32; a near tie could route the gradient elsewhere)
  margin      the head's top-2 margin / rms >= TIE (the exact correct count rests on it)
SEEDS holds, per (model, B), the first of 0, 1, 2, ... for which they hold.
"""
import numpy as np
import torch
import torch.nn.functional as F

import smallnet_oracle as O
from smallnet_oracle import REF_FACTOR, TIE, TOL, bound, rel  # noqa: F401  (the project's bound, re-exported)


# ------------------------------------------------------------------------------------------ models
def _act_padded(tde, K):
    return tde.Sequential([
        K.Conv2D(4, 3, padding="same", activation="tanh", input_shape=(7, 6, 2)),
        K.Conv2D(6, 3, padding="same", activation="sigmoid"),
        K.AveragePooling2D(),
        K.Conv2D(5, (2, 4), padding="same"),
        K.Flatten(),
        K.Dense(9, activation="tanh", use_bias=False),
        K.Dense(5),
    ], name="act_padded")


def _avg_linear(tde, K):
    return tde.Sequential([
        K.Conv2D(32, 3, input_shape=(6, 6, 16)),
        K.AveragePooling2D(),
        K.Flatten(),
        K.Dense(10),
    ], name="avg_linear")


def _tanh_maxpool(tde, K):
    return tde.Sequential([
        K.Conv2D(8, 3, activation="tanh", input_shape=(8, 8, 3)),
        K.MaxPooling2D(),
        K.Conv2D(6, 2, activation="sigmoid"),
        K.Flatten(),
        K.Dense(10, activation="softmax"),
    ], name="tanh_maxpool")


def _act_layers(tde, K):
    return tde.Sequential([
        K.Conv2D(8, 3, input_shape=(6, 6, 4)),
        K.Activation("tanh"),
        K.Flatten(),
        K.Dense(12),
        K.Activation("sigmoid"),
        K.Dense(7, activation="relu"),
        K.Dense(5),
    ], name="act_layers")


def _mlp_tanh(tde, K):
    return tde.Sequential([
        K.Dense(36, activation="tanh", input_shape=(50,)),
        K.Dense(21, activation="sigmoid"),
        K.Dense(10),
    ], name="mlp_tanh")


def _dgrad_tanh(tde, K):
    return tde.Sequential([
        K.Conv2D(6, 5, activation="tanh", input_shape=(18, 18, 1)),
        K.Conv2D(16, 5, activation="tanh"),
        K.AveragePooling2D(),
        K.Flatten(),
        K.Dense(10),
    ], name="dgrad_tanh")


def _lenet5_classic(tde, K):
    return tde.zoo.lenet5_classic()


# name -> (builder, head gives logits, expected entry kinds, expected activation codes, expected mask_in codes)
# kinds: 0 conv, 1 max pool, 2 dense, 3 average pool; codes: 0 linear, 1 relu, 2 tanh, 3 sigmoid
MODELS = {
    "act_padded": (_act_padded, True, [0, 0, 3, 0, 2, 2], [2, 3, 0, 0, 2, 0], [0, 2, 3, 0, 0, 2]),
    "avg_linear": (_avg_linear, True, [0, 3, 2], [0, 0, 0], [0, 0, 0]),
    "tanh_maxpool": (_tanh_maxpool, False, [0, 1, 0, 2], [2, 0, 3, 0], [0, 2, 0, 3]),
    "act_layers": (_act_layers, True, [0, 2, 2, 2], [2, 3, 1, 0], [0, 2, 3, 1]),
    "mlp_tanh": (_mlp_tanh, True, [2, 2, 2], [2, 3, 0], [0, 2, 3]),
    "lenet5_classic": (_lenet5_classic, True, [0, 3, 0, 3, 2, 2, 2], [2, 0, 2, 0, 2, 2, 0], [0, 2, 0, 2, 0, 2, 2]),
    # a compile-time-geometry conv, X(5, 5, 6, 16, 14, 14), whose input IS a tanh conv output (no pool in
    # between): the only way into sn_conv_dgrad_c / sn_conv_dgrad_m with a derivative code
    "dgrad_tanh": (_dgrad_tanh, True, [0, 0, 3, 2], [2, 2, 0, 0], [0, 2, 2, 0]),
}
SMALL = ("act_padded", "avg_linear", "tanh_maxpool", "act_layers", "mlp_tanh")
FAST = ("lenet5_classic", "dgrad_tanh")          # the compile-time-geometry convs
CASES = [(n, B, Bp) for n in SMALL for B, Bp in O.SMALL_BATCHES] + [(n,) + O.FAST_BATCH for n in FAST]

# first seed of 0, 1, 2, ... at which relu_near, pool_gap and margin hold on the oracle; every other case: 0
SEEDS = {("tanh_maxpool", 67): 1}       # seed 0 leaves a pool window with a top-2 gap of 7.6e-7 rms


def seed_of(name, B):
    return SEEDS.get((name, B), 0)


def build(tde, name, B, seed=None):
    fn, logits = MODELS[name][:2]
    m = fn(tde, tde.keras.layers)
    m.compile(loss=tde.losses.SparseCategoricalCrossentropy(from_logits=logits), optimizer=tde.optimizers.SGD(0.01),
              metrics=["accuracy"])
    m.build()
    rng = np.random.default_rng(2000 + (seed_of(name, B) if seed is None else seed))
    m._store.load_dict(O.make_weights(m, rng, None), strict=True)
    return m, rng


def make_case(tde, name, B, Bplan, seed=None):
    """The compiled model with its weights loaded and a randn batch of the plan's size: (model, x, y), on
    the CPU."""
    m, rng = build(tde, name, B, seed)
    x, y = O.make_batch(m, rng, Bplan, None)
    return m, x, y


# ------------------------------------------------------------------------------------------ oracle
_ACTS = {"relu": F.relu, "tanh": torch.tanh, "sigmoid": torch.sigmoid}


def _forward(model, W, x):
    """-> (head pre-activation, records).  records: ("relu", layer, pre-activation) for every ReLU and
    ("maxpool", layer, pool input) for every max pool whose input is a tanh / sigmoid output."""
    from tensorflow_distributed_example_amd.models import layers as L
    h = x
    rec = []
    last_act = None        # activation that produced h, while h is still a conv output
    layers = [l for l in model.layers if not isinstance(l, L.InputLayer)]

    def act(name, owner, z):
        if name is None:
            return z
        if name == "relu":
            rec.append(("relu", owner, z))
        return _ACTS[name](z)

    for i, layer in enumerate(layers):
        if isinstance(layer, L.Conv2D):
            assert layer.strides == (1, 1)
            (pt, pb), (pl, pr) = layer.pads(tuple(h.shape[1:]))
            xc = F.pad(h.permute(0, 3, 1, 2), (pl, pr, pt, pb))
            b = W[f"{layer.name}/bias"] if layer.use_bias else None
            z = F.conv2d(xc, W[f"{layer.name}/kernel"].permute(3, 2, 0, 1), b).permute(0, 2, 3, 1)
            h = act(layer.activation, layer.name, z)
            last_act = layer.activation
        elif isinstance(layer, L.Activation):
            h = act(layer.activation, layer.name, h)
            last_act = layer.activation
        elif isinstance(layer, (L.MaxPooling2D, L.AveragePooling2D)):
            assert layer.pool_size == (2, 2) and layer.strides == (2, 2) and layer.padding == "valid"
            hc = h.permute(0, 3, 1, 2)
            if isinstance(layer, L.MaxPooling2D):
                if last_act in ("tanh", "sigmoid"):
                    rec.append(("maxpool", layer.name, h))
                h = F.max_pool2d(hc, 2).permute(0, 2, 3, 1)      # floor: odd edges dropped
            else:
                h = F.avg_pool2d(hc, 2).permute(0, 2, 3, 1)
            last_act = None
        elif isinstance(layer, L.Flatten):
            h = h.reshape(h.shape[0], -1)
        elif isinstance(layer, L.Reshape):
            h = h.reshape((h.shape[0],) + tuple(layer.target_shape))
        elif isinstance(layer, L.Dense):
            z = h @ W[f"{layer.name}/kernel"]
            if layer.use_bias:
                z = z + W[f"{layer.name}/bias"]
            if i == len(layers) - 1:
                assert layer.activation in (None, "softmax")
                return z, rec
            h = act(layer.activation, layer.name, z)
            last_act = None
        else:
            raise NotImplementedError(type(layer).__name__)
    raise AssertionError("no Dense head")


def _window_gap(h):
    """Smallest (largest - second largest) over the 2x2 floor windows of h [B, H, W, C], relative to h's rms."""
    B, H, W, C = h.shape
    w = h[:, :H // 2 * 2, :W // 2 * 2].reshape(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(-1, 4)
    top = w.topk(2, dim=1).values
    return ((top[:, 0] - top[:, 1]).min() / h.pow(2).mean().sqrt()).item()


def oracle(model, store, x, y, B, global_batch):
    """float64 forward + autograd.  -> dict(grads {name: f64}, loss (sum of CE), correct, count, out (what
    predict returns), relu_near, pool_gap, margin); a condition with nothing to decide reports 1.0."""
    W = O._weights(model, store, torch.float64, True)
    xd = x[:B].detach().cpu().double()
    yl = y[:B].detach().cpu().long()
    z, rec = _forward(model, W, xd)
    ls = -torch.log_softmax(z, dim=1).gather(1, yl[:, None]).squeeze(1)
    (ls.sum() / float(global_batch)).backward()
    grads = {n: w.grad.detach() for n, w in W.items() if w.requires_grad}
    zd = z.detach()
    top = zd.topk(2, dim=1).values
    near = gap = 1.0
    for kind, _, t in rec:
        t = t.detach()
        if kind == "relu":
            near = min(near, (t.abs().min() / t.pow(2).mean().sqrt()).item())
        else:
            gap = min(gap, _window_gap(t))
    softmax = model.layers[-1].activation == "softmax"
    return dict(grads=grads, loss=ls.sum().item(), correct=int((zd.argmax(1) == yl).sum()), count=B,
                out=torch.softmax(zd, 1) if softmax else zd, relu_near=near, pool_gap=gap,
                margin=((top[:, 0] - top[:, 1]).min() / zd.pow(2).mean().sqrt()).item())


def conditions_hold(orc):
    return orc["relu_near"] >= TIE and orc["pool_gap"] >= TIE and orc["margin"] >= TIE


# ------------------------------------------------------------------------------------------ comparisons
def measure(tde, name, B, Bplan):
    """One (model, batch) on the GPU in step mode "plain" against the oracle.  -> a JSON-able dict of
    figures, every error as [kernel, fp32 CPU reference]; ``check`` asserts on it."""
    from tensorflow_distributed_example_amd.train import program as PG
    m, x, y = make_case(tde, name, B, Bplan)
    st = m._store
    fig = dict(name=name, B=B, Bplan=Bplan)
    orc = oracle(m, st, x, y, B, Bplan)
    fig.update(relu_near=orc["relu_near"], pool_gap=orc["pool_gap"], margin=orc["margin"])
    ref = O.reference_errors(tde, m, x, y, B, Bplan, orc)
    plan = PG.make_plan(m, st, "cuda", Bplan, Bplan, m.optimizer, m.loss)
    fig["kind"] = plan.kind
    if plan.kind != "fused_smallnet":
        return fig
    xg, yg = x.cuda(), y.cuda()
    plan.train_step(xg, yg, B)
    torch.cuda.synchronize()
    names = st.names(trainable=True)
    fig["grads"] = {n: [rel(st.grad(n), orc["grads"][n]), ref["grads"][n]] for n in names}
    fig["conv_grad_hash"] = O.grad_hash(st, O.conv_kernel_names(m))
    mt = plan.metrics.cpu()
    fig.update(loss=[abs(mt[0].item() - orc["loss"]) / abs(orc["loss"]), ref["loss"]],
               correct=[mt[1].item(), orc["correct"]], count=[mt[2].item(), B], iterations=int(plan.iterations.item()))
    plan.reset_metrics()
    plan.eval_step(xg, yg, B)
    p = plan.predict(xg, B).clone()
    torch.cuda.synchronize()
    me = plan.metrics.cpu()
    fig.update(eval_loss=[abs(me[0].item() - orc["loss"]) / abs(orc["loss"]), ref["eval_loss"]],
               eval_correct=[me[1].item(), orc["correct"]], eval_count=[me[2].item(), B],
               predict=[rel(p, orc["out"]), ref["predict"]], predict_shape=list(p.shape),
               iterations_after_eval=int(plan.iterations.item()))
    return fig


def check(fig):
    """Print every figure, then assert the bounds."""
    tag = f"{fig['name']} B={fig['B']}/{fig['Bplan']}"
    assert fig["kind"] == "fused_smallnet", (tag, fig["kind"])
    print(f"[{tag}] relu_near={fig['relu_near']:.3g} pool_gap={fig['pool_gap']:.3g} margin={fig['margin']:.3g}")
    for n, (e, r) in fig["grads"].items():
        print(f"[{tag}] grad {n}: kernel {e:.3g}  cpu-fp32 {r:.3g}  bound {bound(r):.3g}")
    for k in ("loss", "eval_loss", "predict"):
        print(f"[{tag}] {k}: kernel {fig[k][0]:.3g}  cpu-fp32 {fig[k][1]:.3g}  bound {bound(fig[k][1]):.3g}")
    assert fig["relu_near"] >= TIE and fig["pool_gap"] >= TIE and fig["margin"] >= TIE, tag
    for n, (e, r) in fig["grads"].items():
        assert e <= bound(r), (tag, n, e, r)
    for k in ("loss", "eval_loss", "predict"):
        assert fig[k][0] <= bound(fig[k][1]), (tag, k, fig[k])
    assert fig["predict_shape"][0] == fig["B"], (tag, fig["predict_shape"])
    assert fig["correct"][0] == fig["correct"][1] and fig["eval_correct"][0] == fig["eval_correct"][1], tag
    assert fig["count"][0] == fig["B"] and fig["eval_count"][0] == fig["B"], tag
    assert fig["iterations"] == 1 and fig["iterations_after_eval"] == 1, tag
