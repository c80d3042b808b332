"""Float64 oracle, quantizer and test models for the fused small-net plan (train/smallnet.py,
csrc/kernels/smallnet.hip).  A plain helper module: tests/test_smallnet_oracle.py (CPU),
tests/test_smallnet_forms_gpu.py and tests/_smallnet_forms_child.py (GPU) import it.

The oracle walks ``model.layers`` with torch double ops on the CPU and covers exactly what
``match_smallnet`` accepts: Conv2D (stride 1, explicit ``F.pad`` from ``layer.pads``, asymmetric where
TF's are), ``Activation("relu")``, ``MaxPooling2D(2)`` (floor), Flatten / Reshape, Dense with or without
bias, a logits or a softmax head, loss = sum(CE) / global_batch.

Quantizer.  Inputs are integers / 2^in_bits, conv kernels and conv biases are rounded to multiples of
2^-w_bits, so the pre-activation of the k-th conv of the trunk is a sum of multiples of
step_k = 2^-(in_bits + k w_bits).  Such a sum is exact in fp32 under ANY summation order (FMA chains,
MFMA, sliced partial sums) as long as the sum of |terms| of one output stays below 2^24 step_k: every
partial sum is then a multiple of step_k below 2^24 step_k, which fp32 represents.  ``trunk_check``
evaluates that bound on the data at hand and also compares an fp32 CPU forward of the trunk with the
float64 one bit for bit.  With exact conv outputs every ReLU and max-pool decision of the trunk is the
same decision in fp32 and float64 (equal values tie the same way: first maximum in scan order in the
kernel and in torch).  Dense ReLU units cannot be made exact; for them the oracle reports the smallest
|pre-activation| relative to the layer's rms (``near_tie``) and the tests require it above 1e-4 (fp32
error is ~1e-6, so no unit can flip).  The same goes for the head's top-2 margin (``margin``), which the
exact correct count rests on.  Both are conditions on the inputs, evaluated on the oracle alone; SEEDS
holds seeds for which they hold.
"""
import hashlib

import numpy as np
import torch
import torch.nn.functional as F

TOL = 1e-5          # the project's bound for every f32 kernel against float64
REF_FACTOR = 4.0    # ... or four times the fp32 torch CPU reference's own error, whichever is larger
TIE = 1e-4          # smallest allowed |dense ReLU pre-activation| / rms, and top-2 logit margin / rms


# ------------------------------------------------------------------------------------------ models
def _padded(tde, K):
    return tde.Sequential([
        K.Conv2D(4, 3, padding="same", activation="relu", input_shape=(7, 6, 2)),
        K.Conv2D(6, 3, padding="same", activation="relu"),
        K.MaxPooling2D(),
        K.Conv2D(5, (2, 4), padding="same"),
        K.Flatten(),
        K.Dense(9, activation="relu", use_bias=False),
        K.Dense(5),
    ], name="padded")


def _wide_taps(tde, K):
    return tde.Sequential([
        K.Conv2D(16, 3, activation="relu", input_shape=(8, 8, 8)),
        K.Conv2D(20, 3, activation="relu", use_bias=False),
        K.Flatten(),
        K.Dense(10, activation="softmax"),
    ], name="wide_taps")


def _wide_out(tde, K):
    return tde.Sequential([
        K.Conv2D(8, 1, input_shape=(6, 6, 16)),
        K.Conv2D(32, 3, activation="relu"),
        K.Flatten(),
        K.Dense(10),
    ], name="wide_out")


def _wide_scratch(tde, K):
    return tde.Sequential([
        K.Conv2D(32, 3, input_shape=(6, 6, 16)),
        K.MaxPooling2D(),
        K.Flatten(),
        K.Dense(10),
    ], name="wide_scratch")


def _geo3(tde, K):
    return tde.Sequential([
        K.Conv2D(32, 3, activation="relu", input_shape=(28, 28, 1)),
        K.Flatten(),
        K.Dense(10),
    ], name="geo3")


def _lenet5(tde, K):
    return tde.zoo.lenet5()


def _lenet5_nobias(tde, K):
    return tde.Sequential([
        K.Conv2D(6, 5, padding="same", activation="relu", use_bias=False, input_shape=(28, 28, 1)),
        K.MaxPooling2D(),
        K.Conv2D(16, 5, activation="relu", use_bias=False),
        K.MaxPooling2D(),
        K.Flatten(),
        K.Dense(120, activation="relu"),
        K.Dense(84, activation="relu"),
        K.Dense(10),
    ], name="lenet5_nobias")


# name -> (builder, head gives logits, input bits, conv weight bits).  Three-conv chains take coarser
# grids (the fractional bits of successive convs add up).
MODELS = {
    "padded": (_padded, True, 2, 4),
    "wide_taps": (_wide_taps, False, 4, 6),
    "wide_out": (_wide_out, True, 4, 6),
    "wide_scratch": (_wide_scratch, True, 4, 6),
    "geo3": (_geo3, True, 4, 6),
    "lenet5": (_lenet5, True, 4, 6),
    "lenet5_nobias": (_lenet5_nobias, True, 4, 6),
}
SMALL = ("padded", "wide_taps", "wide_out", "wide_scratch")
FAST = ("lenet5", "lenet5_nobias", "geo3")      # the compile-time-geometry convs
SMALL_BATCHES = ((5, 8), (67, 67))              # (B, plan batch): ragged image quads / past the 64-image block
FAST_BATCH = (37, 64)
CASES = [(n, B, Bp) for n in SMALL for B, Bp in SMALL_BATCHES] + [(n,) + FAST_BATCH for n in FAST]

# seeds for which the near-tie and margin conditions hold (found by trying 0, 1, 2, ... on the oracle)
SEEDS = {("lenet5_nobias", 37, "grid"): 2}     # every other case: 0


def seed_of(name, B, data="grid"):
    return SEEDS.get((name, B, data), 0)


# ------------------------------------------------------------------------------------------ data
def grid_round(t, bits):
    return np.round(np.asarray(t, dtype=np.float64) * 2.0 ** bits) / 2.0 ** bits


def _specs(model):
    return [s for layer in model.layers for s in layer.weight_specs]


def make_weights(model, rng, w_bits):
    """Glorot-uniform kernels and non-zero biases (a zero bias would hide a dropped bias add) from
    ``rng``; conv kernels and conv biases on the 2^-w_bits grid when ``w_bits`` is given."""
    out = {}
    for s in _specs(model):
        conv = len(s.layer.weight_specs[0].shape) == 4
        if s.name == "kernel":
            rf = int(np.prod(s.shape[:-2]))
            lim = np.sqrt(6.0 / (rf * s.shape[-2] + rf * s.shape[-1]))
            v = rng.uniform(-lim, lim, s.shape)
        else:
            v = rng.uniform(-0.25, 0.25, s.shape)
        if conv and w_bits is not None:
            v = grid_round(v, w_bits)
        out[s.full_name] = torch.from_numpy(np.asarray(v, dtype=np.float32))
    return out


def make_batch(model, rng, n, in_bits):
    shp = tuple(model.input_shape[1:])
    ncls = model.output_shape[-1]
    if in_bits is None:
        x = rng.standard_normal((n,) + shp)
    else:
        x = rng.integers(-2 * 2 ** in_bits, 2 * 2 ** in_bits + 1, (n,) + shp) / 2.0 ** in_bits
    y = rng.integers(0, ncls, n)
    return torch.from_numpy(x.astype(np.float32)), torch.from_numpy(y.astype(np.int32))


def build(tde, name, B, data="grid"):
    """The compiled model with its weights loaded, and the batch: (model, x, y) -- x, y on the CPU,
    sized for the plan batch by the caller."""
    fn, logits, in_bits, w_bits = MODELS[name]
    m = fn(tde, tde.keras.layers)
    m.compile(loss=tde.losses.SparseCategoricalCrossentropy(from_logits=logits), optimizer=tde.optimizers.SGD(0.01),
              metrics=["accuracy"])
    m.build()
    rng = np.random.default_rng(1000 + seed_of(name, B, data))
    m._store.load_dict(make_weights(m, rng, w_bits if data == "grid" else None), strict=True)
    return m, rng


def make_case(tde, name, B, Bplan, data="grid"):
    m, rng = build(tde, name, B, data)
    x, y = make_batch(m, rng, Bplan, MODELS[name][2] if data == "grid" else None)
    return m, x, y


# ------------------------------------------------------------------------------------------ oracle
def _weights(model, store, dtype, grad):
    W = {}
    for s in _specs(model):
        t = store.view(s.full_name).detach().cpu().to(dtype).clone()
        W[s.full_name] = t.requires_grad_(True) if grad and s.trainable else t
    return W


def _forward(model, W, x, trunk_only=False):
    """-> (head pre-activation or the trunk's output, records).  records: (kind, layer name, tensor) with
    kind "conv" (every conv pre-activation), "relu_conv" / "relu_dense" (what a ReLU is applied to)."""
    from tensorflow_distributed_example_amd.models import layers as L
    h = x
    rec = []
    last = None
    layers = [l for l in model.layers if not isinstance(l, L.InputLayer)]
    for i, layer in enumerate(layers):
        if isinstance(layer, L.Conv2D):
            assert layer.strides == (1, 1)
            (pt, pb), (pl, pr) = layer.pads(tuple(h.shape[1:]))
            xc = F.pad(h.permute(0, 3, 1, 2), (pl, pr, pt, pb))
            b = W[f"{layer.name}/bias"] if layer.use_bias else None
            z = F.conv2d(xc, W[f"{layer.name}/kernel"].permute(3, 2, 0, 1), b).permute(0, 2, 3, 1)
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
            h = F.max_pool2d(h.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)    # floor: odd edges dropped
        elif isinstance(layer, L.Flatten):
            h = h.reshape(h.shape[0], -1)
        elif isinstance(layer, L.Reshape):
            h = h.reshape((h.shape[0],) + tuple(layer.target_shape))
        elif isinstance(layer, L.Dense):
            if trunk_only:
                return h, rec
            z = h @ W[f"{layer.name}/kernel"]
            if layer.use_bias:
                z = z + W[f"{layer.name}/bias"]
            last = "dense"
            if i == len(layers) - 1:
                assert layer.activation in (None, "softmax")
                return z, rec
            if layer.activation == "relu":
                rec.append(("relu_dense", layer.name, z))
                z = F.relu(z)
            else:
                assert layer.activation is None
            h = z
        else:
            raise NotImplementedError(type(layer).__name__)
    raise AssertionError("no Dense head")


def oracle(model, store, x, y, B, global_batch):
    """float64 forward + autograd.  -> dict(grads {name: f64}, loss (sum of CE), correct, count,
    out (what predict returns: probabilities for a softmax head, logits otherwise), preacts
    [(kind, layer, f64)], near_tie, margin)."""
    W = _weights(model, store, torch.float64, True)
    xd = x[:B].detach().cpu().double()
    yl = y[:B].detach().cpu().long()
    z, rec = _forward(model, W, xd)
    ls = -torch.log_softmax(z, dim=1).gather(1, yl[:, None]).squeeze(1)
    (ls.sum() / float(global_batch)).backward()
    grads = {n: w.grad.detach() for n, w in W.items() if w.requires_grad}
    zd = z.detach()
    softmax = model.layers[-1].activation == "softmax"
    top = zd.topk(2, dim=1).values
    near = 1.0
    for kind, _, t in rec:
        if kind == "relu_dense":
            t = t.detach()
            near = min(near, (t.abs().min() / t.pow(2).mean().sqrt()).item())
    return dict(grads=grads, loss=ls.sum().item(), correct=int((zd.argmax(1) == yl).sum()), count=B,
                out=torch.softmax(zd, 1) if softmax else zd,
                preacts=[(k, n, t.detach()) for k, n, t in rec if k.startswith("relu_")],
                near_tie=near, margin=((top[:, 0] - top[:, 1]).min() / zd.pow(2).mean().sqrt()).item())


def trunk_check(model, store, x, B, in_bits, w_bits):
    """The quantizer's premise as a checked condition.  -> (exact, headroom): ``exact`` -- the fp32 CPU
    forward of the conv trunk equals the float64 one bit for bit, at every conv; ``headroom`` -- the
    smallest, over the convs, of 2^24 step_k / max sum|terms| (must be > 1)."""
    W64 = _weights(model, store, torch.float64, False)
    W32 = {n: w.float() for n, w in W64.items()}
    xd = x[:B].detach().cpu()
    _, r64 = _forward(model, W64, xd.double(), trunk_only=True)
    _, r32 = _forward(model, W32, xd.float(), trunk_only=True)
    Wabs = {n: w.abs() for n, w in W64.items()}
    c64 = [(n, t) for k, n, t in r64 if k == "conv"]
    c32 = [t for k, n, t in r32 if k == "conv"]
    exact = len(c64) == len(c32) and all(torch.equal(a.double(), b) for a, (_, b) in zip(c32, c64))
    # sum of |terms| per conv output: the conv of |input| with |kernel| (+ |bias|), on the true inputs
    headroom = float("inf")
    h = xd.double()
    k = 0
    from tensorflow_distributed_example_amd.models import layers as L
    for layer in model.layers:
        if isinstance(layer, L.Dense):
            break
        if isinstance(layer, L.Conv2D):
            k += 1
            (pt, pb), (pl, pr) = layer.pads(tuple(h.shape[1:]))
            xc = F.pad(h.abs().permute(0, 3, 1, 2), (pl, pr, pt, pb))
            b = Wabs[f"{layer.name}/bias"] if layer.use_bias else None
            tot = F.conv2d(xc, Wabs[f"{layer.name}/kernel"].permute(3, 2, 0, 1), b).max().item()
            headroom = min(headroom, 2.0 ** 24 * 2.0 ** -(in_bits + k * w_bits) / max(tot, 1e-30))
            h = dict((n, t) for n, t in c64)[layer.name]
            if layer.activation == "relu":
                h = F.relu(h)
        elif isinstance(layer, L.Activation):
            h = F.relu(h)
        elif isinstance(layer, L.MaxPooling2D):
            h = F.max_pool2d(h.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
        elif isinstance(layer, L.Reshape):
            h = h.reshape((h.shape[0],) + tuple(layer.target_shape))
    return exact, headroom


# ------------------------------------------------------------------------------------------ comparisons
def rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def reference_errors(tde, model, x, y, B, Bplan, orc):
    """The repository's fp32 torch reference plan on the CPU against the oracle: dict(grads {name: err},
    loss, correct, count, predict, eval_loss, eval_correct)."""
    from tensorflow_distributed_example_amd.train import program as PG
    st = model._store.clone_to("cpu")
    ref = PG.ReferencePlan(model, st, "cpu", Bplan, Bplan, model.optimizer, model.loss)
    xc, yc = x.cpu(), y.long().cpu()
    ref.train_step(xc, yc, B)
    out = dict(grads={n: rel(st.grad(n), orc["grads"][n]) for n in st.names(trainable=True)})
    mt = ref.metrics.clone()
    out.update(loss=abs(mt[0].item() - orc["loss"]) / abs(orc["loss"]), correct=int(mt[1].item()), count=int(mt[2].item()))
    ref.reset_metrics()
    ref.eval_step(xc, yc, B)
    me = ref.metrics.clone()
    out.update(eval_loss=abs(me[0].item() - orc["loss"]) / abs(orc["loss"]), eval_correct=int(me[1].item()),
               predict=rel(ref.predict(xc, B), orc["out"]))
    return out


def grad_hash(store, names):
    return {n: hashlib.sha256(store.grad(n).detach().cpu().contiguous().numpy().tobytes()).hexdigest() for n in names}


def conv_kernel_names(model):
    return [s.full_name for s in _specs(model) if s.name == "kernel" and len(s.shape) == 4]


def measure(tde, name, B, Bplan, data="grid"):
    """One (model, batch) on the GPU in step mode "plain" against the oracle.  -> a JSON-able dict of
    figures; ``check`` asserts on it."""
    from tensorflow_distributed_example_amd.train import program as PG
    m, x, y = make_case(tde, name, B, Bplan, data)
    st = m._store
    in_bits, w_bits = MODELS[name][2:]
    fig = dict(name=name, B=B, Bplan=Bplan, data=data)
    if data == "grid":
        exact, headroom = trunk_check(m, st, x, B, in_bits, w_bits)
        fig.update(trunk_exact=bool(exact), headroom=headroom)
    orc = oracle(m, st, x, y, B, Bplan)
    fig.update(near_tie=orc["near_tie"], margin=orc["margin"])
    ref = reference_errors(tde, m, x, y, B, Bplan, orc)
    plan = PG.make_plan(m, st, "cuda", Bplan, Bplan, m.optimizer, m.loss)
    fig["kind"] = plan.kind
    if plan.kind != "fused_smallnet":
        return fig
    xg, yg = x.cuda(), y.cuda()
    plan.train_step(xg, yg, B)
    torch.cuda.synchronize()
    names = st.names(trainable=True)
    fig["grads"] = {n: [rel(st.grad(n), orc["grads"][n]), ref["grads"][n]] for n in names}
    fig["conv_grad_hash"] = grad_hash(st, conv_kernel_names(m))
    mt = plan.metrics.cpu()
    fig.update(loss=[abs(mt[0].item() - orc["loss"]) / abs(orc["loss"]), ref["loss"]], correct=[mt[1].item(), orc["correct"]],
               count=[mt[2].item(), B], iterations=int(plan.iterations.item()))
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


def bound(ref_err):
    return max(TOL, REF_FACTOR * ref_err)


def check(fig):
    """Print every figure, then assert the bounds."""
    tag = f"{fig['name']} B={fig['B']}/{fig['Bplan']} {fig['data']}"
    assert fig["kind"] == "fused_smallnet", (tag, fig["kind"])
    print(f"[{tag}] near_tie={fig['near_tie']:.3g} margin={fig['margin']:.3g}"
          + (f" trunk_exact={fig['trunk_exact']} headroom={fig['headroom']:.3g}" if fig["data"] == "grid" else ""))
    for n, (e, r) in fig["grads"].items():
        print(f"[{tag}] grad {n}: kernel {e:.3g}  cpu-fp32 {r:.3g}  bound {bound(r):.3g}")
    for k in ("loss", "eval_loss", "predict"):
        print(f"[{tag}] {k}: kernel {fig[k][0]:.3g}  cpu-fp32 {fig[k][1]:.3g}")
    if fig["data"] == "grid":
        assert fig["trunk_exact"] and fig["headroom"] > 1.0, (tag, fig["trunk_exact"], fig["headroom"])
        assert fig["near_tie"] > TIE and fig["margin"] > TIE, (tag, fig["near_tie"], fig["margin"])
    for n, (e, r) in fig["grads"].items():
        assert e <= bound(r), (tag, n, e, r)
    assert fig["loss"][0] <= TOL and fig["eval_loss"][0] <= TOL, (tag, fig["loss"], fig["eval_loss"])
    assert fig["predict"][0] <= TOL and fig["predict_shape"][0] == fig["B"], (tag, fig["predict"], fig["predict_shape"])
    if fig["data"] == "grid":     # exact counts rest on the margin condition
        assert fig["correct"][0] == fig["correct"][1] and fig["eval_correct"][0] == fig["eval_correct"][1], tag
    assert fig["count"][0] == fig["B"] and fig["eval_count"][0] == fig["B"], tag
    assert fig["iterations"] == 1 and fig["iterations_after_eval"] == 1, tag
