"""Test models, batches and seeds of the fused small-net plan's suites (train/smallnet.py,
csrc/kernels/smallnet.hip): data for the float64 oracle of tests/smallnet_oracle.py.  A plain helper module,
imported by the small-net test files and by tests/_smallnet_child.py.

Suites.  ``forms``: every conv form and padded edge, relu and max pool, on quantized data (inputs and conv
weights on dyadic grids, see smallnet_oracle) and one unquantized LeNet-5 step.  ``act``: tanh, sigmoid and
the average pool, which are smooth and take randn data and Glorot weights.  ``dropout``: Dropout layers, on
quantized data; a Dropout in front of a conv keeps the trunk exact only when its scale is a power of two, so
``conv_drop`` drops at rate 0.5 (scale 2: one bit of headroom); ``pool_drop`` and ``lenet5_drop`` drop behind
the last conv, where the scale may be anything.

Seeds.  The rng of a case is seeded with the suite's base + SEEDS[(name, B, data)] (default 0) and draws the
weights first, then the batch.  SEEDS holds the first of 0, 1, 2, ... at which the suite's conditions on the
inputs hold on the oracle alone, on the CPU (``smallnet_oracle.find_seed``).
"""
from typing import Callable, NamedTuple, Optional

import numpy as np

import smallnet_oracle as O

MODEL_SEED = 11      # backend seed under which unseeded Dropout layers draw their Philox keys


# ------------------------------------------------------------------------------------------ forms
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


# ------------------------------------------------------------------------------------------ act
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


# ------------------------------------------------------------------------------------------ dropout
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


def _union(tde, K, rate=0.5):
    """Needs a tanh conv, an average pool and a Dropout in one walk (tests/test_smallnet_oracle.py)."""
    return tde.Sequential([
        K.Conv2D(4, 3, activation="tanh", input_shape=(6, 6, 2)),
        K.AveragePooling2D(),
        K.Dropout(rate, seed=9),
        K.Flatten(),
        K.Dense(7, activation="relu"),
        K.Dense(4),
    ], name="union")


def _union_rate0(tde, K):
    return _union(tde, K, 0.0)


# ------------------------------------------------------------------------------------------ tables
class Row(NamedTuple):
    builder: Callable
    logits: bool                        # the head gives logits (else probabilities)
    bits: Optional[tuple] = None        # (input bits, conv weight bits) of the quantizer; None: randn data
    base: int = 1000                    # the case's rng is seeded with base + seed
    model_seed: Optional[int] = None    # backend seed set before the model is built
    codes: Optional[tuple] = None       # expected plan entry (kinds, activation codes, mask_in codes)


def _drop(builder, logits, bits):
    return Row(builder, logits, bits, base=2000, model_seed=MODEL_SEED)


def _act(builder, logits, *codes):
    return Row(builder, logits, base=2000, codes=codes)


# Three-conv chains take coarser grids (the fractional bits of successive convs add up).
# act codes -- kinds: 0 conv, 1 max pool, 2 dense, 3 average pool; activations: 0 linear, 1 relu, 2 tanh, 3 sigmoid
MODELS = {
    "forms": {
        "padded": Row(_padded, True, (2, 4)),
        "wide_taps": Row(_wide_taps, False, (4, 6)),
        "wide_out": Row(_wide_out, True, (4, 6)),
        "wide_scratch": Row(_wide_scratch, True, (4, 6)),
        "geo3": Row(_geo3, True, (4, 6)),
        "lenet5": Row(_lenet5, True, (4, 6)),
        "lenet5_nobias": Row(_lenet5_nobias, True, (4, 6)),
    },
    "act": {
        "act_padded": _act(_act_padded, True, [0, 0, 3, 0, 2, 2], [2, 3, 0, 0, 2, 0], [0, 2, 3, 0, 0, 2]),
        "avg_linear": _act(_avg_linear, True, [0, 3, 2], [0, 0, 0], [0, 0, 0]),
        "tanh_maxpool": _act(_tanh_maxpool, False, [0, 1, 0, 2], [2, 0, 3, 0], [0, 2, 0, 3]),
        "act_layers": _act(_act_layers, True, [0, 2, 2, 2], [2, 3, 1, 0], [0, 2, 3, 1]),
        "mlp_tanh": _act(_mlp_tanh, True, [2, 2, 2], [2, 3, 0], [0, 2, 3]),
        "lenet5_classic": _act(_lenet5_classic, True, [0, 3, 0, 3, 2, 2, 2], [2, 0, 2, 0, 2, 2, 0], [0, 2, 0, 2, 0, 2, 2]),
        # a compile-time-geometry conv, X(5, 5, 6, 16, 14, 14), whose input IS a tanh conv output (no pool in
        # between): the only way into sn_conv_dgrad_c / sn_conv_dgrad_m with a derivative code
        "dgrad_tanh": _act(_dgrad_tanh, True, [0, 0, 3, 2], [2, 2, 0, 0], [0, 2, 2, 0]),
    },
    "dropout": {
        "mask_probe": _drop(_mask_probe, True, (4, 6)),
        "pool_drop": _drop(_pool_drop, True, (4, 6)),
        "conv_drop": _drop(_conv_drop, True, (2, 4)),
        "linear_drop": _drop(_linear_drop, False, (4, 6)),
        "linear_rate0": _drop(_linear_rate0, False, (4, 6)),
        "linear_plain": _drop(_linear_plain, False, (4, 6)),
        "lenet5_drop": _drop(_lenet5_drop, True, (4, 6)),
        "union": _drop(_union, True, None),
        "union_rate0": _drop(_union_rate0, True, None),
    },
}
SMALL = {
    "forms": ("padded", "wide_taps", "wide_out", "wide_scratch"),
    "act": ("act_padded", "avg_linear", "tanh_maxpool", "act_layers", "mlp_tanh"),
    "dropout": ("pool_drop", "conv_drop", "linear_drop"),
}
FAST = {                                        # the compile-time-geometry convs
    "forms": ("lenet5", "lenet5_nobias", "geo3"),
    "act": ("lenet5_classic", "dgrad_tanh"),
    "dropout": ("lenet5_drop",),
}
SMALL_BATCHES = ((5, 8), (67, 67))              # (B, plan batch): ragged image quads / past the 64-image block
FAST_BATCH = (37, 64)
CASES = {s: [(n, B, Bp) for n in SMALL[s] for B, Bp in SMALL_BATCHES] + [(n,) + FAST_BATCH for n in FAST[s]]
         for s in MODELS}
TRAJ = ("pool_drop", 5, 8)                      # the three-step SGD trajectory of the dropout suite
TRAJ_STEPS = 3

# (name, B, data) -> seed; every other case: 0
SEEDS = {
    ("lenet5_nobias", 37, "grid"): 2,       # near_tie, margin; seed 0 leaves a Dense ReLU unit at 3.6e-5 rms
    ("lenet5_drop", 37, "grid"): 1,         # near_tie, margin at step 0 (TRAJ: along the three steps at seed 0)
    ("tanh_maxpool", 67, "randn"): 1,       # relu_near, pool_gap, margin; seed 0 leaves a pool window with a
    #                                         top-2 gap of 7.6e-7 rms
    ("union", 5, "randn"): 0,               # relu_near 0.022, margin 0.10 at step 0: the first seed tried holds
    ("union_rate0", 5, "randn"): 0,         # the same inputs
}


def data_of(suite, name):
    """The kind of data a model takes by default: "grid" (quantized) or "randn"."""
    return "grid" if MODELS[suite][name].bits else "randn"


def build(tde, suite, name, B, data=None, seed=None):
    """-> (the compiled model with its weights loaded, the rng the batch is drawn from next)."""
    row = MODELS[suite][name]
    data = data or data_of(suite, name)
    if row.model_seed is not None:
        tde.backend.set_random_seed(row.model_seed)
    m = row.builder(tde, tde.keras.layers)
    m.compile(loss=tde.losses.SparseCategoricalCrossentropy(from_logits=row.logits),
              optimizer=tde.optimizers.SGD(0.01), metrics=["accuracy"])
    m.build()
    rng = np.random.default_rng(row.base + (SEEDS.get((name, B, data), 0) if seed is None else seed))
    m._store.load_dict(O.make_weights(m, rng, row.bits[1] if data == "grid" else None), strict=True)
    return m, rng


def make_case(tde, suite, name, B, Bplan, data=None, seed=None):
    """-> (model, x, y), on the CPU, the batch sized for the plan.  ``data`` "randn" on a quantized model: the
    same model on unquantized weights and inputs; ``seed`` replaces the SEEDS entry."""
    data = data or data_of(suite, name)
    m, rng = build(tde, suite, name, B, data, seed)
    x, y = O.make_batch(m, rng, Bplan, MODELS[suite][name].bits[0] if data == "grid" else None)
    return m, x, y
