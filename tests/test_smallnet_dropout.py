"""CPU side of Dropout on the fused small-net plan: the matcher, the shared seed / layer-id helper
against what the layer-wise plan holds, and the float64 oracle's mask plumbing and input conditions
(tests/smallnet_oracle.py on the dropout suite of tests/smallnet_cases.py).  The kernels themselves:
tests/test_smallnet_dropout_gpu.py."""
import numpy as np
import pytest
import torch

import smallnet_cases as C
import smallnet_oracle as O


def _tde():
    import tensorflow_distributed_example_amd as tde
    return tde, tde.keras.layers


def _logits(tde):
    return tde.losses.SparseCategoricalCrossentropy(from_logits=True)


def _owners(spec):
    return [None if s["drop"] is None else s["drop"].name for s in spec]


def test_matcher_accepts_dropout_with_the_right_owner():
    from tensorflow_distributed_example_amd.models import layers as L
    from tensorflow_distributed_example_amd.train.smallnet import CONV, DENSE, POOL, match_smallnet
    tde, K = _tde()
    for name in ("mask_probe", "pool_drop", "conv_drop", "linear_drop", "linear_rate0", "lenet5_drop"):
        m, _, _ = C.make_case(tde, "dropout", name, 5, 8)
        spec = match_smallnet(m, m.loss)
        assert spec is not None, name
        drops = [l.name for l in m.layers if isinstance(l, L.Dropout)]
        assert [o for o in _owners(spec) if o] == drops, name
    m, _, _ = C.make_case(tde, "dropout", "pool_drop", 5, 8)
    spec = match_smallnet(m, m.loss)
    assert [s["kind"] for s in spec] == [CONV, POOL, DENSE, DENSE]
    assert [o is not None for o in _owners(spec)] == [False, True, True, False]
    m, _, _ = C.make_case(tde, "dropout", "conv_drop", 5, 8)
    assert [o is not None for o in _owners(match_smallnet(m, m.loss))] == [True, False, False]
    # a Flatten and a standalone ReLU between the owner and its Dropout
    m = tde.Sequential([K.Conv2D(4, 3, input_shape=(6, 6, 2)), K.Activation("relu"), K.Flatten(), K.Dropout(0.3),
                        K.Dense(8), K.Activation("relu"), K.Dropout(0.4), K.Dense(3)])
    spec = match_smallnet(m, _logits(tde))
    assert [s["kind"] for s in spec] == [CONV, DENSE, DENSE] and [s["relu"] for s in spec] == [1, 1, 0]
    assert [o is not None for o in _owners(spec)] == [True, True, False]
    assert spec[0]["drop"].rate == 0.3 and spec[1]["drop"].rate == 0.4
    # the Keras quick-start MLP and a Dropout in front of LeNet-5's head
    m = tde.Sequential([K.Flatten(input_shape=(28, 28, 1)), K.Dense(128, activation="relu"), K.Dropout(0.2), K.Dense(10)])
    assert _owners(match_smallnet(m, _logits(tde)))[0] is not None
    # models without Dropout: every entry without one
    for zoo in (tde.zoo.lenet5, tde.zoo.mnist_mlp):
        assert all(s["drop"] is None for s in match_smallnet(zoo(), _logits(tde)))


def test_matcher_rejects():
    from tensorflow_distributed_example_amd.train.smallnet import match_smallnet
    tde, K = _tde()
    lg = _logits(tde)
    bad = {
        "raw input": [K.Dropout(0.5, input_shape=(6,)), K.Dense(4, activation="relu"), K.Dense(3)],
        "raw input behind a Flatten": [K.Flatten(input_shape=(4, 4, 1)), K.Dropout(0.5), K.Dense(4), K.Dense(3)],
        "between a conv and its pool": [K.Conv2D(4, 3, activation="relu", input_shape=(6, 6, 2)), K.Dropout(0.5),
                                        K.MaxPooling2D(), K.Flatten(), K.Dense(3)],
        "after the head": [K.Dense(4, activation="relu", input_shape=(6,)), K.Dense(3), K.Dropout(0.5)],
        "twice on one activation": [K.Dense(4, activation="relu", input_shape=(6,)), K.Dropout(0.5), K.Dropout(0.5),
                                    K.Dense(3)],
        "twice, a Flatten between": [K.Conv2D(4, 3, input_shape=(6, 6, 2)), K.Dropout(0.5), K.Flatten(), K.Dropout(0.5),
                                     K.Dense(3)],
        "rate 1": [K.Dense(4, activation="relu", input_shape=(6,)), K.Dropout(1.0), K.Dense(3)],
        "rate above 1": [K.Dense(4, activation="relu", input_shape=(6,)), K.Dropout(1.5), K.Dense(3)],
        "negative rate": [K.Dense(4, activation="relu", input_shape=(6,)), K.Dropout(-0.1), K.Dense(3)],
        "a ReLU behind the Dropout": [K.Dense(4, input_shape=(6,)), K.Dropout(0.5), K.Activation("relu"), K.Dense(3)],
    }
    for why, layers in bad.items():
        assert match_smallnet(tde.Sequential(layers), lg) is None, why
    ok = [K.Dense(4, activation="relu", input_shape=(6,)), K.Dropout(0.0), K.Dense(3)]
    assert match_smallnet(tde.Sequential(ok), lg) is not None       # rate 0: accepted, the identity


def _act_models(tde, K):
    absorbed = tde.Sequential([K.Conv2D(4, 3, input_shape=(6, 6, 2)), K.Activation("relu"), K.Dropout(0.3), K.Flatten(),
                               K.Dense(8), K.Activation("relu"), K.Dropout(0.4, seed=9), K.Dense(3)], name="absorbed")
    shifted = tde.Sequential([K.Conv2D(4, 3, input_shape=(6, 6, 2)), K.Activation("relu"), K.Flatten(), K.Dropout(0.3),
                              K.Dense(8, activation="relu"), K.Dropout(0.4), K.Dense(3)], name="shifted")
    return {"absorbed": (absorbed, [0, 1]), "shifted": (shifted, [1, 2])}


@pytest.mark.parametrize("which", ["pool_drop", "conv_drop", "linear_drop", "lenet5_drop", "absorbed", "shifted"])
def test_seed_and_lid_helper_matches_layerwise_plan(which):
    """``dropout_ids`` returns what the layer-wise plan (built on the CPU) holds in its DropSpecs; standalone
    Activation layers open stages of their own and shift the ids."""
    from tensorflow_distributed_example_amd.models import layers as L
    from tensorflow_distributed_example_amd.train.elementwise_ids import dropout_ids
    from tensorflow_distributed_example_amd.train.layerwise import LayerwisePlan, _Elementwise
    tde, K = _tde()
    tde.backend.set_global_policy("float32")
    try:
        want_lids = None
        if which in C.MODELS["dropout"]:
            m, _, _ = C.make_case(tde, "dropout", which, 5, 8)
            want_lids = {"pool_drop": [0, 1], "conv_drop": [0], "linear_drop": [0], "lenet5_drop": [0, 1]}[which]
        else:
            tde.backend.set_random_seed(C.MODEL_SEED)
            m, want_lids = _act_models(tde, K)[which]
            m.compile(loss=_logits(tde), optimizer=tde.optimizers.SGD(0.01))
            m.build()
        plan = LayerwisePlan(m, m._store, "cpu", 8, 8, m.optimizer, m.loss)
        held = [(st.drop.rate, st.drop.layer_id, st.drop.seed) for st in plan.stages
                if isinstance(st, _Elementwise) and st.drop.iterations is not None]
        ids = dropout_ids(m)
        drops = [l for l in m.layers if isinstance(l, L.Dropout)]
        assert held == [(l.rate,) + ids[l.name] for l in drops]
        assert [h[1] for h in held] == want_lids
        for l, h in zip(drops, held):
            if l.seed is not None:
                assert h[2] == l.seed
            else:
                assert 0 <= h[2] < 2 ** 62
        assert dropout_ids(m) == ids        # a pure function of the model and the backend seed
    finally:
        tde.backend.set_global_policy(None)


@pytest.mark.parametrize("step", [0, 41])
def test_oracle_mask_plumbing(step):
    """With all-ones activations the oracle's dropped activation IS the keep scales, reshaped: [B, 10] behind a
    Dense (Philox blocks straddle rows) and [B, 2, 2, 4] in NHWC order behind a pool."""
    from tensorflow_distributed_example_amd.ops.philox import keep_scales
    tde, _ = _tde()
    B = 7
    for name in ("mask_probe", "pool_drop"):
        m, x, y = C.make_case(tde, "dropout", name, B, 8)
        first = m.layers[0] if m.layers[0].weight_specs else m.layers[1]
        st = m._store
        st.view(f"{first.name}/kernel").zero_()
        st.view(f"{first.name}/bias").fill_(1.0)
        orc = O.oracle(m, st, x, y, B, 8, step)
        tab = O.drop_table(m)
        dname = [n for n in tab][0]
        rate, seed, lid = tab[dname]
        got = orc["dropped"][dname]
        Dn = int(np.prod(got.shape[1:]))
        want = keep_scales(rate, seed, step, lid, B * Dn).reshape((B,) + tuple(got.shape[1:]))
        assert Dn == {"mask_probe": 10, "pool_drop": 16}[name]
        assert torch.equal(got, torch.from_numpy(want).double())
        assert 0 < (want == 0).mean() < 1
        if name == "mask_probe":
            assert (rate, seed, lid) == (0.5, 1234, 0)
        none = O.oracle(m, st, x, y, B, 8, None)["dropped"][dname]
        assert torch.equal(none, torch.ones_like(none))


@pytest.mark.parametrize("name,B,Bplan", C.CASES["dropout"])
def test_conditions_hold_and_fp32_reference_is_close(name, B, Bplan):
    """The input conditions the GPU tests rest on (exact conv trunk, headroom, near-tie, margin), and the
    fp32 CPU evaluation of the oracle (the reference whose error sets the GPU bound) against float64."""
    tde, _ = _tde()
    c = O.conditions(tde, name, B, Bplan)
    print(f"[{name} B={B}/{Bplan}] {c}")
    assert c["trunk_exact"] and c["headroom"] > 1.0
    assert c["near_tie"] > O.TIE and c["margin"] > O.TIE
    m, x, y = C.make_case(tde, "dropout", name, B, Bplan)
    o64 = O.oracle(m, m._store, x, y, B, Bplan, 0)
    o32 = O.oracle(m, m._store, x, y, B, Bplan, 0, dtype=torch.float32)
    assert set(o64["grads"]) == set(m._store.names(trainable=True))
    for n, g in o64["grads"].items():
        e = O.rel(o32["grads"][n], g)
        print(f"[{name} B={B}/{Bplan}] grad {n}: cpu-fp32 {e:.2g}")
        assert torch.isfinite(g).all() and g.abs().max() > 0 and e < O.TOL, (n, e)
    assert o32["correct"] == o64["correct"]
    # the masks matter: another step index gives other gradients
    o1 = O.oracle(m, m._store, x, y, B, Bplan, 1)
    assert any(O.rel(o1["grads"][n], g) > 1e-2 for n, g in o64["grads"].items())


def test_trajectory_conditions():
    """Near-tie and margin along the three SGD steps of the trajectory test, on the oracle alone."""
    tde, _ = _tde()
    name, B, Bplan = C.TRAJ
    m, x, y = C.make_case(tde, "dropout", name, B, Bplan)
    _, figs = O.trajectory(m, m._store, x, y, B, Bplan, 0.01, C.TRAJ_STEPS)
    for k, f in enumerate(figs):
        print(f"[traj step {k}] near_tie={f['near_tie']:.3g} margin={f['margin']:.3g}")
        assert f["near_tie"] > O.TIE and f["margin"] > O.TIE
