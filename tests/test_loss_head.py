"""CategoricalCrossentropy, label smoothing and ``fit(class_weight=)`` on the CPU: the interface, hand-computed
examples, the one-hot conversion, the refusals, the reference plan against the float64 oracle of
tests/loss_head_oracle.py, ``evaluate`` / validation, two Mirrored CPU replicas and the choice of plan."""
import math
import warnings

import numpy as np
import pytest
import torch

import tensorflow_distributed_example_amd as tde
from tensorflow_distributed_example_amd import losses as LS
from tensorflow_distributed_example_amd import metrics as MT
from tensorflow_distributed_example_amd import optimizers as OP
from tensorflow_distributed_example_amd.models import layers as L
from tensorflow_distributed_example_amd.train import program as PG

import loss_head_oracle as H

B = 8


@pytest.fixture(autouse=True)
def _fresh():
    tde.backend.clear_session()
    tde.backend.set_random_seed(11)
    yield
    tde.backend.clear_session()


def _mlp(loss, opt=None, w0=None, metrics=("accuracy",)):
    m = tde.keras.Sequential([L.Dense(16, activation="relu", input_shape=(12,)), L.Dense(10)])
    m.compile(loss=loss, optimizer=opt or OP.SGD(0.1), metrics=list(metrics))
    m.build()
    if w0 is not None:
        m.set_weights(w0)
    return m


# ------------------------------------------------------------------------------------ the interface
def test_get_strings_constructor_and_config_round_trip():
    for s in ("categorical_crossentropy", "CategoricalCrossentropy"):
        l = LS.get(s)
        assert type(l) is LS.CategoricalCrossentropy and l.label_smoothing == 0.0 and l.from_logits is False
    assert type(LS.get("sparse_categorical_crossentropy")) is LS.SparseCategoricalCrossentropy
    with pytest.raises(ValueError, match="unsupported loss"):
        LS.get("mse")
    l = LS.CategoricalCrossentropy(from_logits=True, label_smoothing=0.25)
    assert LS.get(l) is l and l.name == "categorical_crossentropy" and l.reduction == LS.Reduction.AUTO
    cfg = l.get_config()
    assert cfg == {"from_logits": True, "label_smoothing": 0.25, "reduction": "auto", "name": "categorical_crossentropy"}
    back = LS.CategoricalCrossentropy.from_config(cfg)
    assert back.get_config() == cfg
    assert LS.nontrivial(l) and not LS.nontrivial(LS.CategoricalCrossentropy()) \
        and not LS.nontrivial(LS.SparseCategoricalCrossentropy())
    assert LS.nontrivial(LS.with_class_weight(LS.SparseCategoricalCrossentropy()))
    assert not LS.class_weighted(l) and type(LS.with_class_weight(l)) is type(l)


@pytest.mark.parametrize("bad", [-0.1, 1.0, 1.5, float("nan"), float("inf"), "x", None])
def test_label_smoothing_outside_0_1_raises(bad):
    with pytest.raises(ValueError, match="label_smoothing"):
        LS.CategoricalCrossentropy(label_smoothing=bad)


def test_hand_computed_examples():
    # l = (ln 1, ln 2, ln 5): lse = ln 8, mean = ln(10) / 3; label 1
    z = torch.tensor([[0.0, math.log(2.0), math.log(5.0)]], dtype=torch.float64)
    y = torch.tensor([1])
    nll, sm = math.log(8.0) - math.log(2.0), math.log(8.0) - math.log(10.0) / 3
    want = 0.9 * nll + 0.1 * sm
    got = LS.CategoricalCrossentropy(from_logits=True, label_smoothing=0.1).per_sample(
        np.array([[0, 1, 0]], dtype=np.float32), z.float())
    assert got.shape == (1,) and float(got) == pytest.approx(want, rel=1e-6)
    o = H.head(z, y, 0.1, None)
    assert float(o["loss"]) == pytest.approx(want, rel=1e-14)
    t = torch.tensor([0.1 / 3, 0.9 + 0.1 / 3, 0.1 / 3], dtype=torch.float64)
    assert torch.allclose(o["dlogits"][0], torch.tensor([1 / 8, 2 / 8, 5 / 8], dtype=torch.float64) - t, atol=1e-15)
    # class_weight {0: 2, 2: 0}: rows labelled 0, 1, 2 weigh 2, 1, 0
    z3 = z.repeat(3, 1)
    tab = LS.class_weight_table({0: 2.0, 2: 0.0}, 3)
    assert tab.dtype == np.float32 and tab.tolist() == [2.0, 1.0, 0.0]
    got = LS.SparseCategoricalCrossentropy(from_logits=True).per_sample(
        torch.tensor([0, 1, 2]), z3.float(), class_weight=torch.from_numpy(tab))
    want3 = [2.0 * math.log(8.0), math.log(4.0), 0.0]
    assert got.tolist() == pytest.approx(want3, rel=1e-6)
    o = H.head(z3, torch.tensor([0, 1, 2]), 0.0, tab)
    assert o["loss"].tolist() == pytest.approx(want3, rel=1e-14) and o["dlogits"][2].abs().max() == 0.0
    assert o["dlogits"][0].tolist() == pytest.approx([2 * (1 / 8 - 1), 2 * 2 / 8, 2 * 5 / 8], rel=1e-14)
    # F.cross_entropy(weight=, label_smoothing=) is something else: it weights the smoothing term per class
    fce = torch.nn.functional.cross_entropy(z3, torch.tensor([0, 1, 2]), weight=torch.from_numpy(tab).double(),
                                            label_smoothing=0.1, reduction="none")
    mine = H.head(z3, torch.tensor([0, 1, 2]), 0.1, tab)["loss"]
    assert (fce - mine).abs().max() > 1e-3
    # a label outside [0, C): weight 1, l_y := max, no one-hot term
    o = H.head(z, torch.tensor([5]), 0.1, tab)
    assert float(o["loss"]) == pytest.approx(0.9 * (math.log(8.0) - math.log(5.0)) + 0.1 * sm, rel=1e-14)
    got = LS.softmax_ce(z.float(), torch.tensor([5]), 0.1, torch.from_numpy(tab))
    assert float(got) == pytest.approx(float(o["loss"]), rel=1e-6)


@pytest.mark.parametrize("dtype", [np.float32, np.uint8, np.int64, np.float64, np.bool_])
def test_one_hot_conversion(dtype):
    y = np.array([3, 0, 9, 9, 1])
    idx = LS.onehot_to_index(H.onehot(y, 10, dtype), 10)
    assert idx.dtype == np.int32 and idx.tolist() == y.tolist()
    assert LS.labels_for(LS.CategoricalCrossentropy(), torch.from_numpy(H.onehot(y, 10, np.float32)), 10).tolist() \
        == y.tolist()
    # the sparse loss keeps [N] and [N, 1] labels as they are
    for lab in (y, y[:, None]):
        out = LS.labels_for(LS.SparseCategoricalCrossentropy(), lab, 10)
        assert out.shape == (5,) and out.tolist() == y.tolist()


def test_rows_that_are_not_one_hot_raise():
    soft = np.array([[0.0, 1.0, 0.0], [0.1, 0.8, 0.1]], dtype=np.float32)
    two = np.array([[0, 1, 1]], dtype=np.uint8)
    none = np.zeros((1, 3), dtype=np.int64)
    for bad in (soft, two, none, np.array([[0.0, 2.0, -1.0]]), np.array([[np.nan, 1.0, 0.0]])):
        with pytest.raises(ValueError, match="soft targets are not supported.*label_smoothing"):
            LS.onehot_to_index(bad, 3)
    for bad in (np.eye(4), np.array([0, 1, 2]), np.zeros((2, 3, 1))):
        with pytest.raises(ValueError, match=r"one-hot labels of shape \[N, 3\]"):
            LS.onehot_to_index(bad, 3)
    m = _mlp(LS.CategoricalCrossentropy(from_logits=True))
    x = np.zeros((B, 12), dtype=np.float32)
    y = H.onehot(np.arange(B) % 10, 10)
    with pytest.raises(ValueError, match="soft targets"):
        m.fit(x, y * 0.5, batch_size=B, verbose=0)
    with pytest.raises(ValueError, match=r"\[N, 10\]"):
        m.fit(x, y[:, :9], batch_size=B, verbose=0)
    with pytest.raises(ValueError, match=r"\[N, 10\]"):
        m.evaluate(x, np.arange(B) % 10, batch_size=B, verbose=0)


def test_class_weight_validation():
    assert LS.class_weight_table({}, 4).tolist() == [1.0] * 4
    assert LS.class_weight_table({np.int64(3): 0, 0: np.float32(0.5)}, 4).tolist() == [0.5, 1.0, 1.0, 0.0]
    for bad in ({4: 1.0}, {-1: 1.0}, {1.0: 1.0}, {"1": 1.0}, {True: 1.0}):
        with pytest.raises(ValueError, match="keys must be ints in"):
            LS.class_weight_table(bad, 4)
    for bad in ({0: -0.5}, {0: float("nan")}, {0: float("inf")}, {0: 1e39}, {0: "x"}, {0: None}):
        with pytest.raises(ValueError, match=r"class_weight\[0\]"):
            LS.class_weight_table(bad, 4)
    with pytest.raises(ValueError, match="must be a dict"):
        LS.class_weight_table([1.0, 2.0], 2)
    m = _mlp(LS.SparseCategoricalCrossentropy(from_logits=True))
    x, y = np.zeros((B, 12), dtype=np.float32), np.arange(B) % 10
    with pytest.raises(ValueError, match="keys must be ints"):
        m.fit(x, y, batch_size=B, verbose=0, class_weight={10: 2.0})


def test_sample_weight_and_weighted_metrics_raise_by_name():
    m = _mlp(LS.SparseCategoricalCrossentropy(from_logits=True))
    x, y = np.zeros((B, 12), dtype=np.float32), np.arange(B) % 10
    with pytest.raises(NotImplementedError, match="sample_weight"):
        m.fit(x, y, batch_size=B, verbose=0, sample_weight=np.ones(B))
    with pytest.raises(NotImplementedError, match="sample_weight"):
        m.evaluate(x, y, batch_size=B, verbose=0, sample_weight=np.ones(B))
    with pytest.raises(NotImplementedError, match="weighted_metrics"):
        m.compile(loss="sparse_categorical_crossentropy", optimizer="sgd", weighted_metrics=["accuracy"])
    m.compile(loss="sparse_categorical_crossentropy", optimizer="sgd", weighted_metrics=[])
    m.compile(loss="sparse_categorical_crossentropy", optimizer="sgd", weighted_metrics=None)
    # other keyword arguments of fit keep being accepted
    m.fit(x, y, batch_size=B, verbose=0, workers=2, use_multiprocessing=False, sample_weight=None, class_weight=None)


def test_categorical_accuracy_is_the_alias_under_the_categorical_loss():
    assert MT.resolve(["categorical_accuracy"], LS.CategoricalCrossentropy()) == ["accuracy"]
    assert MT.resolve(["accuracy"], LS.CategoricalCrossentropy()) == ["accuracy"]
    assert MT.resolve(["accuracy"]) == ["accuracy"]
    with pytest.raises(ValueError, match="unsupported metric"):
        MT.resolve(["categorical_accuracy"], LS.SparseCategoricalCrossentropy())
    m = _mlp(LS.CategoricalCrossentropy(from_logits=True), metrics=("categorical_accuracy",))
    rng = np.random.default_rng(0)
    x, yi = rng.standard_normal((2 * B, 12)).astype(np.float32), rng.integers(0, 10, 2 * B)
    ev = m.evaluate(x, H.onehot(yi, 10), batch_size=B, verbose=0, return_dict=True)
    want = float((m.predict(x).argmax(axis=1) == yi).mean())
    assert ev["accuracy"] == want


# ------------------------------------------------------------------------------------ the reference plan
def _loss_of(smooth, categorical=True):
    if categorical:
        return LS.CategoricalCrossentropy(from_logits=True, label_smoothing=smooth)
    assert smooth == 0.0
    return LS.SparseCategoricalCrossentropy(from_logits=True)


def _run_reference(m, batches, class_weight):
    st = m._store
    plan = PG.make_plan(m, st, "cpu", B, B, m.optimizer, m.loss, class_weight=class_weight is not None)
    assert plan.kind == "reference"
    if class_weight is not None:
        plan.set_class_weight(LS.class_weight_table(class_weight, 10))
    losses = []
    for x, y in batches:
        plan.reset_metrics()
        plan.train_step(x, y)
        plan.apply()
        assert float(plan.metrics[2]) == len(y)
        losses.append(float(plan.metrics[0] / plan.metrics[2]))
    return {n: st.view(n).detach().double().clone() for n in st.names(trainable=True)}, losses, plan


@pytest.mark.parametrize("case", list(H.CASES))
def test_reference_plan_against_the_float64_oracle(case):
    smooth, cw = H.CASES[case]
    # class weights alone are a property of fit: under the sparse loss too
    m = _mlp(_loss_of(smooth, categorical=case != "class_weight"), OP.SGD(0.1, momentum=0.5))
    batches = H.batches(m, B, 3, 5)
    w0 = {n: m._store.view(n).detach().double().clone() for n in m._store.names(trainable=True)}
    want, want_loss = H.trajectory(m, batches, m.optimizer, smooth, cw)
    got, got_loss, plan = _run_reference(m, batches, cw)
    assert (plan.class_w is not None) == (cw is not None) and plan.smooth == smooth
    for n in want:
        step = float((want[n] - w0[n]).abs().max())
        e = float((got[n] - want[n]).abs().max())
        print(f"[{case}] {n}: |reference - float64| {e:.3g}, moved {step:.3g}")
        # float32 against float64 over three steps (the bound of tests/test_weight_reg.py); a missing weight or
        # smoothing term is of the order of the step itself
        assert step > 0 and e <= 2e-6 + 1e-3 * step, (n, e, step)
    for k, (a, b) in enumerate(zip(got_loss, want_loss)):
        print(f"[{case}] step {k}: loss {a!r} float64 {b!r}")
        assert abs(a - b) <= 4e-6 * abs(b), (k, a, b)
    # the plain loss from the same start ends elsewhere and logs another loss
    tde.backend.clear_session()
    twin = _mlp(_loss_of(0.0), OP.SGD(0.1, momentum=0.5), w0=[w0[n].float().numpy() for n in w0])
    tw, tl, _ = _run_reference(twin, batches, None)
    assert abs(tl[0] - got_loss[0]) > 1e-3 * tl[0]
    assert max(float((tw[a] - want[b]).abs().max()) for a, b in zip(tw, want)) > 1e-4


def test_categorical_without_smoothing_is_the_sparse_loss_bitwise():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((3 * B, 12)).astype(np.float32)
    yi = rng.integers(0, 10, 3 * B)
    a = _mlp(_loss_of(0.0, categorical=False))
    w0 = a.get_weights()
    ha = a.fit(x, yi, batch_size=B, epochs=2, verbose=0, shuffle=False)
    tde.backend.clear_session()
    b = _mlp(_loss_of(0.0), w0=w0)
    hb = b.fit(x, H.onehot(yi, 10, np.uint8), batch_size=B, epochs=2, verbose=0, shuffle=False)
    assert ha.history == hb.history
    for u, v in zip(a.get_weights(), b.get_weights()):
        assert np.array_equal(u, v)
    assert a.evaluate(x, yi, batch_size=B, verbose=0) == b.evaluate(x, H.onehot(yi, 10), batch_size=B, verbose=0)


def test_evaluate_smooths_and_ignores_class_weights_and_validation_is_unweighted():
    smooth, cw = H.CASES["both"]
    m = _mlp(_loss_of(smooth), OP.SGD(0.0))          # lr 0: the weights stay
    (x, y), = H.batches(m, 2 * B, 1, 9)
    yh = H.onehot(y.numpy(), 10)
    unweighted = H.eval_loss(m, x, y, smooth)
    _, (weighted,) = H.trajectory(m, [(x, y)], m.optimizer, smooth, cw)
    assert abs(weighted - unweighted) > 0.05 * unweighted and abs(unweighted - H.eval_loss(m, x, y, 0.0)) > 1e-3
    h = m.fit(x.numpy(), yh, batch_size=B, epochs=1, verbose=0, shuffle=False, class_weight=cw,
              validation_data=(x.numpy(), yh))
    ev = m.evaluate(x.numpy(), yh, batch_size=B, verbose=0, return_dict=True)
    print(f"fit {h.history['loss'][0]!r} (float64 {weighted!r}) val {h.history['val_loss'][0]!r} evaluate "
          f"{ev['loss']!r} (float64 {unweighted!r})")
    assert h.history["loss"][0] == pytest.approx(weighted, rel=4e-6)
    assert h.history["val_loss"][0] == pytest.approx(unweighted, rel=4e-6) == pytest.approx(ev["loss"], rel=4e-6)
    # the accuracy is unweighted everywhere
    acc = float((m.predict(x.numpy()).argmax(axis=1) == y.numpy()).mean())
    assert h.history["accuracy"][0] == h.history["val_accuracy"][0] == ev["accuracy"] == acc


def test_a_second_fit_with_other_weights_reuses_the_program():
    m = _mlp(_loss_of(0.0, categorical=False), OP.SGD(0.0))
    (x, y), = H.batches(m, B, 1, 2)
    plain = m.fit(x.numpy(), y.numpy(), batch_size=B, verbose=0, shuffle=False).history["loss"][0]
    p0 = m._program("train", B)
    h1 = m.fit(x.numpy(), y.numpy(), batch_size=B, verbose=0, shuffle=False, class_weight={0: 2.0})
    p1 = m._program("train", B, class_weight=True)
    h2 = m.fit(x.numpy(), y.numpy(), batch_size=B, verbose=0, shuffle=False, class_weight={0: 0.0, 2: 3.0})
    assert m._program("train", B, class_weight=True) is p1 and p1 is not p0 and m._program("train", B) is p0
    assert p0.plans[0].class_w is None and p1.plans[0].class_w.tolist() == [0.0, 1.0, 3.0] + [1.0] * 7
    for h, cw in ((h1, {0: 2.0}), (h2, {0: 0.0, 2: 3.0})):
        _, (want,) = H.trajectory(m, [(x, y)], m.optimizer, 0.0, cw)
        assert h.history["loss"][0] == pytest.approx(want, rel=4e-6) and abs(want - plain) > 1e-3


def test_two_mirrored_cpu_replicas_equal_one_at_the_same_global_batch():
    smooth, cw = H.CASES["both"]
    rng = np.random.default_rng(8)
    x = rng.standard_normal((4 * B, 12)).astype(np.float32)
    yh = H.onehot(np.concatenate([[0, 2, 7], rng.integers(0, 10, 4 * B - 3)]), 10)

    def run(strategy, w0=None):
        with strategy.scope():
            m = _mlp(_loss_of(smooth), OP.SGD(0.1), w0=w0)
        start = m.get_weights()
        ds = tde.data.Dataset.from_tensor_slices((x, yh)).batch(2 * B)
        h = m.fit(ds, epochs=2, verbose=0, class_weight=cw)
        return m, start, h.history

    m2, w0, h2 = run(tde.distribute.MirroredStrategy(["cpu", "cpu"]))
    prog = m2._program("train", 2 * B, class_weight=True)
    assert len(prog.plans) == 2 and prog.B == B and all(p.class_w is not None for p in prog.plans)
    tde.backend.clear_session()
    m1, _, h1 = run(tde.distribute.OneDeviceStrategy("cpu"), w0)
    for a, b in zip(m2.get_weights(), m1.get_weights()):
        assert np.allclose(a, b, rtol=1e-4, atol=2e-5)      # the tolerance of tests/test_distributed_cpu.py
    assert h2["loss"] == pytest.approx(h1["loss"], rel=1e-5) and h2["accuracy"] == h1["accuracy"]
    assert any(not np.array_equal(a, b) for a, b in zip(m1.get_weights(), w0))


# ------------------------------------------------------------------------------------ which plan runs what
def test_matchers_accept_the_trivial_spec_and_decline_the_rest_with_one_warning():
    from tensorflow_distributed_example_amd.train import bncnn, smallnet
    cnn, bn, mlp = tde.zoo.mnist_cnn(), tde.zoo.mnist_bn_cnn(), tde.zoo.mnist_mlp()
    for model, match in ((cnn, PG.match_convnet), (bn, bncnn.match_bncnn)):
        fl = model.layers[-1].activation != "softmax"
        sparse = LS.SparseCategoricalCrossentropy(from_logits=fl)
        cat0 = LS.CategoricalCrossentropy(from_logits=fl)
        cat1 = LS.CategoricalCrossentropy(from_logits=fl, label_smoothing=0.1)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            assert match(model, sparse) is not None and match(model, cat0) is not None
        for loss, names in ((cat1, "label_smoothing=0.1"), (LS.with_class_weight(sparse), "class_weight"),
                            (LS.with_class_weight(cat1), "label_smoothing=0.1.*class_weight")):
            with pytest.warns(UserWarning, match=f"no loss head for .*{names}.*per-layer kernel plan") as rec:
                assert match(model, loss) is None
            assert len(rec) == 1
    # the small-net step has a loss-head variant: it takes every spec
    fl = mlp.layers[-1].activation != "softmax"
    cat1 = LS.CategoricalCrossentropy(from_logits=fl, label_smoothing=0.1)
    for loss in (LS.SparseCategoricalCrossentropy(from_logits=fl), LS.CategoricalCrossentropy(from_logits=fl), cat1,
                 LS.with_class_weight(cat1)):
        assert smallnet.match_smallnet(mlp, loss) is not None
    assert smallnet.match_smallnet(mlp, object()) is None and PG.match_convnet(cnn, object()) is None


def test_make_plan_on_the_cpu_is_the_reference_plan_for_every_spec():
    for loss, cw in ((_loss_of(0.0), False), (_loss_of(0.1), False), (_loss_of(0.0, False), True)):
        m = _mlp(loss)
        plan = PG.make_plan(m, m._store, "cpu", B, B, m.optimizer, m.loss, class_weight=cw)
        assert plan.kind == "reference" and plan.loss_spec == (cw or LS.smoothing(loss) != 0)
        assert (plan.class_w is not None) == cw
        if not cw:
            with pytest.raises(RuntimeError, match="not built for class weights"):
                plan.set_class_weight(np.ones(10, dtype=np.float32))
        else:
            with pytest.raises(ValueError, match="10 classes"):
                plan.set_class_weight(np.ones(9, dtype=np.float32))
        tde.backend.clear_session()
