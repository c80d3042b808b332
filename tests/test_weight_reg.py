"""Weight regularizers (l1 / l2 / l1_l2 on the layers) and decoupled weight decay (``weight_decay``, ``AdamW``)
on the CPU: the interface, ``Model.losses`` by hand, the reference plan against the float64 autograd oracle of
tests/weight_reg_oracle.py (which differentiates ``mean CE + sum P`` itself), the order against clipping, the
refusals, and the table builder of the device launches."""
import json

import numpy as np
import pytest
import torch

import tensorflow_distributed_example_amd as tde
from tensorflow_distributed_example_amd import _native as N
from tensorflow_distributed_example_amd import optimizers as OP
from tensorflow_distributed_example_amd import regularizers as RG
from tensorflow_distributed_example_amd.models import layers as L
from tensorflow_distributed_example_amd.train import program as PG

import weight_reg_oracle as W

B = 8


@pytest.fixture(autouse=True)
def _fresh():
    tde.backend.clear_session()
    tde.backend.set_random_seed(5)
    yield
    tde.backend.clear_session()


def _loss():
    return tde.losses.SparseCategoricalCrossentropy(from_logits=True)


def _mlp(opt, kernel=None, bias=None, out_kernel=None, w0=None):
    """zoo.mnist_mlp's layers, regularized."""
    m = tde.keras.Sequential([L.Flatten(input_shape=(28, 28, 1)),
                              L.Dense(128, activation="relu", kernel_regularizer=kernel, bias_regularizer=bias),
                              L.Dense(10, kernel_regularizer=out_kernel)])
    m.compile(loss=_loss(), optimizer=opt, metrics=["accuracy"])
    m.build()
    if w0 is not None:
        m.set_weights(w0)
    return m


# ------------------------------------------------------------------------------------ the regularizer classes
def test_classes_aliases_strings_and_configs():
    assert tde.regularizers is RG and tde.keras.regularizers is RG
    assert RG.l1 is RG.L1 and RG.l2 is RG.L2
    a, b, c = RG.L1(0.25), RG.L2(0.5), RG.L1L2(l1=0.125, l2=2.0)
    assert a.coefficients == (0.25, 0.0) and b.coefficients == (0.0, 0.5) and c.coefficients == (0.125, 2.0)
    assert RG.l1_l2(l1=0.125, l2=2.0) == c and RG.l1_l2().coefficients == (0.01, 0.01)
    assert RG.L1().l1 == 0.01 and RG.L2().l2 == 0.01 and RG.L1L2().coefficients == (0.0, 0.0)
    assert a.get_config() == {"l1": 0.25} and b.get_config() == {"l2": 0.5} and c.get_config() == {"l1": 0.125, "l2": 2.0}
    for r in (a, b, c):
        assert type(r)(**r.get_config()) == r and RG.get(RG.serialize(r)) == r and RG.get(r) is r
    assert RG.get(None) is None
    assert RG.get("l1") == RG.L1(0.01) and RG.get("l2") == RG.L2(0.01) and RG.get("l1_l2") == RG.L1L2(0.01, 0.01)
    with pytest.raises(ValueError, match="unsupported regularizer"):
        RG.get("l3")
    x = torch.tensor([[1.0, -2.0], [0.0, -0.0]], dtype=torch.float64)
    assert float(a(x)) == 0.75 and float(b(x)) == 2.5 and float(c(x)) == 0.375 + 10.0
    for dt in (torch.float32, torch.float64, torch.bfloat16):
        assert c(x.to(dt)).dtype == dt


@pytest.mark.parametrize("bad", [-1e-3, float("nan"), float("inf"), -float("inf"), "x"])
def test_negative_or_non_finite_coefficients_raise(bad):
    for make in (lambda: RG.L1(bad), lambda: RG.L2(bad), lambda: RG.L1L2(l1=bad), lambda: RG.L1L2(l2=bad),
                 lambda: RG.l1_l2(0.1, bad)):
        with pytest.raises(ValueError, match="finite float >= 0"):
            make()


def test_activity_regularizer_is_refused_by_name():
    for make in (lambda: L.Dense(4, activity_regularizer=RG.L2(0.1)),
                 lambda: L.Conv2D(4, 3, activity_regularizer="l2"),
                 lambda: L.BatchNormalization(activity_regularizer=RG.L1(0.1))):
        with pytest.raises(TypeError, match="activity_regularizer is not supported"):
            make()
    with pytest.raises(TypeError, match="unexpected argument 'kernel_regulariser'"):
        L.Dense(4, kernel_regulariser=RG.L2(0.1))
    with pytest.raises(TypeError, match="unexpected argument"):
        L.MaxPooling2D(kernel_regularizer=RG.L2(0.1))


def test_layer_arguments_reach_the_weight_specs_and_configs_round_trip():
    d = L.Dense(64, kernel_regularizer=RG.l2(0.5), bias_regularizer="l1")
    cv = L.Conv2D(4, 3, kernel_regularizer=RG.l1_l2(0.25, 0.125), bias_regularizer=RG.L2(2.0))
    bn = L.BatchNormalization(gamma_regularizer=RG.L2(0.25), beta_regularizer=RG.L1(0.5))
    plain = L.Dense(3)
    m = tde.keras.Sequential([L.Conv2D(2, 1, input_shape=(6, 6, 1)), cv, bn, L.Flatten(), d, plain])
    m.build()
    spec = {s.full_name: (s.l1, s.l2) for l in m.layers for s in l.weight_specs}
    assert spec[f"{d.name}/kernel"] == (0.0, 0.5) and spec[f"{d.name}/bias"] == (0.01, 0.0)
    assert spec[f"{cv.name}/kernel"] == (0.25, 0.125) and spec[f"{cv.name}/bias"] == (0.0, 2.0)
    assert spec[f"{bn.name}/gamma"] == (0.0, 0.25) and spec[f"{bn.name}/beta"] == (0.5, 0.0)
    assert spec[f"{bn.name}/moving_mean"] == (0.0, 0.0) and spec[f"{plain.name}/kernel"] == (0.0, 0.0)
    assert "kernel_regularizer" not in plain.get_config() and "bias_regularizer" not in plain.get_config()
    assert L.WeightSpec("k", (1,), None).l1 == 0.0 and L.WeightSpec("k", (1,), None).l2 == 0.0
    for layer in (d, cv, bn):
        cfg = layer.get_config()
        json.dumps(cfg)
        back = L.from_config(type(layer).__name__, cfg)
        assert back.get_config() == cfg
    again = tde.keras.Sequential.from_config(json.loads(m.to_json())["config"])
    again.build()
    assert {s.full_name: (s.l1, s.l2) for l in again.layers for s in l.weight_specs} == spec
    lay = L.Layer(name="custom")
    s = lay.add_weight("w", (3,), regularizer=RG.l1_l2(0.5, 0.25))
    assert (s.l1, s.l2) == (0.5, 0.25) and lay.add_weight("v", (3,)).l2 == 0.0


def test_model_losses_by_hand():
    m = _mlp(OP.SGD(0.1), kernel=RG.l1_l2(0.5, 0.25), bias=RG.L2(2.0))
    st = m._store
    k, b = st.view(m.layers[1].name + "/kernel"), st.view(m.layers[1].name + "/bias")
    b.copy_(torch.linspace(-1, 1, 128))
    got = m.losses
    assert len(got) == 2 and all(t.dtype == torch.float64 and t.device.type == "cpu" and t.dim() == 0 for t in got)
    k64, b64 = k.double().numpy(), b.double().numpy()
    want = [0.5 * np.abs(k64).sum() + 0.25 * (k64 * k64).sum(), 2.0 * (b64 * b64).sum()]
    assert [float(t) for t in got] == pytest.approx(want, rel=1e-14)
    assert _mlp(OP.SGD(0.1)).losses == []
    r = tde.zoo.mini_resnet(l2=1e-4)
    convs_and_dense = [l for l in r.layers if isinstance(l, (L.Conv2D, L.Dense))]
    assert len(r.losses) == len(convs_and_dense) == len(RG.coefficients(r))
    assert all(n.endswith("/kernel") and c == (0.0, 1e-4) for n, c in RG.coefficients(r).items())
    assert tde.zoo.mini_resnet().losses == [] and tde.zoo.resnet18(input_shape=(32, 32, 3), classes=10, l2=None).losses == []


# ------------------------------------------------------------------------------------ the optimizers
def test_weight_decay_argument_config_and_key():
    for make in (lambda **k: OP.SGD(0.1, **k), lambda **k: OP.SGD(0.1, momentum=0.5, **k), lambda **k: OP.Adam(**k),
                 lambda **k: OP.RMSprop(**k)):
        off, zero, on = make(), make(weight_decay=0), make(weight_decay=0.25)
        assert off.weight_decay is None and off.decay is None and zero.weight_decay == 0.0 and zero.decay is None
        assert on.weight_decay == on.decay == 0.25
        assert "weight_decay" not in off.get_config() and on.get_config()["weight_decay"] == 0.25
        assert zero.get_config()["weight_decay"] == 0.0
        assert on.key() != off.key() and zero.key() == off.key() and make(weight_decay=0.25).key() == on.key()
        assert make(weight_decay=0.5).key() != on.key()
        back = type(on)(**on.get_config())
        assert back.key() == on.key() and back.get_config() == on.get_config()
        ex = make(weight_decay=0.25)
        ex.exclude_from_weight_decay(var_names=["bias"])
        assert ex.key() != on.key() and hash(ex.key()) is not None
        for bad in (-0.1, float("nan"), float("inf"), "much"):
            with pytest.raises(ValueError, match="weight_decay must be a finite float >= 0"):
                make(weight_decay=bad)
    with pytest.raises(TypeError):
        OP.GradientDescentOptimizer(0.1, weight_decay=0.1)
    with pytest.raises(TypeError):
        OP.GradientDescentOptimizer(0.1, kernel_regularizer=RG.L2(0.1))
    assert "weight_decay" not in OP.GradientDescentOptimizer(0.1).get_config()


def test_adamw_defaults_and_get():
    o = OP.AdamW()
    assert (o.learning_rate, o.weight_decay, o.beta_1, o.beta_2, o.epsilon, o.name) == (0.001, 0.004, 0.9, 0.999, 1e-7, "AdamW")
    assert o.kind == "adam" and o.slot_names() == ["m", "v"] and isinstance(OP.get("adamw"), OP.AdamW)
    assert OP.AdamW(**o.get_config()).key() == o.key()
    with pytest.raises(ValueError, match="AdamW needs a weight_decay"):
        OP.AdamW(weight_decay=None)
    assert OP.AdamW(0.01, 0.5, clipnorm=1.0).clip == ("clipnorm", 1.0)


def test_exclude_from_weight_decay_matches_and_closes_after_build():
    o = OP.AdamW()
    m = _mlp(o)
    names = m._store.names(trainable=True)
    k1 = m.layers[1].weight_specs[0]
    o.exclude_from_weight_decay(var_list=[k1], var_names=["bias"])
    assert [o.decays(n) for n in names] == [False, False, True, False]
    assert not OP.SGD(0.1).decays(names[0])
    with pytest.raises(TypeError):
        o.exclude_from_weight_decay(var_list=[3.5])
    plan = PG.make_plan(m, m._store, "cpu", B, B, o, m.loss)
    assert plan.decay_segments() == [(m._store.segments[names[2]].offset, m._store.segments[names[2]].numel)]
    with pytest.raises(ValueError, match="before the optimizer has built a plan"):
        o.exclude_from_weight_decay(var_names=["kernel"])


def test_decay_and_regularizer_by_hand():
    """One variable w = (2, -1, +0, -0), g = 1/2: l1 = 1/4, l2 = 1/8, wd = 1/2, lr = 1/4, SGD."""
    opt = OP.SGD(0.25, weight_decay=0.5)
    w = torch.tensor([2.0, -1.0, 0.0, -0.0])
    g = torch.full((4,), 0.5)
    RG.reg_reference(w, g, [(0, 4, 0.25, 0.125)])
    assert g.tolist() == [0.5 + 0.5 + 0.25, 0.5 - 0.25 - 0.25, 0.5, 0.5]          # sgn(+-0) = 0
    assert float(RG.penalty(w.double(), [(0, 4, 0.25, 0.125)])) == 0.25 * 3 + 0.125 * 5
    opt.decay_reference(w, [(0, 2)], 0)                                           # the last two do not decay
    assert w.tolist() == [2.0 - 0.25, -1.0 + 0.125, 0.0, -0.0]
    opt.apply_reference(w, g, {}, 0)
    assert w.tolist() == [1.75 - 0.3125, -0.875, -0.125, -0.125]
    # under a schedule the decay uses the step's rate, and Adam's decay is not bias-corrected
    sch = tde.optimizers.schedules.PiecewiseConstantDecay([1], [0.5, 0.125])
    a = OP.AdamW(sch, weight_decay=0.5)
    w = torch.tensor([4.0])
    a.decay_reference(w, [(0, 1)], 0)
    assert w.item() == 3.0
    a.decay_reference(w, [(0, 1)], 2)                        # past the boundary: the second rate
    assert w.item() == 3.0 - 3.0 * 0.5 * 0.125


# ------------------------------------------------------------------------------------ the reference plan
def _run_reference(m, batches):
    """Three steps of the CPU reference plan.  -> (weights {name: float64}, [the step's logged loss])."""
    st = m._store
    plan = PG.make_plan(m, st, "cpu", B, B, m.optimizer, m.loss)
    assert plan.kind == "reference" and plan.step_mode == "plain"
    losses = []
    for x, y in batches:
        plan.reset_metrics()
        plan.train_step(x, y)
        plan.apply()
        losses.append(float(plan.metrics[0] / plan.metrics[2]))
    assert int(plan.iterations) == len(batches)
    return {n: st.view(n).detach().double().clone() for n in st.names(trainable=True)}, losses


CASES = {
    # (the optimizer, the regularizers, the names excluded from the decay, the twin without the feature)
    "sgd_l2": lambda: (OP.SGD(0.05), dict(kernel=RG.L2(0.01), out_kernel=RG.L2(0.02)), None, OP.SGD(0.05)),
    "adam_l1_l2": lambda: (OP.Adam(1e-3), dict(kernel=RG.l1_l2(1e-4, 1e-3), bias=RG.L1(1e-3), out_kernel="l1_l2"), None,
                           OP.Adam(1e-3)),
    "adamw_schedule_excluded_bias": lambda: (
        OP.AdamW(tde.optimizers.schedules.ExponentialDecay(2e-3, 1, 0.5), weight_decay=0.05),
        dict(kernel=RG.L2(1e-3)), ["bias"], OP.Adam(tde.optimizers.schedules.ExponentialDecay(2e-3, 1, 0.5))),
}


@pytest.mark.parametrize("case", list(CASES))
def test_reference_plan_against_the_float64_autograd_oracle(case):
    opt, regs, exclude, twin_opt = CASES[case]()
    if exclude:
        opt.exclude_from_weight_decay(var_names=exclude)
    m = _mlp(opt, **regs)
    batches = W.batches(m, B, 3, 31)
    w0 = {n: m._store.view(n).detach().double().clone() for n in m._store.names(trainable=True)}
    want, want_loss, _ = W.trajectory(m, batches, opt, decays=opt.decays)
    got, got_loss = _run_reference(m, batches)
    for n in want:
        step = float((want[n] - w0[n]).abs().max())
        e = float((got[n] - want[n]).abs().max())
        print(f"[{case}] {n}: |reference - float64| {e:.3g}, moved {step:.3g}")
        assert step > 0
        # float32 against float64 over three steps: a few 2^-24 of |w| <= 1 and of the step, Adam's division
        # included; a missing penalty gradient or decay is of the order of the step itself
        assert e <= 2e-6 + 1e-3 * step, (n, e, step)
    for k, (a, b) in enumerate(zip(got_loss, want_loss)):
        print(f"[{case}] step {k}: loss {a!r} float64 {b!r}")
        assert abs(a - b) <= 4e-6 * abs(b), (k, a, b)
    # the penalty is a visible part of the logged loss, and the unregularized / undecayed twin ends elsewhere
    tde.backend.clear_session()
    twin = _mlp(twin_opt, w0=[w0[n].float().numpy() for n in w0])
    tw, tl = _run_reference(twin, batches)
    assert got_loss[0] - tl[0] > 1e-3 * tl[0]
    assert max(float((tw[n2] - want[n]).abs().max()) for n, n2 in zip(want, tw)) > 1e-5


def test_fit_and_evaluate_report_the_penalty():
    m = _mlp(OP.SGD(0.0), kernel=RG.L2(0.05), bias=RG.L1(0.5))
    m._store.view(m.layers[1].name + "/bias").fill_(0.25)
    m._weights_changed()
    pen = float(sum(m.losses))
    assert pen > 0.25 * 0.5 * 128
    x, y = W.batches(m, 2 * B, 1, 3)[0]
    x, y = x.numpy(), y.numpy()
    h = m.fit(x, y, batch_size=B, epochs=1, verbose=0, shuffle=False, validation_data=(x, y))
    ev = m.evaluate(x, y, batch_size=B, verbose=0, return_dict=True)
    tde.backend.clear_session()
    twin = _mlp(OP.SGD(0.0), w0=m.get_weights())
    tv = twin.evaluate(x, y, batch_size=B, verbose=0, return_dict=True)
    for got in (h.history["loss"][0], h.history["val_loss"][0], ev["loss"]):   # lr = 0: the weights never move
        assert got == pytest.approx(tv["loss"] + pen, rel=2e-6)
    assert ev["accuracy"] == tv["accuracy"] == h.history["val_accuracy"][0]
    assert np.array_equal(m.predict(x[:4]), twin.predict(x[:4]))


def test_the_clipped_norm_includes_the_regularizer_gradient():
    """global_clipnorm: with the penalty's gradient inside the norm the step is c long exactly; clipped before
    it were added, the step would be longer by the penalty's gradient."""
    c = 0.05
    opt = OP.SGD(1.0, global_clipnorm=c)
    m = _mlp(opt, kernel=RG.L2(0.5))
    batches = W.batches(m, B, 1, 8)
    st = m._store
    w0 = st.w.clone()
    want, _, norms = W.trajectory(m, batches, opt)
    assert norms[0] > 10 * c
    got, _ = _run_reference(m, batches)
    assert float((st.w - w0).double().norm()) == pytest.approx(c, rel=1e-5)      # lr 1: |step| = |clipped g| = c
    for n in want:
        assert float((got[n] - want[n]).abs().max()) <= 1e-6
    # the data gradient alone clipped to c and the penalty's gradient put on top would be a much longer step
    seg = st.segments[m.layers[1].name + "/kernel"]
    assert float((2 * 0.5 * w0[seg.offset: seg.offset + seg.numel].double()).norm()) > 10 * c


# ------------------------------------------------------------------------------------ placement and refusals
def test_plans_run_plain_with_the_feature_and_unchanged_without():
    for opt, regs in ((OP.SGD(0.1), dict(kernel=RG.L2(0.1))), (OP.SGD(0.1, weight_decay=0.1), {}),
                      (OP.AdamW(), {}), (OP.Adam(1e-3), dict(bias="l1"))):
        m = _mlp(opt, **regs)
        plan = PG.make_plan(m, m._store, "cpu", B, B, m.optimizer, m.loss)
        assert plan.step_mode == "plain" and not plan._opt_fused()
        assert not plan.supports_step_mode("local") and not plan.supports_step_mode("xgmi")
        tde.backend.clear_session()
    # all-zero coefficients and weight_decay None / 0: the plan reports what it reported before
    for opt in (OP.SGD(0.1), OP.SGD(0.1, weight_decay=None), OP.Adam(1e-3, weight_decay=0)):
        m = _mlp(opt, kernel=RG.L1L2(0.0, 0.0), bias=RG.L2(0.0))
        plan = PG.make_plan(m, m._store, "cpu", B, B, m.optimizer, m.loss)
        assert plan._opt_fused() and plan.reg_segs == [] and m.losses == []
        tde.backend.clear_session()
    m = _mlp(OP.RMSprop(1e-3))
    assert not PG.make_plan(m, m._store, "cpu", B, B, m.optimizer, m.loss)._opt_fused()      # as before: kind 4


def _ps_estimator(monkeypatch, tmp_path, m):
    monkeypatch.setenv("TF_CONFIG", json.dumps({"cluster": {"ps": ["127.0.0.1:1"], "worker": ["127.0.0.1:2"]},
                                                "task": {"type": "worker", "index": 0}}))
    st = tde.distribute.experimental.ParameterServerStrategy()
    assert st.is_distributed
    return tde.estimator.Estimator(m, model_dir=str(tmp_path),
                                   config=tde.estimator.RunConfig(model_dir=str(tmp_path), train_distribute=st))


def _no_input():
    raise AssertionError("the input pipeline must not start")


def test_parameter_server_refuses_both_by_name(monkeypatch, tmp_path):
    from tensorflow_distributed_example_amd.parallel.ps import PSClient
    est = _ps_estimator(monkeypatch, tmp_path, _mlp(OP.Adam(1e-3, weight_decay=0.25)))
    with pytest.raises(ValueError, match="ParameterServerStrategy.*weight_decay=0.25"):
        est.train(_no_input, max_steps=1)
    assert est._psc is None
    tde.backend.clear_session()
    m = _mlp(OP.Adam(1e-3), bias=RG.L1(0.5))
    est = _ps_estimator(monkeypatch, tmp_path, m)
    with pytest.raises(ValueError, match=f"ParameterServerStrategy.*bias_regularizer of {m.layers[1].name}"):
        est.train(_no_input, max_steps=1)
    assert est._psc is None
    c = PSClient.__new__(PSClient)
    c.conns = []
    with pytest.raises(ValueError, match="weight_decay=0.25"):
        c.set_optimizer(3, weight_decay=0.25)
    with pytest.raises(ValueError, match="kernel_regularizer.*not supported under ParameterServerStrategy"):
        c.set_optimizer(3, regularizers={"dense/kernel": (0.0, 0.1)})
    c.set_optimizer(3, weight_decay=None, regularizers={})
    c.set_optimizer(0, weight_decay=0.0)


# ------------------------------------------------------------------------------------ the table builder
SEG_DT = np.dtype([("off", "<i8"), ("rows", "<i4"), ("cols", "<i4"), ("sh", "<i8"), ("sht", "<i8")])


@pytest.mark.skipif(not N.hip_available(), reason="libtde_hip.so not built")
def test_reg_table_holds_the_regularized_segments_only():
    numels = [1, 4096, 4101, 10, 300 * 4096 + 3, 70]
    coefs = [(0.5, 0.0), (0.0, 0.0), (0.0, 0.25), (0.0, 0.0), (0.125, 0.125), (0.0, 0.0)]
    off, rows = 0, []
    for n in numels:
        rows.append((off, 1, n, -1, -1))
        off += (n + 63) // 64 * 64
    arr = np.array(rows, dtype=SEG_DT)
    co = np.array(coefs, dtype=np.float32)
    lib = N.hip()
    want = W.table(numels, coefs)
    assert len(want) == 1 + 2 + 301 and {s for s, _ in want} == {0, 2, 4}
    assert lib.tde_reg_table_size(arr.ctypes.data, co.ctypes.data, len(arr)) == len(want)
    ents = np.full((len(want) + 1, 2), -9, dtype=np.int32)
    assert lib.tde_reg_build_table(arr.ctypes.data, co.ctypes.data, len(arr), ents.ctypes.data) == len(want)
    assert [tuple(e) for e in ents[:-1].tolist()] == want and ents[-1].tolist() == [-9, -9]
    assert lib.tde_reg_table_size(arr.ctypes.data, co.ctypes.data, 0) == 0
    assert lib.tde_reg_table_size(arr.ctypes.data, np.zeros_like(co).ctypes.data, len(arr)) == 0
    # null pointers and bad coefficients: a negative code, nothing written
    assert lib.tde_reg_table_size(None, co.ctypes.data, len(arr)) == -1
    assert lib.tde_reg_table_size(arr.ctypes.data, None, len(arr)) == -1
    assert lib.tde_reg_build_table(arr.ctypes.data, co.ctypes.data, len(arr), None) == -1
    for bad in (-0.5, float("nan"), float("inf")):
        for col in (0, 1):
            cb = co.copy()
            cb[3, col] = bad
            ents[:] = -9
            assert lib.tde_reg_table_size(arr.ctypes.data, cb.ctypes.data, len(arr)) == -3
            assert lib.tde_reg_build_table(arr.ctypes.data, cb.ctypes.data, len(arr), ents.ctypes.data) == -3
            assert (ents == -9).all()
