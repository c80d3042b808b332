"""RMSprop on the CPU: the float64 oracle of tests/optim_rmsprop_oracle.py against hand-computed numbers and
against ``RMSprop.apply_reference``, the exact grid the GPU test relies on, the public interface
(``optimizers.get``, ``compile()``'s default, kinds / slots / hyper-parameters, errors, config), the
parameter-server refusal, both checkpoint layouts and a CPU ``fit()``."""
import json
import math

import numpy as np
import pytest
import torch

import optim_rmsprop_oracle as R

import tensorflow_distributed_example_amd as tde
from tensorflow_distributed_example_amd import optimizers as OP

DEFAULTS = dict(lr=0.001, mom=0.9, b1=0.0, b2=0.9, eps=1e-7)


def _t(x):
    return torch.tensor([x], dtype=torch.float64)


# ------------------------------------------------------------------------------------------ the oracle
def test_oracle_hand_computed_step():
    """w = 1, g = 2, r = 0 (q = 0), Keras defaults, step 1, worked in 40-digit decimal arithmetic on the
    float32-rounded hyper-parameters rho = 0.899999976158142, lr = 0.00100000004749745, eps = 1.00000001168610e-7:
    r1 = 4 (1 - rho) = 0.400000095367431640625 (exact).
    kind 4: sqrt(r1) + eps = 0.632455707428247, step = 2 lr / that = 0.00316227693339585, w1 = 0.996837723066604
    kind 5: sqrt(r1 + eps) = 0.632455686485174, q1 = 2 lr / that = 0.00316227703811117, w1 = 0.996837722961889"""
    rho, lr, eps = R.f32(0.9), R.f32(0.001), R.f32(1e-7)
    r1 = (1.0 - rho) * 4.0
    assert r1 == 0.400000095367431640625
    w, r, q = R.oracle_step("rmsprop", DEFAULTS, _t(1.0), _t(2.0), _t(0.0), None)
    assert q is None and r.item() == r1
    step4 = lr * 2.0 / (math.sqrt(r1) + eps)
    assert abs(step4 - 0.00316227693339585) < 1e-16
    assert abs(w.item() - (1.0 - step4)) < 1e-16 and abs(w.item() - 0.996837723066604) < 1e-15
    w, r, q = R.oracle_step("rmsprop_momentum", DEFAULTS, _t(1.0), _t(2.0), _t(0.0), _t(0.0))
    q1 = lr * 2.0 / math.sqrt(r1 + eps)
    assert abs(q1 - 0.00316227703811117) < 1e-16 and q1 > step4 * (1 + 1e-8)     # epsilon inside the root: a larger step
    assert r.item() == r1 and abs(q.item() - q1) < 1e-16 and abs(w.item() - 0.996837722961889) < 1e-15
    # a second step of kind 5 carries the momentum: q2 = mom q1 + lr g / sqrt(r2 + eps)
    w2, r2, q2 = R.oracle_step("rmsprop_momentum", DEFAULTS, w, _t(2.0), r, q)
    r2_want = rho * r1 + (1.0 - rho) * 4.0
    assert abs(r2.item() - r2_want) < 1e-15
    assert abs(q2.item() - (R.f32(0.9) * q1 + lr * 2.0 / math.sqrt(r2_want + eps))) < 1e-16
    assert abs(w2.item() - (w.item() - q2.item())) < 1e-16


@pytest.mark.parametrize("kind", R.KINDS)
def test_apply_reference_matches_oracle(kind):
    """``RMSprop.apply_reference`` in float64 over three steps follows the oracle (hyper-parameters chosen as
    floats, so both sides see the same numbers)."""
    hyper = dict(lr=0.125, mom=0.5 if kind == "rmsprop_momentum" else 0.0, b1=0.0, b2=0.75, eps=2.0 ** -20)
    opt = OP.RMSprop(hyper["lr"], rho=hyper["b2"], momentum=hyper["mom"], epsilon=hyper["eps"])
    assert opt.kind == kind
    gen = torch.Generator().manual_seed(5)
    n = 257
    w = torch.randn(n, generator=gen, dtype=torch.float64)
    ow, orr, oq = w.clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    slots = {s: torch.zeros(n, dtype=torch.float64) for s in opt.slot_names()}
    for step in range(3):
        g = torch.randn(n, generator=gen, dtype=torch.float64)
        opt.apply_reference(w, g, slots, step)
        ow, orr, oq = R.oracle_step(kind, hyper, ow, g, orr, oq)
        assert float((w - ow).abs().max()) < 1e-14
        assert float((slots["rms"] - orr).abs().max()) < 1e-14
        if kind == "rmsprop_momentum":
            assert float((slots["momentum"] - oq).abs().max()) < 1e-14


@pytest.mark.parametrize("grad_scale,bits,lim", [(1.0, 15, 16.0), (0.25, 19, 4.0)])
def test_exact_grid_keeps_rms_representable(grad_scale, bits, lim):
    """rho = 2^-1, r0 = |grid_slot|, g on the 2^-6 grid: every r of three steps is a multiple of 2^-bits below
    lim (19 resp. 21 bits), so fp32 holds it exactly and the kernel has to reproduce it bit for bit."""
    idx = torch.arange(70000)
    w, r, q = R.grid_w(idx), R.grid_r(idx), R.grid_q(idx)
    assert float(r.min()) >= 0.0 and float(r.max()) < 4.0
    for step in range(3):
        g = R.grid_g(idx, step)
        w, r, q = R.oracle_step("rmsprop_momentum", R.GRID_HYPER, w, g, r, q, grad_scale)
        scaled = r * 2.0 ** bits
        assert torch.equal(scaled, scaled.round()) and float(r.max()) < lim and float(r.min()) >= 0.0
        assert torch.equal(r.float().double(), r)
        # and the fp32 host sample of r is that same value
        hr = R.fp32_step("rmsprop", R.GRID_HYPER, w.float(), g.float(), r.float(), None, grad_scale)[1]
        assert hr.dtype == torch.float32


def test_fp32_step_is_close_to_oracle():
    gen = torch.Generator().manual_seed(9)
    n = 4096
    w, g = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    r, q = torch.rand(n, generator=gen), 0.01 * torch.randn(n, generator=gen)
    for kind in R.KINDS:
        hw, hr, hq = R.fp32_step(kind, DEFAULTS, w, g, r, q)
        ow, orr, oq = R.oracle_step(kind, DEFAULTS, w.double(), g.double(), r.double(), q.double())
        assert float((hw.double() - ow).abs().max()) < 2.0 ** -21 * float(ow.abs().max())
        assert float((hr.double() - orr).abs().max()) < 2.0 ** -22 * float(orr.abs().max())


# ------------------------------------------------------------------------------------ public interface
def _mlp(opt=None, **kw):
    tde.backend.set_random_seed(11)
    m = tde.zoo.mnist_mlp()
    if opt is None:
        m.compile(loss=tde.losses.SparseCategoricalCrossentropy(from_logits=True), metrics=["accuracy"], **kw)
    else:
        m.compile(loss=tde.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=opt,
                  metrics=["accuracy"], **kw)
    m.build()
    return m


def test_get_and_compile_default_give_rmsprop():
    for o in (OP.get("rmsprop"), OP.get("RMSprop"), _mlp().optimizer, _mlp("rmsprop").optimizer):
        assert type(o) is OP.RMSprop and o.learning_rate == 0.001 and o.kind == "rmsprop"
    o = OP.RMSprop(lr=0.02)
    assert o.learning_rate == 0.02 and o.lr == 0.02
    assert OP.get(o) is o


def test_kinds_slots_hparams():
    a = OP.RMSprop()
    assert (a.kind, a.kind_id, a.slot_names()) == ("rmsprop", 4, ["rms"])
    assert a.hparams() == dict(mom=0.0, b1=0.0, b2=0.9, eps=1e-7)
    b = OP.RMSprop(0.01, rho=0.8, momentum=0.5, epsilon=1e-5)
    assert (b.kind, b.kind_id, b.slot_names()) == ("rmsprop_momentum", 5, ["rms", "momentum"])
    assert b.hparams() == dict(mom=0.5, b1=0.0, b2=0.8, eps=1e-5)
    assert OP.KIND["rmsprop"] == 4 and OP.KIND["rmsprop_momentum"] == 5


def test_errors():
    with pytest.raises(ValueError, match="slot"):
        OP.RMSprop(centered=True)
    for rho in (1.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="rho"):
            OP.RMSprop(rho=rho)
    with pytest.raises(ValueError, match="momentum"):
        OP.RMSprop(momentum=-0.1)
    assert OP.RMSprop(rho=0.0).rho == 0.0


def test_get_config_round_trips():
    a = OP.RMSprop(0.02, rho=0.8, momentum=0.3, epsilon=1e-6, name="rp")
    cfg = a.get_config()
    assert cfg == dict(name="rp", learning_rate=0.02, rho=0.8, momentum=0.3, epsilon=1e-6, centered=False)
    b = OP.RMSprop(**cfg)
    assert b.get_config() == cfg and b.kind == a.kind and b.hparams() == a.hparams()


def test_parameter_server_refuses_rmsprop(monkeypatch, tmp_path):
    """The ps tasks apply kinds 0..3 themselves: RMSprop is refused by name before anything connects (the
    cluster's addresses are never opened: nothing listens on them)."""
    monkeypatch.setenv("TF_CONFIG", json.dumps({"cluster": {"ps": ["127.0.0.1:1"], "worker": ["127.0.0.1:2"]},
                                                "task": {"type": "worker", "index": 0}}))
    st = tde.distribute.experimental.ParameterServerStrategy()
    assert st.is_distributed
    m = _mlp(OP.RMSprop())
    est = tde.estimator.Estimator(m, model_dir=str(tmp_path),
                                  config=tde.estimator.RunConfig(model_dir=str(tmp_path), train_distribute=st))

    def input_fn():
        raise AssertionError("the input pipeline must not start")
    with pytest.raises(ValueError, match="RMSprop"):
        est.train(input_fn, max_steps=1)
    assert est._psc is None
    from tensorflow_distributed_example_amd.parallel.ps import PSClient
    c = PSClient.__new__(PSClient)
    c.conns = []
    for kind in (4, 5):
        with pytest.raises(ValueError, match="RMSprop"):
            c.set_optimizer(kind)


def test_cpu_plans_run_plain_and_nothing_fuses_rmsprop():
    """No fused placement takes RMSprop on the CPU; the reference plan applies it (``apply_reference``)."""
    from tensorflow_distributed_example_amd.train import program as PG
    m = _mlp(OP.RMSprop())
    plan = PG.make_plan(m, m._store, "cpu", 8, 8, m.optimizer, m.loss)
    assert plan.step_mode == "plain" and not plan.supports_step_mode("local") and not plan.supports_step_mode("xgmi")
    assert not plan._opt_fused()
    assert PG.make_plan(m, m._store, "cpu", 8, 8, OP.Adam(), m.loss)._opt_fused()


# ----------------------------------------------------------------------------------------- persistence
def _fill_state(m, step):
    st = m._store
    n = st.w.numel()
    for k, name in enumerate(m.optimizer.slot_names()):
        st.slot(name).copy_((torch.arange(n, dtype=torch.float32) % 977) * 2.0 ** -9 + k)
    m._set_iterations(step)
    return {name: st.slot(name).clone() for name in m.optimizer.slot_names()}


def _seg_equal(m, slot, want):
    st = m._store
    mask = R.seg_mask(st)
    return torch.equal(st.slot(slot)[mask], want[mask])


@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_keras_save_weights_round_trips_slots(momentum, tmp_path):
    m = _mlp(OP.RMSprop(momentum=momentum))
    want = _fill_state(m, 17)
    assert sorted(want) == sorted(["rms", "momentum"] if momentum else ["rms"])
    prefix = str(tmp_path / "w" / "ckpt")
    m.save_weights(prefix)
    from tensorflow_distributed_example_amd.io import tensor_bundle as TB
    keys = TB.read_bundle(prefix)
    for s in want:
        assert any(k.endswith(f"/.OPTIMIZER_SLOT/optimizer/{s}/.ATTRIBUTES/VARIABLE_VALUE") for k in keys), s
    m2 = _mlp(OP.RMSprop(momentum=momentum))
    m2._store.w.add_(1.0)
    m2.load_weights(prefix)
    assert m2.optimizer.iterations == 17
    assert torch.equal(m2._store.w[R.seg_mask(m2._store)], m._store.w[R.seg_mask(m._store)])
    for s in want:
        assert _seg_equal(m2, s, want[s]), s


def test_estimator_checkpoint_round_trips_slots(tmp_path):
    tde.backend.clear_session()     # Estimator checkpoints go by TF1 variable names: name both models as a
    m = _mlp(OP.RMSprop(momentum=0.9))     # fresh process would
    want = _fill_state(m, 0)
    est = tde.estimator.Estimator(m, model_dir=str(tmp_path))
    est.manager.save(m, 23)
    from tensorflow_distributed_example_amd.io import tensor_bundle as TB
    vals = TB.read_bundle(est.latest_checkpoint())
    assert int(vals["global_step"]) == 23
    assert sum("/.OPTIMIZER_SLOT/rms" in k for k in vals) == 4 and sum("/.OPTIMIZER_SLOT/momentum" in k for k in vals) == 4
    tde.backend.clear_session()
    m2 = _mlp(OP.RMSprop(momentum=0.9))
    est2 = tde.estimator.Estimator(m2, model_dir=str(tmp_path))
    assert est2._start_step() == 23
    for s in ("rms", "momentum"):
        assert _seg_equal(m2, s, want[s]), s
    # and the resumed run counts on from there
    x, y = R.row_band_task(64)

    def input_fn():
        return tde.data.Dataset.from_tensor_slices((x, y.reshape(-1, 1))).repeat().batch(32)
    est2.train(input_fn, max_steps=25)
    assert m2.optimizer.iterations == 25
    assert not _seg_equal(m2, "rms", want["rms"])


# ------------------------------------------------------------------------------------------------- fit
def test_cpu_fit_mnist_mlp_rmsprop_learns():
    """zoo.mnist_mlp with RMSprop() (the reference plan, ``apply_reference``) on the row-band task, batch 128,
    FIT_EPOCHS = 3 epochs: last-epoch loss < half of the first.  The epoch count was chosen here, on the
    reference plan, for a ratio below 0.25; it reached 0.0126 (losses 0.4405, 0.0202, 0.0055)."""
    with tde.distribute.OneDeviceStrategy("cpu").scope():     # the CPU also where a GPU is present
        m = _mlp(OP.RMSprop())
    x, y = R.row_band_task()
    h = m.fit(x, y, batch_size=R.FIT_BATCH, epochs=R.FIT_EPOCHS, verbose=0)
    prog = m._program("train", R.FIT_BATCH)
    assert prog.plan_kind == "reference" and prog.plans[0].step_mode == "plain"
    ratio = h.history["loss"][-1] / h.history["loss"][0]
    print(f"[rmsprop cpu fit] losses {h.history['loss']} ratio {ratio:.4f}")
    assert ratio < 0.5
    assert m.optimizer.iterations == R.FIT_EPOCHS * (2048 // R.FIT_BATCH)
