"""Learning-rate schedules on the CPU: the five schedules of ``optimizers.schedules`` against hand-computed
values and the float64 oracle of tests/lr_schedule_oracle.py, their configuration round trip and refusals, the
optimizers' side of it (``lr_at``, ``current_lr``, ``key``, ``get_config``), the reference plan under
``fit`` -- alone and under two Mirrored CPU replicas -- against two constant-rate runs chained by hand, the
parameter-server refusals, the ``LearningRateScheduler`` callback and the size of the ``LrSched`` descriptor.
"""
import ctypes
import json
import math

import numpy as np
import pytest

import lr_schedule_oracle as S
import tensorflow_distributed_example_amd as tde
from tensorflow_distributed_example_amd import _native as N
from tensorflow_distributed_example_amd import optimizers as OP

SCH = OP.schedules


# ------------------------------------------------------------------------------------ hand-computed values
def _close(a, b):
    return a == pytest.approx(b, rel=1e-14, abs=0.0)


def test_exponential_decay_by_hand():
    s = SCH.ExponentialDecay(0.1, 16, 0.5)
    assert s(0) == 0.1 and _close(s(16), 0.05) and _close(s(32), 0.025)
    assert _close(s(1), 0.1 * 0.5 ** 0.0625) and _close(s(15), 0.1 * 0.5 ** 0.9375)
    assert _close(s(17), 0.1 * 0.5 ** 1.0625) and _close(s(1600), 0.1 * 2.0 ** -100)
    st = SCH.ExponentialDecay(0.1, 16, 0.5, staircase=True)
    assert [st(k) for k in (0, 1, 15)] == [0.1] * 3 and _close(st(16), 0.05) and _close(st(17), 0.05)
    assert _close(st(31), 0.05) and _close(st(32), 0.025) and _close(st(1600), 0.1 * 2.0 ** -100)


def test_inverse_time_decay_by_hand():
    s = SCH.InverseTimeDecay(0.1, 10, 0.5)
    assert s(0) == 0.1 and _close(s(1), 0.1 / 1.05) and _close(s(9), 0.1 / 1.45) and _close(s(10), 0.1 / 1.5)
    assert _close(s(11), 0.1 / 1.55) and _close(s(10 ** 6), 0.1 / 50001.0)
    st = SCH.InverseTimeDecay(0.1, 10, 0.5, staircase=True)
    assert [st(k) for k in (0, 1, 9)] == [0.1] * 3 and _close(st(10), 0.1 / 1.5) and _close(st(11), 0.1 / 1.5)
    assert _close(st(19), 0.1 / 1.5) and _close(st(20), 0.05) and _close(st(10 ** 6 + 9), 0.1 / 50001.0)


def test_polynomial_decay_by_hand():
    s = SCH.PolynomialDecay(0.5, 50, end_learning_rate=0.125)          # power 1: a straight line, then flat
    assert s(0) == 0.5 and _close(s(1), 0.375 * 0.98 + 0.125) and _close(s(49), 0.375 * 0.02 + 0.125)
    assert s(50) == 0.125 and s(51) == 0.125 and s(10 ** 9) == 0.125
    assert SCH.PolynomialDecay(0.1, 10).end_learning_rate == 1e-4 and SCH.PolynomialDecay(0.1, 10).power == 1.0
    q = SCH.PolynomialDecay(0.5, 4, end_learning_rate=0.25, power=2.0)
    assert _close(q(1), 0.25 * 0.5625 + 0.25) and _close(q(3), 0.25 * 0.0625 + 0.25) and q(4) == 0.25
    c = SCH.PolynomialDecay(0.5, 4, end_learning_rate=0.25, power=2.0, cycle=True)
    assert c(0) == 0.5 and _close(c(1), q(1)) and _close(c(3), q(3)) and c(4) == 0.25   # the first cycle: D = 4
    assert _close(c(5), 0.25 * (1 - 5 / 8) ** 2 + 0.25) and c(8) == 0.25                # the second: D = 8
    assert _close(c(9), 0.25 * (1 - 9 / 12) ** 2 + 0.25)                               # the third: D = 12
    assert _close(c(4001), 0.25 * (1 - 4001 / 4004) ** 2 + 0.25)


def test_cosine_decay_by_hand():
    s = SCH.CosineDecay(0.5, 16)
    assert s(0) == 0.5 and abs(s(8) - 0.25) < 1e-16
    assert _close(s(1), 0.25 * (1 + math.cos(math.pi / 16))) and _close(s(15), 0.25 * (1 + math.cos(15 * math.pi / 16)))
    assert s(16) == 0.0 and s(17) == 0.0 and s(10 ** 9) == 0.0
    a = SCH.CosineDecay(0.5, 16, alpha=0.25)
    assert a(0) == 0.5 and a(16) == 0.125 and a(17) == 0.125 and a(10 ** 9) == 0.125
    assert _close(a(4), 0.5 * (0.75 * 0.5 * (1 + math.cos(math.pi / 4)) + 0.25))


def test_piecewise_constant_decay_by_hand():
    s = SCH.PiecewiseConstantDecay([3, 10, 11], [0.1, 0.03, 0.007, 1e-4])
    want = {0: 0.1, 2: 0.1, 3: 0.1, 4: 0.03, 9: 0.03, 10: 0.03, 11: 0.007, 12: 1e-4, 10 ** 12: 1e-4, -5: 0.1}
    assert {k: s(k) for k in want} == want
    big = SCH.PiecewiseConstantDecay([7, S.BIG + 6], [0.1, 0.02, 0.003])
    assert big(S.BIG + 6) == 0.02 and big(S.BIG + 7) == 0.003 and big(2 ** 32 + 7) == 0.02 and big(7) == 0.1
    assert SCH.PiecewiseConstantDecay([], [0.3])(99) == 0.3


def test_host_schedules_equal_the_oracle_on_the_whole_table():
    """``__call__`` (float64, a Python float) against lr_schedule_oracle.eval64 written from the formulas; and
    the conditions the GPU test's bound rests on: amplification <= 4, exact rows exact in float32 arithmetic."""
    worst = 0.0
    for ci, name, kw, it, bias, exact in S.rows():
        step = it + bias
        got, want = S.make(tde, name, kw)(step), S.eval64(name, kw, step)
        assert isinstance(got, float)
        assert got == pytest.approx(want, rel=1e-13, abs=1e-18), (ci, name, step)
        worst = max(worst, S.amplification(name, kw, step))
        assert S.amplification(name, kw, step) <= 4.0, (ci, name, step)
        if exact:
            assert S.eval32(name, kw, step) == S.F(want), (ci, name, step)
    print(f"largest amplification in the table {worst:.3g}")
    assert {name for name, *_ in S.TABLE} == set(S.KINDS)


# ------------------------------------------------------------------------------------ configuration
@pytest.mark.parametrize("ci", range(len(S.TABLE)))
def test_config_round_trip(ci):
    name, kw, steps, _ = S.TABLE[ci]
    a = S.make(tde, name, kw)
    cfg = a.get_config()
    json.dumps(cfg)
    b = type(a).from_config(cfg)
    assert type(b) is type(a) and b.get_config() == cfg and b.key() == a.key()
    assert [b(s) for s in steps] == [a(s) for s in steps]
    assert isinstance(a, SCH.LearningRateSchedule)
    d = SCH.deserialize(SCH.serialize(a))
    assert type(d) is type(a) and d.get_config() == cfg


def test_keras_names_and_defaults():
    assert tde.keras.optimizers.schedules is SCH and tde.optimizers.schedules is SCH
    assert SCH.ExponentialDecay(0.1, 5, 0.9).staircase is False and SCH.InverseTimeDecay(0.1, 5, 0.9).staircase is False
    p = SCH.PolynomialDecay(0.1, 5)
    assert (p.end_learning_rate, p.power, p.cycle) == (1e-4, 1.0, False)
    assert SCH.CosineDecay(0.1, 5).alpha == 0.0
    with pytest.raises(NotImplementedError):
        SCH.LearningRateSchedule()(0)


def test_piecewise_refusals_name_the_cause():
    with pytest.raises(ValueError, match="at most 8 boundaries"):
        SCH.PiecewiseConstantDecay(list(range(1, 10)), [0.1] * 10)
    SCH.PiecewiseConstantDecay(list(range(1, 9)), [0.1] * 9)          # 8 is taken
    with pytest.raises(ValueError, match=r"len\(values\) must be len\(boundaries\) \+ 1"):
        SCH.PiecewiseConstantDecay([1, 2], [0.1, 0.2])
    with pytest.raises(ValueError, match=r"len\(values\)"):
        SCH.PiecewiseConstantDecay([1], [0.1, 0.2, 0.3])
    with pytest.raises(ValueError, match="decay_steps"):
        SCH.ExponentialDecay(0.1, 0, 0.5)


# ------------------------------------------------------------------------------------ optimizers
def _optimizers(lr):
    return [OP.SGD(lr), OP.SGD(lr, momentum=0.9), OP.SGD(lr, momentum=0.9, nesterov=True), OP.Adam(lr), OP.RMSprop(lr),
            OP.RMSprop(lr, momentum=0.5), OP.GradientDescentOptimizer(lr)]


def test_every_optimizer_takes_a_schedule():
    sch = SCH.ExponentialDecay(0.1, 4, 0.5)
    for o in _optimizers(sch):
        assert o.learning_rate is sch and o.lr is sch and o.schedule is sch
        assert o.lr_at(0) == 0.1 and o.lr_at(4) == pytest.approx(0.05) and o.lr_at(6) == sch(6)
        assert o.current_lr() == 0.1
        k0 = o.key()
        o.iterations = 8
        assert o.current_lr() == sch(8) == pytest.approx(0.025)
        assert o.key() == k0 and hash(k0) is not None                   # constant over the run: no re-capture
        cfg = o.get_config()
        assert cfg["learning_rate"] == {"class_name": "ExponentialDecay", "config": sch.get_config()}
        json.dumps(cfg)
        if not isinstance(o, OP.GradientDescentOptimizer):
            back = type(o)(**cfg)
            assert back.key() == k0 and back.lr_at(5) == o.lr_at(5)
    assert OP.SGD(sch).key() != OP.SGD(SCH.ExponentialDecay(0.1, 4, 0.25)).key()
    assert OP.SGD(sch).key() != OP.SGD(0.1).key()


def test_constant_rates_behave_as_before():
    for o in _optimizers(0.125):
        assert o.learning_rate == 0.125 and isinstance(o.learning_rate, float) and o.lr == 0.125
        assert o.schedule is None and o.lr_at(0) == o.lr_at(10 ** 6) == o.current_lr() == 0.125
        assert o.key()[1] == 0.125 and o.get_config()["learning_rate"] == 0.125
        o.learning_rate = 0.25
        assert o.key()[1] == 0.25 and o.lr_at(3) == 0.25
    assert OP.SGD(lr=0.5).learning_rate == 0.5


def test_apply_reference_uses_the_rate_of_its_step():
    import torch
    sch = SCH.PiecewiseConstantDecay([1], [0.125, 0.25])
    for mk in (lambda lr: OP.SGD(lr), lambda lr: OP.SGD(lr, momentum=0.5, nesterov=True), lambda lr: OP.Adam(lr),
               lambda lr: OP.RMSprop(lr, momentum=0.5), lambda lr: OP.RMSprop(lr)):
        a = mk(sch)
        g = torch.linspace(-1, 1, 7)
        for step in (0, 1, 2, 5):
            b = mk(sch(step))
            wa, wb = torch.ones(7), torch.ones(7)
            sa = {n: torch.full((7,), 0.5) for n in a.slot_names()}
            sb = {n: torch.full((7,), 0.5) for n in b.slot_names()}
            a.apply_reference(wa, g, sa, step)
            b.apply_reference(wb, g, sb, step)
            assert torch.equal(wa, wb) and all(torch.equal(sa[n], sb[n]) for n in sa), (a.name, step)


# ------------------------------------------------------------------------------------ fit on the reference plan
GB, NSTEP, BOUNDARY = 32, 5, 2      # steps 0..2 at the first rate, steps 3..4 at the second
RATES = [0.05, 0.0125]


def _task():
    rng = np.random.default_rng(5)
    return rng.random((GB * NSTEP, 28, 28, 1), dtype=np.float32), rng.integers(0, 10, size=GB * NSTEP)


def _mlp(strategy, opt, w0=None):
    with strategy.scope():
        m = tde.zoo.mnist_mlp()
        m.compile(loss=tde.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=opt, metrics=["accuracy"])
    m.build()
    if w0 is not None:
        m.set_weights(w0)
    return m


def _fit(m, x, y):
    return m.fit(tde.data.Dataset.from_tensor_slices((x, y)).batch(GB), epochs=1, verbose=0)


def _scheduled_equals_chained(make_strategy):
    x, y = _task()
    sch = SCH.PiecewiseConstantDecay([BOUNDARY], RATES)
    a = _mlp(make_strategy(), OP.SGD(sch))
    w0 = a.get_weights()
    _fit(a, x, y)
    assert a.optimizer.iterations == NSTEP and a.optimizer.current_lr() == RATES[1]
    tde.backend.clear_session()
    b = _mlp(make_strategy(), OP.SGD(RATES[0]), w0)
    k = (BOUNDARY + 1) * GB
    _fit(b, x[:k], y[:k])
    assert b.optimizer.iterations == BOUNDARY + 1
    b.optimizer.learning_rate = RATES[1]
    _fit(b, x[k:], y[k:])
    assert b.optimizer.iterations == NSTEP
    for wa, wb, w in zip(a.get_weights(), b.get_weights(), w0):
        assert np.array_equal(wa, wb)
        assert not np.array_equal(wa, w)
    tde.backend.clear_session()
    c = _mlp(make_strategy(), OP.SGD(RATES[0]), w0)          # and the second rate did matter
    _fit(c, x, y)
    assert any(not np.array_equal(wa, wc) for wa, wc in zip(a.get_weights(), c.get_weights()))
    return a


def test_reference_fit_equals_two_constant_runs_chained_at_the_boundary():
    a = _scheduled_equals_chained(lambda: tde.distribute.OneDeviceStrategy("cpu"))
    assert a._program("train", GB).plans[0].kind == "reference"


def test_mirrored_cpu_replicas_equal_two_constant_runs_chained_at_the_boundary():
    a = _scheduled_equals_chained(lambda: tde.distribute.MirroredStrategy(devices=["/cpu:0", "/cpu:0"]))
    prog = a._program("train", GB)
    assert len(prog.plans) == 2 and all(p.kind == "reference" for p in prog.plans)
    st = prog.stores
    assert np.array_equal(st[0].w.numpy(), st[1].w.numpy())


def test_cpu_plan_runs_plain_under_a_schedule():
    from tensorflow_distributed_example_amd.train import program as PG
    m = _mlp(tde.distribute.OneDeviceStrategy("cpu"), OP.SGD(SCH.CosineDecay(0.1, 10)))
    plan = PG.make_plan(m, m._store, "cpu", 8, 8, m.optimizer, m.loss)
    assert plan.step_mode == "plain" and not plan._opt_fused()
    assert not plan.supports_step_mode("local") and not plan.supports_step_mode("xgmi")
    assert PG.make_plan(m, m._store, "cpu", 8, 8, OP.SGD(0.1), m.loss)._opt_fused()


# ------------------------------------------------------------------------------------ refusals
def test_parameter_server_refuses_a_schedule(monkeypatch, tmp_path):
    monkeypatch.setenv("TF_CONFIG", json.dumps({"cluster": {"ps": ["127.0.0.1:1"], "worker": ["127.0.0.1:2"]},
                                                "task": {"type": "worker", "index": 0}}))
    st = tde.distribute.experimental.ParameterServerStrategy()
    assert st.is_distributed
    tde.backend.set_random_seed(11)
    m = tde.zoo.mnist_mlp()
    m.compile(loss=tde.losses.SparseCategoricalCrossentropy(from_logits=True),
              optimizer=OP.SGD(SCH.ExponentialDecay(0.1, 10, 0.5)), metrics=["accuracy"])
    m.build()
    est = tde.estimator.Estimator(m, model_dir=str(tmp_path),
                                  config=tde.estimator.RunConfig(model_dir=str(tmp_path), train_distribute=st))

    def input_fn():
        raise AssertionError("the input pipeline must not start")
    with pytest.raises(ValueError, match="schedule.*ExponentialDecay"):
        est.train(input_fn, max_steps=1)
    assert est._psc is None
    from tensorflow_distributed_example_amd.parallel.ps import PSClient
    c = PSClient.__new__(PSClient)
    c.conns = []
    with pytest.raises(ValueError, match="schedule"):
        c.set_optimizer(0, learning_rate=SCH.CosineDecay(0.1, 10))
    c.set_optimizer(0, learning_rate=0.1)
    c.set_optimizer(3)


# ------------------------------------------------------------------------------------ callback
def test_learning_rate_scheduler_sets_the_rate_per_epoch_and_logs_it():
    x, y = _task()
    m = _mlp(tde.distribute.OneDeviceStrategy("cpu"), OP.SGD(0.1))
    seen = []

    def fn(epoch, lr):
        seen.append((epoch, lr))
        return lr * 0.5
    cb = tde.keras.callbacks.LearningRateScheduler(fn, verbose=0)
    logged = []
    probe = tde.keras.callbacks.LambdaCallback(on_epoch_end=lambda e, logs: logged.append(dict(logs)))
    h = _fit_epochs(m, x, y, [cb, probe], 3)
    assert seen == [(0, 0.1), (1, 0.05), (2, 0.025)]
    assert m.optimizer.learning_rate == 0.0125
    assert h.history["lr"] == [0.05, 0.025, 0.0125] and len(h.history["loss"]) == 3
    assert [l["lr"] for l in logged] == [0.05, 0.025, 0.0125]
    one = tde.keras.callbacks.LearningRateScheduler(lambda epoch: 0.01 * (epoch + 1))     # schedule(epoch)
    h = _fit_epochs(m, x, y, [one], 2)
    assert h.history["lr"] == [0.01, 0.02]
    m2 = _mlp(tde.distribute.OneDeviceStrategy("cpu"), OP.SGD(SCH.CosineDecay(0.1, 10)))
    with pytest.raises(ValueError, match="CosineDecay"):
        _fit_epochs(m2, x, y, [cb], 1)


def _fit_epochs(m, x, y, cbs, epochs):
    return m.fit(tde.data.Dataset.from_tensor_slices((x, y)).batch(GB), epochs=epochs, verbose=0, callbacks=cbs)


# ------------------------------------------------------------------------------------ ABI
def test_descriptor_struct():
    from tensorflow_distributed_example_amd.ops import kernels as K
    assert ctypes.sizeof(K.LrSched) == 144
    assert [f[0] for f in K.LrSched._fields_] == ["kind", "flags", "lr0", "p", "decay_steps", "nb", "bound", "val"]
    assert (K.LrSched.decay_steps.offset, K.LrSched.bound.offset, K.LrSched.val.offset) == (24, 40, 104)
    d = K.lr_sched(SCH.PiecewiseConstantDecay([7, S.BIG + 6], [0.5, 0.25, 0.125]))
    assert (d.kind, d.nb, list(d.bound)[:2], list(d.val)[:3]) == (5, 2, [7, S.BIG + 6], [0.5, 0.25, 0.125])
    d = K.lr_sched(SCH.PolynomialDecay(0.5, 9, 0.25, power=2.0, cycle=True))
    assert (d.kind, d.flags, d.lr0, list(d.p)[:2], d.decay_steps) == (3, 2, 0.5, [0.25, 2.0], 9)
    d = K.lr_sched(SCH.ExponentialDecay(0.5, 9, 0.25, staircase=True))
    assert (d.kind, d.flags, d.lr0, d.p[0], d.decay_steps) == (1, 1, 0.5, 0.25, 9)
    assert K.lr_sched(SCH.InverseTimeDecay(0.5, 9, 0.25)).kind == 2 and K.lr_sched(SCH.CosineDecay(0.5, 9)).kind == 4


@pytest.mark.skipif(not N.hip_available(), reason="libtde_hip.so not built")
def test_descriptor_size_matches_the_kernels():
    from tensorflow_distributed_example_amd.ops import kernels as K
    out = (ctypes.c_longlong * 1)()
    assert N.hip().tde_sched_abi_sizes(out, 1) == 1
    assert out[0] == ctypes.sizeof(K.LrSched)
