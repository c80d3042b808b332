"""Gradient clipping on the CPU: the constructor rules of ``clipvalue`` / ``clipnorm`` / ``global_clipnorm``,
``key()`` and the configuration round trip, a hand-computed two-variable example of each mode through the
reference plan, ``fit`` on the reference plan where the clip bites (against the float64 oracle of
tests/grad_clip_oracle.py applied to the plan's own gradients) and where it does not (bitwise the unclipped
run), two Mirrored CPU replicas against one replica at the same global batch (the clip follows the
aggregation), the parameter-server refusals and the sum-of-squares table builder of csrc/kernels/gradclip.hip.
"""
import json
import types

import numpy as np
import pytest
import torch

import grad_clip_oracle as G
import optim_oracle as OO
import tensorflow_distributed_example_amd as tde
from tensorflow_distributed_example_amd import _native as N
from tensorflow_distributed_example_amd import optimizers as OP
from tensorflow_distributed_example_amd.train import program as PG


def _optimizers(**kw):
    return [OP.SGD(0.1, **kw), OP.SGD(0.1, momentum=0.5, nesterov=True, **kw), OP.Adam(1e-3, **kw),
            OP.RMSprop(1e-3, **kw), OP.RMSprop(1e-3, momentum=0.9, **kw)]


# ------------------------------------------------------------------------------------ constructor rules
@pytest.mark.parametrize("mode", G.MODES)
def test_every_optimizer_takes_each_kind(mode):
    for o in _optimizers(**{mode: 2}):
        assert o.clip == (mode, 2.0) and isinstance(o.clip[1], float)
        assert [getattr(o, m) for m in G.MODES] == [2.0 if m == mode else None for m in G.MODES]
        with pytest.raises(AttributeError):
            setattr(o, mode, 3.0)                       # constructor-only
        with pytest.raises(AttributeError):
            o.clip = None
    for o in _optimizers():
        assert o.clip is None and o.clipnorm is None and o.clipvalue is None and o.global_clipnorm is None


def test_more_than_one_kind_is_refused_by_name():
    for kw in (dict(clipnorm=1.0, clipvalue=1.0), dict(clipnorm=1.0, global_clipnorm=1.0),
               dict(clipvalue=1.0, global_clipnorm=1.0), dict(clipnorm=1.0, clipvalue=1.0, global_clipnorm=1.0)):
        for cls in (OP.SGD, OP.Adam, OP.RMSprop):
            with pytest.raises(ValueError, match="clipnorm.*clipvalue.*global_clipnorm"):
                cls(**kw)


@pytest.mark.parametrize("c", [0.0, -1.0, float("inf"), float("-inf"), float("nan"), "x"])
def test_c_must_be_positive_and_finite(c):
    for mode in G.MODES:
        for cls in (OP.SGD, OP.Adam, OP.RMSprop):
            with pytest.raises(ValueError, match=mode):
                cls(**{mode: c})


def test_unknown_keyword_arguments_raise():
    for cls in (OP.SGD, OP.Adam, OP.RMSprop):
        with pytest.raises(TypeError, match="clip_norm"):
            cls(1e-3, clip_norm=1.0)
        with pytest.raises(TypeError, match="decay"):
            cls(decay=1e-4)
        assert cls(lr=0.5).learning_rate == 0.5 and cls(lr=0.5, clipnorm=1.0).clip == ("clipnorm", 1.0)
    with pytest.raises(ValueError, match="centered"):
        OP.RMSprop(centered=True, clipnorm=1.0)


def test_the_tf1_optimizer_takes_none_of_them():
    for mode in G.MODES:
        with pytest.raises(TypeError, match=mode):
            OP.GradientDescentOptimizer(0.1, **{mode: 1.0})
    assert OP.GradientDescentOptimizer(0.1).clip is None


def test_key_and_config_round_trip():
    for mode in G.MODES:
        for o in _optimizers(**{mode: 0.75}):
            twin = [x for x in _optimizers() if type(x) is type(o) and x.kind == o.kind][0]
            assert o.key() != twin.key() and hash(o.key()) is not None
            assert o.key() != type(o)(**{**o.get_config(), mode: 0.5}).key()
            cfg = o.get_config()
            assert cfg[mode] == 0.75 and not any(m in cfg for m in G.MODES if m != mode)
            json.dumps(cfg)
            back = type(o)(**cfg)
            assert back.clip == o.clip and back.key() == o.key() and back.get_config() == cfg
            assert not any(m in twin.get_config() for m in G.MODES)


# ------------------------------------------------------------------------------------ two variables by hand
# a = (3, 4): norm 5;  b = (12): norm 12;  both: norm 13.  SGD(1.0) from w = 0, so w = -clipped gradient.
HAND = {
    "clipvalue": (3.5, [-3.0, -3.5], [-3.5]),
    "clipnorm": (2.5, [-1.5, -2.0], [-2.5]),             # a * 2.5 / 5, b * 2.5 / 12
    "global_clipnorm": (6.5, [-1.5, -2.0], [-6.0]),      # both * 6.5 / 13
}


def _reference_plan(store, opt):
    model = types.SimpleNamespace(layers=[types.SimpleNamespace(activation=None)])
    return PG.ReferencePlan(model, store, "cpu", 1, 1, opt, None)


@pytest.mark.parametrize("mode", G.MODES)
def test_two_variables_by_hand(mode):
    c, wa, wb = HAND[mode]
    st = OO.make_store([("a", (2,)), ("b", (1,))], "cpu")
    plan = _reference_plan(st, OP.SGD(1.0, **{mode: c}))
    gap = ~OO.seg_mask(st)
    st.grad("a").copy_(torch.tensor([3.0, 4.0]))
    st.grad("b").copy_(torch.tensor([12.0]))
    st.g[gap] = OO.W_SENTINEL                    # what lies between the variables takes no part in a norm
    segs = G.store_segments(st)
    assert segs == [(0, 2), (64, 1)]
    want = {"clipvalue": None, "clipnorm": [5.0, 12.0], "global_clipnorm": [13.0]}[mode]
    if want:
        assert G.norms(st.g, segs, mode).tolist() == want
    plan.apply()
    assert st.view("a").tolist() == wa and st.view("b").tolist() == wb
    assert plan.iterations.item() == 1 and float(st.g.abs().max()) == 0.0
    # a zero gradient: scale exactly 1, nothing becomes NaN
    plan.apply()
    assert st.view("a").tolist() == wa and st.view("b").tolist() == wb


def test_negative_values_and_signed_zero_under_clipvalue():
    g = torch.tensor([-5.0, -2.0, -0.0, 0.0, 2.0, 5.0])
    out = OP.SGD(0.1, clipvalue=2.0).clip_reference(g.clone(), [(0, 6)])
    assert out.tolist() == [-2.0, -2.0, -0.0, 0.0, 2.0, 2.0]
    assert torch.signbit(out).tolist() == [True, True, True, False, False, False]
    assert torch.equal(G.clip(g, [(0, 6)], "clipvalue", 2.0).float(), out)


# ------------------------------------------------------------------------------------ fit on the reference plan
GB, NSTEP, LR = 32, 4, 0.05
C_BITES = {"clipvalue": 1e-3, "clipnorm": 0.02, "global_clipnorm": 0.05}


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


def _one():
    return tde.distribute.OneDeviceStrategy("cpu")


def _by_hand(w0, x, y, mode, c):
    """The reference plan's own gradients, clipped by the float64 oracle, applied as plain SGD.  -> (flat
    float64 weights, the oracle norm of every step or the largest |g| under clipvalue)."""
    m = _mlp(_one(), OP.SGD(LR), w0)
    st = m._store
    plan = PG.make_plan(m, st, "cpu", GB, GB, m.optimizer, m.loss)
    assert plan.kind == "reference"
    segs = G.store_segments(st)
    w = st.w.double().clone()
    size = []
    for k in range(NSTEP):
        st.w.copy_(w.float())
        st.g.zero_()
        plan.train_step(torch.from_numpy(x[k * GB:(k + 1) * GB]), torch.from_numpy(y[k * GB:(k + 1) * GB]))
        g = st.g.clone()
        size.append(float(g.abs().max()) if mode == "clipvalue" else G.norms(g, segs, mode).tolist())
        w = w - LR * G.clip(g, segs, mode, c)
    return w, size


@pytest.mark.parametrize("mode", G.MODES)
def test_reference_fit_clips_where_the_norm_exceeds_c(mode):
    x, y = _task()
    c = C_BITES[mode]
    a = _mlp(_one(), OP.SGD(LR, **{mode: c}))
    assert a._program("train", GB).plans[0].kind == "reference"
    w0 = a.get_weights()
    _fit(a, x, y)
    assert a.optimizer.iterations == NSTEP
    tde.backend.clear_session()
    want, size = _by_hand(w0, x, y, mode, c)
    for k in (0, 1):      # the clip bites on the first steps: every norm of step k (the largest |g|) exceeds c
        assert min(size[k]) > c if mode != "clipvalue" else size[k] > c, (k, size[k])
    tde.backend.clear_session()
    b = _mlp(_one(), OP.SGD(LR), w0)
    _fit(b, x, y)
    st = a._store
    got, plain = st.w.double(), b._store.w.double()
    for o, n in G.store_segments(st):
        e = float((got[o: o + n] - want[o: o + n]).abs().max())
        moved = float((plain[o: o + n] - want[o: o + n]).abs().max())
        print(f"[{mode}] segment at {o}: |fit - by hand| {e:.3g}, |unclipped - by hand| {moved:.3g}")
        # float32 against float64 over four SGD steps of |update| <= lr * |g|: a few 2^-24 of |w| <= 1
        assert e <= 1e-6, (o, e)
    assert float((plain - want).abs().max()) > 1e-4          # and unclipped is somewhere else altogether


@pytest.mark.parametrize("mode", G.MODES)
def test_a_large_c_leaves_the_trajectory_bitwise_unclipped(mode):
    x, y = _task()
    a = _mlp(_one(), OP.Adam(1e-3, **{mode: 1e6}))
    w0 = a.get_weights()
    _fit(a, x, y)
    tde.backend.clear_session()
    b = _mlp(_one(), OP.Adam(1e-3), w0)
    _fit(b, x, y)
    for wa, wb, w in zip(a.get_weights(), b.get_weights(), w0):
        assert np.array_equal(wa, wb) and not np.array_equal(wa, w)


@pytest.mark.parametrize("mode", G.MODES)
def test_mirrored_cpu_replicas_clip_after_the_aggregation(mode):
    """Two replicas of 16 against one replica of 32: equal up to the order of the gradient sum.  Clipped before
    the aggregation, each half gradient (norm far above c) would come out at c and the update at about twice
    its size (clipvalue: wherever the halves' signs agree)."""
    x, y = _task()
    c = C_BITES[mode]
    a = _mlp(tde.distribute.MirroredStrategy(devices=["/cpu:0", "/cpu:0"]), OP.SGD(LR, **{mode: c}))
    w0 = a.get_weights()
    _fit(a, x, y)
    prog = a._program("train", GB)
    assert len(prog.plans) == 2 and all(p.kind == "reference" and p.step_mode == "plain" for p in prog.plans)
    assert np.array_equal(prog.stores[0].w.numpy(), prog.stores[1].w.numpy())
    tde.backend.clear_session()
    b = _mlp(_one(), OP.SGD(LR, **{mode: c}), w0)
    _fit(b, x, y)
    for wa, wb, w in zip(a.get_weights(), b.get_weights(), w0):
        upd = float(np.abs(wb - w).max())
        assert upd > 0
        # the two sums differ by float32 roundings of the gradient; a clip before the aggregation by about upd
        assert float(np.abs(wa - wb).max()) <= 1e-3 * upd + 1e-7, (float(np.abs(wa - wb).max()), upd)


def test_cpu_plan_runs_plain_under_clipping():
    for mode in G.MODES:
        m = _mlp(_one(), OP.SGD(0.1, **{mode: 1.0}))
        plan = PG.make_plan(m, m._store, "cpu", 8, 8, m.optimizer, m.loss)
        assert plan.step_mode == "plain" and not plan._opt_fused()
        assert not plan.supports_step_mode("local") and not plan.supports_step_mode("xgmi")
        tde.backend.clear_session()
    m = _mlp(_one(), OP.SGD(0.1))
    assert PG.make_plan(m, m._store, "cpu", 8, 8, OP.SGD(0.1), m.loss)._opt_fused()


# ------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("mode", G.MODES)
def test_parameter_server_refuses_clipping_by_name(mode, monkeypatch, tmp_path):
    monkeypatch.setenv("TF_CONFIG", json.dumps({"cluster": {"ps": ["127.0.0.1:1"], "worker": ["127.0.0.1:2"]},
                                                "task": {"type": "worker", "index": 0}}))
    st = tde.distribute.experimental.ParameterServerStrategy()
    assert st.is_distributed
    tde.backend.set_random_seed(11)
    m = tde.zoo.mnist_mlp()
    m.compile(loss=tde.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=OP.Adam(1e-3, **{mode: 1.0}),
              metrics=["accuracy"])
    m.build()
    est = tde.estimator.Estimator(m, model_dir=str(tmp_path),
                                  config=tde.estimator.RunConfig(model_dir=str(tmp_path), train_distribute=st))

    def input_fn():
        raise AssertionError("the input pipeline must not start")
    with pytest.raises(ValueError, match=f"ParameterServerStrategy.*{mode}=1.0"):
        est.train(input_fn, max_steps=1)
    assert est._psc is None
    from tensorflow_distributed_example_amd.parallel.ps import PSClient
    c = PSClient.__new__(PSClient)
    c.conns = []
    with pytest.raises(ValueError, match=f"{mode}=1.0"):
        c.set_optimizer(3, clip=(mode, 1.0))
    c.set_optimizer(3, clip=None)
    c.set_optimizer(0)


# ------------------------------------------------------------------------------------ the table builder
SEG_DT = np.dtype([("off", "<i8"), ("rows", "<i4"), ("cols", "<i4"), ("sh", "<i8"), ("sht", "<i8")])


@pytest.mark.skipif(not N.hip_available(), reason="libtde_hip.so not built")
def test_clip_table_covers_every_segment():
    shapes = OO.SHAPES + [(n, s) for n, s, _ in G.EXTRA_SEGMENTS]
    st = OO.make_store(shapes, "cpu")
    segs = G.store_segments(st)
    assert [n for _, n in segs[-3:]] == [1, G.CHUNK, G.CHUNK + 5]
    rows = []
    for name in st.names(trainable=True):
        s = st.segments[name]
        r, c = (int(np.prod(s.shape[:-1])), s.shape[-1]) if len(s.shape) >= 2 else (1, s.numel)
        rows.append((s.offset, r, c, -1, -1))
    arr = np.array(rows, dtype=SEG_DT)
    lib = N.hip()
    ents_want, ranges_want = G.table(segs)
    assert [c for _, c in ranges_want[-3:]] == [1, 1, 2] and ranges_want[OO.SHAPES.index(("v4100", (4100,)))][1] == 2
    ne = lib.tde_clip_table_size(arr.ctypes.data, len(arr))
    assert ne == len(ents_want) == sum(G.chunks(n) for _, n in segs)
    ents = np.full((ne + 1, 2), -9, dtype=np.int32)
    ranges = np.full((len(arr) + 1, 2), -9, dtype=np.int32)
    assert lib.tde_clip_build_table(arr.ctypes.data, len(arr), ents.ctypes.data, ranges.ctypes.data) == ne
    assert [tuple(e) for e in ents[:ne].tolist()] == ents_want
    assert [tuple(r) for r in ranges[:len(arr)].tolist()] == ranges_want
    assert ents[ne].tolist() == [-9, -9] and ranges[len(arr)].tolist() == [-9, -9]      # nothing past the end
    # every element of every segment lies in exactly one entry's chunk
    for i, (_, n) in enumerate(segs):
        first, count = ranges_want[i]
        covered = sum(min((c + 1) * G.CHUNK, n) - c * G.CHUNK for s, c in ents_want[first: first + count] if s == i)
        assert covered == n
    assert lib.tde_clip_table_size(arr.ctypes.data, 0) == 0
