"""Top-k accuracy, crossentropy as a metric and the F-score on the GPU (csrc/include/tde_metric.h,
csrc/kernels/metrichead.hip, the metric variants of the small-net step), against the float64 oracle of
tests/metric_oracle.py:

1. ``tde_metric_rows`` alone on crafted dyadic logits (ties, +-inf, labels out of range): counts equal, sums
   within the bound of tests/test_loss_head_gpu.py::test_kernel_against_float64;
2. the small-net metric variants on logits that are the head's bias exactly: counts equal, and everything else
   bitwise what the same model compiled with "accuracy" alone computes;
3. the zoo's plans against float64, row margins below 1e-4 left out; hipGraph against eager,
   ``steps_per_execution``, the reset between epochs, ``fit`` / ``evaluate`` / validation logs, two Mirrored
   replicas in a child process; which plan the fused-CNN models get.

``-s`` prints every figure before it is asserted.
"""
import ctypes
import json
import os
import signal
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import loss_head_oracle as H
import metric_oracle as MO
import smallnet_oracle as SO

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BP = 8
SEED = 31          # picked on the CPU: no row of the three zoo models' batches is within 1e-4 of a boundary


def _tde():
    import tensorflow_distributed_example_amd as tde
    from tensorflow_distributed_example_amd.train import program as PG
    return tde, PG


def _spec(C, ks, smooths, cm):
    from tensorflow_distributed_example_amd.ops import metric_ops as OM
    s = OM.MetricSpec(n_topk=len(ks), n_ce=len(smooths), cm=int(cm), off_topk=0, off_ce=len(ks),
                      off_cm=len(ks) + len(smooths), words=len(ks) + len(smooths) + (C * C if cm else 0))
    for i, k in enumerate(ks):
        s.k[i] = k
    for i, e in enumerate(smooths):
        s.smooth[i] = e
    return s


# ------------------------------------------------------------------------------------- 1. the kernel alone
def _crafted(B, C, seed):
    """Logits on the grid of quarters in [-2, 2] (ties in every row), and from five rows on: l_y = -inf, a +inf
    beside the label, a label past the classes and a negative one."""
    rng = np.random.default_rng(seed)
    z = (rng.integers(-8, 9, (B, C)) / 4.0).astype(np.float32)
    y = rng.integers(0, C, B).astype(np.int32)
    z[0, y[0]] = z[0].max()                     # tied with the row's maximum or alone there
    finite = z.copy()
    if B >= 5:
        z[1, y[1]] = -np.inf
        z[2, (y[2] + 1) % C] = np.inf
        y[3], y[4] = C + 2, -1
    return z, finite, y


def _rows(z, y, C, spec, ldl, launches=1):
    from tensorflow_distributed_example_amd.ops import metric_ops as OM
    B = z.shape[0]
    pad = np.full((B, ldl), 99.0, dtype=np.float32)     # the columns behind C are never read
    pad[:, :C] = z
    lg, yy = torch.from_numpy(pad).to(DEV), torch.from_numpy(y).to(DEV)
    ext = torch.zeros(spec.words, device=DEV)
    for _ in range(launches):
        OM.metric_rows(lg, yy, B, C, spec, ext, ldl=ldl)
    torch.cuda.synchronize()
    return ext.cpu().double().numpy()


@pytest.mark.parametrize("B", [1, 5, 7])
@pytest.mark.parametrize("C", [3, 10, 64, 65, 130])
def test_metric_rows_against_float64(C, B):
    from tensorflow_distributed_example_amd.ops import layer_ops32 as O32
    z, finite, y = _crafted(B, C, 1000 + 10 * C + B)
    ks, sm = (1, 2, 5, C), (0.0, 0.1)
    spec = _spec(C, ks, sm, True)
    got = _rows(z, y, C, spec, C + 3)
    want = MO.words(z, y, ks, sm, True)
    print(f"[{B}x{C}] top-k {got[:4].tolist()} float64 {want['topk'].tolist()}; ce {got[4:6].tolist()} "
          f"float64 {want['ce'].tolist()}")
    assert got[:4].tolist() == want["topk"].tolist()
    assert np.array_equal(got[6:].reshape(C, C), want["cm"]) and want["cm"].sum() == (B if B < 5 else B - 2)
    for g, w in zip(got[4:6], want["ce"]):      # a non-finite sum stays one (the finite sums: below)
        assert np.isfinite(w) or not np.isfinite(g)
    # k past the classes: every row with a valid label and a finite l_y
    got_big = _rows(z, y, C, _spec(C, (C + 3,), (), False), C + 3)
    assert got_big.tolist() == MO.words(z, y, (C + 3,))["topk"].tolist() == [float(B if B < 5 else B - 3)]
    # the sums on the finite twin, within the bound of tests/test_loss_head_gpu.py::test_kernel_against_float64:
    # 1e-5, or twice the plain xent32 launch's own error on these rows where that is more
    gf = _rows(finite, y, C, spec, C + 3)
    wf = MO.words(finite, y, ks, sm, True)
    met = torch.zeros(4, device=DEV)
    O32.xent(torch.from_numpy(finite).to(DEV), torch.from_numpy(y).to(DEV), B, C, scale=1.0, metrics=met)
    torch.cuda.synchronize()
    pl_el = abs(met[0].item() - wf["ce"][0]) / wf["ce"][0]
    tl = max(1e-5, 2 * pl_el)
    for i in range(2):
        el = abs(gf[4 + i] - wf["ce"][i]) / wf["ce"][i]
        print(f"[{B}x{C}] ce e={sm[i]}: {gf[4 + i]!r} float64 {wf['ce'][i]!r} err {el:.3g} (plain {pl_el:.3g})")
        assert wf["ce"][i] > 0 and el <= tl
    assert gf[:4].tolist() == wf["topk"].tolist() and np.array_equal(gf[6:].reshape(C, C), wf["cm"])
    # a second launch without a reset: exactly twice the counts
    twice = _rows(z, y, C, spec, C + 3, launches=2)
    assert twice[:4].tolist() == (2 * want["topk"]).tolist() and np.array_equal(twice[6:], 2 * want["cm"].reshape(-1))


def test_a_bad_spec_or_shape_returns_minus_one():
    from tensorflow_distributed_example_amd import _native as N
    from tensorflow_distributed_example_amd.ops import metric_ops as OM
    C, B = 10, 4
    lg = torch.zeros(B, C, device=DEV)
    yy = torch.zeros(B, dtype=torch.int32, device=DEV)
    ext = torch.zeros(4 + C * C, device=DEV)

    def rc(spec, c=C, ldl=C):
        return N.hip().tde_metric_rows(lg.data_ptr(), ldl, yy.data_ptr(), B, c, ctypes.byref(spec) if spec else None,
                                       ext.data_ptr(), N.stream_ptr())

    assert rc(_spec(C, (1, 2), (0.0,), True)) == 0
    bad = [_spec(C, (0,), (), False), _spec(C, (1,), (1.0,), False), _spec(C, (1,), (-0.5,), False),
           _spec(C, (), (), False)]
    s = _spec(C, (1,), (), False)
    s.n_topk = 5
    bad.append(s)
    s = _spec(C, (1,), (0.0,), True)
    s.words += 1
    bad.append(s)
    s = _spec(C, (1,), (0.0,), True)
    s.off_cm = 1
    bad.append(s)
    s = _spec(C, (1,), (), False)
    s.cm = 2
    bad.append(s)
    assert [rc(b) for b in bad] == [-1] * len(bad)
    assert rc(None) == -1 and rc(_spec(C, (1,), (), False), ldl=C - 1) == -1 and rc(_spec(C, (1,), (), False), c=0) == -1
    assert rc(_spec(1025, (1,), (), True), c=1025, ldl=1025) == -1       # no confusion block past 1024 classes
    torch.cuda.synchronize()
    assert ext[:2].tolist() == [B, B] and ext[3].item() == B and ext[4:].sum().item() == 0   # the one good launch
    with pytest.raises(ValueError, match="ext"):
        OM.metric_rows(lg, yy, B, C, _spec(C, (1,), (), True), ext[:50])


# ------------------------------------------------------------------------------------- 2. the small-net variants
def _bias_model(tde, C, metrics, smooth, bias):
    L = tde.keras.layers
    m = tde.keras.Sequential([L.Dense(8, activation="relu", input_shape=(12,)), L.Dense(C)])
    loss = (tde.losses.CategoricalCrossentropy(from_logits=True, label_smoothing=smooth) if smooth
            else tde.losses.SparseCategoricalCrossentropy(from_logits=True))
    m.compile(loss=loss, optimizer=tde.optimizers.SGD(0.05), metrics=metrics)
    m.build()
    w = m.get_weights()
    w[2] = np.zeros_like(w[2])
    w[3] = bias.astype(np.float32)
    m.set_weights(w)
    return m


@pytest.mark.parametrize("smooth", [0.0, 0.1], ids=["plain", "loss"])
@pytest.mark.parametrize("C", [10, 70])
def test_smallnet_variant_counts_are_exact_and_nothing_else_changes(C, smooth):
    tde, _ = _tde()
    KM = tde.keras.metrics
    rng = np.random.default_rng(C)
    bias = (rng.integers(-8, 1, C) / 4.0)
    bias[[0, 1]] = 1.0                      # a tie at the maximum: the argmax is class 0
    bias[[2, 3, 4]] = 0.5                   # tied across the k = 3 boundary (two greater)
    bias[C - 1] = 0.25
    x = torch.from_numpy(rng.standard_normal((5, 12)).astype(np.float32))
    y = torch.tensor([0, 1, 3, C - 1, 5], dtype=torch.int32)
    sparse = not smooth
    topk = KM.SparseTopKCategoricalAccuracy if sparse else KM.TopKCategoricalAccuracy
    ce = (KM.SparseCategoricalCrossentropy(from_logits=True) if sparse
          else KM.CategoricalCrossentropy(from_logits=True, label_smoothing=0.1))
    ks = (1, 2, 3, 6)
    mets = ["accuracy"] + [topk(k, name=f"t{k}") for k in ks] + [ce, KM.F1Score(average="macro")]
    z = np.tile(bias, (5, 1))
    want = MO.words(z, y.numpy(), ks, (float(smooth),), True)
    # labels 0 and 1 share the maximum (nothing greater: hits at every k, but only class 0 is the argmax), label 3
    # has two classes greater and is tied with two more, label C - 1 has five greater, label 5 at least six
    assert want["topk"].tolist() == [2.0, 2.0, 3.0, 4.0] and want["correct"] == 1
    out = []
    for metrics in (mets, ["accuracy"]):
        tde.backend.clear_session()
        tde.backend.set_random_seed(4)
        m = _bias_model(tde, C, metrics, smooth, bias)
        # evaluation adds each row's loss with an atomic of its own, in any order: one row per launch, so that the
        # sums can be compared bit for bit (row by row; the counts are exact in any order)
        ev = m._program("eval", 5)
        ev.reset_metrics()
        per_row = []
        for i in range(5):
            before = ev.global_metrics()
            ev.eval_batch([(x[i:i + 1].numpy(), y[i:i + 1].numpy())])
            ev.sync()
            per_row.append((ev.global_metrics() - before)[:4])
        em = ev.global_metrics()
        prog = m._program("train", 5)
        plan = prog.plans[0]
        assert plan.kind == "fused_smallnet" and bool(plan.loss_spec) == bool(smooth)
        assert (plan.metrics_ext is not None) == (metrics is mets)
        prog.reset_metrics()
        prog.stage([(x[None].to(DEV), y[None].to(DEV))])
        prog.run()
        prog.sync()
        tm = prog.global_metrics()
        out.append((em, tm, [w.copy() for w in m.get_weights()], per_row))
    (em, tm, w, rows), (em0, tm0, w0, rows0) = out
    assert em[1:4].tolist() == em0[1:4].tolist() == [1.0, 5.0, 0.0]
    for tag, a, b in (("eval", em, em0), ("train", tm, tm0)):
        print(f"[C={C} e={smooth} {tag}] ext {a[4:10].tolist()} float64 {want['flat'][:5].tolist()}")
        if tag == "train":      # the step's loss sum is reduced in a fixed order: metrics[0..3] bitwise
            assert torch.equal(a[:4].float().view(torch.int32), b.float().view(torch.int32))
        assert a[4:8].tolist() == want["topk"].tolist()
        assert np.array_equal(a[9:].numpy().reshape(C, C), want["cm"])
        assert abs(a[8].item() - want["ce"][0]) <= 1e-5 * want["ce"][0]       # the loss' bound on this plan
    # evaluation, row by row: the first row's words bitwise, the others as differences of float32 partial sums
    assert torch.equal(rows[0].float().view(torch.int32), rows0[0].float().view(torch.int32))
    assert all(torch.equal(r, r0) for r, r0 in zip(rows, rows0))
    assert all(np.array_equal(u.view(np.int32), v.view(np.int32)) for u, v in zip(w, w0))
    assert any(not np.array_equal(u, v) for u, v in zip(w, _bias_model(tde, C, ["accuracy"], smooth, bias).get_weights()))


# ------------------------------------------------------------------------------------- 3. plans against float64
KS = (1, 2, 5)


def _metrics(tde):
    KM = tde.keras.metrics
    return ["accuracy"] + [KM.SparseTopKCategoricalAccuracy(k, name=f"top{k}") for k in KS] + \
        [KM.SparseCategoricalCrossentropy(from_logits=True), KM.F1Score(average="macro")]


def _zoo(tde, name, metrics=None, opt=None, spe=None):
    m = getattr(tde.zoo, name)()
    logits = m.layers[-1].activation != "softmax"
    m.compile(loss=tde.losses.SparseCategoricalCrossentropy(from_logits=logits), optimizer=opt or tde.optimizers.SGD(0.05),
              metrics=_metrics(tde) if metrics is None else metrics, steps_per_execution=spe)
    m.build()
    return m


def _logits64(m, x):
    """Float64 logits of the model's current weights."""
    return SO._forward(m, SO._weights(m, m._store, torch.float64, False), x.double())[0].numpy()


def _check_step(tag, z, y, got, tl, left_out):
    """One step's accumulators ``got`` [4 + words] against the float64 logits ``z`` of the weights it ran with."""
    yn = y.numpy()
    mk, ma = MO.margins(z, yn, KS)
    C, n = z.shape[1], len(yn)
    assert got[2].item() == n
    for j, k in enumerate(KS):
        near = mk[:, j] < 1e-4
        lo = MO.words(z[~near], yn[~near], (k,))["topk"][0]
        print(f"[{tag}] top-{k}: {got[4 + j].item()} float64 {lo} (+ {int(near.sum())} rows near the boundary)")
        assert lo <= got[4 + j].item() <= lo + near.sum()
        left_out[0] += int(near.sum())
        left_out[1] += n
    near = ma < 1e-4
    w = MO.words(z[~near], yn[~near], (), (), True)
    cm = got[4 + len(KS) + 1:].numpy().reshape(C, C)
    print(f"[{tag}] correct {got[1].item()} float64 {w['correct']} (+ {int(near.sum())}); cm trace {np.trace(cm)}")
    assert (cm >= w["cm"]).all() and cm.sum() == n and w["correct"] <= got[1].item() <= w["correct"] + near.sum()
    assert np.trace(cm) == got[1].item()
    left_out[0] += int(near.sum())
    left_out[1] += n
    ce = MO.words(z, yn, (), (0.0,))["ce"][0]
    e = abs(got[4 + len(KS)].item() - ce) / ce
    print(f"[{tag}] crossentropy {got[4 + len(KS)].item()!r} float64 {ce!r} err {e:.3g} bound {tl:.3g}")
    assert e <= tl
    assert abs(got[0].item() - ce) <= tl * ce          # no smoothing, weights or penalty: the metric is the loss


@pytest.mark.parametrize("mode", ["local", "plain"])
@pytest.mark.parametrize("name", ["mnist_mlp", "lenet5"])
def test_smallnet_plans_against_float64(name, mode, monkeypatch):
    tde, _ = _tde()
    monkeypatch.setenv("TDE_FUSED_STEP", "1" if mode == "local" else "0")
    tde.backend.clear_session()
    tde.backend.set_random_seed(SEED)
    m = _zoo(tde, name)
    prog = m._program("train", BP)
    plan = prog.plans[0]
    assert plan.kind == "fused_smallnet" and plan.step_mode == mode and plan.metrics_ext is not None
    left_out = [0, 0]
    for k, (x, y) in enumerate(H.batches(m, BP, 3, SEED + 100)):
        prog.sync()
        prog.reset_metrics()
        z = _logits64(m, x)         # of the weights in front of the step
        prog.stage([(x[None].to(DEV), y[None].to(DEV))])
        prog.run()
        prog.sync()
        # 1e-5: the bound of tests/test_loss_head_gpu.py::test_smallnet_plan_against_float64 for the loss
        _check_step(f"{name} {mode} step {k}", z, y, prog.global_metrics(), 1e-5, left_out)
    print(f"[{name} {mode}] left out {left_out[0]} of {left_out[1]}")
    assert left_out[0] <= 0.05 * left_out[1]


@pytest.mark.parametrize("policy", ["float32", "mixed_bfloat16"])
def test_mnist_cnn_declines_to_the_layerwise_plan_and_matches_float64(policy):
    tde, PG = _tde()
    from tensorflow_distributed_example_amd.train.layerwise import LayerwisePlan
    tde.keras.mixed_precision.set_global_policy(policy)
    try:
        tde.backend.clear_session()
        tde.backend.set_random_seed(SEED)
        m = _zoo(tde, "mnist_cnn")
        with pytest.warns(UserWarning, match="no metric head for top1, top2, top5, sparse_categorical_crossentropy, "
                                             "f1_score") as rec:
            plan = PG.make_plan(m, m._store, DEV, BP, BP, m.optimizer, m.loss)
        assert len([w for w in rec if "metric head" in str(w.message)]) == 1
        assert isinstance(plan, LayerwisePlan) and not plan.stages[-1].fused and plan.metrics_ext is not None
        assert plan.compute_dtype == ("fp32" if policy == "float32" else "bf16")
        left_out = [0, 0]
        # the bounds of tests/test_loss_head_gpu.py::test_layerwise_plan_against_float64 for the loss
        tl = 1e-5 if policy == "float32" else 6e-2
        for k, (x, y) in enumerate(H.batches(m, BP, 3, SEED + 100)):
            plan.reset_metrics()
            plan.train_step(x.to(DEV, plan.input_dtype).contiguous(), y.to(DEV), BP)
            torch.cuda.synchronize()
            got = plan.all_metrics().cpu().double()
            _check_step(f"mnist_cnn {policy} step {k}", _logits64(m, x), y, got, tl, left_out)   # before apply()
            plan.apply()
        x, y = H.batches(m, BP, 1, SEED + 200)[0]
        plan.reset_metrics()
        plan.eval_step(x.to(DEV, plan.input_dtype).contiguous(), y.to(DEV), BP)
        torch.cuda.synchronize()
        _check_step(f"mnist_cnn {policy} eval", _logits64(m, x), y, plan.all_metrics().cpu().double(), tl, left_out)
        print(f"[mnist_cnn {policy}] left out {left_out[0]} of {left_out[1]}")
        assert left_out[0] <= 0.05 * left_out[1]
    finally:
        tde.keras.mixed_precision.set_global_policy("float32")


def test_fused_plans_stay_with_accuracy_alone_and_decline_with_a_warning_otherwise():
    tde, PG = _tde()
    from tensorflow_distributed_example_amd.train.layerwise import LayerwisePlan
    for zoo, kind in (("mnist_cnn", "fused_convnet"), ("mnist_bn_cnn", "fused_bncnn")):
        tde.backend.clear_session()
        m = _zoo(tde, zoo, metrics=["accuracy"])
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            plan = PG.make_plan(m, m._store, DEV, BP, BP, m.optimizer, m.loss)
        assert plan.kind == kind and plan.metrics_ext is None
        tde.backend.clear_session()
        m = _zoo(tde, zoo, metrics=["accuracy", tde.keras.metrics.F1Score(average="micro")])
        with pytest.warns(UserWarning, match="no metric head for f1_score"):
            plan = PG.make_plan(m, m._store, DEV, BP, BP, m.optimizer, m.loss)
        assert isinstance(plan, LayerwisePlan) and plan.metrics_ext.numel() == 100


def _run_steps(tde, graph, spe, monkeypatch, w0=None):
    monkeypatch.setenv("TDE_GRAPH", "1" if graph else "0")
    tde.backend.clear_session()
    tde.backend.set_random_seed(SEED)
    m = _zoo(tde, "mnist_mlp", spe=spe)
    if w0 is not None:
        m.set_weights(w0)
    start = m.get_weights()
    prog = m._program("train", BP)
    assert prog.use_graph == graph and prog.S == spe
    bs = H.batches(m, BP, 4, SEED + 300)
    prog.reset_metrics()
    for i in range(0, 4, spe):
        xs = torch.stack([b[0] for b in bs[i:i + spe]]).to(DEV)
        ys = torch.stack([b[1] for b in bs[i:i + spe]]).to(DEV)
        prog.stage([(xs, ys)])
        prog.run()
    prog.sync()
    return start, prog.global_metrics(), m.get_weights(), (prog.graph is not None)


def test_graph_replay_and_steps_per_execution_give_the_eager_counts(monkeypatch):
    tde, _ = _tde()
    w0, eager, we, g0 = _run_steps(tde, False, 1, monkeypatch)
    _, graph, wg, g1 = _run_steps(tde, True, 1, monkeypatch, w0)
    _, spe2, w2, _ = _run_steps(tde, True, 2, monkeypatch, w0)
    assert not g0 and g1 and eager[2].item() == 4 * BP and eager[4:7].sum() > 0
    n = 4 + len(KS)
    print(f"eager {eager[:n + 1].tolist()} graph {graph[:n + 1].tolist()} spe 2 {spe2[:n + 1].tolist()}")
    for other in (graph, spe2):
        assert other[1:n].tolist() == eager[1:n].tolist() and torch.equal(other[n + 1:], eager[n + 1:])   # the counts
        assert abs(other[n].item() - eager[n].item()) <= 1e-6 * eager[n].item()      # the sum: another atomic order
    assert all(np.array_equal(a, b) for a, b in zip(we, wg)) and all(np.array_equal(a, b) for a, b in zip(we, w2))


def test_fit_evaluate_and_validation_logs_carry_every_name_and_reset_between_epochs():
    tde, _ = _tde()
    tde.backend.clear_session()
    tde.backend.set_random_seed(SEED)
    m = _zoo(tde, "mnist_mlp", opt=tde.optimizers.SGD(0.0))      # lr 0: every epoch sees the same weights
    rng = np.random.default_rng(2)
    x = rng.random((3 * BP + 3, 28, 28, 1), dtype=np.float32)   # a ragged last batch
    y = rng.integers(0, 10, len(x))
    h = m.fit(x, y, batch_size=BP, epochs=2, verbose=0, shuffle=False, validation_data=(x[:BP], y[:BP])).history
    names = ["accuracy", "top1", "top2", "top5", "sparse_categorical_crossentropy", "f1_score"]
    assert list(h) == ["loss"] + names + ["val_loss"] + ["val_" + n for n in names]
    ev = m.evaluate(x, y, batch_size=BP, verbose=0, return_dict=True)
    # (a second evaluation adds its rows' losses in another atomic order: the sums agree to rounding)
    assert list(ev) == ["loss"] + names and m.evaluate(x, y, batch_size=BP, verbose=0) == pytest.approx(list(ev.values()),
                                                                                                    rel=1e-6)
    z = SO._forward(m, SO._weights(m, m._store, torch.float64, False), torch.from_numpy(x).double())[0].numpy()
    mk, ma = MO.margins(z, y, KS)
    assert mk.min() >= 1e-4 and ma.min() >= 1e-4      # data seed 2: no row near a boundary (checked on the CPU)
    w = MO.words(z, y, KS, (0.0,), True)
    for k in names:
        print(f"{k}: fit {h[k]} evaluate {ev[k]!r}")
        assert h[k][0] == h[k][1] or k == "sparse_categorical_crossentropy"       # reset between the epochs
        assert h[k][0] == pytest.approx(ev[k], rel=1e-6)
    assert ev["top1"] == ev["accuracy"] == w["correct"] / len(y)
    assert [ev[f"top{k}"] for k in KS] == [c / len(y) for c in w["topk"]]
    assert ev["f1_score"] == pytest.approx(MO.fbeta(w["cm"], 1.0, "macro"), rel=1e-12)
    assert ev["sparse_categorical_crossentropy"] == pytest.approx(w["ce"][0] / len(y), rel=1e-5)


CHILD_TIMEOUT = 90


def test_mirrored_replicas_count_what_one_replica_counts():
    """Two Mirrored replicas rehearsed on cuda:0 and, in the same child, one replica at the same global batch."""
    env = dict(os.environ, TDE_HEARTBEAT="0", OMP_NUM_THREADS="2", TDE_XGMI_TIMEOUT="20")
    p = subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "metric_head_mirrored_child.py")], env=env,
                         cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, start_new_session=True)
    try:
        out, _ = p.communicate(timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        os.killpg(p.pid, signal.SIGKILL)
        out, _ = p.communicate()
        raise AssertionError(f"timed out:\n{out[-3000:]}")
    assert p.returncode == 0, out[-4000:]
    res = json.loads([l for l in out.splitlines() if l.startswith("RESULT ")][0][7:])
    print(res)
    assert res["plan"] == "fused_smallnet" and res["ext"] == [True, True] and res["rows"] == res["one_rows"] == 64.0
    assert res["counts"] == res["one_counts"] == res["want_counts"] and sum(res["counts"]) > 0, res
    assert abs(res["ce"] - res["one_ce"]) <= 1e-5 * res["one_ce"] and abs(res["ce"] - res["want_ce"]) <= 1e-5 * res["want_ce"]
