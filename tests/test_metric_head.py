"""Top-k accuracy, crossentropy as a metric and the F-score on the CPU: constructors and refusals, configuration
round trips, hand-computed examples, the ``MetricSpec`` ABI, and the reference plan (``fit``, ``evaluate``,
``val_*``, a ragged last batch, two Mirrored replicas) against the float64 oracle of tests/metric_oracle.py."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import tensorflow_distributed_example_amd as tde
from tensorflow_distributed_example_amd import _native as N
from tensorflow_distributed_example_amd import losses as LS
from tensorflow_distributed_example_amd import metrics as MT
from tensorflow_distributed_example_amd import optimizers as OP
from tensorflow_distributed_example_amd.models import layers as L
from tensorflow_distributed_example_amd.train import program as PG

import metric_oracle as MO
import smallnet_oracle as SO

B = 8
KM = tde.keras.metrics


@pytest.fixture(autouse=True)
def _fresh():
    tde.backend.clear_session()
    tde.backend.set_random_seed(11)
    yield
    tde.backend.clear_session()


def _sparse(from_logits=True):
    return LS.SparseCategoricalCrossentropy(from_logits=from_logits)


def _mlp(metrics, loss=None, opt=None, w0=None, classes=10, softmax=False, reg=None):
    m = tde.keras.Sequential([L.Dense(16, activation="relu", input_shape=(12,), kernel_regularizer=reg),
                              L.Dense(classes, activation="softmax" if softmax else None)])
    m.compile(loss=loss or _sparse(not softmax), optimizer=opt or OP.SGD(0.1), metrics=list(metrics))
    m.build()
    if w0 is not None:
        m.set_weights(w0)
    return m


def _all_metrics():
    return ["accuracy", KM.SparseTopKCategoricalAccuracy(k=2), KM.SparseTopKCategoricalAccuracy(k=5, name="top5"),
            KM.SparseCategoricalCrossentropy(from_logits=True), KM.F1Score(average="macro"),
            KM.FBetaScore(average="weighted", beta=2.0), KM.F1Score(average="micro", name="f1_micro")]


def _logits64(m, x):
    W = SO._weights(m, m._store, torch.float64, False)
    return SO._forward(m, W, torch.as_tensor(x).double())[0].numpy()


def _want(m, z, y):
    """The logged values of float64 logits ``z`` for the compiled metrics of ``m``."""
    lay = m._metric_names.layout
    w = MO.words(z, y, lay.k, lay.smooth, bool(lay.cm))
    out = {}
    for met, i in lay.entries:
        if met.kind == "topk":
            out[met.name] = w["topk"][i] / len(y)
        elif met.kind == "ce":
            out[met.name] = w["ce"][i] / len(y)
        else:
            out[met.name] = MO.fbeta(w["cm"], met.beta, met.average)
    if "accuracy" in m._metric_names:
        out["accuracy"] = w["correct"] / len(y)
    return out, w


# ------------------------------------------------------------------------------------ the interface
def test_this_feature_compiles_a_top_k_metric():
    m = _mlp([KM.SparseTopKCategoricalAccuracy(2)])
    assert m._metric_names == ["sparse_top_k_categorical_accuracy"] and m._metric_names.layout.k == [2]


def test_strings_names_and_config_round_trips():
    r = MT.resolve(["acc", "accuracy", "sparse_top_k_categorical_accuracy", "sparse_categorical_crossentropy"],
                   _sparse())
    assert r == ["accuracy", "sparse_top_k_categorical_accuracy", "sparse_categorical_crossentropy"]
    assert r[1].k == 5 and r[2].from_logits is None and r.extra == r[1:]
    r = MT.resolve(["top_k_categorical_accuracy", "categorical_crossentropy", "categorical_accuracy"],
                   LS.CategoricalCrossentropy())
    assert r == ["top_k_categorical_accuracy", "categorical_crossentropy", "accuracy"]
    for obj in (KM.SparseTopKCategoricalAccuracy(k=3, name="t3"), KM.TopKCategoricalAccuracy(),
                KM.SparseCategoricalCrossentropy(from_logits=True),
                KM.CategoricalCrossentropy(from_logits=True, label_smoothing=0.25, name="ce"),
                KM.F1Score(average="macro"), KM.FBetaScore(average="weighted", beta=0.5, name="fb")):
        cfg = obj.get_config()
        back = type(obj).from_config(cfg)
        assert back.get_config() == cfg and back == obj and back.name == obj.name
    assert KM.F1Score(average="micro").name == "f1_score" and KM.FBetaScore(average="micro").name == "fbeta_score"
    assert KM.F1Score(average="micro").beta == 1.0


def test_refusals_by_name():
    with pytest.raises(ValueError, match="SparseTopKCategoricalAccuracy.*CategoricalCrossentropy"):
        MT.resolve([KM.SparseTopKCategoricalAccuracy()], LS.CategoricalCrossentropy())
    with pytest.raises(ValueError, match="categorical_crossentropy.*SparseCategoricalCrossentropy"):
        MT.resolve(["categorical_crossentropy"], _sparse())
    with pytest.raises(ValueError, match="from_logits=False contradicts"):
        _mlp([KM.SparseCategoricalCrossentropy(from_logits=False)])
    with pytest.raises(ValueError, match="from_logits=True contradicts"):
        _mlp([KM.SparseCategoricalCrossentropy(from_logits=True)], softmax=True)
    with pytest.raises(NotImplementedError, match=r"F1Score\(average=None\)"):
        KM.F1Score()
    with pytest.raises(NotImplementedError, match=r"FBetaScore\(average=None\)"):
        KM.FBetaScore(average=None)
    with pytest.raises(NotImplementedError, match=r"FBetaScore\(threshold=0.5\)"):
        KM.FBetaScore(average="macro", threshold=0.5)
    with pytest.raises(ValueError, match="average"):
        KM.F1Score(average="samples")
    for bad in (0, -1, 2.0, True, "3", None):
        with pytest.raises(ValueError, match="k must be an int >= 1"):
            KM.SparseTopKCategoricalAccuracy(k=bad)
    with pytest.raises(ValueError, match="duplicate metric name 'sparse_top_k_categorical_accuracy'"):
        MT.resolve([KM.SparseTopKCategoricalAccuracy(1), KM.SparseTopKCategoricalAccuracy(2)], _sparse())
    with pytest.raises(ValueError, match="f1_score.*at most 1024 classes.*1025"):
        _mlp([KM.F1Score(average="macro")], classes=1025)
    assert _mlp([KM.SparseTopKCategoricalAccuracy(3)], classes=1025)._metric_names.layout.words == 1
    with pytest.raises(ValueError, match="unsupported metric"):
        MT.resolve(["auc"], _sparse())
    m = _mlp(["accuracy"])
    with pytest.raises(NotImplementedError, match="weighted_metrics"):
        m.compile(loss=_sparse(), optimizer="sgd", weighted_metrics=[KM.F1Score(average="micro")])
    with pytest.raises(NotImplementedError, match="sample_weight"):
        m.fit(np.zeros((B, 12), np.float32), np.zeros(B, np.int64), sample_weight=np.ones(B), verbose=0)


# ------------------------------------------------------------------------------------ the ABI
def test_metric_spec_struct_and_offsets():
    from tensorflow_distributed_example_amd.ops import metric_ops as OM
    S = OM.MetricSpec
    assert ctypes.sizeof(S) == 52
    assert [f[0] for f in S._fields_] == ["n_topk", "k", "n_ce", "smooth", "cm", "off_topk", "off_ce", "off_cm",
                                          "words"]
    assert (S.k.offset, S.n_ce.offset, S.smooth.offset, S.cm.offset, S.off_topk.offset, S.words.offset) == \
        (4, 20, 24, 32, 36, 48)
    mets = MT.resolve(_all_metrics() + [KM.SparseTopKCategoricalAccuracy(2, name="again")], _sparse())
    lay = MT.metric_spec(mets, _sparse(), 7)
    assert lay.fields() == dict(n_topk=2, k=[2, 5], n_ce=1, smooth=[0.0], cm=1, off_topk=0, off_ce=2, off_cm=3,
                                words=3 + 49)
    assert [(m.name, i) for m, i in lay.entries] == [
        ("sparse_top_k_categorical_accuracy", 0), ("top5", 1), ("sparse_categorical_crossentropy", 0),
        ("f1_score", None), ("fbeta_score", None), ("f1_micro", None), ("again", 0)]
    s = lay.struct()
    assert (s.n_topk, list(s.k), s.n_ce, list(s.smooth), s.cm, s.off_topk, s.off_ce, s.off_cm, s.words) == \
        (2, [2, 5, 0, 0], 1, [0.0, 0.0], 1, 0, 2, 3, 52)
    assert MT.metric_spec(MT.resolve(["accuracy"]), _sparse(), 7) is None
    with pytest.raises(ValueError, match="at most 4 different k"):
        MT.metric_spec(MT.resolve([KM.SparseTopKCategoricalAccuracy(k, name=f"t{k}") for k in range(1, 6)]), None, 7)
    ce = [KM.CategoricalCrossentropy(label_smoothing=e, name=f"c{i}") for i, e in enumerate((0.0, 0.1, 0.2))]
    assert MT.metric_spec(ce[:2], None, 7).smooth == [0.0, 0.1]
    with pytest.raises(ValueError, match="at most 2 different label_smoothing"):
        MT.metric_spec(ce, None, 7)


@pytest.mark.skipif(not N.hip_available(), reason="libtde_hip.so not built")
def test_metric_spec_size_matches_the_kernels():
    from tensorflow_distributed_example_amd.ops import metric_ops as OM
    out = (ctypes.c_longlong * 4)()
    assert N.hip().tde_metric_abi(out, 4) == 4
    assert list(out) == [ctypes.sizeof(OM.MetricSpec), OM.MAX_TOPK, OM.MAX_CE, OM.MAX_CM_CLASSES]
    assert (MT.MAX_TOPK, MT.MAX_CE, MT.MAX_CM_CLASSES) == (OM.MAX_TOPK, OM.MAX_CE, OM.MAX_CM_CLASSES)


# ------------------------------------------------------------------------------------ hand-computed examples
def _acc_by_hand(metrics, z, y, loss=None, classes=4):
    """The reference plan's accumulation of crafted logits, and the logs of them."""
    m = _mlp(metrics, loss=loss, classes=classes)
    plan = PG.make_plan(m, m._store, "cpu", len(y), len(y), m.optimizer, m.loss)
    assert plan.kind == "reference" and plan.metrics_ext.numel() == m._metric_names.layout.words
    zz, yy = torch.tensor(z, dtype=torch.float32), torch.tensor(y)
    plan._acc(zz, yy, LS.softmax_ce(zz, yy.long()))
    return plan, MT.logs_from(plan.all_metrics(), m._metric_names)


def test_top_k_by_hand():
    inf = float("inf")
    z = [[3.0, 1.0, 1.0, 0.0],    # y = 2: one class greater, tied with class 1 across the k = 2 boundary -> hit at 2
         [3.0, 1.0, 1.0, 0.0],    # y = 3: three greater -> miss at 2, hit at 4
         [0.5, 0.5, 0.5, 0.5],    # y = 1: all tied, none greater -> hit at 1
         [1.0, 2.0, 3.0, 4.0],    # y = 7: out of range -> never
         [1.0, inf, 0.0, 0.0],    # y = 1: l_y = +inf -> never (not finite)
         [1.0, -inf, 0.0, 0.0]]   # y = 1: l_y = -inf -> never, even at k >= C
    y = [2, 3, 1, 7, 1, 1]
    mets = [KM.SparseTopKCategoricalAccuracy(k, name=f"t{k}") for k in (1, 2, 4, 9)]
    plan, logs = _acc_by_hand(mets, z, y)
    assert plan.metrics_ext.tolist() == [1.0, 2.0, 3.0, 3.0]
    assert [logs[f"t{k}"] for k in (1, 2, 4, 9)] == [1 / 6, 2 / 6, 3 / 6, 3 / 6]
    assert MO.words(z, y, (1, 2, 4, 9))["topk"].tolist() == [1.0, 2.0, 3.0, 3.0]


def test_crossentropy_by_hand():
    ln = np.log
    z = [[0.0, 0.0, 0.0, 0.0], [ln(1.0), ln(2.0), ln(1.0), ln(4.0)], [0.0, 0.0, 0.0, 0.0]]
    y = [1, 3, 9]       # the last label is out of range: l_y := max
    mets = [KM.CategoricalCrossentropy(from_logits=True), KM.CategoricalCrossentropy(from_logits=True,
                                                                                    label_smoothing=0.5, name="sm")]
    plan, logs = _acc_by_hand(mets, z, y, loss=LS.CategoricalCrossentropy(from_logits=True))
    # row 0: lse = ln 4, nll = ln 4, lse - mean = ln 4; row 1: lse = ln 8, nll = ln 2, mean l = ln(8) / 4
    plain = (ln(4.0) + ln(2.0) + ln(4.0)) / 3
    smooth = (ln(4.0) + (0.5 * ln(2.0) + 0.5 * (ln(8.0) - ln(8.0) / 4)) + ln(4.0)) / 3
    assert logs["categorical_crossentropy"] == pytest.approx(plain, rel=1e-6)
    assert logs["sm"] == pytest.approx(smooth, rel=1e-6)
    w = MO.words(z, y, (), (0.0, 0.5))
    assert w["ce"][0] / 3 == pytest.approx(plain, rel=1e-12) and w["ce"][1] / 3 == pytest.approx(smooth, rel=1e-12)


def test_f_score_by_hand():
    # predictions (lowest-index argmax): 0, 0, 1, 1, 2, 0 (a tie at the maximum goes to class 0), label 5 is left out
    z = [[2.0, 1, 0, 0], [2.0, 1, 0, 0], [0.0, 2, 1, 0], [0.0, 2, 1, 0], [0.0, 0, 2, 1], [1.0, 0, 1, 0], [0.0, 0, 0, 1]]
    y = [0, 1, 1, 1, 2, 2, 5]
    mets = [KM.F1Score(average="micro", name="mi"), KM.F1Score(average="macro", name="ma"),
            KM.F1Score(average="weighted", name="we"), KM.FBetaScore(average="macro", beta=2.0, name="b2")]
    plan, logs = _acc_by_hand(mets, z, y)
    cm = plan.metrics_ext.view(4, 4).tolist()
    assert cm == [[1, 0, 0, 0], [1, 2, 0, 0], [1, 0, 1, 0], [0, 0, 0, 0]]
    e = 1e-7
    # class 0: tp 1 fp 2 fn 0; class 1: tp 2 fp 0 fn 1; class 2: tp 1 fp 0 fn 1; class 3: nothing
    def f(tp, fp, fn, b=1.0):
        p, r = tp / (tp + fp + e), tp / (tp + fn + e)
        return (1 + b * b) * p * r / (b * b * p + r + e)
    fc = [f(1, 2, 0), f(2, 0, 1), f(1, 0, 1), f(0, 0, 0)]
    assert logs["mi"] == pytest.approx(f(4, 2, 2), rel=1e-12)
    assert logs["ma"] == pytest.approx(sum(fc) / 4, rel=1e-12)
    assert logs["we"] == pytest.approx((fc[0] * 1 + fc[1] * 3 + fc[2] * 2) / 6, rel=1e-12)
    assert logs["b2"] == pytest.approx((f(1, 2, 0, 2) + f(2, 0, 1, 2) + f(1, 0, 1, 2) + 0.0) / 4, rel=1e-12)
    w = MO.words(z, y, cm=True)
    assert w["cm"].tolist() == cm
    assert [MO.fbeta(w["cm"], 1.0, a) for a in ("micro", "macro", "weighted")] == \
        pytest.approx([logs["mi"], logs["ma"], logs["we"]], rel=1e-12)


# ------------------------------------------------------------------------------------ the reference plan
def _data(n, seed, classes=10):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, 12)).astype(np.float32), rng.integers(0, classes, n)


def _assert_logs(got, want, w, n, tag):
    for name, v in want.items():
        print(f"[{tag}] {name}: {got[name]!r} float64 {v!r}")
        # counts are exact unless a float32 row sits on a float64 boundary (none at these seeds); sums and the
        # F-score's 1e-7 terms in float64 from float32 rows: the loss' own bound in tests/test_loss_head.py
        assert got[name] == pytest.approx(v, rel=4e-6), name


def test_fit_evaluate_and_validation_against_the_oracle():
    m = _mlp(_all_metrics(), opt=OP.SGD(0.0))       # lr 0: one set of weights for every batch
    x, y = _data(3 * B + 3, 5)                      # a ragged last batch of 3 rows
    vx, vy = _data(2 * B, 6)
    h = m.fit(x, y, batch_size=B, epochs=2, verbose=0, shuffle=False, validation_data=(vx, vy))
    want, w = _want(m, _logits64(m, x), y)
    vwant, _ = _want(m, _logits64(m, vx), vy)
    names = ["accuracy", "sparse_top_k_categorical_accuracy", "top5", "sparse_categorical_crossentropy", "f1_score",
             "fbeta_score", "f1_micro"]
    assert list(h.history) == ["loss"] + names + ["val_loss"] + ["val_" + n for n in names]
    for ep in range(2):          # the accumulators are reset between the epochs
        _assert_logs({k: v[ep] for k, v in h.history.items()}, want, w, len(y), f"fit epoch {ep}")
        _assert_logs({k[4:]: v[ep] for k, v in h.history.items() if k.startswith("val_")}, vwant, w, len(vy), "val")
    ev = m.evaluate(x, y, batch_size=B, verbose=0)
    evd = m.evaluate(x, y, batch_size=B, verbose=0, return_dict=True)
    assert list(evd) == ["loss"] + names and ev == [evd[k] for k in evd]
    _assert_logs(evd, want, w, len(y), "evaluate")
    assert 0 < want["sparse_top_k_categorical_accuracy"] < want["top5"] < 1 and 0 < want["f1_score"] < 1
    # without smoothing, weights or a penalty the crossentropy metric is the loss
    assert evd["sparse_categorical_crossentropy"] == pytest.approx(evd["loss"], rel=1e-6)


def test_progbar_prints_every_name(capsys):
    m = _mlp(["accuracy", KM.SparseTopKCategoricalAccuracy(2), KM.F1Score(average="macro")])
    x, y = _data(2 * B, 4)
    m.fit(x, y, batch_size=B, epochs=1, verbose=2)
    out = capsys.readouterr().out
    assert "sparse_top_k_categorical_accuracy" in out and "f1_score" in out and "accuracy" in out


def test_the_crossentropy_metric_leaves_the_penalty_out():
    reg = tde.keras.regularizers.l2(0.05)
    m = _mlp([KM.SparseCategoricalCrossentropy(from_logits=True)], opt=OP.SGD(0.0), reg=reg)
    x, y = _data(2 * B, 7)
    ev = m.evaluate(x, y, batch_size=B, verbose=0, return_dict=True)
    want, _ = _want(m, _logits64(m, x), y)
    pen = 0.05 * float((torch.as_tensor(m.get_weights()[0]).double() ** 2).sum())
    assert ev["sparse_categorical_crossentropy"] == pytest.approx(want["sparse_categorical_crossentropy"], rel=4e-6)
    assert pen > 1e-2 and ev["loss"] == pytest.approx(ev["sparse_categorical_crossentropy"] + pen, rel=1e-5)


def test_categorical_forms_and_a_softmax_head_rank_the_logits():
    mets = ["categorical_accuracy", KM.TopKCategoricalAccuracy(k=3),
            KM.CategoricalCrossentropy(label_smoothing=0.1), KM.F1Score(average="weighted")]
    m = _mlp(mets, loss=LS.CategoricalCrossentropy(label_smoothing=0.1), opt=OP.SGD(0.0), softmax=True)
    x, y = _data(2 * B + 1, 8)
    ev = m.evaluate(x, np.eye(10, dtype=np.float32)[y], batch_size=B, verbose=0, return_dict=True)
    want, w = _want(m, _logits64(m, x), y)
    _assert_logs(ev, want, w, len(y), "categorical")
    assert ev["categorical_crossentropy"] == pytest.approx(ev["loss"], rel=1e-6)   # the same smoothing


def test_two_mirrored_cpu_replicas_equal_one_at_the_same_global_batch():
    x, y = _data(4 * B, 9)

    def run(strategy, w0=None):
        with strategy.scope():
            m = _mlp(_all_metrics(), opt=OP.SGD(0.1), w0=w0)
        start = m.get_weights()
        ds = tde.data.Dataset.from_tensor_slices((x, y)).batch(2 * B)
        h = m.fit(ds, epochs=2, verbose=0)
        return m, start, h.history

    m2, w0, h2 = run(tde.distribute.MirroredStrategy(["cpu", "cpu"]))
    prog = m2._program("train", 2 * B)
    assert len(prog.plans) == 2 and all(p.metrics_ext is not None for p in prog.plans)
    assert prog.global_metrics().numel() == 4 + m2._metric_names.layout.words
    tde.backend.clear_session()
    m1, _, h1 = run(tde.distribute.OneDeviceStrategy("cpu"), w0)
    for k in h1:
        # counts: equal; sums: the tolerance of tests/test_loss_head.py's Mirrored test
        assert h2[k] == pytest.approx(h1[k], rel=1e-5), k
    for k in ("sparse_top_k_categorical_accuracy", "top5", "accuracy", "f1_micro"):
        assert h2[k] == h1[k]


def test_cpu_matchers_decline_extra_metrics_with_a_warning_naming_them():
    m = tde.zoo.mnist_cnn()
    m.compile(loss=_sparse(), optimizer="sgd", metrics=["accuracy", KM.SparseTopKCategoricalAccuracy(5)])
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        assert PG.match_convnet(m, m.loss) is None
    assert len(rec) == 1 and "sparse_top_k_categorical_accuracy" in str(rec[0].message) \
        and "per-layer kernel plan" in str(rec[0].message)
    m.compile(loss=_sparse(), optimizer="sgd", metrics=["accuracy"])
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        assert PG.match_convnet(m, m.loss) is not None
    assert not rec
