"""The softmax-CE head with label smoothing and class weights on the GPU (csrc/include/tde_loss.h,
csrc/kernels/losshead.hip, smallnet_step_loss_kernel):

1. the kernel alone against the float64 oracle of tests/loss_head_oracle.py at its shapes, f32 and bf16 dlogits,
   one label out of range; with smoothing 0 and all-ones weights bitwise the plain xent32 / xent launch;
2. three steps of the small-net plan ("local" and "plain", hipGraph and eager) and of the layer-wise plan (f32 and
   bf16) against the float64 trajectory; the trivial categorical spec bitwise the sparse loss; which plan
   zoo.mnist_cnn gets; a second fit with other class weights on the same program; evaluate;
3. two Mirrored replicas in a child process.

``-s`` prints every figure before it is asserted.
"""
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
import smallnet_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
bf = torch.bfloat16


def _tde():
    import tensorflow_distributed_example_amd as tde
    from tensorflow_distributed_example_amd.train import program as PG
    return tde, PG


def _rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


# ------------------------------------------------------------------------------------- 1. the kernel alone
def _kernel_inputs(B, C, weights, seed):
    rng = np.random.default_rng(seed)
    logits = torch.from_numpy((rng.standard_normal((B, C)) * 3).astype(np.float32))
    y = rng.integers(0, C, B).astype(np.int32)
    y[0] = int(logits[0].argmax())                  # a correct row
    if B > 1:
        y[B - 1] = C + 3                            # one label out of range
    if B > 2:
        y[1] = 0                                    # the zero of the "zero" table is hit
    # one or two rows: the zero sits at a class no row has, the loss sum stays positive
    return logits, torch.from_numpy(y), H.kernel_weights(weights, C, rng, zero_at=0 if B > 2 else (int(y[0]) + 1) % C)


def _launch(logits, y, B, C, smooth, w, dtype, scale=0.5):
    from tensorflow_distributed_example_amd.ops import loss_ops as OL
    lg, yy = logits.to(DEV), y.to(DEV)
    cw = None if w is None else torch.from_numpy(w).to(DEV)
    dl = torch.full((B, C), 7.0, dtype=dtype, device=DEV)
    met = torch.zeros(4, device=DEV)
    it = torch.zeros(1, dtype=torch.int64, device=DEV)
    OL.xent_spec(lg, yy, B, C, smooth=smooth, class_w=cw, scale=scale, dlogits=dl, metrics=met, iterations=it)
    probs, copy = torch.zeros(B, C, device=DEV), torch.zeros(B, C, device=DEV)
    OL.xent_spec(lg, yy, B, C, smooth=smooth, class_w=cw, probs=probs, bf16=dtype == bf)
    OL.xent_spec(lg, yy, B, C, smooth=smooth, class_w=cw, probs=copy, probs_are_logits=True, bf16=dtype == bf)
    torch.cuda.synchronize()
    return dl.cpu(), met.cpu(), int(it.item()), probs.cpu(), copy.cpu()


def _plain(logits, y, B, C, dtype, scale=0.5):
    from tensorflow_distributed_example_amd.ops import layer_ops as OB
    from tensorflow_distributed_example_amd.ops import layer_ops32 as O32
    ops = O32 if dtype == torch.float32 else OB
    lg, yy = logits.to(DEV), y.to(DEV)
    dl = torch.full((B, C), 7.0, dtype=dtype, device=DEV)
    met = torch.zeros(4, device=DEV)
    it = torch.zeros(1, dtype=torch.int64, device=DEV)
    ops.xent(lg, yy, B, C, scale=scale, dlogits=dl, metrics=met, iterations=it)
    probs = torch.zeros(B, C, device=DEV)
    ops.xent(lg, yy, B, C, probs=probs)
    torch.cuda.synchronize()
    return dl.cpu(), met.cpu(), int(it.item()), probs.cpu()


@pytest.mark.parametrize("dtype", [torch.float32, bf], ids=["f32", "bf16"])
@pytest.mark.parametrize("weights", H.WEIGHTS)
@pytest.mark.parametrize("smooth", H.SMOOTH)
@pytest.mark.parametrize("shape", H.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_against_float64(shape, smooth, weights, dtype):
    B, C = shape
    logits, y, w = _kernel_inputs(B, C, weights, 100 + B)
    want = H.head(logits, y, smooth, w, scale=0.5)
    dl, met, it, probs, copy = _launch(logits, y, B, C, smooth, w, dtype)
    loss = float(want["loss"].sum())
    # the bounds of the plain kernels: tests/test_layers_f32_gpu.py::test_gap_pad_xent32 (loss 1e-5, dlogits 1e-6) and
    # tests/test_layers_gpu.py::test_gap_pad_xent (loss 1e-3, dlogits 1e-2, probabilities 1e-5), or twice the plain
    # kernel's own error on these inputs where that is more (the variant adds one C-term sum and three roundings per
    # row; at 1 x 2 the one row's p - 1 cancels and the plain kernel itself misses 1e-6)
    pl_dl, pl_met, _, _ = _plain(logits, y, B, C, dtype)
    pl_want = H.head(logits, y, 0.0, None, scale=0.5)
    pl_el = abs(pl_met[0].item() - float(pl_want["loss"].sum())) / float(pl_want["loss"].sum())
    pl_ed = _rel(pl_dl.float(), pl_want["dlogits"])
    tl, td = (1e-5, 1e-6) if dtype == torch.float32 else (1e-3, 1e-2)
    tl, td = max(tl, 2 * pl_el), max(td, 2 * pl_ed)
    el, ed, ep = abs(met[0].item() - loss) / loss, _rel(dl.float(), want["dlogits"]), _rel(probs, want["probs"])
    print(f"[{B}x{C} e={smooth} w={weights} {dtype}] loss err {el:.3g} (plain {pl_el:.3g}) dlogits err {ed:.3g} "
          f"(plain {pl_ed:.3g}) probs err {ep:.3g}")
    assert met[2].item() == B and met[1].item() == want["correct"] and met[3].item() == 0 and it == 1
    assert want["correct"] >= 1 and loss > 0
    assert el <= tl and ed <= td and ep <= 1e-5
    assert torch.equal(copy, logits)
    if weights == "zero" and B > 2:                  # a zero-weight row: no loss, no gradient
        assert float(want["w"][1]) == 0.0 and dl[1].float().abs().max().item() == 0.0


@pytest.mark.parametrize("dtype", [torch.float32, bf], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", H.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_trivial_spec_is_the_plain_kernel_bitwise(shape, dtype):
    B, C = shape
    logits, y, _ = _kernel_inputs(B, C, "none", 200 + B)
    ones = np.ones(C, dtype=np.float32)
    pl_dl, pl_met, pl_it, pl_probs = _plain(logits, y, B, C, dtype)
    for w in (ones, None):
        dl, met, it, probs, _ = _launch(logits, y, B, C, 0.0, w, dtype)
        idt = torch.int32 if dtype == torch.float32 else torch.int16
        assert torch.equal(dl.view(idt), pl_dl.view(idt)) and torch.equal(probs.view(torch.int32), pl_probs.view(torch.int32))
        assert it == pl_it == 1 and met[1:].tolist() == pl_met[1:].tolist()
        if B <= 4:      # one workgroup: its one atomic add is the whole sum
            assert torch.equal(met.view(torch.int32), pl_met.view(torch.int32))
        else:
            assert abs(met[0].item() - pl_met[0].item()) <= 1e-6 * pl_met[0].item()


def test_wrapper_checks_its_arguments():
    from tensorflow_distributed_example_amd.ops import loss_ops as OL
    lg = torch.zeros(4, 5, device=DEV)
    y = torch.zeros(4, dtype=torch.int32, device=DEV)
    for kw in (dict(smooth=1.0), dict(smooth=-0.1), dict(smooth=float("nan")), dict(class_w=torch.ones(4, device=DEV)),
               dict(class_w=torch.ones(5, dtype=torch.float64, device=DEV)), dict(dlogits=torch.zeros(4, 4, device=DEV)),
               dict(dlogits=torch.zeros(4, 5, dtype=torch.float16, device=DEV)), dict(probs=torch.zeros(19, device=DEV)),
               dict(class_w=torch.ones(5))):
        with pytest.raises(ValueError):
            OL.xent_spec(lg, y, 4, 5, **kw)
    with pytest.raises(ValueError):
        OL.xent_spec(lg, y.long(), 4, 5)
    with pytest.raises(ValueError):
        OL.xent_spec(lg, y, 5, 5)
    from tensorflow_distributed_example_amd import _native as N
    assert N.hip().tde_xent_spec(lg.data_ptr(), 5, y.data_ptr(), 4, 5, 1.0, None, 5, 0, None, None, 0, None, 1.0, None,
                                 N.stream_ptr()) == -1
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------- 2. the plans
BP = 8


def _loss(tde, smooth, categorical=True):
    if categorical:
        return tde.losses.CategoricalCrossentropy(from_logits=True, label_smoothing=smooth)
    return tde.losses.SparseCategoricalCrossentropy(from_logits=True)


def _model(tde, name):
    L = tde.keras.layers
    if name == "mlp":
        return tde.zoo.mnist_mlp()
    if name == "conv":      # Conv2D · MaxPooling2D · Flatten · Dense: the small-net plan's, no fused-CNN pattern
        return tde.keras.Sequential([L.Conv2D(4, 3, activation="relu", input_shape=(10, 10, 2)), L.MaxPooling2D(2),
                                     L.Flatten(), L.Dense(10)])
    if name == "convdense":  # the layer-wise plan's tiny Conv · Dense
        return tde.keras.Sequential([L.Conv2D(8, 3, activation="relu", input_shape=(8, 8, 3)), L.Flatten(),
                                     L.Dense(10, name="fc")])
    raise KeyError(name)


def _build(tde, name, loss, opt=None, w0=None):
    m = _model(tde, name)
    m.compile(loss=loss, optimizer=opt or tde.optimizers.SGD(0.05, momentum=0.5), metrics=["accuracy"])
    m.build()
    if w0 is not None:
        m.set_weights(w0)
    return m


def _reference_errors(tde, PG, name, loss, w_init, batches, cw, want, w0):
    """The float32 torch reference plan on the CPU against the oracle, per variable (what smallnet_oracle.bound
    scales the plan suites' bound by)."""
    tde.backend.clear_session()
    m = _build(tde, name, loss, w0=w_init)
    st = m._store.clone_to("cpu")
    plan = PG.make_plan(m, st, "cpu", BP, BP, m.optimizer, m.loss, class_weight=cw is not None)
    if cw is not None:
        plan.set_class_weight(tde.losses.class_weight_table(cw, 10))
    for x, y in batches:
        plan.train_step(x, y)
        plan.apply()
    return {n: O.rel(st.view(k).detach().double() - w0[n], want[n] - w0[n]) for n, k in zip(want, st.names(trainable=True))}


def _check(tag, names, got, want, w0, bound):
    for n in names:
        e, b = O.rel(got[n] - w0[n], want[n] - w0[n]), bound(n)
        print(f"[{tag}] {n}: vs float64 {e:.3g} bound {b:.3g}")
        assert float((got[n] - w0[n]).abs().max()) > 0 and e <= b, (tag, n, e, b)


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("mode", ["local", "plain"])
@pytest.mark.parametrize("case", list(H.CASES))
@pytest.mark.parametrize("name", ["mlp", "conv"])
def test_smallnet_plan_against_float64(name, case, mode, graph, monkeypatch):
    tde, PG = _tde()
    smooth, cw = H.CASES[case]
    monkeypatch.setenv("TDE_FUSED_STEP", "1" if mode == "local" else "0")
    monkeypatch.setenv("TDE_GRAPH", "1" if graph else "0")
    tde.backend.clear_session()
    tde.backend.set_random_seed(21)
    loss = _loss(tde, smooth, categorical=case != "class_weight")
    m = _build(tde, name, loss)
    st = m._store
    w_init = m.get_weights()
    names = st.names(trainable=True)
    w0 = {n: st.view(n).detach().cpu().double().clone() for n in names}
    batches = H.batches(m, BP, 3, 60)
    want, want_loss = H.trajectory(m, batches, m.optimizer, smooth, cw)
    prog = m._program("train", BP, class_weight=cw is not None)
    plan = prog.plans[0]
    assert plan.kind == "fused_smallnet" and plan.step_mode == mode and prog.use_graph == graph and plan.loss_spec
    if cw is not None:
        prog.set_class_weight(tde.losses.class_weight_table(cw, 10))
    losses = []
    for x, y in batches:
        prog.reset_metrics()
        prog.stage([(x[None].to(DEV), y[None].to(DEV))])
        prog.run()
        prog.sync()
        mt = prog.global_metrics()
        assert mt[2].item() == BP
        losses.append(float(mt[0] / mt[2]))
    assert plan.iterations.item() == 3 and (prog.graph is not None) == graph
    got = {n: st.view(n).detach().cpu().double() for n in names}
    ref = _reference_errors(tde, PG, name, loss, w_init, batches, cw, want, w0)
    _check(f"{name} {case} {mode}", names, got, want, w0, lambda n: O.bound(ref[n]))
    for k, (a, b) in enumerate(zip(losses, want_loss)):
        print(f"[{name} {case} {mode}] step {k}: loss {a!r} float64 {b!r}")
        assert abs(a - b) <= 1e-5 * abs(b), (k, a, b)


@pytest.mark.parametrize("mode", ["local", "plain"])
def test_smallnet_categorical_without_smoothing_is_the_sparse_loss_bitwise(mode, monkeypatch):
    tde, _ = _tde()
    monkeypatch.setenv("TDE_FUSED_STEP", "1" if mode == "local" else "0")
    rng = np.random.default_rng(5)
    x = rng.standard_normal((3 * BP, 28, 28, 1)).astype(np.float32)
    yi = rng.integers(0, 10, 3 * BP)
    out = []
    w0 = None
    for categorical in (False, True):
        tde.backend.clear_session()
        tde.backend.set_random_seed(3)
        m = _build(tde, "mlp", _loss(tde, 0.0, categorical), w0=w0)
        w0 = w0 or m.get_weights()
        y = H.onehot(yi, 10) if categorical else yi
        h = m.fit(x, y, batch_size=BP, epochs=2, verbose=0, shuffle=False)
        ev = m.evaluate(x, y, batch_size=BP, verbose=0)
        plan = m._program("train", BP).plans[0]
        assert plan.kind == "fused_smallnet" and plan.step_mode == mode and not plan.loss_spec and m._device_feed
        out.append((h.history, ev, m.get_weights()))
    assert out[0][0] == out[1][0] and out[0][1] == out[1][1]
    assert all(np.array_equal(a, b) for a, b in zip(out[0][2], out[1][2]))


@pytest.mark.parametrize("policy", ["float32", "mixed_bfloat16"])
def test_layerwise_plan_against_float64(policy):
    tde, PG = _tde()
    from tensorflow_distributed_example_amd.train.layerwise import LayerwisePlan
    smooth, cw = H.CASES["both"]
    tde.keras.mixed_precision.set_global_policy(policy)
    try:
        tde.backend.clear_session()
        tde.backend.set_random_seed(22)
        loss = _loss(tde, smooth)
        m = _build(tde, "convdense", loss)
        st = m._store
        w_init = m.get_weights()
        names = st.names(trainable=True)
        w0 = {n: st.view(n).detach().cpu().double().clone() for n in names}
        batches = H.batches(m, BP, 3, 61)
        want, want_loss = H.trajectory(m, batches, m.optimizer, smooth, cw)
        plan = PG.make_plan(m, st, DEV, BP, BP, m.optimizer, m.loss, prefer="layerwise", class_weight=True)
        assert isinstance(plan, LayerwisePlan) and plan.loss_spec and not plan.stages[-1].fused
        assert plan.compute_dtype == ("fp32" if policy == "float32" else "bf16")
        plan.set_class_weight(tde.losses.class_weight_table(cw, 10))
        losses = []
        for x, y in batches:
            plan.reset_metrics()
            plan.train_step(x.to(DEV, plan.input_dtype).contiguous(), y.to(DEV), BP)
            plan.apply()
            torch.cuda.synchronize()
            mt = plan.metrics.cpu().double()
            assert mt[2].item() == BP
            losses.append(float(mt[0] / mt[2]))
        got = {n: st.view(n).detach().cpu().double() for n in names}
        # the evaluation of the same plan: the smoothing, no weights; predict: probabilities of the logits model
        xe, ye = batches[0]
        plan.reset_metrics()
        plan.eval_step(xe.to(DEV, plan.input_dtype).contiguous(), ye.to(DEV), BP)
        torch.cuda.synchronize()
        ev = float(plan.metrics[0] / plan.metrics[2])
        ev_want = H.eval_loss(m, xe, ye, smooth)
        if policy == "float32":
            ref = _reference_errors(tde, PG, "convdense", loss, w_init, batches, cw, want, w0)
            bound, tl = (lambda n: O.bound(ref[n])), 1e-5
        else:   # the bounds of tests/test_weight_reg_gpu.py / tests/test_layers_gpu.py under bf16 activations
            bound, tl = (lambda n: 0.05 if n.startswith("fc/") else 0.5), 6e-2
        _check(f"layerwise {policy}", names, got, want, w0, bound)
        for k, (a, b) in enumerate(zip(losses, want_loss)):
            print(f"[layerwise {policy}] step {k}: loss {a!r} float64 {b!r}")
            assert abs(a - b) <= tl * abs(b), (k, a, b)
        print(f"[layerwise {policy}] evaluate {ev!r} float64 {ev_want!r}")
        assert abs(ev - ev_want) <= tl * ev_want
    finally:
        tde.keras.mixed_precision.set_global_policy("float32")


def test_mnist_cnn_falls_to_the_layerwise_plan_with_one_warning_and_stays_fused_when_trivial():
    tde, PG = _tde()
    from tensorflow_distributed_example_amd.train.layerwise import LayerwisePlan
    tde.backend.clear_session()
    m = tde.zoo.mnist_cnn()
    m.compile(loss=_loss(tde, 0.1), optimizer=tde.optimizers.SGD(0.01), metrics=["accuracy"])
    with pytest.warns(UserWarning, match="no loss head for CategoricalCrossentropy\\(label_smoothing=0.1\\)") as rec:
        plan = PG.make_plan(m, m._store, DEV, BP, BP, m.optimizer, m.loss)
    assert isinstance(plan, LayerwisePlan) and plan.loss_spec and len([w for w in rec if "loss head" in str(w.message)]) == 1
    rng = np.random.default_rng(1)
    x = torch.from_numpy(rng.random((BP, 28, 28, 1), dtype=np.float32))
    y = torch.from_numpy(rng.integers(0, 10, BP).astype(np.int32))
    plan.train_step(x.to(DEV, plan.input_dtype).contiguous(), y.to(DEV), BP)
    torch.cuda.synchronize()
    got = float(plan.metrics[0] / plan.metrics[2])
    want = H.eval_loss(m, x, y, 0.1)
    assert abs(got - want) <= (1e-5 if plan.f32 else 6e-2) * want
    tde.backend.clear_session()
    m = tde.zoo.mnist_cnn()
    m.compile(loss=_loss(tde, 0.0), optimizer=tde.optimizers.SGD(0.01), metrics=["categorical_accuracy"])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        plan = PG.make_plan(m, m._store, DEV, BP, BP, m.optimizer, m.loss)
    assert plan.kind == "fused_convnet" and not plan.loss_spec
    with pytest.warns(UserWarning, match="no loss head for fit\\(class_weight=\\)"):
        plan = PG.make_plan(m, m._store, DEV, BP, BP, m.optimizer, m.loss, class_weight=True)
    assert isinstance(plan, LayerwisePlan) and plan.class_w is not None


def test_a_second_fit_with_other_class_weights_replays_the_same_graph_and_evaluate_smooths():
    tde, _ = _tde()
    tde.backend.clear_session()
    tde.backend.set_random_seed(23)
    smooth = 0.1
    m = _build(tde, "mlp", _loss(tde, smooth), opt=tde.optimizers.SGD(0.05))
    b1, b2 = H.batches(m, BP, 1, 70), H.batches(m, BP, 1, 71)
    cw1, cw2 = {0: 2.0, 2: 0.0, 7: 0.5}, {0: 0.25, 2: 3.0}
    fit = lambda b, cw: m.fit(b[0][0].numpy(), H.onehot(b[0][1].numpy(), 10), batch_size=BP, epochs=1, verbose=0,  # noqa: E731
                              shuffle=False, class_weight=cw).history["loss"][0]
    w0 = {n: m._store.view(n).detach().cpu().double().clone() for n in m._store.names(trainable=True)}
    want1, (l1,) = H.trajectory(m, b1, m.optimizer, smooth, cw1)
    got1 = fit(b1, cw1)
    prog = m._program("train", BP, class_weight=True)
    graphs = dict(prog.graphs)
    assert prog.use_graph and len(graphs) >= 1 and prog.plan_kind == "fused_smallnet"
    want2, (l2,) = H.trajectory(m, b2, m.optimizer, smooth, cw2)      # from the weights the first fit left
    mid = {n: m._store.view(n).detach().cpu().double().clone() for n in want2}
    got2 = fit(b2, cw2)
    assert m._program("train", BP, class_weight=True) is prog
    assert dict(prog.graphs) == graphs and all(prog.graphs[k][0] is graphs[k][0] for k in graphs)   # no re-capture
    assert prog.plans[0].class_w.cpu().tolist() == tde.losses.class_weight_table(cw2, 10).tolist()
    print(f"fit 1 {got1!r} float64 {l1!r}; fit 2 {got2!r} float64 {l2!r}")
    assert abs(got1 - l1) <= 1e-5 * l1 and abs(got2 - l2) <= 1e-5 * l2
    names = list(want2)
    got = {n: m._store.view(n).detach().cpu().double() for n in names}
    for n in names:     # the first step ended where float64 ends, the second step's change against float64
        assert O.rel(mid[n] - w0[n], want1[n] - w0[n]) <= 1e-4
        e = O.rel(got[n] - mid[n], want2[n] - mid[n])
        print(f"[second fit] {n}: {e:.3g}")
        assert e <= 1e-4, (n, e)
    assert max(float((got[n] - w0[n]).abs().max()) for n in names) > 0
    # evaluate: the smoothing, not the weights
    x, y = b1[0]
    ev = m.evaluate(x.numpy(), H.onehot(y.numpy(), 10), batch_size=BP, verbose=0, return_dict=True)
    want_ev = H.eval_loss(m, x, y, smooth)
    assert m._program("eval", BP).plans[0].loss_spec and m._program("eval", BP).plans[0].class_w is None
    print(f"evaluate {ev['loss']!r} float64 {want_ev!r} (unsmoothed {H.eval_loss(m, x, y, 0.0)!r})")
    assert abs(ev["loss"] - want_ev) <= 1e-5 * want_ev and abs(want_ev - H.eval_loss(m, x, y, 0.0)) > 1e-3
    assert ev["accuracy"] == float((m.predict(x.numpy()).argmax(axis=1) == y.numpy()).mean())


# ------------------------------------------------------------------------------------- 3. mirrored
CHILD_TIMEOUT = 90


def test_mirrored_replicas_equal_one_replica():
    """Two Mirrored replicas rehearsed on cuda:0 and, in the same child, one replica at the same global batch,
    within the tolerance of tests/test_mirrored_gpu.py (rtol 1e-4, atol 1e-5); scale = 1 / global batch."""
    env = dict(os.environ, TDE_HEARTBEAT="0", OMP_NUM_THREADS="2", TDE_XGMI_TIMEOUT="20")
    p = subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "loss_head_mirrored_child.py")], env=env, cwd=ROOT,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, start_new_session=True)
    try:
        out, _ = p.communicate(timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        os.killpg(p.pid, signal.SIGKILL)
        out, _ = p.communicate()
        raise AssertionError(f"timed out:\n{out[-3000:]}")
    assert p.returncode == 0, out[-4000:]
    res = json.loads([l for l in out.splitlines() if l.startswith("RESULT ")][0][7:])
    print(res)
    assert res["plan"] == "fused_smallnet" and res["loss_spec"] == [True, True] and res["iterations"] == [3, 3], res
    assert res["w_identical"] and res["tables_identical"] and res["w_moved"] > 0, res
    assert res["worst_excess"] <= 0.0, res
    for two, one, want in zip(res["losses"], res["one_losses"], res["want_losses"]):
        assert abs(two - one) <= 1e-5 * one and abs(one - want) <= 1e-5 * want, res
