"""Model B (mnist_keras_distributed.py:79-109) on the fused float32 BN-CNN plan (csrc/kernels/bncnn.hip)
vs float64 autograd oracles: every gradient <= 1e-5 relative (norm-wise), BN moving statistics, the
loss / accuracy metrics, evaluation with moving statistics and prediction.

The oracle (tests/bncnn_oracle.py, shared with the family suite tests/test_bncnn_family_gpu.py) takes each ReLU
decision from the plan's own f32 pre-activations (its stored raw conv / dense outputs and saved batch
statistics): a pre-activation within one f32 ulp of zero may be decided differently in f64, and a flipped ReLU
moves a whole gradient element; everything else is f64."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from bncnn_cases import model_b as _model_b, model_b_data
from bncnn_oracle import plan_oracle as _oracle, rel as _rel

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("fp32_policy")]

DEV = "cuda"


def _data(B, seed):
    return model_b_data(B, seed, DEV)


@pytest.mark.parametrize("B", [128, 50])
def test_bncnn_step_gradients_match_float64(B):
    import tensorflow_distributed_example_amd as tde
    from tensorflow_distributed_example_amd.train import program as PG
    m = _model_b(tde)
    st = m._store
    plan = PG.make_plan(m, st, DEV, 128, 128, m.optimizer, m.loss)
    assert plan.kind == "fused_bncnn" and plan.compute_dtype == "fp32"
    before = {n: st.view(n).detach().double().clone() for n in st.order}
    x, y = _data(128, 11)
    plan.train_step(x, y, B)
    torch.cuda.synchronize()
    # the oracle from the pre-step weights / moving statistics
    after = {n: st.view(n).detach().clone() for n in st.order}
    for n in st.order:
        st.view(n).copy_(before[n])
    grads, moving, loss, _ = _oracle(plan, x, y, B)
    for n in st.order:
        st.view(n).copy_(after[n])
    for n, gr in grads.items():
        assert _rel(st.grad(n), gr) < 1e-5, (n, _rel(st.grad(n), gr))
    for n, v in moving.items():
        assert _rel(st.view(n), v) < 1e-6, (n, _rel(st.view(n), v))
    met = plan.metrics.double().cpu()
    assert met[2].item() == B and abs(met[0].item() / B - loss) < 1e-5 * abs(loss)


def test_bncnn_later_steps_gradients_match_float64():
    """Steps 2 and 3 (after optimizer updates): every statistics partial is rewritten by its producer
    each step (no memset, no atomics), so a later step must match the float64 oracle like the first."""
    import tensorflow_distributed_example_amd as tde
    from tensorflow_distributed_example_amd.train import program as PG
    m = _model_b(tde)
    st = m._store
    plan = PG.make_plan(m, st, DEV, 128, 128, m.optimizer, m.loss)
    for step in range(3):
        x, y = _data(128, 20 + step)
        before = {n: st.view(n).detach().double().clone() for n in st.order}
        plan.train_step(x, y)
        torch.cuda.synchronize()
        after = {n: st.view(n).detach().clone() for n in st.order}
        for n in st.order:
            st.view(n).copy_(before[n])
        grads, moving, _, _ = _oracle(plan, x, y, 128)
        for n in st.order:
            st.view(n).copy_(after[n])
        for n, gr in grads.items():
            assert _rel(st.grad(n), gr) < 1e-5, (step, n, _rel(st.grad(n), gr))
        for n, v in moving.items():
            assert _rel(st.view(n), v) < 1e-6, (step, n, _rel(st.view(n), v))
        plan.apply()
        plan.iterations += 1
        torch.cuda.synchronize()


def test_bncnn_step_is_bitwise_deterministic():
    """Same weights, same batch -> bit-identical gradients and moving statistics: statistics travel as
    per-workgroup partials summed in a fixed order, the dense / logit partials likewise."""
    import tensorflow_distributed_example_amd as tde
    from tensorflow_distributed_example_amd.train import program as PG
    m = _model_b(tde)
    st = m._store
    plan = PG.make_plan(m, st, DEV, 128, 128, m.optimizer, m.loss)
    x, y = _data(128, 31)
    w0 = st.w.clone()
    runs = []
    for _ in range(3):
        st.w.copy_(w0)
        plan.train_step(x, y)
        torch.cuda.synchronize()
        runs.append((st.g.clone(), st.w.clone()))
    for g, w in runs[1:]:
        assert torch.equal(g, runs[0][0]) and torch.equal(w, runs[0][1])


def test_bncnn_eval_and_predict_use_moving_statistics():
    import tensorflow_distributed_example_amd as tde
    from tensorflow_distributed_example_amd.train import program as PG
    m = _model_b(tde)
    st = m._store
    g = torch.Generator(device="cpu").manual_seed(5)
    for n in st.order:
        if "moving" in n:
            v = st.view(n)
            v.copy_((torch.rand(v.shape, generator=g) + (0.5 if "variance" in n else -0.5)).to(v.device))
    plan = PG.make_plan(m, st, DEV, 64, 64, None, m.loss)
    x, y = _data(64, 12)
    probs = plan.predict(x, 64).clone()
    plan.eval_step(x, y, 64)
    torch.cuda.synchronize()
    m.layers  # noqa: B018
    ref = m(x.cpu().numpy())   # the torch reference forward (inference: moving statistics, no dropout)
    ref = (ref if torch.is_tensor(ref) else torch.as_tensor(np.asarray(ref))).to(DEV, torch.float64)
    assert _rel(probs, ref) < 1e-5, _rel(probs, ref)
    met = plan.metrics.double().cpu()
    want = F.nll_loss(torch.log(ref), y.long(), reduction="sum").item()
    assert abs(met[0].item() - want) < 1e-4 * abs(want) and met[2].item() == 64
    assert met[1].item() == (ref.argmax(1) == y.long()).sum().item()


def test_bncnn_fit_matches_reference_executor(monkeypatch):
    """fit() over 4 steps (hipGraph executions) on the fused plan vs the torch fp32 reference executor
    (dropout off so both are deterministic): same weights, moving statistics and loss to fp32 accuracy.

    Tolerance: two fp32 implementations may decide a ReLU whose pre-activation is within an ulp of zero
    differently (measured: one element in ~10^6, e.g. image 82 pixel (10, 14) channel 1 of the first
    BN's output); one such tie moves the first conv's 4-step update by ~2.5e-3 of its norm.  The exact
    per-step numerics are pinned at 1e-5 by the float64 oracle tests above, which share the plan's
    ReLU decisions."""
    import tensorflow_distributed_example_amd as tde
    rng = np.random.default_rng(0)
    x = rng.random((128 * 4, 784), dtype=np.float32)
    y = rng.integers(0, 10, 128 * 4)
    mf = _model_b(tde)
    w0 = mf.get_weights()
    hf = mf.fit(x, y, batch_size=128, epochs=1, shuffle=False, verbose=0)
    prog = mf._program("train", 128)
    assert prog.plan_kind == "fused_bncnn"
    tde.backend.clear_session()
    monkeypatch.setenv("TDE_EXECUTOR", "reference")
    mr = _model_b(tde)
    mr.set_weights(w0)
    hr = mr.fit(x, y, batch_size=128, epochs=1, shuffle=False, verbose=0)
    for name, a, b, w in zip(mf.variable_names(), mf.get_weights(), mr.get_weights(), w0):
        rel = np.linalg.norm(a - b) / (np.linalg.norm(b - w) + np.linalg.norm(b) * 1e-6 + 1e-12)
        assert rel < 1e-2, (name, rel)
    assert abs(hf.history["loss"][0] - hr.history["loss"][0]) < 1e-4


def test_bncnn_dropout_is_active_in_training_only():
    """Dropout(0.5) of Model B: training steps differ from the dropout-free step; evaluation without the
    forced learning phase is deterministic; set_learning_phase(1) (quirk Q4) keeps dropout and batch
    statistics in prediction (two predictions at different steps differ)."""
    import tensorflow_distributed_example_amd as tde
    from tensorflow_distributed_example_amd.train import program as PG
    m = _model_b(tde, rate=0.5)
    st = m._store
    plan = PG.make_plan(m, st, DEV, 128, 128, m.optimizer, m.loss)
    x, y = _data(128, 13)
    plan.train_step(x, y)
    g_drop = st.grad(f"{plan.head.name}/kernel").clone()
    st.g.zero_()
    plan.iterations += 1
    plan.train_step(x, y)
    g_drop2 = st.grad(f"{plan.head.name}/kernel").clone()
    torch.cuda.synchronize()
    assert torch.isfinite(g_drop).all() and not torch.equal(g_drop, g_drop2)   # new mask per step
    p1 = plan.predict(x, 128).clone()
    p2 = plan.predict(x, 128).clone()
    assert torch.equal(p1, p2)
    tde.backend.set_learning_phase(1)
    try:
        q1 = plan.predict(x, 128).clone()
        plan.iterations += 1
        q2 = plan.predict(x, 128).clone()
    finally:
        tde.backend.set_learning_phase(None)
    assert not torch.equal(q1, q2)


@pytest.mark.parametrize("kind", ["sgd", "momentum", "adam"])
def test_bncnn_fused_reduce_optimizer_matches_separate_launch(kind):
    """Step mode "local" (the optimizer applied inside the weight-gradient reduce launch, BN betas
    included) vs "plain" (bucket + the multi-tensor optimizer launch): 3 steps (dropout on, so the step
    counter that seeds the masks must advance identically) give bitwise-equal weights and slots."""
    import tensorflow_distributed_example_amd as tde
    from tensorflow_distributed_example_amd.train import program as PG
    opts = {"sgd": lambda: tde.optimizers.SGD(0.05), "momentum": lambda: tde.optimizers.SGD(0.05, momentum=0.9),
            "adam": lambda: tde.optimizers.Adam(1e-3)}
    res = {}
    for mode in ("plain", "local"):
        tde.backend.set_random_seed(11)
        m = _model_b(tde, rate=0.3, opt=opts[kind]())
        plan = PG.make_plan(m, m._store, DEV, 128, 128, m.optimizer, m.loss)
        assert plan.supports_step_mode("local")
        plan.set_step_mode(mode)
        for i in range(3):
            x, y = _data(128, 20 + i)
            plan.train_step(x, y)
            if mode == "plain":
                plan.apply()
        torch.cuda.synchronize()
        st = m._store
        res[mode] = (st.w.clone(), {k: v.clone() for k, v in st.slots.items()}, int(plan.iterations.item()))
    (wp, sp, ip), (wl, sl, il) = res["plain"], res["local"]
    assert ip == il == 3
    assert torch.equal(wp, wl), float((wp - wl).abs().max())
    for k in sp:
        assert torch.equal(sp[k], sl[k]), k


def test_bncnn_local_graph_picks_up_learning_rate_change(monkeypatch):
    """A hyper-parameter change between two hipGraph executions, step mode "local" against "plain"
    (TDE_FUSED_STEP=0): momentum SGD, batch 16, dropout on, two executions of two steps over the same data,
    the learning rate halved on both models in between.  The reduce launch's descriptor carries the rate by
    value, so the change has to go through ``refresh()``, the descriptor rebuild and the Program's recapture;
    a missed refresh applies the old rate for two steps.  After each execution weights and slots are bitwise
    equal, the bound of ``test_bncnn_fused_reduce_optimizer_matches_separate_launch``; the step counter ends
    at 4."""
    import tensorflow_distributed_example_amd as tde
    progs = []
    for mode in ("local", "plain"):
        if mode == "plain":
            monkeypatch.setenv("TDE_FUSED_STEP", "0")
        tde.backend.set_random_seed(11)
        m = _model_b(tde, rate=0.3, opt=tde.optimizers.SGD(0.05, momentum=0.9))
        m.steps_per_execution = 2
        prog = m._program("train", 16)
        assert prog.use_graph and prog.plan_kind == "fused_bncnn" and prog.plans[0].step_mode == mode
        progs.append((m, prog))
    (ml, pl), (mp, pp) = progs
    assert torch.equal(ml._store.w, mp._store.w)
    data = [_data(16, 40 + s) for s in range(2)]
    xs, ys = torch.stack([d[0] for d in data]), torch.stack([d[1] for d in data])
    for e in range(2):
        for prog in (pl, pp):
            prog.stage([(xs, ys)])
            prog.run()
            prog.sync()
        sl, sp = ml._store, mp._store
        print(f"execution {e}: local vs plain max |dw| {float((sl.w - sp.w).abs().max()):.3e}")
        assert torch.equal(sl.w, sp.w), (e, float((sl.w - sp.w).abs().max()))
        for k in sp.slots:
            assert torch.equal(sl.slots[k], sp.slots[k]), (e, k)
        ml.optimizer.learning_rate = mp.optimizer.learning_rate = 0.025
    assert int(pl.plans[0].iterations) == int(pp.plans[0].iterations) == 4


@pytest.mark.parametrize("B", [128, 50])
def test_bncnn_dropout_matches_float64_with_the_plan_mask(B):
    """Dropout(0.5) of Model B as the reference trains it (mnist_keras_distributed.py:106): the fused head's
    Philox keep mask (debug export, plan.dropout_mask) is the host Philox4x32-10 mask bit for bit
    (ops/philox.py), its keep fraction is within binomial bounds, and every gradient matches the float64
    oracle that applies that mask with the x2 scale <= 1e-5 (so the forward and the backward used the same
    mask); over 2 steps the mask changes.  Evaluation / prediction without quirk Q4 apply no mask."""
    import tensorflow_distributed_example_amd as tde
    from tensorflow_distributed_example_amd.ops.philox import keep_scales
    from tensorflow_distributed_example_amd.train import program as PG
    m = _model_b(tde, rate=0.5)
    st = m._store
    plan = PG.make_plan(m, st, DEV, 128, 128, m.optimizer, m.loss)
    assert plan.kind == "fused_bncnn" and plan.drop is not None
    masks = []
    for step in range(2):
        x, y = _data(128, 40 + step)
        before = {n: st.view(n).detach().double().clone() for n in st.order}
        st.g.zero_()
        plan.train_step(x, y, B)
        mask = plan.dropout_mask(B)
        torch.cuda.synchronize()
        it = int(plan.iterations.item())
        host = keep_scales(0.5, plan.drop_seed, it, 0, B * plan.D).reshape(B, plan.D)
        assert np.array_equal(mask.cpu().numpy(), host), "device mask != host Philox4x32-10"
        frac = float((mask > 0).double().mean())
        n = B * plan.D
        assert abs(frac - 0.5) < 5 * np.sqrt(0.25 / n), frac
        assert set(torch.unique(mask).tolist()) <= {0.0, 2.0}
        masks.append(mask.clone())
        after = {n_: st.view(n_).detach().clone() for n_ in st.order}
        for n_ in st.order:
            st.view(n_).copy_(before[n_])
        grads, moving, loss, _ = _oracle(plan, x, y, B, drop_mask=mask)
        for n_ in st.order:
            st.view(n_).copy_(after[n_])
        for n_, gr in grads.items():
            assert _rel(st.grad(n_), gr) < 1e-5, (step, n_, _rel(st.grad(n_), gr))
        for n_, v in moving.items():
            # moving means near 1e-3: the f32 batch sums over B*H*W values set the relative error (B=128:
            # 1.0e-6 measured on MI355X)
            assert _rel(st.view(n_), v) < 4e-6, (step, n_, _rel(st.view(n_), v))
        plan.apply()
        torch.cuda.synchronize()
    assert not torch.equal(masks[0], masks[1])
    # inference without the forced learning phase: moving statistics and NO dropout mask
    ev = PG.make_plan(m, st, DEV, 64, 64, None, m.loss)
    xe, _ = _data(64, 50)
    probs = ev.predict(xe, 64).clone()
    ref = m(xe.cpu().numpy())
    ref = (ref if torch.is_tensor(ref) else torch.as_tensor(np.asarray(ref))).to(DEV, torch.float64)
    assert _rel(probs, ref) < 1e-5, _rel(probs, ref)


@pytest.mark.parametrize("B", [128, 50])
def test_bncnn_head_folded_into_dense_backward_matches_head_launch(B, monkeypatch):
    """The training head inside the dense backward (TDE_BNCNN_HEAD_FOLD=1, opt-in: every workgroup recomputes the
    head of all rows; dense_fwd stores the dropout keep flags) vs the separate head launch (the default): 3 steps with dropout
    0.5 — gradients, moving statistics and metrics equal to fp32 summation-order noise, keep masks identical."""
    import tensorflow_distributed_example_amd as tde
    from tensorflow_distributed_example_amd.train import program as PG
    res = {}
    for fold in ("1", "0"):
        monkeypatch.setenv("TDE_BNCNN_HEAD_FOLD", fold)
        tde.backend.set_random_seed(5)
        m = _model_b(tde, rate=0.5)
        st = m._store
        plan = PG.make_plan(m, st, DEV, 128, 128, m.optimizer, m.loss)
        assert plan.head_fold_ok(B) == (fold == "1")
        grads, masks = [], []
        for step in range(3):
            x, y = _data(128, 60 + step)
            st.g.zero_()
            plan.train_step(x, y, B)
            masks.append(plan.dropout_mask(B).clone())
            grads.append(st.g.clone())
            plan.apply()
        torch.cuda.synchronize()
        res[fold] = (grads, masks, st.w.clone(), plan.metrics.clone())
    (g1, m1, w1, met1), (g0, m0, w0, met0) = res["1"], res["0"]
    for a, b in zip(m1, m0):
        assert torch.equal(a, b)
    for step, (a, b) in enumerate(zip(g1, g0)):
        assert _rel(a, b) < 1e-5, (step, _rel(a, b))
    assert _rel(w1, w0) < 1e-6
    assert abs(met1[0].item() - met0[0].item()) <= 1e-5 * abs(met0[0].item()) and met1[2].item() == met0[2].item()
