"""Dropout inside the fused small-net step (csrc/kernels/smallnet.hip, train/smallnet.py) on the GPU.

The mask is observed directly (an all-ones activation times the keep scale lands in the head's input
record) at step indices 0, 1 and a restored 41, at a batch of more workgroups than fit on the device at
once -- where a step index read from ``iterations`` by late workgroups would show as rows drawn from
step + 1.  Gradients, loss and counts are compared with the float64 oracle of tests/smallnet_oracle.py on
the dropout suite of tests/smallnet_cases.py under the project's bound, max(1e-5, 4 x the error of the same oracle
in torch fp32 on the CPU with the same masks); the conditions on the inputs (exact conv trunk, near-tie,
margin) are asserted on the CPU in tests/test_smallnet_dropout.py.

Figures on an MI355X (``-s`` prints every one before it is asserted): gradient errors of both plans
between 6e-8 and 2.3e-7 (worst: pool_drop B=5, conv2d/bias) where the fp32 CPU oracle has 3e-8 to 3.4e-7,
bound 1e-5; losses below 7e-8; the three-step weight deltas 9e-7 to 5.8e-6 against the fp32 oracle's
9e-7 to 5.7e-6 (the f32 weight store's own rounding of small deltas), bound 1e-5 to 2.3e-5, and 0.37 to
0.68 away from the trajectory with the step index frozen at 0.
"""
import types

import numpy as np
import pytest
import torch

import smallnet_cases as C
import smallnet_oracle as O

pytestmark = pytest.mark.gpu


def _tde():
    import tensorflow_distributed_example_amd as tde
    from tensorflow_distributed_example_amd.train import program as PG
    return tde, PG


def _plan(PG, m, Bplan, prefer=None):
    plan = PG.make_plan(m, m._store, "cuda", Bplan, Bplan, m.optimizer, m.loss, prefer=prefer)
    if prefer is None:
        assert plan.kind == "fused_smallnet"
    return plan


def _compare(tag, st, orc, o32, what="kernel"):
    """Every trainable variable's gradient in ``st`` against the float64 oracle, bounded by the fp32 CPU
    oracle's own error."""
    for n in st.names(trainable=True):
        e, r = O.rel(st.grad(n), orc["grads"][n]), O.rel(o32["grads"][n], orc["grads"][n])
        print(f"[{tag}] grad {n}: {what} {e:.3g}  cpu-fp32 {r:.3g}  bound {O.bound(r):.3g}")
    for n in st.names(trainable=True):
        e, r = O.rel(st.grad(n), orc["grads"][n]), O.rel(o32["grads"][n], orc["grads"][n])
        assert e <= O.bound(r), (tag, n, e, r)


@pytest.mark.parametrize("batch", ["5of8", "two_waves_of_workgroups"])
def test_mask_observed_directly(batch):
    """Dense(10, relu) with zero kernel and bias 1 gives all ones; what the head records as its input is the
    keep scale itself.  D = 10: Philox blocks straddle rows."""
    from tensorflow_distributed_example_amd.ops.philox import keep_scales
    tde, PG = _tde()
    if batch == "5of8":
        B, Bplan = 5, 8
    else:
        B = Bplan = 2 * torch.cuda.get_device_properties(0).multi_processor_count + 37
    m, _, _ = C.make_case(tde, "dropout", "mask_probe", B, Bplan)
    st = m._store
    first = [l for l in m.layers if l.weight_specs][0]
    st.view(f"{first.name}/kernel").zero_()
    st.view(f"{first.name}/bias").fill_(1.0)
    plan = _plan(PG, m, Bplan)
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.standard_normal((Bplan, 6)).astype(np.float32)).cuda()
    y = torch.from_numpy(rng.integers(0, 3, Bplan).astype(np.int32)).cuda()
    xo = int(plan.dense[1][2])
    assert int(plan.dense[1][0]) == 10

    def step_and_check(step, iters_after):
        plan.train_step(x, y, B)
        torch.cuda.synchronize()
        got = plan.rec[:B, xo:xo + 10].cpu()
        want = torch.from_numpy(keep_scales(0.5, 1234, step, 0, B * 10).reshape(B, 10))
        bad = (got != want).any(dim=1).nonzero().flatten().tolist()
        assert not bad, (step, len(bad), bad[:8])
        assert plan.iterations.item() == iters_after

    step_and_check(0, 1)
    step_and_check(1, 2)
    # a restored counter, through Model._set_iterations and the plan's hook
    m._programs["probe"] = types.SimpleNamespace(plans=[plan])
    try:
        m._set_iterations(41)
    finally:
        del m._programs["probe"]
    assert plan.iterations.item() == 41
    step_and_check(41, 42)
    step_and_check(42, 43)


@pytest.mark.parametrize("name,B,Bplan", C.CASES["dropout"])
def test_gradients_loss_and_counts_match_oracle(name, B, Bplan):
    tde, PG = _tde()
    m, x, y = C.make_case(tde, "dropout", name, B, Bplan)
    st = m._store
    orc = O.oracle(m, st, x, y, B, Bplan, 0)
    o32 = O.oracle(m, st, x, y, B, Bplan, 0, dtype=torch.float32)
    plan = _plan(PG, m, Bplan)
    assert len(plan.drops) == sum(r > 0 for r, _, _ in O.drop_table(m).values())
    plan.train_step(x.cuda(), y.cuda(), B)
    torch.cuda.synchronize()
    tag = f"{name} B={B}/{Bplan}"
    _compare(tag, st, orc, o32)
    mt = plan.metrics.cpu()
    le, lr = abs(mt[0].item() - orc["loss"]) / abs(orc["loss"]), abs(o32["loss"] - orc["loss"]) / abs(orc["loss"])
    print(f"[{tag}] loss: kernel {le:.3g}  cpu-fp32 {lr:.3g}")
    assert le <= O.bound(lr), (tag, le, lr)
    assert mt[1].item() == orc["correct"] and mt[2].item() == B, (tag, mt.tolist(), orc["correct"])
    assert plan.iterations.item() == 1


def test_eval_and_predict_are_mask_free():
    tde, PG = _tde()
    name, (B, Bplan) = "pool_drop", (5, 8)
    m, x, y = C.make_case(tde, "dropout", name, B, Bplan)
    orc = O.oracle(m, m._store, x, y, B, Bplan, None)
    plan = _plan(PG, m, Bplan)
    xg, yg = x.cuda(), y.cuda()
    plan.train_step(xg, yg, B)
    plan.reset_metrics()
    plan.eval_step(xg, yg, B)
    p = plan.predict(xg, B).clone()
    torch.cuda.synchronize()
    me = plan.metrics.cpu()
    le = abs(me[0].item() - orc["loss"]) / abs(orc["loss"])
    print(f"[{name}] eval loss {le:.3g} predict {O.rel(p, orc['out']):.3g}")
    assert le <= O.TOL and O.rel(p, orc["out"]) <= O.TOL
    assert me[1].item() == orc["correct"] and me[2].item() == B and tuple(p.shape) == (B, 5)
    assert plan.iterations.item() == 1
    # and the masked loss is another number: eval really ran without the masks
    masked = O.oracle(m, m._store, x, y, B, Bplan, 1)["loss"]
    assert abs(masked - orc["loss"]) / abs(orc["loss"]) > 1e-3


def test_three_local_sgd_steps_follow_the_masks_of_steps_0_1_2():
    tde, PG = _tde()
    name, B, Bplan = C.TRAJ
    m, x, y = C.make_case(tde, "dropout", name, B, Bplan)
    st = m._store
    lr = float(m.optimizer.learning_rate)
    w0 = {n: st.view(n).detach().cpu().double().clone() for n in st.names(trainable=True)}
    w64, figs = O.trajectory(m, st, x, y, B, Bplan, lr, C.TRAJ_STEPS)
    w32, _ = O.trajectory(m, st, x, y, B, Bplan, lr, C.TRAJ_STEPS, dtype=torch.float32)
    frozen, _ = O.trajectory(m, st, x, y, B, Bplan, lr, C.TRAJ_STEPS, mask_steps=[0] * C.TRAJ_STEPS)
    # the step-1 gradient with the step-0 mask is another gradient (oracle alone, at the step-1 weights)
    w1, _ = O.trajectory(m, st, x, y, B, Bplan, lr, 1)
    g_same = O.oracle(m, st, x, y, B, Bplan, 0, weights=w1)["grads"]
    assert any(O.rel(g_same[n], figs[1]["grads"][n]) > 1e-2 for n in g_same)
    plan = _plan(PG, m, Bplan)
    plan.set_step_mode("local")
    xg, yg = x.cuda(), y.cuda()
    for _ in range(C.TRAJ_STEPS):
        plan.train_step(xg, yg, B)
    torch.cuda.synchronize()
    assert plan.iterations.item() == C.TRAJ_STEPS
    far = []
    for n in w0:
        d = st.view(n).detach().cpu().double() - w0[n]
        e, r = O.rel(d, w64[n] - w0[n]), O.rel(w32[n].double() - w0[n], w64[n] - w0[n])
        f = O.rel(d, frozen[n] - w0[n])
        print(f"[traj] delta {n}: kernel {e:.3g}  cpu-fp32 {r:.3g}  bound {O.bound(r):.3g}  vs frozen step index {f:.3g}")
        far.append(f)
    for n in w0:
        d = st.view(n).detach().cpu().double() - w0[n]
        e, r = O.rel(d, w64[n] - w0[n]), O.rel(w32[n].double() - w0[n], w64[n] - w0[n])
        assert e <= O.bound(r), (n, e, r)
    assert max(far) > 1e-2      # a step index frozen at 0 gives other weights


@pytest.mark.parametrize("name", ["linear_drop", "pool_drop"])
def test_layerwise_plan_draws_the_same_masks(name):
    """The oracle uses one mask; both plans within its bound means both drew that mask."""
    tde, PG = _tde()
    B, Bplan = 5, 8
    m, x, y = C.make_case(tde, "dropout", name, B, Bplan)
    st = m._store
    orc = O.oracle(m, st, x, y, B, Bplan, 0)
    o32 = O.oracle(m, st, x, y, B, Bplan, 0, dtype=torch.float32)
    fused = _plan(PG, m, Bplan)
    lw = _plan(PG, m, Bplan, prefer="layerwise")
    assert lw.kind == "layerwise" and lw.compute_dtype == "fp32"
    xg, yg = x.cuda(), y.cuda()
    for tag, plan in (("fused", fused), ("layerwise", lw)):
        st.g.zero_()
        plan.train_step(xg, yg, B)
        torch.cuda.synchronize()
        _compare(f"{name} {tag}", st, orc, o32, what=tag)
        assert plan.iterations.item() == 1


def test_rate_zero_is_the_model_without_the_layer():
    """Dense-only, hence deterministic: the gradients are equal bit for bit, and so are the layer tables."""
    tde, PG = _tde()
    B, Bplan = 67, 67
    got = []
    for name in ("linear_rate0", "linear_plain"):
        m, x, y = C.make_case(tde, "dropout", name, B, Bplan)
        plan = _plan(PG, m, Bplan)
        assert not plan.drops and plan.step_word is None
        plan.train_step(x.cuda(), y.cuda(), B)
        torch.cuda.synchronize()
        st = m._store
        got.append((plan.layers.copy(), [st.grad(n).cpu().clone() for n in st.names(trainable=True)], x, y))
    (la, ga, xa, ya), (lb, gb, xb, yb) = got
    assert torch.equal(xa, xb) and torch.equal(ya, yb)
    assert np.array_equal(la, lb) and not la[:, -5:].any()
    assert len(ga) == len(gb) == 5
    for a, b in zip(ga, gb):
        assert a.abs().max() > 0 and torch.equal(a, b)
