"""The fused float32 BN-CNN plan (train/bncnn.py, csrc/kernels/bncnn.hip) over its FAMILY, not only Model B:
small relatives (tests/bncnn_cases.py) that each take a branch of the host planners and the kernels Model B
never takes, and the row counts around the thresholds of the step (stack staging, ragged 16-row tiles, a second
pass of the 8-partial loops, three 64-row blocks), against the float64 oracle of tests/bncnn_oracle.py.

Bound of every gradient: ``max(1e-5 * |g64|, 4 * |g32 - g64|)`` (norm-wise), g32 being the same oracle in
float32 on the CPU with the same ReLU decisions — the project's 1e-5 where a BN has many values, and the error
of a second f32 implementation (x4 for another summation order) where few values per statistic amplify f32
rounding through rstd and cancellation.  tests/test_bncnn_oracle.py checks on the CPU that this bound stays
below 1e-4 * |g64| for every case and row count run here.  Moving statistics: 1e-6.  Each test prints its
figures before it asserts (profiles/bncnn_family/NOTES.md records them)."""
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bncnn_cases as BC
import bncnn_oracle as BO

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("fp32_policy")]

DEV = "cuda"


def _plan(m, batch, train=True):
    from tensorflow_distributed_example_amd.train import program as PG
    plan = PG.make_plan(m, m._store, DEV, batch, batch, m.optimizer if train else None, m.loss)
    assert plan.kind == "fused_bncnn" and plan.compute_dtype == "fp32"
    return plan


def _step_and_oracles(plan, x, y, B):
    """One training step over B rows, then the float64 (GPU) and float32 (CPU) oracles at the pre-step weights
    with the plan's ReLU decisions."""
    st = plan.store
    before = {n: st.view(n).detach().clone() for n in st.order}
    st.g.zero_()
    plan.metrics.zero_()
    plan.train_step(x, y, B)
    torch.cuda.synchronize()
    after = {n: st.view(n).detach().clone() for n in st.order}
    for n in st.order:
        st.view(n).copy_(before[n])
    o64 = BO.plan_oracle(plan, x, y, B)
    o32 = BO.plan_oracle(plan, x, y, B, dtype=torch.float32, device="cpu")
    for n in st.order:
        st.view(n).copy_(after[n])
    return o64, o32


def _check_gradient(tag, n, got, g64, g32):
    err = (got.double() - g64).norm().item()
    ref = (g32.double().to(g64.device) - g64).norm().item()
    nrm = g64.norm().item()
    print(f"FAMILY {tag} {n}: |g64| {nrm:.3e} kernel err {err:.3e} ({err / (nrm + 1e-300):.2e} rel) "
          f"f32 reference err {ref:.3e} ({ref / (nrm + 1e-300):.2e} rel)")
    assert err <= BO.bound(g64, g32.to(g64.device)), (tag, n, err, ref, nrm)


def _check_moving(tag, st, moving, tol=1e-6):
    for n, v in moving.items():
        r = BO.rel(st.view(n), v)
        print(f"FAMILY {tag} {n}: rel {r:.2e}")
        assert r < tol, (tag, n, r)


def _check_metrics(tag, plan, B, loss, logits, y):
    met = plan.metrics.double().cpu()
    print(f"FAMILY {tag} loss {met[0].item() / B:.7f} oracle {loss:.7f} rows {met[2].item():.0f}")
    assert met[2].item() == B and abs(met[0].item() / B - loss) < 1e-5 * abs(loss)
    assert met[1].item() == (logits.argmax(1) == y[:B].long()).sum().item()


def _check_step(tag, plan, x, y, B):
    (g64, mv64, loss, logits), (g32, _, _, _) = _step_and_oracles(plan, x, y, B)
    st = plan.store
    assert torch.isfinite(st.g).all() and torch.isfinite(st.w).all()
    assert set(g64) == set(st.names(trainable=True))
    for n, gr in g64.items():
        _check_gradient(tag, n, st.grad(n), gr, g32[n])
    _check_moving(tag, st, mv64)
    _check_metrics(tag, plan, B, loss, logits, y)


def _check_one_row_step(tag, plan, x, y):
    """One row: the dense BN's output is beta whatever the input, so its backward is identically zero and the
    conv gradients are what f32 cancellation leaves.  The head's gradients, the loss and the moving statistics
    are well defined; the dense-kernel gradient is zero to ``4 * |g32| + 1e-5 * |g_head|``."""
    (g64, mv64, loss, logits), (g32, _, _, _) = _step_and_oracles(plan, x, y, 1)
    st = plan.store
    assert torch.isfinite(st.g).all() and torch.isfinite(st.w).all()
    hk, hb, dk = f"{plan.head.name}/kernel", f"{plan.head.name}/bias", f"{plan.dense.name}/kernel"
    for n in (hk, hb):
        _check_gradient(tag, n, st.grad(n), g64[n], g32[n])
    zero_bound = 4 * g32[dk].double().norm().item() + 1e-5 * g64[hk].norm().item()
    got = st.grad(dk).double().norm().item()
    print(f"FAMILY {tag} {dk}: |g| {got:.3e} bound {zero_bound:.3e}")
    assert got <= zero_bound, (tag, got, zero_bound)
    _check_moving(tag, st, mv64)
    _check_metrics(tag, plan, 1, loss, logits, y)


# ---------------------------------------------------------------------------------------------- the case table
@pytest.mark.parametrize("case", sorted(BC.CASES))
def test_case_takes_its_planner_branch(case):
    """The planner outputs each case exists for (tests/bncnn_cases.py): forward (ks, msplit), backward (wgrad
    items, dgrad items, wg_split, ksd, staged floats), the stride classes and N tiles of the input gradient."""
    import tensorflow_distributed_example_amd as tde
    c = BC.CASES[case]
    plan = _plan(BC.build(tde, case), c["batch"])
    assert len(plan.blocks) == len(c["convs"]) and (plan.D, plan.NC) == (c["D"], c["NC"])
    for li, (blk, want, derived) in enumerate(zip(plan.blocks, c["plan"], c["derived"])):
        g = blk["geo"]
        print(f"FAMILY {case} block {li}: fwd cfg {blk['cfg']} bwd plan {blk['bwd'][:6]} stack rows {blk['stack_rows']}")
        assert tuple(blk["cfg"][1:3]) == want["fwd"], (case, li, blk["cfg"])
        got = tuple(blk["bwd"][1:6]) if li > 0 else (blk["bwd"][1], 0, blk["bwd"][3], None, 0)
        assert got == want["bwd"], (case, li, blk["bwd"])
        assert (blk["wstack"] is None) == (want["bwd"][4] == 0)
        if derived is not None:
            ncls = g.sh * g.sw
            assert (ncls, -(-ncls * g.C // 16)) == derived, (case, li)
    if case == "A":
        g = plan.blocks[1]["geo"]
        assert (g.Ho, g.Wo, g.Co) == (2, 1, 17) and plan.K == 34 and plan.Dp == 32 and plan.blocks[1]["stack_rows"] == 6
    if case == "B":
        pads = [b["conv"].pads(b["conv"].input_shape) for b in plan.blocks]
        assert pads == [((1, 1), (1, 2)), ((1, 1), (0, 1)), ((0, 0), (0, 0))] and plan.K == 270
    if case == "D":
        (pt, pb), (pl, pr) = plan.blocks[0]["conv"].pads(plan.blocks[0]["conv"].input_shape)
        assert (pt, pb, pl, pr) == (1, 2, 1, 2)
    if case == "I":
        assert plan.blocks[1]["bwd"][5] == 0 and plan.blocks[1]["stack_rows"] == 0   # wgather == 0


@pytest.mark.parametrize("case", sorted(BC.CASES))
def test_case_step_matches_float64(case):
    """Every gradient (gammas included), every moving statistic, the loss / accuracy / row count of one training
    step at the case's full plan batch (24 rows: one full and one ragged 16-row tile)."""
    import tensorflow_distributed_example_amd as tde
    c = BC.CASES[case]
    m = BC.build(tde, case)
    plan = _plan(m, c["batch"])
    x, y = BC.data(case, c["batch"], 11, DEV)
    _check_step(f"{case} rows={c['batch']}", plan, x, y, c["batch"])


@pytest.mark.parametrize("case", sorted(BC.CASES))
def test_case_eval_and_predict_use_moving_statistics(case):
    import tensorflow_distributed_example_amd as tde
    c = BC.CASES[case]
    m = BC.build(tde, case)
    plan = _plan(m, c["batch"], train=False)
    B = c["batch"] - 3
    x, y = BC.data(case, c["batch"], 12, DEV)
    out = plan.predict(x, B).clone()
    plan.metrics.zero_()
    plan.eval_step(x, y, B)
    torch.cuda.synchronize()
    logits, probs = BO.inference(m._store, BO.spec_of(plan), x, B)
    want = probs if c["softmax"] else logits
    print(f"FAMILY {case} predict rel {BO.rel(out, want):.2e}")
    assert out.shape == want.shape and BO.rel(out, want) < 1e-5, BO.rel(out, want)
    met = plan.metrics.double().cpu()
    loss = F.cross_entropy(logits, y[:B].long(), reduction="sum").item()
    assert abs(met[0].item() - loss) < 1e-4 * abs(loss) and met[2].item() == B
    assert met[1].item() == (logits.argmax(1) == y[:B].long()).sum().item()


# ---------------------------------------------------------------------------------------------- row counts
@pytest.mark.parametrize("B", [1, 2, 5, 6, 17, 50, 130])
def test_case_a_row_counts(B):
    """Case A on a plan of batch 130 (9 row tiles, 3 row blocks): below (1, 2, 5), at (6) and above the rows its
    second block's forward needs to stage the class-stacked weights; 17 and 50 end in a ragged 16-row tile;
    130 runs the second pass of the 8-partial loops and the three-block dense reduce."""
    import tensorflow_distributed_example_amd as tde
    m = BC.build(tde, "A")
    plan = _plan(m, 130)
    assert plan.nrb == 3 and plan.blocks[1]["stack_rows"] == 6
    assert (plan._wstack(plan.blocks[1], B) is not None) == (B >= 6)
    x, y = BC.data("A", 130, 11, DEV)
    if B == 1:
        _check_one_row_step("A rows=1", plan, x, y)
    else:
        _check_step(f"A rows={B}", plan, x, y, B)


@pytest.mark.parametrize("B", [1, 2, 3, 4, 5])
def test_model_b_trains_on_one_to_five_rows(B):
    """Model B on its 128-row plan with the 1-5 rows of a short last batch: its third conv stages 10752 stack
    floats with 2048 forward threads per row (6 rows), its second 3584 (2 rows); below that the step runs
    without the staged stack."""
    import tensorflow_distributed_example_amd as tde
    m = BC.model_b(tde)
    plan = _plan(m, 128)
    assert [b["stack_rows"] for b in plan.blocks] == [0, 2, 6]
    x, y = BC.model_b_data(128, 11, DEV)
    if B == 1:
        _check_one_row_step("ModelB rows=1", plan, x, y)
    else:
        _check_step(f"ModelB rows={B}", plan, x, y, B)


def test_model_b_step_at_full_batch_still_stages_the_stack():
    import tensorflow_distributed_example_amd as tde
    plan = _plan(BC.model_b(tde), 128)
    assert all(plan._wstack(b, 128) is b["wstack"] and b["wstack"] is not None for b in plan.blocks[1:])


def test_model_b_fit_with_a_three_row_last_batch():
    """fit() over 64 + 3 rows at batch 64: the partial batch runs train_step(x, y, 3) on the 64-row plan."""
    import tensorflow_distributed_example_amd as tde
    rng = np.random.default_rng(0)
    x = rng.random((67, 784), dtype=np.float32)
    y = rng.integers(0, 10, 67)
    m = BC.model_b(tde)
    h = m.fit(x, y, batch_size=64, epochs=1, shuffle=False, verbose=0)
    assert m._program("train", 64).plan_kind == "fused_bncnn"
    assert np.isfinite(h.history["loss"][0]) and all(np.isfinite(w).all() for w in m.get_weights())


# ---------------------------------------------------------------------------------------------- step modes
def test_case_a_fused_reduce_optimizer_with_gammas_matches_separate_launch():
    """Step mode "local" with every BN's gamma and beta among the reduce launch's segments vs "plain": 3 steps
    of momentum SGD give bitwise-equal weights and slots."""
    import tensorflow_distributed_example_amd as tde
    res = {}
    for mode in ("plain", "local"):
        tde.backend.set_random_seed(11)
        m = BC.build(tde, "A", opt=tde.optimizers.SGD(0.05, momentum=0.9))
        plan = _plan(m, 24)
        assert plan.supports_step_mode("local") and len(plan._bn_segs) == 6
        plan.set_step_mode(mode)
        for i in range(3):
            x, y = BC.data("A", 24, 20 + i, DEV)
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


def test_case_b_head_folded_into_dense_backward_matches_head_launch(monkeypatch):
    """TDE_BNCNN_HEAD_FOLD=1 on case B (gammas, no betas, K = 270, 16 classes) at 50 rows vs the separate head
    launch, as tests/test_bncnn_gpu.py does for Model B: 3 steps with dropout 0.5."""
    import tensorflow_distributed_example_amd as tde
    B = 50
    res = {}
    for fold in ("1", "0"):
        monkeypatch.setenv("TDE_BNCNN_HEAD_FOLD", fold)
        tde.backend.set_random_seed(5)
        m = BC.build(tde, "B", rate=0.5)
        st = m._store
        plan = _plan(m, 64)
        assert plan.head_fold_ok(B) == (fold == "1")
        grads, masks = [], []
        for step in range(3):
            x, y = BC.data("B", 64, 60 + step, DEV)
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
        print(f"FAMILY B fold step {step}: rel {BO.rel(a, b):.2e}")
        assert BO.rel(a, b) < 1e-5, (step, BO.rel(a, b))
    assert BO.rel(w1, w0) < 1e-6
    assert abs(met1[0].item() - met0[0].item()) <= 1e-5 * abs(met0[0].item()) and met1[2].item() == met0[2].item()


# ---------------------------------------------------------------------------------------------- refusals
def _fit_on_fallback(m, shape, classes, why):
    """fit() of a relative the fused step refuses: one warning naming the limit, a non-fused plan, a finite
    loss.  Plan selection only: no fused kernel is launched on the refused geometry."""
    rng = np.random.default_rng(0)
    x = rng.random((32,) + shape, dtype=np.float32)
    y = rng.integers(0, classes, 32)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        h = m.fit(x, y, batch_size=16, epochs=1, shuffle=False, verbose=0)
    msgs = [str(w.message) for w in rec if "fused BN-CNN step" in str(w.message)]
    assert msgs and all(why in s and "per-layer kernel plan" in s for s in msgs), [str(w.message) for w in rec]
    assert m._program("train", 16).plan_kind != "fused_bncnn"
    assert np.isfinite(h.history["loss"][0])


def test_too_many_class_stacked_channels_fall_back_with_a_warning():
    """17 channels into a stride-2x2 conv: C * sh * sw = 68 > 64 columns of class-stacked weights, which
    ``tde_bncnn_conv_bwd_plan`` refuses (-1); the model trains on the per-layer plan."""
    import ctypes as C

    import tensorflow_distributed_example_amd as tde
    from tensorflow_distributed_example_amd import _native as N
    from tensorflow_distributed_example_amd.train import bncnn
    case = dict(input=(8, 8, 1), convs=[(17, (3, 3), (1, 1), "same", BC._FT), (4, (3, 3), (2, 2), "same", BC._FT)],
                D=16, NC=10, bnd=BC._FT, softmax=True)
    out = (C.c_int * 12)()
    assert N.hip().tde_bncnn_conv_bwd_plan(C.byref(bncnn.Geo(8, 8, 17, 4, 4, 4, 3, 3, 2, 2, 0, 0)), 1, out) == -1
    _fit_on_fallback(BC.build(tde, case), (8, 8, 1), 10, "backward tiles do not fit")


def test_flattened_width_past_the_dense_kernel_falls_back_with_a_warning():
    """28x28x1 · Conv2D(6, 3, same) · Flatten: K = 4704 > 1536 (dense_fwd_kernel's 16 waves x 96 K steps)."""
    import tensorflow_distributed_example_amd as tde
    case = dict(input=(28, 28, 1), convs=[(6, (3, 3), (1, 1), "same", BC._FT)], D=32, NC=10, bnd=BC._FT, softmax=True)
    _fit_on_fallback(BC.build(tde, case), (28, 28, 1), 10, "4704 flattened inputs (<= 1536)")
