"""Learning-rate schedules on the GPU (csrc/include/tde_sched.h, csrc/kernels/schedule.hip, the scheduled
weight-gradient launch of csrc/kernels/smallnet.hip, ``OptimizerKernel``): the schedule kernel on the whole
case table of tests/lr_schedule_oracle.py against its float64 oracle, the multi-tensor optimizer launch under
a schedule on the exact grid of tests/optim_oracle.py / tests/optim_rmsprop_oracle.py, a rate that changes
between two steps of one hipGraph replay, the small-net plan's in-step update against "plain" and against the
float64 trajectory of tests/smallnet_oracle.py, the fused CNN plans falling back to "plain", a restored step
counter and ``fit``.

Figures on an MI355X (``-s`` prints every one before it is asserted) are in profiles/lr_schedule/NOTES.md.
"""
import ctypes

import numpy as np
import pytest
import torch

import lr_schedule_oracle as S
import optim_oracle as OO
import optim_rmsprop_oracle as R
import smallnet_cases as C
import smallnet_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _tde():
    import tensorflow_distributed_example_amd as tde
    from tensorflow_distributed_example_amd.train import program as PG
    return tde, PG


def _K():
    from tensorflow_distributed_example_amd import _native as N
    from tensorflow_distributed_example_amd.ops import kernels as K
    return N, K


def _bits(x):
    return np.float32(x).view(np.int32).item()


# ------------------------------------------------------------------------------------- 1. the schedule kernel
def test_schedule_kernel_against_the_float64_oracle():
    tde, _ = _tde()
    N, K = _K()
    rows = S.rows()
    it = torch.tensor([r[3] for r in rows], dtype=torch.int64, device=DEV)
    out = torch.full((len(rows),), -7.0, dtype=torch.float32, device=DEV)
    descs = {}
    for i, (ci, name, kw, iters, bias, exact) in enumerate(rows):
        if ci not in descs:
            descs[ci] = K.lr_sched(S.make(tde, name, kw))
        K.lr_schedule(descs[ci], it[i:i + 1], bias, out[i:i + 1])
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    worst, fails = {}, []
    for i, (ci, name, kw, iters, bias, exact) in enumerate(rows):
        step = iters + bias
        want, b = S.eval64(name, kw, step), S.bound(name, kw, step)
        e = abs(float(got[i]) - want)
        worst[name] = max(worst.get(name, 0.0), e / S.lr0_of(name, kw))
        if exact and _bits(got[i]) != _bits(want):
            fails.append(("not exact", ci, name, step, bias, float(got[i]), want))
        if not e <= b:
            fails.append(("bound", ci, name, step, bias, e, b))
    for name in S.KINDS:
        print(f"[schedule kernel] {name}: largest |device - float64| / lr0 = {worst[name]:.3g} "
              f"= {worst[name] * 2 ** 24:.3g} x 2^-24 (bound 4 x 2^-24 or 4 x the fp32 twin's)")
    assert not fails, fails
    assert any(r[3] + r[4] == S.BIG + 7 and r[1] == "PiecewiseConstantDecay" for r in rows)
    assert any(r[4] == -1 for r in rows) and any(r[3] + r[4] < 0 for r in rows)


def test_schedule_kernel_refusals_leave_the_word():
    tde, _ = _tde()
    N, K = _K()
    lib = N.hip()
    it = torch.zeros(1, dtype=torch.int64, device=DEV)
    out = torch.full((1,), -7.0, dtype=torch.float32, device=DEV)
    good = K.lr_sched(tde.optimizers.schedules.PiecewiseConstantDecay([1], [0.5, 0.25]))

    def call(d, itp=it.data_ptr(), outp=out.data_ptr()):
        return lib.tde_lr_schedule(ctypes.byref(d) if d is not None else None, itp, 0, outp, N.stream_ptr())
    bad = []
    for kind in (0, 6, -1):
        d = K.lr_sched(tde.optimizers.schedules.ExponentialDecay(0.5, 4, 0.5))
        d.kind = kind
        bad.append(d)
    d = K.lr_sched(tde.optimizers.schedules.PiecewiseConstantDecay([1], [0.5, 0.25]))
    d.nb = 9
    bad.append(d)
    d = K.lr_sched(tde.optimizers.schedules.PiecewiseConstantDecay([1], [0.5, 0.25]))
    d.nb = -1
    bad.append(d)
    for d in bad:
        assert call(d) < 0
    assert call(None) < 0 and call(good, itp=None) < 0 and call(good, outp=None) < 0
    torch.cuda.synchronize()
    assert out.item() == -7.0
    assert call(good) == 0
    torch.cuda.synchronize()
    assert out.item() == 0.5


# ------------------------------------------------------------------------------------- 2. the plain path
# the small segment list: scalar tails, float4 bodies with tails, the 16 x 64 tile edge (a second row tile of
# one row, a partial column tile), a chunk crossing, alignment gaps between all of them
SEGMENTS = [s for s in OO.SEGMENTS if s[0] in ("v1", "t5x130", "v10", "t17x64", "conv3x3x1x6", "v2049")]
ALL_KINDS = OO.KINDS + R.KINDS


def _grid_optimizer(tde, kind, lr):
    OP = tde.optimizers
    if kind == "adam":
        h = OO.GRID_HYPER
        return OP.Adam(lr, h["b1"], h["b2"], h["eps"]), h
    if kind in R.KINDS:
        h = R.GRID_HYPER
        return OP.RMSprop(lr, rho=h["b2"], momentum=h["mom"] if kind == "rmsprop_momentum" else 0.0, epsilon=h["eps"]), h
    h = OO.GRID_HYPER
    return OP.SGD(lr, momentum=0.0 if kind == "sgd" else h["mom"], nesterov=kind == "nesterov"), h


@pytest.mark.parametrize("kind", ALL_KINDS)
def test_plain_path_three_steps_across_the_boundary(kind):
    """``OptimizerKernel.apply()`` under PiecewiseConstantDecay([1], [2^-3, 2^-2]) on the exact grid: w and the
    slots against the oracle stepped with lr = schedule(k); kinds 0..2 and rms bit for bit, Adam and the
    RMSprop w / q under the bounds of their own suites; gaps untouched; the word holds schedule(2)."""
    tde, PG = _tde()
    sch = tde.optimizers.schedules.PiecewiseConstantDecay([1], [0.125, 0.25])
    opt, hyper = _grid_optimizer(tde, kind, sch)
    assert opt.kind == kind and opt.kind_id == ALL_KINDS.index(kind)
    st = OO.make_store([(n, s) for n, s, _ in SEGMENTS], DEV)
    slots = [st.slot(s) for s in opt.slot_names()]
    it = torch.zeros(1, dtype=torch.int64, device=DEV)
    ok = PG.OptimizerKernel(st, opt, {n: sh for n, _, sh in SEGMENTS if sh}, it)
    assert ok.lr_word is not None and ok.sched_bias == -1
    idx = torch.arange(st.n_trainable)
    w = OO.grid_w(idx)
    if kind in R.KINDS:
        state = [R.grid_r(idx), R.grid_q(idx)]
    elif kind == "adam":
        state = [OO.grid_slot(idx), OO.grid_slot(idx).abs()]
    else:
        state = [OO.grid_slot(idx), None]
    host = [w.float()] + [None if s is None else s.float() for s in state]
    st.w.copy_(w.float())
    for buf, s in zip(slots, state):
        buf.copy_(s.float())
    ok.refresh_shadows()
    gaps, shgaps = OO.fill_store_gaps(st), OO.fill_shadow_gaps(ok)
    mask = OO.seg_mask(st)
    names = st.names(trainable=True)

    def seg(name, flat):
        s = st.segments[name]
        return flat[s.offset: s.offset + s.numel]
    fails = []
    for k in range(3):
        g = OO.grid_g(idx, k)
        st.g.copy_(torch.where(mask, g.float(), torch.tensor(OO.W_SENTINEL)))
        it += 1                      # the step's loss kernel advances the counter before the optimizer runs
        ok.apply()
        h = dict(hyper, lr=sch(k))
        if kind in R.KINDS:
            nw, r, q = R.oracle_step(kind, h, w, g, state[0], state[1])
            w, state = nw, [r, q]
            hw, hr, hq = R.fp32_step(kind, h, host[0], g.float(), host[1], host[2])
            host = [hw, hr, hq]
        else:
            w, m, v = OO.oracle_step(kind, h, w, g, state[0], state[1], k + 1)
            state = [m, v]
            host = list(OO.fp32_step(kind, h, host[0], g.float(), host[1], host[2], k + 1))
        torch.cuda.synchronize()
        dev = [st.w.cpu()] + [b.cpu() for b in slots]
        tag = f"{kind} step {k} lr {sch(k)}"
        for name in names:
            for key, d, o, hh in zip(("w", "slot0", "slot1"), dev, [w] + state, host):
                exact = kind in ("sgd", "momentum", "nesterov") or (kind in R.KINDS and key == "slot0")
                if exact:
                    diff = OO.first_diff(seg(name, d).double(), seg(name, o), bitwise=False)
                    assert not diff, f"{tag} {name} {key}: {diff}"
                elif kind == "adam":
                    oo = seg(name, o)
                    e_dev = float((seg(name, d).double() - oo).abs().max())
                    e_host = float((seg(name, hh).double() - oo).abs().max())
                    b = max(4.0 * e_host, 2.0 ** -22 * float(oo.abs().max())) + \
                        (sch(k) * S.rho_bound(k + 1, hyper) if key == "w" else 0.0)
                    print(f"[{tag}] {key} {name}: dev {e_dev:.3g} host {e_host:.3g} bound {b:.3g}")
                    if not e_dev <= b:
                        fails.append((tag, key, name, e_dev, b))
                else:
                    R.compare(tag, key, name, seg(name, d), seg(name, hh), seg(name, o), fails)
            assert not OO.first_diff(seg(name, st.g.cpu()), torch.zeros(st.segments[name].numel)), (tag, name)
        OO.assert_store_gaps(st, gaps)
        OO.assert_shadow_gaps(ok, shgaps)
        assert ok.lr_word.item() == sch(k)
    assert not fails, fails
    assert it.item() == 3 and ok.lr_word.item() == sch(2) == 0.25


# ------------------------------------------------------------------------------------- 3. inside one replay
def test_the_rate_changes_between_two_steps_of_one_replay():
    """pool_drop (5, 8) geometry at the plan's batch, SGD + PiecewiseConstantDecay([1], [lr, 0]), step mode
    "local", four steps per execution in one hipGraph: the per-step trace shows steps 0 and 1 moving the
    weights and steps 2 and 3 leaving them bit-identical; three executions, no graph beyond the first."""
    tde, PG = _tde()
    name, B, Bplan = C.TRAJ
    m, x, y = C.make_case(tde, "dropout", name, B, Bplan)
    lr = 0.01
    sch = tde.optimizers.schedules.PiecewiseConstantDecay([1], [lr, 0.0])
    m.compile(loss=tde.losses.SparseCategoricalCrossentropy(from_logits=C.MODELS["dropout"][name].logits),
              optimizer=tde.optimizers.SGD(sch), metrics=["accuracy"], steps_per_execution=4)
    prog = m._program("train", Bplan)
    plan = prog.plans[0]
    assert prog.plan_kind == "fused_smallnet" and plan.step_mode == "local" and prog.use_graph and prog.S == 4
    captures = []
    capture = prog.capture
    prog.capture = lambda: (captures.append(1), capture())[1]
    prog.enable_trace()
    st = plan.store
    nw = st.w.numel()
    w0 = st.w.cpu().clone()
    xs = x[:Bplan].to(DEV, plan.input_dtype).unsqueeze(0).repeat(4, *([1] * x.dim())).contiguous()
    ys = y[:Bplan].to(DEV, torch.int32).unsqueeze(0).repeat(4, 1).contiguous()
    prog.stage([(xs, ys)])
    prog.run()
    prog.sync()
    tr = prog.trace[0][:, :nw].cpu()
    assert not torch.equal(tr[0], w0) and not torch.equal(tr[1], tr[0])          # steps 0 and 1: rate lr
    assert OO.first_diff(tr[2], tr[1]) == "" and OO.first_diff(tr[3], tr[1]) == ""   # steps 2 and 3: rate 0
    assert OO.first_diff(st.w.cpu(), tr[1]) == ""
    assert plan.iterations.item() == 4
    assert plan.opt.lr_word.item() == 0.0
    graphs = dict(prog.graphs)
    n0 = len(captures)
    assert n0 >= 1 and len(graphs) == n0
    for _ in range(2):
        prog.stage([(xs, ys)])
        prog.run()
    prog.sync()
    assert len(captures) == n0 and prog.graphs.keys() == graphs.keys()
    assert all(prog.graphs[k][0] is graphs[k][0] for k in graphs)
    assert plan.iterations.item() == 12 and OO.first_diff(st.w.cpu(), tr[1]) == ""


# ------------------------------------------------------------------------------------- 4. small-net local
def _lenet(tde, opt):
    m = tde.zoo.lenet5()
    m.compile(loss=tde.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=opt, metrics=["accuracy"])
    m.build()
    return m


def _mlp_case(tde, opt):
    m, x, y = C.make_case(tde, "act", "mlp_tanh", 5, 8)
    m.compile(loss=tde.losses.SparseCategoricalCrossentropy(from_logits=C.MODELS["act"]["mlp_tanh"].logits),
              optimizer=opt, metrics=["accuracy"])
    return m, x, y


def _batch(m, n, seed):
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.standard_normal((n,) + tuple(m.input_shape[1:])).astype(np.float32))
    y = torch.from_numpy(rng.integers(0, 10, n).astype(np.int32))
    return x, y


def _opt_sched(tde, which):
    OP, SC = tde.optimizers, tde.optimizers.schedules
    if which == "sgd_exponential":
        return OP.SGD(SC.ExponentialDecay(S.F(0.05), 2, 0.5)), "sgd"
    if which == "adam_cosine":
        return OP.Adam(SC.CosineDecay(S.F(1e-3), 4, alpha=S.F(0.1))), "adam"
    return OP.RMSprop(SC.InverseTimeDecay(S.F(1e-3), 2, 0.5, staircase=True), momentum=0.9), "rmsprop_momentum"


def _trajectory(m, st, batches, B, gb, opt, kind, dtype):
    """The optimizer's float64 (or torch float32) trajectory from the store's weights: gradients of
    smallnet_oracle.oracle, the update of optim_oracle / optim_rmsprop_oracle with lr = schedule(k)."""
    W = {n: w.detach().clone() for n, w in O._weights(m, st, dtype, False).items()}
    z = {n: torch.zeros_like(w) for n, w in W.items()}
    s0, s1 = dict(z), {n: t.clone() for n, t in z.items()}
    hp = opt.hparams()
    for k, (x, y) in enumerate(batches):
        g = O.oracle(m, st, x, y, B, gb, None, dtype, weights=W)["grads"]
        h = dict(lr=opt.lr_at(k), **hp)
        for n in g:
            gn = g[n].to(dtype)
            if kind in R.KINDS:
                step = R.oracle_step if dtype == torch.float64 else R.fp32_step
                W[n], s0[n], s1[n] = step(kind, h, W[n], gn, s0[n], s1[n])
            else:
                step = OO.oracle_step if dtype == torch.float64 else OO.fp32_step
                W[n], a, b = step(kind, h, W[n], gn, s0[n], s1[n], k + 1)
                s0[n], s1[n] = (a if a is not None else s0[n]), (b if b is not None else s1[n])
    return W


@pytest.mark.parametrize("which", ["sgd_exponential", "adam_cosine", "rmsprop_momentum_inverse_time"])
@pytest.mark.parametrize("model", ["lenet5", "mlp_tanh"])
def test_smallnet_local_step_under_a_schedule(model, which):
    """Three steps: the scheduled weight-gradient launch ("local") against gradients to the bucket + the
    schedule launch + the multi-tensor launch ("plain") on a cloned store (1e-5 per variable and slot, the
    figure of test_smallnet_local_step_matches_plain), and against the float64 trajectory stepped with
    schedule(k) under max(TOL, REF_FACTOR x the torch-fp32 trajectory's error)."""
    tde, PG = _tde()
    tde.backend.set_random_seed(3)
    opt, kind = _opt_sched(tde, which)
    if model == "lenet5":
        m = _lenet(tde, opt)
        B = Bplan = 64
        batches = [_batch(m, 64, 10 + s) for s in range(3)]
    else:
        m, x, y = _mlp_case(tde, opt)
        B, Bplan = 5, 8
        batches = [(x, y)] * 3
    st = m._store
    st2 = st.clone_to(DEV)
    w0 = {n: st.view(n).detach().cpu().double().clone() for n in st.names(trainable=True)}
    w64 = _trajectory(m, st, batches, B, Bplan, opt, kind, torch.float64)
    w32 = _trajectory(m, st, batches, B, Bplan, opt, kind, torch.float32)
    a = PG.make_plan(m, st, DEV, Bplan, Bplan, m.optimizer, m.loss)
    b = PG.make_plan(m, st2, DEV, Bplan, Bplan, _opt_sched(tde, which)[0], m.loss)
    assert a.kind == "fused_smallnet" and a.supports_step_mode("local") and not a.supports_step_mode("xgmi")
    a.set_step_mode("local")
    assert a.step_mode == "local" and b.step_mode == "plain"
    for xx, yy in batches:
        xg, yg = xx.to(DEV), yy.to(DEV)
        a.train_step(xg, yg, B)
        b.train_step(xg, yg, B)
        b.apply()
    torch.cuda.synchronize()
    assert a.iterations.item() == b.iterations.item() == 3
    for n in w0:
        da, db = st.view(n).detach().cpu().double() - w0[n], st2.view(n).detach().cpu().double() - w0[n]
        r = O.rel(da, db)
        e, ref = O.rel(da, w64[n] - w0[n]), O.rel(w32[n].double() - w0[n], w64[n] - w0[n])
        print(f"[{model} {which}] {n}: local vs plain {r:.3g}; vs float64 {e:.3g}  torch-fp32 {ref:.3g}  "
              f"bound {O.bound(ref):.3g}")
        assert float(da.abs().max()) > 0
        assert r < 1e-5, (n, r)
        assert e <= O.bound(ref), (n, e, ref)
    for s in m.optimizer.slot_names():
        r = O.rel(st.slot(s), st2.slot(s))
        print(f"[{model} {which}] slot {s}: local vs plain {r:.3g}")
        assert r < 1e-5, (s, r)
    sch = m.optimizer.schedule
    name, kw = type(sch).__name__, {k: v for k, v in sch.get_config().items() if k != "name"}
    for plan in (a, b):
        assert abs(plan.opt.lr_word.item() - S.eval64(name, kw, 2)) <= S.bound(name, kw, 2), plan.step_mode
    assert abs(sch(2) - S.eval64(name, kw, 2)) <= 1e-15


# ------------------------------------------------------------------------------------- 5. fused plans fall back
def test_fused_cnn_runs_plain_under_a_schedule():
    """zoo.mnist_cnn + SGD(ExponentialDecay): the fused CNN plan in step mode "plain"; one train_step, then
    ``apply()`` on the gradient it left against the float64 oracle applied to that same gradient with the
    rate in the word, which is schedule(1) (one step was fitted before)."""
    tde, PG = _tde()
    tde.backend.set_random_seed(0)
    m = tde.zoo.mnist_cnn()
    kw = dict(initial_learning_rate=S.F(0.05), decay_steps=4, decay_rate=0.5)
    opt = tde.optimizers.SGD(tde.optimizers.schedules.ExponentialDecay(**kw))
    m.compile(loss=tde.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=opt, metrics=["accuracy"])
    rng = np.random.default_rng(0)
    x = rng.random((64, 28, 28, 1), dtype=np.float32)
    y = rng.integers(0, 10, size=64)
    h = m.fit(x, y, batch_size=64, epochs=1, verbose=0)
    assert np.isfinite(h.history["loss"][0])
    prog = m._program("train", 64)
    plan = prog.plans[0]
    assert prog.plan_kind == "fused_convnet" and plan.step_mode == "plain"
    assert not plan.supports_step_mode("local") and not plan.supports_step_mode("xgmi")
    prog.sync()
    assert plan.iterations.item() == 1
    assert abs(plan.opt.lr_word.item() - S.eval64("ExponentialDecay", kw, 0)) <= S.bound("ExponentialDecay", kw, 0)
    st = plan.store
    plan.train_step(torch.from_numpy(x).to(DEV, plan.input_dtype), torch.from_numpy(y.astype(np.int32)).to(DEV))
    torch.cuda.synchronize()
    g, w = st.g.cpu().clone(), st.w.cpu().clone()
    assert float(g.abs().max()) > 0
    plan.apply()
    torch.cuda.synchronize()
    lr = plan.opt.lr_word.item()
    e = abs(lr - S.eval64("ExponentialDecay", kw, 1))
    print(f"[mnist_cnn plain] lr word {lr!r}: |device - float64| {e:.3g} bound {S.bound('ExponentialDecay', kw, 1):.3g}")
    assert e <= S.bound("ExponentialDecay", kw, 1)
    hyper = dict(lr=lr, **opt.hparams())
    ow = OO.oracle_step("sgd", hyper, w.double(), g.double(), None, None, 2)[0]
    hw = OO.fp32_step("sgd", hyper, w, g, None, None, 2)[0]
    dw = st.w.cpu()
    fails = []
    for name in st.names(trainable=True):
        s = st.segments[name]
        sl = slice(s.offset, s.offset + s.numel)
        R.compare("mnist_cnn plain", "w", name, dw[sl], hw[sl], ow[sl], fails)
        assert float((dw[sl] - w[sl]).abs().max()) > 0, name
    assert not fails, fails
    assert float(st.g.abs().max()) == 0.0


@pytest.mark.parametrize("zoo", ["generic", "bn_cnn"])
def test_generic_and_bn_cnn_plans_report_plain(zoo):
    tde, PG = _tde()
    m = tde.zoo.mnist_cnn(filters=16, units=32) if zoo == "generic" else tde.zoo.mnist_bn_cnn()
    opt = tde.optimizers.Adam(tde.optimizers.schedules.CosineDecay(1e-3, 100))
    loss = tde.losses.SparseCategoricalCrossentropy(from_logits=True) if zoo == "generic" else "sparse_categorical_crossentropy"
    m.compile(loss=loss, optimizer=opt, metrics=["accuracy"])
    prog = m._program("train", 64)
    plan = prog.plans[0]
    assert prog.plan_kind == ("fused_convnet_generic" if zoo == "generic" else "fused_bncnn")
    assert plan.step_mode == "plain" and not plan.supports_step_mode("local") and not plan.supports_step_mode("xgmi")
    if zoo == "generic":
        m.compile(loss=loss, optimizer=tde.optimizers.Adam(1e-3), metrics=["accuracy"])     # the constant twin fuses
        assert m._program("train", 64).plans[0].step_mode == "local"


# ------------------------------------------------------------------------------------- 6. restore
@pytest.mark.parametrize("mode", ["local", "plain"])
def test_a_restored_step_counter_moves_the_rate(mode):
    tde, PG = _tde()
    kw = dict(initial_learning_rate=S.F(0.1), decay_steps=16, decay_rate=S.F(0.96))
    opt = tde.optimizers.SGD(tde.optimizers.schedules.ExponentialDecay(**kw))
    m, x, y = _mlp_case(tde, opt)
    B, Bplan = 5, 8
    st = m._store
    plan = PG.make_plan(m, st, DEV, Bplan, Bplan, m.optimizer, m.loss)
    plan.set_step_mode(mode)
    plan.set_iterations(100)
    w0 = {n: st.view(n).detach().cpu().double().clone() for n in st.names(trainable=True)}
    g64 = O.oracle(m, st, x, y, B, Bplan)["grads"]
    g32 = O.oracle(m, st, x, y, B, Bplan, dtype=torch.float32)["grads"]
    plan.train_step(x.to(DEV), y.to(DEV), B)
    if mode == "plain":
        plan.apply()
    torch.cuda.synchronize()
    assert plan.iterations.item() == 101
    lr = plan.opt.lr_word.item()
    e, b = abs(lr - S.eval64("ExponentialDecay", kw, 100)), S.bound("ExponentialDecay", kw, 100)
    print(f"[restore {mode}] lr word {lr!r}: |device - float64| {e:.3g} bound {b:.3g}")
    assert e <= b and abs(lr - kw["initial_learning_rate"]) > 0.01
    for n in w0:
        d = st.view(n).detach().cpu().double() - w0[n]
        err, ref = O.rel(d, -lr * g64[n]), O.rel(-(torch.tensor(lr, dtype=torch.float32) * g32[n]), -lr * g64[n])
        print(f"[restore {mode}] delta {n}: kernel {err:.3g}  torch-fp32 {ref:.3g}  bound {O.bound(ref):.3g}")
        assert err <= O.bound(ref), (n, err, ref)


# ------------------------------------------------------------------------------------- 7. fit
def test_fit_lenet5_adam_under_exponential_decay():
    tde, PG = _tde()
    tde.backend.set_random_seed(4)
    m = tde.zoo.lenet5()
    sch = tde.optimizers.schedules.ExponentialDecay(1e-3, 16, 0.5)
    m.compile(loss=tde.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=tde.optimizers.Adam(sch),
              metrics=["accuracy"], steps_per_execution=4)
    x, y = R.row_band_task()
    h = m.fit(x, y, batch_size=R.FIT_BATCH, epochs=R.FIT_EPOCHS, verbose=0)
    prog = m._program("train", R.FIT_BATCH)
    assert prog.plan_kind == "fused_smallnet" and prog.use_graph and len(prog.graphs) >= 1
    assert prog.plans[0].step_mode == "local"
    print(f"[schedule gpu fit] losses {h.history['loss']}")
    assert h.history["loss"][-1] < 0.5 * h.history["loss"][0]
    n = R.FIT_EPOCHS * (2048 // R.FIT_BATCH)
    assert m.optimizer.iterations == n == prog.plans[0].iterations.item()
    assert m.optimizer.current_lr() == sch(n)
    # the word holds the rate of the last update applied, number n - 1 (the device is given float32 parameters)
    kw = dict(initial_learning_rate=S.F(1e-3), decay_steps=16, decay_rate=0.5)
    e = abs(prog.plans[0].opt.lr_word.item() - S.eval64("ExponentialDecay", kw, n - 1))
    assert e <= S.bound("ExponentialDecay", kw, n - 1), e
