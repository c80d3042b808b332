"""RMSprop on the GPU: the multi-tensor launch (``tde_optim_apply`` kinds 4 / 5, csrc/kernels/optim.hip) on the
store of every awkward segment against the float64 oracle of tests/optim_rmsprop_oracle.py, the refusals of
the entry points that do not take the new kinds, the small-net plan's in-step update ("local",
csrc/kernels/smallnet.hip) against "plain", the fused CNN plan falling back to "plain", fit() and two
Mirrored replicas.

rms runs on the exact grid and must equal the oracle bit for bit; w and the momentum accumulator go through a
square root and a division and are held per tensor to max(4 e_host, 2^-22 max |oracle|), e_host being the
error of the same operations in torch float32 on the host.  Each comparison prints e_dev, e_host and the bound.
"""
import ctypes
import json
import os
import signal
import subprocess
import sys

import numpy as np
import pytest
import torch

import optim_rmsprop_oracle as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Rig:
    """The SEGMENTS store with the optimizer kernel of one RMSprop kind, and a sentinel-filled buffer that
    kind 4 receives as `v`."""

    def __init__(self, kind, hyper=R.GRID_HYPER):
        from tensorflow_distributed_example_amd.train.program import OptimizerKernel
        self.kind, self.hyper = kind, hyper
        self.store = st = R.make_store([(n, s) for n, s, _ in R.SEGMENTS], DEV)
        self.opt = R.optimizer(kind, hyper)
        assert self.opt.kind == kind and self.opt.kind_id == R.KIND_ID[kind]
        for s in self.opt.slot_names():
            st.slot(s)
        self.it = torch.zeros(1, dtype=torch.int64, device=DEV)
        self.ok = OptimizerKernel(st, self.opt, {n: sh for n, _, sh in R.SEGMENTS if sh}, self.it)
        self.idx = torch.arange(st.n_trainable)
        self.names = st.names(trainable=True)
        self.r = st.slot("rms")
        self.q = st.slot("momentum") if kind == "rmsprop_momentum" else None
        self.vsent = torch.full_like(st.w, R.V_SENTINEL) if self.q is None else None

    def load(self, w, r, q):
        self.store.w.copy_(w.float())
        self.r.copy_(r.float())
        if self.q is not None:
            self.q.copy_(q.float())
        self.ok.refresh_shadows()
        self.gaps = R.fill_store_gaps(self.store)
        self.shgaps = R.fill_shadow_gaps(self.ok)

    def set_grad(self, g):
        mask = R.seg_mask(self.store)
        self.store.g.copy_(torch.where(mask, g.float(), torch.tensor(R.O.W_SENTINEL)))

    def raw_apply(self, kind_id=None, lr=None, grad_scale=1.0, zero_grad=1, lr_ptr=None, v="default"):
        from tensorflow_distributed_example_amd import _native as N
        st, ok, h = self.store, self.ok, self.hyper
        vbuf = (self.q if self.q is not None else self.vsent) if isinstance(v, str) else v
        return N.hip().tde_optim_apply(st.w.data_ptr(), st.g.data_ptr(), N.ptr(self.r), N.ptr(vbuf),
                                       ok.shadow.data_ptr(), ok.segs_dev.data_ptr(), ok.table_dev.data_ptr(),
                                       ok.nblocks, self.it.data_ptr(),
                                       R.KIND_ID[self.kind] if kind_id is None else kind_id,
                                       h["lr"] if lr is None else lr, h["mom"], h["b1"], h["b2"], h["eps"], grad_scale,
                                       zero_grad, N.ptr(lr_ptr), N.stream_ptr())

    def seg(self, name, flat):
        s = self.store.segments[name]
        return flat[s.offset: s.offset + s.numel]

    def snapshot(self):
        bufs = [self.store.w, self.store.g, self.ok.shadow, self.r] + [b for b in (self.q, self.vsent) if b is not None]
        torch.cuda.synchronize()
        return [b.cpu().clone() for b in bufs]

    def assert_unchanged(self, snap, what):
        for a, b in zip(self.snapshot(), snap):
            d = R.first_diff(a, b)
            assert not d, f"{what}: {d}"

    def check(self, tag, orc, host, grad_zero=True, g_before=None):
        """rms bitwise == oracle; w (and q) within the bound; gradient zeroed (or bit-identical); shadows ==
        bf16 of the device's own weights; every gap and kind 4's `v` buffer untouched."""
        st, ok = self.store, self.ok
        torch.cuda.synchronize()
        dw, dr, dg = st.w.cpu(), self.r.cpu(), st.g.cpu()
        dq = self.q.cpu() if self.q is not None else None
        assert torch.isfinite(dw).all()
        fails = []
        for name in self.names:
            d = R.first_diff(self.seg(name, dr), self.seg(name, orc["r"]).float())
            assert not d, f"{tag} {name}: rms differs from the oracle: {d}"
            R.compare(tag, "w", name, self.seg(name, dw), self.seg(name, host["w"]), self.seg(name, orc["w"]), fails)
            if dq is not None:
                R.compare(tag, "q", name, self.seg(name, dq), self.seg(name, host["q"]), self.seg(name, orc["q"]), fails)
            if grad_zero:
                d = R.first_diff(self.seg(name, dg), torch.zeros(st.segments[name].numel))
                assert not d, f"{tag} {name}: gradient not zeroed: {d}"
            w2 = R.view2d(st, name, dw)
            if (name, "row") in ok.shadow_views:
                d = R.first_diff(ok.shadow_views[(name, "row")], w2.to(torch.bfloat16))
                assert not d, f"{tag} {name}: row shadow: {d}"
            if (name, "col") in ok.shadow_views:
                d = R.first_diff(ok.shadow_views[(name, "col")], w2.T.contiguous().to(torch.bfloat16))
                assert not d, f"{tag} {name}: col shadow: {d}"
        assert not fails, fails
        if g_before is not None:
            d = R.first_diff(dg, g_before)
            assert not d, f"{tag}: zero_grad = 0 changed g: {d}"
        R.assert_store_gaps(st, self.gaps)
        R.assert_shadow_gaps(ok, self.shgaps)
        if self.vsent is not None:
            d = R.first_diff(self.vsent, torch.full_like(self.vsent, R.V_SENTINEL))
            assert not d, f"{tag}: kind 4 touched the v buffer: {d}"


def _start(kind, hyper=R.GRID_HYPER):
    rig = Rig(kind, hyper)
    orc = dict(w=R.grid_w(rig.idx), r=R.grid_r(rig.idx), q=R.grid_q(rig.idx))
    host = {k: v.float() for k, v in orc.items()}
    rig.load(orc["w"], orc["r"], orc["q"])
    return rig, orc, host


def _advance(kind, hyper, orc, host, g, grad_scale=1.0):
    momentum = kind == "rmsprop_momentum"
    w, r, q = R.oracle_step(kind, hyper, orc["w"], g, orc["r"], orc["q"], grad_scale)
    orc.update(w=w, r=r, q=q if momentum else orc["q"])
    w, r, q = R.fp32_step(kind, hyper, host["w"], g.float(), host["r"], host["q"], grad_scale)
    host.update(w=w, r=r, q=q if momentum else host["q"])


@pytest.mark.parametrize("kind", R.KINDS)
def test_apply_three_steps_against_oracle(kind):
    rig, orc, host = _start(kind)
    for step in range(3):
        g = R.grid_g(rig.idx, step)
        rig.set_grad(g)
        rig.it += 1
        if step == 0:
            assert rig.raw_apply() == 0          # the raw entry point, kind 4 with a sentinel-filled v
        else:
            rig.ok.apply()                        # the plan's own call (kind 4 passes no v)
        _advance(kind, R.GRID_HYPER, orc, host, g)
        rig.check(f"{kind} step {step + 1}", orc, host)
    assert rig.it.item() == 3


def test_apply_grad_scale():
    kind = "rmsprop_momentum"
    rig, orc, host = _start(kind)
    g = R.grid_g(rig.idx, 0)
    rig.set_grad(g)
    plain = R.oracle_step(kind, R.GRID_HYPER, orc["w"], g, orc["r"], orc["q"])
    assert rig.raw_apply(grad_scale=0.25) == 0
    _advance(kind, R.GRID_HYPER, orc, host, g, grad_scale=0.25)
    assert not torch.equal(orc["r"], plain[1])
    rig.check(f"{kind} grad_scale", orc, host)


def test_apply_keeps_grad():
    kind = "rmsprop"
    rig, orc, host = _start(kind)
    g = R.grid_g(rig.idx, 0)
    rig.set_grad(g)
    g_before = rig.store.g.cpu().clone()
    assert rig.raw_apply(zero_grad=0) == 0
    _advance(kind, R.GRID_HYPER, orc, host, g)
    rig.check(f"{kind} zero_grad=0", orc, host, grad_zero=False, g_before=g_before)
    assert rig.raw_apply(zero_grad=1) == 0       # the kept gradient again, now zeroed
    _advance(kind, R.GRID_HYPER, orc, host, g)
    rig.check(f"{kind} zero_grad=1", orc, host)


def test_apply_lr_ptr_overrides_lr():
    kind = "rmsprop_momentum"
    rig, orc, host = _start(kind)
    g = R.grid_g(rig.idx, 0)
    rig.set_grad(g)
    lr_dev = torch.tensor([0.25], dtype=torch.float32, device=DEV)
    assert rig.raw_apply(lr=0.5, lr_ptr=lr_dev) == 0
    hyper = dict(R.GRID_HYPER, lr=0.25)
    other = R.oracle_step(kind, dict(hyper, lr=0.5), orc["w"], g, orc["r"], orc["q"])[0]
    _advance(kind, hyper, orc, host, g)
    assert not torch.equal(orc["w"], other)
    rig.check(f"{kind} lr_ptr", orc, host)
    assert lr_dev.item() == 0.25


def test_refusals_write_nothing():
    from tensorflow_distributed_example_amd import _native as N
    rig, orc, host = _start("rmsprop_momentum")
    g = R.grid_g(rig.idx, 0)
    rig.set_grad(g)
    snap = rig.snapshot()
    assert rig.raw_apply(kind_id=6) != 0
    rig.assert_unchanged(snap, "kind 6")
    assert rig.raw_apply(kind_id=-1) != 0
    rig.assert_unchanged(snap, "kind -1")
    assert rig.raw_apply(v=None) != 0
    rig.assert_unchanged(snap, "kind 5 without v")
    st, h = rig.store, R.GRID_HYPER
    rng = (ctypes.c_int * 2)(0, 8)
    pend = torch.ones(1, dtype=torch.int32, device=DEV)
    count = torch.zeros(1, dtype=torch.int64, device=DEV)
    for kind_id in (4, 5):
        rc = N.hip().tde_flat_apply(st.w.data_ptr(), st.g.data_ptr(), rig.r.data_ptr(), rig.q.data_ptr(),
                                    rig.it.data_ptr(), pend.data_ptr(), kind_id, h["lr"], h["mom"], h["b1"], h["b2"],
                                    h["eps"], rng, 1, 0, st.w.numel(), count.data_ptr(), N.stream_ptr())
        assert rc == -1
    rig.assert_unchanged(snap, "tde_flat_apply with an RMSprop kind")
    assert pend.item() == 1 and count.item() == 0
    assert rig.raw_apply() == 0                   # and the same arguments do update when accepted
    _advance("rmsprop_momentum", R.GRID_HYPER, orc, host, g)
    rig.check("after refusals", orc, host)


# --------------------------------------------------------------------------------- small-net "local"
def _lenet(tde, opt):
    m = tde.zoo.lenet5()
    m.compile(loss=tde.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=opt, metrics=["accuracy"])
    m.build()
    return m


def _batch(m, n, seed):
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.standard_normal((n,) + tuple(m.input_shape[1:])).astype(np.float32)).cuda()
    y = torch.from_numpy(rng.integers(0, 10, n).astype(np.int32)).cuda()
    return x, y


def _rel(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()


@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_smallnet_local_step_matches_plain(momentum):
    """LeNet-5, batch 64, three steps: the in-step update against gradients to the bucket + the multi-tensor
    launch on a cloned store, as tests/test_smallnet_gpu.py::test_smallnet_local_step_matches_plain."""
    import tensorflow_distributed_example_amd as tde
    from tensorflow_distributed_example_amd.train import program as PG

    def mk():
        return tde.optimizers.RMSprop(1e-3, momentum=momentum)
    tde.backend.set_random_seed(3)
    m = _lenet(tde, mk())
    st = m._store
    st2 = st.clone_to("cuda")
    w0 = st.w.clone()
    a = PG.make_plan(m, st, "cuda", 64, 64, m.optimizer, m.loss)
    b = PG.make_plan(m, st2, "cuda", 64, 64, mk(), m.loss)
    assert a.kind == "fused_smallnet" and a.supports_step_mode("local") and not a.supports_step_mode("xgmi")
    a.set_step_mode("local")
    for s in range(3):
        x, y = _batch(m, 64, 10 + s)
        a.train_step(x, y)
        b.train_step(x, y)
        b.apply()
    torch.cuda.synchronize()
    for n in st.names(trainable=True):
        sg = st.segments[n]
        w = w0[sg.offset: sg.offset + sg.numel].view(sg.shape)
        r = _rel(st.view(n) - w, st2.view(n) - w)    # the accumulated updates
        print(f"[smallnet local vs plain, momentum {momentum}] {n}: {r:.3g}")
        assert r < 1e-5, (n, r)
        assert float((st.view(n) - w).abs().max()) > 0
    for s in m.optimizer.slot_names():
        r = _rel(st.slot(s), st2.slot(s))
        print(f"[smallnet local vs plain, momentum {momentum}] slot {s}: {r:.3g}")
        assert r < 1e-5, (s, r)
    assert a.iterations.item() == b.iterations.item() == 3


# ------------------------------------------------------------------------------- fused CNN fallback
def test_fused_cnn_runs_plain_under_rmsprop():
    """zoo.mnist_cnn + RMSprop: the fused CNN plan, step mode "plain"; one train_step, then ``apply()`` on the
    gradient it left against the float64 oracle applied to that same gradient."""
    import tensorflow_distributed_example_amd as tde
    tde.backend.set_random_seed(0)
    m = tde.zoo.mnist_cnn()
    opt = tde.optimizers.RMSprop()
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
    st = plan.store
    plan.train_step(torch.from_numpy(x).to(DEV, plan.input_dtype), torch.from_numpy(y.astype(np.int32)).to(DEV))
    torch.cuda.synchronize()
    g, w, r = st.g.cpu().clone(), st.w.cpu().clone(), st.slot("rms").cpu().clone()
    assert float(g.abs().max()) > 0 and float(r.max()) > 0
    plan.apply()
    torch.cuda.synchronize()
    hyper = dict(lr=opt.learning_rate, **opt.hparams())
    ow, orr, _ = R.oracle_step("rmsprop", hyper, w.double(), g.double(), r.double(), None)
    hw, hr, _ = R.fp32_step("rmsprop", hyper, w, g, r, None)
    dw, dr = st.w.cpu(), st.slot("rms").cpu()
    fails = []
    for name in st.names(trainable=True):
        s = st.segments[name]
        sl = slice(s.offset, s.offset + s.numel)
        R.compare("mnist_cnn plain", "w", name, dw[sl], hw[sl], ow[sl], fails)
        R.compare("mnist_cnn plain", "rms", name, dr[sl], hr[sl], orr[sl], fails)
        assert float((dw[sl] - w[sl]).abs().max()) > 0, name
    assert not fails, fails
    assert float(st.g.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ fit
def test_fit_lenet5_rmsprop():
    """fit() of LeNet-5 with RMSprop(): the fused small-net plan, hipGraph executions, the in-step update;
    the loss criterion and the epoch count are those fixed on the CPU (optim_rmsprop_oracle.FIT_EPOCHS)."""
    import tensorflow_distributed_example_amd as tde
    tde.backend.set_random_seed(4)
    m = tde.zoo.lenet5()
    m.compile(loss=tde.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=tde.optimizers.RMSprop(),
              metrics=["accuracy"], steps_per_execution=4)
    x, y = R.row_band_task()
    h = m.fit(x, y, batch_size=R.FIT_BATCH, epochs=R.FIT_EPOCHS, verbose=0)
    prog = m._program("train", R.FIT_BATCH)
    assert prog.plan_kind == "fused_smallnet" and prog.use_graph
    assert prog.plans[0].step_mode == "local"
    print(f"[rmsprop gpu fit] losses {h.history['loss']}")
    assert h.history["loss"][-1] < 0.5 * h.history["loss"][0]
    assert m.optimizer.iterations == R.FIT_EPOCHS * (2048 // R.FIT_BATCH)


# ------------------------------------------------------------------------------------------- mirrored
def test_mirrored_replicas_apply_rmsprop_after_a_plain_allreduce():
    """Two Mirrored replicas rehearsed on cuda:0 (tests/rmsprop_mirrored_child.py): the all-reduce does not
    apply the update, every replica's multi-tensor launch does, and the replicas stay bit-identical."""
    env = dict(os.environ, TDE_HEARTBEAT="0", OMP_NUM_THREADS="2", TDE_XGMI_TIMEOUT="20")
    p = subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "rmsprop_mirrored_child.py")], env=env, cwd=ROOT,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, start_new_session=True)
    try:
        out, _ = p.communicate(timeout=90)
    except subprocess.TimeoutExpired:
        os.killpg(p.pid, signal.SIGKILL)
        out, _ = p.communicate()
        raise AssertionError(f"timed out:\n{out[-3000:]}")
    assert p.returncode == 0, out[-4000:]
    res = json.loads([l for l in out.splitlines() if l.startswith("RESULT ")][0][7:])
    print(res)
    assert res["plan"] == "fused_smallnet" and res["step_modes"] == ["plain", "plain"], res
    assert res["comm_applies"] is False, res
    assert res["slots"] == ["rms"] and res["iterations"] == [3, 3], res
    assert res["w_identical"] and res["slots_identical"], res
    assert res["w_moved"] > 0 and res["rms_max"] > 0, res
