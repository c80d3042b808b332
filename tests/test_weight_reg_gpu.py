"""Weight regularizers and decoupled weight decay on the GPU (csrc/include/tde_reg.h, csrc/kernels/weightreg.hip,
the WD variants of csrc/kernels/optim.hip, ``WeightRegKernel`` / ``OptimizerKernel``):

1. the regularizer launches alone on the segments of tests/optim_oracle.py plus a 1-element segment, one of
   exactly one chunk and one of a chunk plus 5, some of them unregularized (bit for bit on a dyadic grid, within
   weight_reg_oracle's bounds of float64 on normal data, bitwise repeatable, gaps and unregularized segments
   poisoned, null g, refusals), and a segment of 300 chunks + 3 for the finish launch's strided loop;
2. the WD apply for the six optimizer kinds x {no clip, clipvalue, global_clipnorm} against the optimizer oracles
   fed the host's f32(w - f32(f32(w * wd) * lr)) under the rules of tests/test_optim_gpu.py /
   tests/test_optim_rmsprop_gpu.py; a wd == 0 segment bitwise the non-WD launch; shadows; a rate through lr_ptr;
3. three steps of the plans against the float64 autograd oracle (lenet5 small-net, mnist_cnn fused CNN,
   mini_resnet layer-wise in fp32 and mixed_bfloat16), the fit / evaluate losses;
4. two Mirrored replicas in a child process.

``-s`` prints every figure before it is asserted.
"""
import json
import os
import signal
import subprocess
import sys

import numpy as np
import pytest
import torch

import grad_clip_oracle as G
import optim_oracle as OO
import optim_rmsprop_oracle as R
import smallnet_oracle as O
import test_grad_clip_gpu as TC
import weight_reg_oracle as W

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEGMENTS = OO.SEGMENTS + G.EXTRA_SEGMENTS
# coefficients by segment index mod 4: an l1_l2, none, an l2, an l1 (powers of two: exact on the dyadic grid)
COEFS = [(0.25, 0.125), (0.0, 0.0), (0.0, 0.5), (0.5, 0.0)]
SENT = OO.W_SENTINEL


def _tde():
    return TC._tde()


def _N():
    return TC._N()


class RegRig:
    """A store of ``segments`` and the regularizer launches over it; coefficient of segment i: coefs[i % len]."""

    def __init__(self, segments=SEGMENTS, coefs=COEFS):
        _, PG = _tde()
        self.store = st = OO.make_store([(n, s) for n, s, _ in segments], DEV)
        self.names = st.names(trainable=True)
        self.coefs = [tuple(OO.f32(c) for c in coefs[i % len(coefs)]) for i in range(len(self.names))]
        self.segs = [(st.segments[n].offset, st.segments[n].numel) for n in self.names]
        self.reg_segs = [(o, n, a, b) for (o, n), (a, b) in zip(self.segs, self.coefs) if a or b]
        self.rk = PG.WeightRegKernel(st, self.reg_segs)
        self.n = st.n_trainable
        self.idx = torch.arange(self.n)
        self.mask = OO.seg_mask(st)
        self.regmask = torch.zeros(self.n, dtype=torch.bool)
        for o, n, _, _ in self.reg_segs:
            self.regmask[o: o + n] = True

    def load(self, w, g):
        """w into the segments (sentinel in the gaps), g into the regularized segments (sentinel elsewhere)."""
        self.store.w.copy_(torch.where(self.mask, w.float(), torch.tensor(SENT)))
        self.store.g.copy_(torch.where(self.regmask, g.float(), torch.tensor(SENT)))
        return self.store.w.cpu().clone(), self.store.g.cpu().clone()

    def want(self, w32, g32):
        """float64: (g after the launch, the partials, the penalty) from the float32 inputs."""
        g = g32.double().clone()
        parts = []
        for o, n, a, b in self.reg_segs:
            x = w32[o: o + n].double()
            g[o: o + n] += W.reg_grad(x, a, b)
            for c in range(W.chunks(n)):
                parts.append(float(W.penalty(x[c * W.CHUNK: (c + 1) * W.CHUNK], a, b)))
        parts = torch.tensor(parts, dtype=torch.float64)
        return g, parts, float(parts.sum())

    def launch(self, g=True, metrics=None, rows=0):
        self.rk.grad(self.store.g if g else None)
        self.rk.finish(metrics, rows)
        torch.cuda.synchronize()
        return self.store.g.cpu().clone(), self.rk.partials.cpu().clone(), self.rk.penalty.cpu().clone()


def _dyadic(rig):
    """w: multiples of 1/8 below 4 with +0, -0 and both signs; g: multiples of 2^-6 below 4.  With the
    power-of-two coefficients every product, the gradient and every partial sum (multiples of 2^-9 below
    2^14) is exact in float32 whatever the order."""
    w = torch.round(OO.grid_w(rig.idx) * 8) / 8
    for o, n, _, _ in rig.reg_segs:
        if n >= 8:
            w[o + 1], w[o + 2], w[o + n - 1] = 0.0, -0.0, -0.0
    return w, OO.grid_g(rig.idx, 0)


# ------------------------------------------------------------------------------------- 1. the kernels alone
def test_table_holds_the_regularized_segments_only():
    rig = RegRig()
    ents = rig.rk.ents_dev.cpu().tolist()[: rig.rk.nent]
    want = [(i, c) for i, ((o, n), (a, b)) in enumerate(zip(rig.segs, rig.coefs)) if a or b for c in range(W.chunks(n))]
    # the kernel's own segment list holds the regularized segments only: entry i names its position there
    pos = {i: k for k, i in enumerate(i for i, (a, b) in enumerate(rig.coefs) if a or b)}
    assert [tuple(e) for e in ents] == [(pos[i], c) for i, c in want]
    assert 0 < len(rig.reg_segs) < len(rig.segs)
    assert sorted(n for _, n, _, _ in rig.reg_segs if n in (1, W.CHUNK, W.CHUNK + 5))   # extra segments take part


def test_bit_exact_on_the_dyadic_grid_with_signed_zeros():
    rig = RegRig()
    w, g = _dyadic(rig)
    w32, g32 = rig.load(w, g)
    assert int(((w32 == 0) & torch.signbit(w32) & rig.regmask).sum()) > 0 and int(((w32 == 0) & ~torch.signbit(w32) & rig.regmask).sum()) > 0
    assert int(((w32 > 0) & rig.regmask).sum()) > 100 and int(((w32 < 0) & rig.regmask).sum()) > 100
    metrics = torch.tensor([1.5, 3.0, 8.0, 0.0], device=DEV)
    g_dev, parts, pen = rig.launch(metrics=metrics, rows=8)
    g64, p64, pen64 = rig.want(w32, g32)
    assert torch.equal(g64.float().double(), g64) and torch.equal(p64.float().double(), p64)      # the construction
    d = OO.first_diff(g_dev, g64.float())
    assert not d, f"g: {d}"
    d = OO.first_diff(parts[: rig.rk.nent], p64.float())
    assert not d, f"partials: {d}"
    print(f"penalty {pen.item()!r} float64 {pen64!r}")
    assert pen.item() == float(np.float32(pen64))
    assert metrics.cpu().tolist() == [float(np.float32(8.0 * float(np.float32(pen64)) + 1.5)), 3.0, 8.0, 0.0]
    # +-0 get no l1 gradient; gaps and unregularized segments untouched, w only read
    z = (w32 == 0) & rig.regmask
    assert torch.equal(g_dev[z], g32[z])
    assert torch.equal(g_dev[~rig.regmask].view(torch.int32), g32[~rig.regmask].view(torch.int32))
    assert bool((g_dev[~rig.regmask] == SENT).all()) and not OO.first_diff(rig.store.w, w32)


def test_normal_data_within_the_derived_bounds_and_bitwise_repeatable():
    rig = RegRig(coefs=[(0.013, 0.0007), (0.0, 0.0), (0.0, 0.021), (0.3, 0.0)])
    gen = torch.Generator().manual_seed(17)
    w32, g32 = rig.load(torch.randn(rig.n, generator=gen), torch.randn(rig.n, generator=gen))
    g_dev, parts, pen = rig.launch()
    g64, p64, pen64 = rig.want(w32, g32)
    worst = 0.0
    for o, n, a, b in rig.reg_segs:
        x = w32[o: o + n].double()
        scale = g32[o: o + n].double().abs() + (2 * b * x).abs() + a
        worst = max(worst, float(((g_dev[o: o + n].double() - g64[o: o + n]).abs() / scale).max()))
    ep = float(((parts[: rig.rk.nent].double() - p64).abs() / p64).max())
    et = abs(pen.item() - pen64) / pen64
    print(f"g rel {worst / 2.0 ** -24:.3g} x 2^-24 (allowed {W.GRAD_TOL / 2.0 ** -24:.3g}); partials rel "
          f"{ep / 2.0 ** -24:.3g}, penalty rel {et / 2.0 ** -24:.3g} x 2^-24 (allowed {W.PENALTY_TOL / 2.0 ** -24:.3g})")
    assert worst <= W.GRAD_TOL and ep <= W.PENALTY_TOL and et <= W.PENALTY_TOL
    assert torch.equal(g_dev[~rig.regmask].view(torch.int32), g32[~rig.regmask].view(torch.int32))
    # a second run from the same inputs: bitwise the same outputs
    rig.store.g.copy_(g32)
    rig.rk.partials.fill_(-3.0)
    rig.rk.penalty.fill_(-3.0)
    g2, parts2, pen2 = rig.launch()
    for a, b, what in ((g2, g_dev, "g"), (parts2, parts, "partials"), (pen2, pen, "penalty")):
        d = OO.first_diff(a, b)
        assert not d, f"second run, {what}: {d}"
    # a null g: the partials and the penalty again, g untouched
    rig.store.g.copy_(g32)
    rig.rk.partials.fill_(-3.0)
    g3, parts3, pen3 = rig.launch(g=False)
    assert not OO.first_diff(g3, g32) and not OO.first_diff(parts3, parts) and not OO.first_diff(pen3, pen)


def test_finish_over_300_chunks_and_3():
    """301 partials: past the 256 threads of the finish launch.  w = +-1/2, l2 = 1: every partial 1024 but the last."""
    rig = RegRig([G.LONG_SEGMENT], coefs=[(0.0, 1.0)])
    assert rig.rk.nent == 301
    w32, g32 = rig.load(torch.where(rig.idx % 2 == 0, 0.5, -0.5), torch.zeros(rig.n))
    g_dev, parts, pen = rig.launch()
    assert parts.tolist() == [1024.0] * 300 + [0.75] and pen.item() == 307200.75
    assert torch.equal(g_dev[rig.regmask], w32[rig.regmask] * 2) and bool((g_dev[~rig.regmask] == SENT).all())
    gen = torch.Generator().manual_seed(3)
    w32, g32 = rig.load(torch.randn(rig.n, generator=gen), torch.zeros(rig.n))
    _, _, pen = rig.launch(g=False)
    pen64 = float(w32[rig.regmask].double().square().sum())
    print(f"long: penalty rel {abs(pen.item() - pen64) / pen64 / 2.0 ** -24:.3g} x 2^-24")
    assert abs(pen.item() - pen64) <= W.PENALTY_TOL * pen64


def test_refusals_launch_nothing():
    rig = RegRig()
    w, g = _dyadic(rig)
    rig.load(w, g)
    rk, st, N = rig.rk, rig.store, _N()
    lib, s = N.hip(), N.stream_ptr()
    rk.partials.fill_(-3.0)
    rk.penalty.fill_(-3.0)
    metrics = torch.full((4,), 2.0, device=DEV)
    bufs = [st.w, st.g, rk.partials, rk.penalty, metrics]
    torch.cuda.synchronize()
    snap = [b.cpu().clone() for b in bufs]
    args = [st.w.data_ptr(), st.g.data_ptr(), rk.segs_dev.data_ptr(), rk.coef_dev.data_ptr(), rk.ents_dev.data_ptr(),
            rk.nent, rk.partials.data_ptr(), s]
    for i, bad in ((0, None), (0, st.w.data_ptr() + 4), (1, st.g.data_ptr() + 4), (2, None), (3, None), (4, None),
                   (5, -1), (6, None), (6, rk.partials.data_ptr() + 2)):
        a = list(args)
        a[i] = bad
        assert lib.tde_reg_grad(*a) == -1, (i, bad)
    fin = [rk.partials.data_ptr(), rk.nent, rk.penalty.data_ptr(), metrics.data_ptr(), 8, s]
    for i, bad in ((0, None), (1, -1), (2, None), (2, rk.penalty.data_ptr() + 2), (3, metrics.data_ptr() + 1), (4, -1)):
        a = list(fin)
        a[i] = bad
        assert lib.tde_reg_finish(*a) == -1, (i, bad)
    torch.cuda.synchronize()
    for b, was in zip(bufs, snap):
        assert not OO.first_diff(b, was)
    assert lib.tde_reg_grad(*args) == 0 and lib.tde_reg_finish(*fin) == 0      # and the same arguments do run
    torch.cuda.synchronize()
    assert rk.penalty.item() > 0 and metrics[0].item() == float(np.float32(2.0 + 8.0 * rk.penalty.item()))


# ------------------------------------------------------------------------------------- 2. the WD apply
WD_PATTERN = [0.5, 0.0, 0.25, 0.125, 0.0]          # by segment index mod 5: some variables excluded
CLIPS = {"none": None, "clipvalue": ("clipvalue", 1.5), "global_clipnorm": ("global_clipnorm", 8.0)}


class WdRig(TC.Rig):
    """tests/test_grad_clip_gpu.py's rig with a decaying optimizer and any clip (or none)."""

    def __init__(self, kind, clip, segments=SEGMENTS, wd=0.5):
        _, PG = _tde()
        self.kind, self.hyper = kind, TC._hyper(kind)
        self.mode, self.c = clip if clip else (None, 0.0)
        self.store = st = OO.make_store([(n, s) for n, s, _ in segments], DEV)
        self.opt = TC._optimizer(kind, weight_decay=wd, **({self.mode: self.c} if clip else {}))
        assert self.opt.kind == kind and self.opt.decay == wd
        self.slots = [st.slot(s) for s in self.opt.slot_names()]
        self.it = torch.zeros(1, dtype=torch.int64, device=DEV)
        self.ok = PG.OptimizerKernel(st, self.opt, {n: sh for n, _, sh in segments if sh}, self.it)
        self.idx = torch.arange(st.n_trainable)
        self.names = st.names(trainable=True)
        self.segs = G.store_segments(st)
        self.mask = OO.seg_mask(st)
        assert self.ok.wd_dev.cpu().tolist() == [wd] * len(self.names)
        self.wd = [WD_PATTERN[i % len(WD_PATTERN)] for i in range(len(self.names))]
        self.wd_dev = torch.tensor(self.wd, dtype=torch.float32, device=DEV)

    def wd_per_element(self):
        out = torch.zeros(self.store.n_trainable, dtype=torch.float32)
        for (o, n), d in zip(self.segs, self.wd):
            out[o: o + n] = d
        return out

    def apply_wd(self, grad_scale=1.0, zero_grad=1, lr_ptr=None, wd="own", mode="own", c=None, scale="own", w_off=0,
                 kind_id=None):
        N, ok, st, h = _N(), self.ok, self.store, self.hyper
        m, v = (self.slots + [None, None])[:2]
        mode = (G.MODE_ID[self.mode] if self.mode else 0) if mode == "own" else mode
        sc = ok.clip_scale if isinstance(scale, str) else scale
        wdp = self.wd_dev if isinstance(wd, str) else wd
        return N.hip().tde_optim_apply_wd(
            st.w.data_ptr() + w_off, st.g.data_ptr(), N.ptr(m), N.ptr(v), ok.shadow.data_ptr(), ok.segs_dev.data_ptr(),
            ok.table_dev.data_ptr(), ok.nblocks, self.it.data_ptr(),
            TC.ALL_KINDS.index(self.kind) if kind_id is None else kind_id, h["lr"], h["mom"], h["b1"], h["b2"], h["eps"],
            grad_scale, zero_grad, N.ptr(lr_ptr), mode, self.c if c is None else c, N.ptr(sc), N.ptr(wdp), N.stream_ptr())

    def plain_apply(self, grad_scale=1.0):
        """The launch without the decay: tde_optim_apply, or tde_optim_apply_clip under a clip."""
        return self.raw_apply(clip=self.mode is not None, grad_scale=grad_scale)

    def decayed(self, w64, lr):
        """The host's f32(w - f32(f32(w * wd) * lr)) from the float64 copy of the float32 weights."""
        w = w64.float()
        return (w - (w * self.wd_per_element()) * torch.tensor(lr, dtype=torch.float32)).double()

    def g_eff(self, g, gs):
        x = g.float() * torch.tensor(gs, dtype=torch.float32)
        if self.mode == "clipvalue":
            return x.clamp(-self.c, self.c)
        if self.mode == "global_clipnorm":
            return x * self.scale_per_element()
        return x


@pytest.mark.parametrize("clip", list(CLIPS))
@pytest.mark.parametrize("kind", TC.ALL_KINDS)
def test_wd_apply_against_the_oracles(kind, clip):
    """Two steps, grad_scale 0.5 then 1 (zero_grad off, then on): the optimizer oracles stepped from the host's
    decayed weight with the effective gradient formed on the host in the kernel's order."""
    rig = WdRig(kind, CLIPS[clip])
    state = rig.start()
    fails = []
    for t, (gs, zg) in enumerate(((0.5, 0), (1.0, 1)), start=1):
        g = OO.grid_g(rig.idx, t)
        rig.set_grad(g)
        g_before = rig.store.g.cpu().clone()
        rig.it += 1
        if clip == "global_clipnorm":
            assert rig.norm_launches() == 0
        assert rig.apply_wd(grad_scale=gs, zero_grad=zg) == 0
        torch.cuda.synchronize()
        if clip == "global_clipnorm":
            assert 0 < rig.ok.clip_scale.item() < 1.0
        start = rig.decayed(state[0], rig.hyper["lr"])
        moved = (start != state[0]) & rig.mask
        assert int(moved.sum()) > 1000 and int((~moved & rig.mask).sum()) > 1000        # decayed and excluded variables
        state = rig.step_and_compare(f"{kind} {clip} t={t}", [start] + state[1:], rig.g_eff(g, gs), t, fails)
        rig.check_layout(f"{kind} {clip} t={t}", grad_zero=bool(zg))                    # shadows == the final weights
        if not zg:
            assert not OO.first_diff(rig.store.g, g_before), "zero_grad = 0 changed g"
        state = [rig.store.w.cpu().double()] + [b.cpu().double() for b in rig.slots] + [None] * (2 - len(rig.slots))
    assert not fails, fails


@pytest.mark.parametrize("kind", ["sgd", "momentum", "nesterov"])
def test_wd_apply_is_bit_exact_on_the_grid(kind):
    """Kinds 0..2 on the exact grid (lr, wd powers of two): the decay and the step are exact, the device equals the
    float64 oracle bit for bit."""
    rig = WdRig(kind, None)
    state = rig.start()
    g = OO.grid_g(rig.idx, 0)
    rig.set_grad(g)
    rig.it += 1
    assert rig.apply_wd() == 0
    torch.cuda.synchronize()
    start = state[0] - (state[0] * rig.wd_per_element().double()) * rig.hyper["lr"]
    assert torch.equal(start.float().double(), start)
    new = OO.oracle_step(kind, rig.hyper, start, g, state[1], state[2], 1)
    dev = [rig.store.w.cpu()] + [b.cpu() for b in rig.slots]
    for name in rig.names:
        for d, o in zip(dev, new):
            diff = OO.first_diff(rig.seg(name, d).double(), rig.seg(name, o), bitwise=False)
            assert not diff, f"{kind} {name}: {diff}"
    rig.check_layout(f"grid {kind}")


@pytest.mark.parametrize("clip", ["none", "global_clipnorm"])
@pytest.mark.parametrize("kind", TC.ALL_KINDS)
def test_a_segment_without_decay_is_bitwise_the_launch_without_it(kind, clip):
    outs = []
    for wd in (True, False):
        rig = WdRig(kind, CLIPS[clip] and ("global_clipnorm", 0.5))
        rig.start(exact_grid=False, seed=3)
        gen = torch.Generator().manual_seed(5)
        rig.set_grad(torch.randn(rig.store.n_trainable, generator=gen).double())
        rig.it += 1
        if clip != "none":
            assert rig.norm_launches() == 0
        assert (rig.apply_wd(grad_scale=0.25) if wd else rig.plain_apply(grad_scale=0.25)) == 0
        torch.cuda.synchronize()
        if clip != "none":
            assert 0 < rig.ok.clip_scale.item() < 1.0
        outs.append([b.cpu().clone() for b in [rig.store.w, rig.store.g] + rig.slots] + [rig])
    (a, b), rig = (o[:-1] for o in outs), outs[0][-1]
    same = differ = 0
    for (o, n), d in zip(rig.segs, rig.wd):
        for x, y in zip(a, b):
            if d == 0.0:
                diff = OO.first_diff(x[o: o + n], y[o: o + n])
                assert not diff, f"{kind} {clip} segment at {o}: {diff}"
        same += d == 0.0
        differ += d != 0.0 and not torch.equal(a[0][o: o + n], b[0][o: o + n])
    assert same >= 4 and differ >= 8
    # and the shadows of both launches are the bf16 of their own final weights
    for o in outs:
        o[-1].check_layout(f"{kind} {clip}")


def test_the_decay_uses_the_scheduled_rate():
    """lr_ptr: the decay and the step read the rate 0.25 from the device word, not the 0.125 passed by value."""
    rig = WdRig("sgd", None)
    state = rig.start()
    g = OO.grid_g(rig.idx, 0)
    rig.set_grad(g)
    lr_dev = torch.tensor([0.25], dtype=torch.float32, device=DEV)
    assert rig.apply_wd(lr_ptr=lr_dev) == 0
    torch.cuda.synchronize()
    rig.hyper = dict(rig.hyper, lr=0.25)
    start = rig.decayed(state[0], 0.25)
    assert float((start - rig.decayed(state[0], 0.125)).abs().max()) > 0.1
    fails = []
    rig.step_and_compare("lr_ptr + wd", [start] + state[1:], g.float(), 1, fails)
    assert not fails, fails
    rig.check_layout("lr_ptr + wd")


def test_wd_refusals_write_nothing():
    rig = WdRig("momentum", ("global_clipnorm", 0.5))
    rig.start()
    rig.set_grad(OO.grid_g(rig.idx, 0))
    assert rig.norm_launches() == 0
    snap = rig.snapshot()
    assert rig.apply_wd(wd=None) == -3
    assert rig.apply_wd(mode=4) == -3 and rig.apply_wd(mode=-1) == -3
    assert rig.apply_wd(mode=1, c=0.0) == -3 and rig.apply_wd(mode=1, c=float("nan")) == -3
    assert rig.apply_wd(scale=None) == -3
    assert rig.apply_wd(w_off=4) == -1 and rig.apply_wd(kind_id=6) == -2
    rig.assert_unchanged(snap, "a refused call")
    assert rig.apply_wd(mode=0, scale=None) == 0                     # no clip needs no scale
    torch.cuda.synchronize()
    assert float((rig.store.w.cpu() - snap[0])[rig.mask].abs().max()) > 0


def test_an_optimizer_without_the_feature_builds_none_of_it():
    _, PG = _tde()
    rig = TC.Rig("sgd", "clipvalue", 1.0)
    assert rig.ok.reg is None and rig.ok.wd_dev is None


# ------------------------------------------------------------------------------------- 3. the plans
BPLAN = 8


def _compile(tde, m, opt):
    m.compile(loss=tde.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=opt, metrics=["accuracy"])
    m.build()
    return m


def _regularize(tde, m, kernel, bias=None):
    """Puts coefficients on every conv / dense kernel (and bias) of a zoo model before its store exists."""
    RG = tde.regularizers
    for layer in m.layers:
        for s in layer.weight_specs:
            r = kernel if s.name == "kernel" else bias if s.name == "bias" else None
            if r is not None:
                s.l1, s.l2 = RG.get(r).coefficients
    return m


def _reference_errors(tde, build, w_init, batches, want, w0):
    """The package's float32 torch reference plan on the CPU against the oracle, per variable: the reference
    error the plan suites scale their bound by (smallnet_oracle.bound)."""
    _, PG = _tde()
    tde.backend.clear_session()
    m = build()
    m.set_weights(w_init)
    st = m._store.clone_to("cpu")
    plan = PG.ReferencePlan(m, st, "cpu", BPLAN, BPLAN, m.optimizer, m.loss)
    for x, y in batches:
        plan.scale = 1.0 / len(y)
        plan.train_step(x, y)
        plan.apply()
    names = st.names(trainable=True)
    return {n: O.rel(st.view(k).detach().double() - w0[n], want[n] - w0[n]) for n, k in zip(want, names)}


def _plan_case(tde, build, kind, seed, bound=None, step_b=(8, 8, 5)):
    """Three steps of the GPU plan (the last one ragged) against the float64 autograd oracle: the weight change
    of every variable within ``bound`` (default: smallnet_oracle.bound of the float32 reference's own error), the
    logged loss of every step (penalty included) within 1e-5 relative + the same factor of the reference."""
    _, PG = _tde()
    tde.backend.clear_session()
    tde.backend.set_random_seed(seed)
    m = build()
    st = m._store
    opt = m.optimizer
    w_init = m.get_weights()
    full = W.batches(m, BPLAN, 3, 40 + seed)
    batches = [(x[:b], y[:b]) for (x, y), b in zip(full, step_b)]
    names = st.names(trainable=True)
    w0 = {n: st.view(n).detach().cpu().double().clone() for n in names}
    # every step divides by its own row count: what fit() does with a ragged last batch (run_single)
    want, want_loss, _ = W.trajectory(m, batches, opt, decays=opt.decays)
    plan = PG.make_plan(m, st, DEV, BPLAN, BPLAN, opt, m.loss)
    assert plan.kind == kind and plan.step_mode == "plain", (plan.kind, plan.step_mode)
    assert not plan.supports_step_mode("local") and not plan.supports_step_mode("xgmi") and not plan._opt_fused()
    losses, pens = [], []
    for (x, y), b in zip(full, step_b):
        plan.reset_metrics()
        scale = plan.scale
        plan.scale = 1.0 / b
        plan.train_step(x.to(DEV, plan.input_dtype).contiguous(), y.to(DEV), b)
        plan.apply()
        plan.scale = scale
        torch.cuda.synchronize()
        mt = plan.metrics.cpu().double()
        assert mt[2].item() == b
        losses.append(float(mt[0] / mt[2]))
        pens.append(plan.opt.reg.penalty.item() if plan.opt.reg is not None else 0.0)
    assert plan.iterations.item() == 3
    got = {n: st.view(n).detach().cpu().double() for n in names}
    ref = None if bound is not None else _reference_errors(tde, build, w_init, batches, want, w0)
    for n in names:
        e = O.rel(got[n] - w0[n], want[n] - w0[n])
        b = bound(n) if bound is not None else O.bound(ref[n])
        print(f"[{m.name} {kind}] {n}: vs float64 {e:.3g} bound {b:.3g}")
        assert float((got[n] - w0[n]).abs().max()) > 0
        assert e <= b, (n, e, b)
    for k, (a, b) in enumerate(zip(losses, want_loss)):
        print(f"[{m.name} {kind}] step {k}: loss {a!r} float64 {b!r} penalty word {pens[k]!r}")
    return m, plan, losses, want_loss, pens


def test_lenet5_smallnet_plan_runs_plain_against_float64():
    tde, _ = _tde()

    def build():
        opt = tde.optimizers.SGD(0.05, weight_decay=0.01)
        opt.exclude_from_weight_decay(var_names=["bias"])
        return _compile(tde, _regularize(tde, tde.zoo.lenet5(), tde.regularizers.l1_l2(1e-4, 1e-3), "l2"), opt)
    m, plan, losses, want_loss, pens = _plan_case(tde, build, "fused_smallnet", 1)
    for a, b, p in zip(losses, want_loss, pens):
        assert abs(a - b) <= 1e-5 * abs(b) and p > 1e-3 * b
    # fit's log and evaluate's loss include the penalty (lr = 0: the weights stay)
    tde.backend.clear_session()
    tde.backend.set_random_seed(2)
    m = _compile(tde, _regularize(tde, tde.zoo.lenet5(), tde.regularizers.L2(0.01)), tde.optimizers.SGD(0.0))
    x, y = W.batches(m, 2 * BPLAN, 1, 9)[0]
    Wd = W._named_weights(m)
    tot, ce, pen = W.total_loss(m, Wd, x.double(), y)
    h = m.fit(x.numpy(), y.numpy(), batch_size=BPLAN, epochs=1, verbose=0, shuffle=False, validation_data=(x.numpy(), y.numpy()))
    ev = m.evaluate(x.numpy(), y.numpy(), batch_size=BPLAN, verbose=0, return_dict=True)
    assert m._program("train", BPLAN).plan_kind == "fused_smallnet" and m._program("eval", BPLAN).plan_kind == "fused_smallnet"
    print(f"fit {h.history['loss'][0]!r} val {h.history['val_loss'][0]!r} evaluate {ev['loss']!r} float64 {float(tot)!r} "
          f"(penalty {float(pen)!r})")
    assert float(pen) > 0.01 * float(ce)
    for got in (h.history["loss"][0], h.history["val_loss"][0], ev["loss"]):
        assert abs(got - float(tot)) <= 1e-5 * float(tot)


def test_mnist_cnn_fused_plan_runs_plain_against_float64():
    tde, _ = _tde()

    def build():
        opt = tde.optimizers.AdamW(tde.optimizers.schedules.ExponentialDecay(1e-3, 1, 0.5), weight_decay=0.05,
                                   global_clipnorm=2.0)
        return _compile(tde, _regularize(tde, tde.zoo.mnist_cnn(), tde.regularizers.L2(1e-3), "l1"), opt)
    m, plan, losses, want_loss, pens = _plan_case(tde, build, "fused_convnet", 2, step_b=(8, 8, 8))
    for a, b, p in zip(losses, want_loss, pens):
        assert abs(a - b) <= 1e-5 * abs(b) and p > 1e-3 * b


@pytest.mark.parametrize("policy", ["float32", "mixed_bfloat16"])
def test_mini_resnet_layerwise_plan_against_float64(policy):
    tde, _ = _tde()
    tde.keras.mixed_precision.set_global_policy(policy)
    try:
        def build():
            m = tde.zoo.mini_resnet(l2=5e-3)
            for layer in m.layers:       # a gamma_regularizer on every BatchNormalization
                for s in layer.weight_specs:
                    if s.name == "gamma":
                        s.l1, s.l2 = tde.regularizers.L2(1e-2).coefficients
            return _compile(tde, m, tde.optimizers.SGD(0.01, momentum=0.5, weight_decay=0.02))
        # float32: the plan suite's bound for this model against float64 (tests/test_layers_f32_gpu.py: 1e-5, or the
        # float32 reference's own error x 4).  mixed_bfloat16: the bounds of tests/test_layers_gpu.py for its
        # gradients against float64-accumulated references (0.05 for the head, 0.5 elsewhere)
        bound = None if policy == "float32" else (lambda n: 0.05 if n.startswith("fc/") else 0.5)
        m, plan, losses, want_loss, pens = _plan_case(tde, build, "layerwise", 3, bound=bound, step_b=(8, 8, 8))
        assert plan.compute_dtype == ("fp32" if policy == "float32" else "bf16")
        assert len(plan.reg_segs) == len([n for n in m._store.names(trainable=True) if n.endswith(("/kernel", "/gamma"))])
        for k, (a, b, p) in enumerate(zip(losses, want_loss, pens)):
            assert p > 1e-2 * b
            # the loss: the suites' own bounds for this model, 1e-5 in float32 (tests/test_layers_f32_gpu.py) and
            # 6e-2 under bf16 activations (tests/test_layers_gpu.py); the penalty itself is float32 work on the
            # float32 master weights under either policy (checked below against Model.losses)
            assert abs(a - b) <= (1e-5 if policy == "float32" else 6e-2) * abs(b), (k, a, b)
        final = float(sum(m.losses))
        plan.opt.reg.grad(None)
        plan.opt.reg.finish(None, 0)
        torch.cuda.synchronize()
        print(f"[{policy}] penalty word {plan.opt.reg.penalty.item()!r} Model.losses {final!r}")
        assert abs(plan.opt.reg.penalty.item() - final) <= W.PENALTY_TOL * final
    finally:
        tde.keras.mixed_precision.set_global_policy("float32")


# ------------------------------------------------------------------------------------- 4. mirrored
CHILD_TIMEOUT = 90


def test_mirrored_replicas_regularize_the_reduced_gradient():
    """Two Mirrored replicas rehearsed on cuda:0 and, in the same child, one replica at the same global batch: a
    plain all-reduce, every replica's own regularizer launches and WD apply, the replicas bit-identical and equal
    to the one-replica run within the tolerance of tests/test_mirrored_gpu.py (rtol 1e-4, atol 1e-5); every replica
    adds its local rows x penalty, so the summed loss holds the penalty once."""
    env = dict(os.environ, TDE_HEARTBEAT="0", OMP_NUM_THREADS="2", TDE_XGMI_TIMEOUT="20")
    p = subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "weight_reg_mirrored_child.py")], env=env, cwd=ROOT,
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
    assert res["plan"] == "fused_smallnet" and res["step_modes"] == ["plain", "plain"], res
    assert res["comm_applies"] is False and res["iterations"] == [3, 3], res
    assert res["w_identical"] and res["words_identical"], res
    assert res["wd"] == [OO.f32(0.02)] * 3 + [0.0] and res["w_moved"] > 0, res
    assert res["one_step_mode"] == "plain" and res["worst_excess"] <= 0.0, res
    for two, one, pen in zip(res["losses"], res["one_losses"], res["penalties"]):
        assert pen > 0.01 and abs(two - one) <= 1e-5 * one and two > pen, res
