"""Gradient clipping on the GPU (csrc/include/tde_clip.h, csrc/kernels/gradclip.hip, the CLIP variants of
csrc/kernels/optim.hip, ``OptimizerKernel``): the norm launches on the segments of tests/optim_oracle.py plus a
1-element segment, one of exactly one chunk and one of a chunk plus 5 (bit for bit on a dyadic gradient,
within grad_clip_oracle.NORM_TOL of float64 on a normal one, bitwise repeatable, gaps poisoned), a segment of
300 chunks + 3 for the strided loop of the scale launch; the clipped apply for the six optimizer kinds against
the optimizer oracles fed the host's f32(f32(g * grad_scale) * scale) under the rules of
tests/test_optim_gpu.py / tests/test_optim_rmsprop_gpu.py; the plans; two Mirrored replicas in a child process.

Figures on an MI355X (``-s`` prints every one before it is asserted) are in profiles/grad_clip/NOTES.md.
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

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_KINDS = OO.KINDS + R.KINDS
NORM_MODES = ("clipnorm", "global_clipnorm")
SEGMENTS = OO.SEGMENTS + G.EXTRA_SEGMENTS
ADAM_HYPER = dict(lr=0.01, mom=0.0, b1=0.9, b2=0.999, eps=1e-7)


def _tde():
    import tensorflow_distributed_example_amd as tde
    from tensorflow_distributed_example_amd.train import program as PG
    return tde, PG


def _N():
    from tensorflow_distributed_example_amd import _native as N
    return N


def _hyper(kind):
    return R.GRID_HYPER if kind in R.KINDS else ADAM_HYPER if kind == "adam" else OO.GRID_HYPER


def _optimizer(kind, **clip):
    tde, _ = _tde()
    h = _hyper(kind)
    if kind in R.KINDS:
        return tde.optimizers.RMSprop(h["lr"], rho=h["b2"], momentum=h["mom"] if kind == "rmsprop_momentum" else 0.0,
                                      epsilon=h["eps"], **clip)
    if kind == "adam":
        return tde.optimizers.Adam(h["lr"], h["b1"], h["b2"], h["eps"], **clip)
    return tde.optimizers.SGD(h["lr"], momentum=0.0 if kind == "sgd" else h["mom"], nesterov=kind == "nesterov", **clip)


class Rig:
    """A store of ``segments`` with the optimizer kernel of one kind and one clip mode on the device."""

    def __init__(self, kind, mode, c, segments=SEGMENTS):
        _, PG = _tde()
        self.kind, self.mode, self.c, self.hyper = kind, mode, c, _hyper(kind)
        self.store = st = OO.make_store([(n, s) for n, s, _ in segments], DEV)
        self.opt = _optimizer(kind, **{mode: c})
        assert self.opt.kind == kind and self.opt.kind_id == ALL_KINDS.index(kind) and self.opt.clip == (mode, c)
        self.slots = [st.slot(s) for s in self.opt.slot_names()]
        self.it = torch.zeros(1, dtype=torch.int64, device=DEV)
        self.ok = PG.OptimizerKernel(st, self.opt, {n: sh for n, _, sh in segments if sh}, self.it)
        self.idx = torch.arange(st.n_trainable)
        self.names = st.names(trainable=True)
        self.segs = G.store_segments(st)
        self.mask = OO.seg_mask(st)

    # ---- state
    def start(self, exact_grid=True, seed=0):
        """Weights and slots on the exact grid (or normal), shadows refreshed, sentinels into every gap.
        -> float64 host state [w, slot0, slot1]."""
        n = self.store.n_trainable
        if exact_grid:
            w = OO.grid_w(self.idx)
            if self.kind in R.KINDS:
                state = [R.grid_r(self.idx), R.grid_q(self.idx)]
            elif self.kind == "adam":
                state = [OO.grid_slot(self.idx), OO.grid_slot(self.idx).abs()]
            else:
                state = [OO.grid_slot(self.idx), None]
        else:
            gen = torch.Generator().manual_seed(seed)
            w = torch.randn(n, generator=gen).double()
            state = [torch.rand(n, generator=gen).double(), torch.rand(n, generator=gen).double()]
        self.store.w.copy_(w.float())
        for buf, s in zip(self.slots, state):
            buf.copy_(s.float())
        self.ok.refresh_shadows()
        self.gaps, self.shgaps = OO.fill_store_gaps(self.store), OO.fill_shadow_gaps(self.ok)
        return [w] + state

    def set_grad(self, g):
        self.store.g.copy_(torch.where(self.mask, g.float(), torch.tensor(OO.W_SENTINEL)))

    def seg(self, name, flat):
        s = self.store.segments[name]
        return flat[s.offset: s.offset + s.numel]

    # ---- launches
    def norm_launches(self, mode=None, c=None):
        N, ok, st = _N(), self.ok, self.store
        lib = N.hip()
        rc = lib.tde_clip_sumsq(st.g.data_ptr(), ok.segs_dev.data_ptr(), ok.clip_ents_dev.data_ptr(), ok.clip_nent,
                                ok.clip_partials.data_ptr(), N.stream_ptr())
        assert rc == 0
        return lib.tde_clip_scale(ok.clip_partials.data_ptr(), ok.clip_ranges_dev.data_ptr(), len(self.names),
                                  ok.clip_nent, G.MODE_ID[self.mode] if mode is None else mode,
                                  self.c if c is None else c, ok.clip_norm.data_ptr(), ok.clip_scale.data_ptr(),
                                  N.stream_ptr())

    def raw_apply(self, clip=True, mode=None, c=None, scale="own", grad_scale=1.0, zero_grad=1, lr_ptr=None, w_off=0,
                  kind_id=None):
        N, ok, st, h = _N(), self.ok, self.store, self.hyper
        m, v = (self.slots + [None, None])[:2]
        head = (st.w.data_ptr() + w_off, st.g.data_ptr(), N.ptr(m), N.ptr(v), ok.shadow.data_ptr(), ok.segs_dev.data_ptr(),
                ok.table_dev.data_ptr(), ok.nblocks, self.it.data_ptr(),
                ALL_KINDS.index(self.kind) if kind_id is None else kind_id, h["lr"], h["mom"], h["b1"], h["b2"], h["eps"],
                grad_scale, zero_grad, N.ptr(lr_ptr))
        if not clip:
            return N.hip().tde_optim_apply(*head, N.stream_ptr())
        sc = ok.clip_scale if isinstance(scale, str) else scale
        return N.hip().tde_optim_apply_clip(*head, G.MODE_ID[self.mode] if mode is None else mode,
                                            self.c if c is None else c, N.ptr(sc), N.stream_ptr())

    def snapshot(self):
        bufs = [self.store.w, self.store.g, self.ok.shadow] + self.slots
        bufs += [b for b in (self.ok.clip_norm, self.ok.clip_scale) if b is not None]
        torch.cuda.synchronize()
        return [b.cpu().clone() for b in bufs]

    def assert_unchanged(self, snap, what):
        for a, b in zip(self.snapshot(), snap):
            d = OO.first_diff(a, b)
            assert not d, f"{what}: {d}"

    def scale_per_element(self):
        """float32 flat tensor: the device's scale of the segment each element lies in (1 in the gaps)."""
        sc = self.ok.clip_scale.cpu()
        out = torch.ones(self.store.n_trainable, dtype=torch.float32)
        for i, (o, n) in enumerate(self.segs):
            out[o: o + n] = sc[i if self.mode == "clipnorm" else 0]
        return out

    def check_layout(self, tag, grad_zero=True):
        """Zeroed gradient, shadows == bf16 of the device's own weights, every gap untouched."""
        st, ok = self.store, self.ok
        dw, dg = st.w.cpu(), st.g.cpu()
        for name in self.names:
            if grad_zero:
                assert not OO.first_diff(self.seg(name, dg), torch.zeros(st.segments[name].numel)), (tag, name)
            w2 = OO.view2d(st, name, dw)
            if (name, "row") in ok.shadow_views:
                d = OO.first_diff(ok.shadow_views[(name, "row")], w2.to(torch.bfloat16), bitwise=False)
                assert not d, f"{tag} {name}: row shadow: {d}"
            if (name, "col") in ok.shadow_views:
                d = OO.first_diff(ok.shadow_views[(name, "col")], w2.T.contiguous().to(torch.bfloat16), bitwise=False)
                assert not d, f"{tag} {name}: col shadow: {d}"
        OO.assert_store_gaps(st, self.gaps)
        OO.assert_shadow_gaps(ok, self.shgaps)

    def step_and_compare(self, tag, state, g_eff32, t, fails):
        """Oracle and host-fp32 step on the effective gradient; the device against them under the suites' rules:
        max(4 x the host's error, 2^-22 max |oracle|) per tensor (Adam's w: + lr rho_t).  -> new float64 state."""
        kind, h = self.kind, self.hyper
        g64 = g_eff32.double()
        host = [None if s is None else s.float() for s in state]
        if kind in R.KINDS:
            new = list(R.oracle_step(kind, h, state[0], g64, state[1], state[2]))
            hst = list(R.fp32_step(kind, h, host[0], g_eff32, host[1], host[2]))
        else:
            new = list(OO.oracle_step(kind, h, state[0], g64, state[1], state[2], t))
            hst = list(OO.fp32_step(kind, h, host[0], g_eff32, host[1], host[2], t))
        torch.cuda.synchronize()
        dev = [self.store.w.cpu()] + [b.cpu() for b in self.slots]
        assert all(torch.isfinite(d).all() for d in dev)
        rho = 0.0
        if kind == "adam":
            p1, p2 = OO.f32(h["b1"]) ** t, OO.f32(h["b2"]) ** t
            rho = 2.0 ** -24 * (4 * (p2 / (2.0 * (1.0 - p2)) + p1 / (1.0 - p1)) + 8.0)     # test_optim_gpu.rho_bound
        for name in self.names:
            for key, d, o, hh in zip(("w", "slot0", "slot1"), dev, new, hst):
                oo = self.seg(name, o)
                e_dev = float((self.seg(name, d).double() - oo).abs().max())
                e_host = float((self.seg(name, hh).double() - oo).abs().max())
                b = max(4.0 * e_host, 2.0 ** -22 * float(oo.abs().max())) + (h["lr"] * rho if key == "w" else 0.0)
                print(f"[{tag}] {key} {name}: dev {e_dev:.3g} host {e_host:.3g} bound {b:.3g}")
                if not e_dev <= b:
                    fails.append((tag, key, name, e_dev, b))
        return [new[0]] + [n if s is not None else None for n, s in zip(new[1:], state[1:])]


# ------------------------------------------------------------------------------------- 1. the norm launches
def _check_norms(tag, rig, g, c):
    want_n = G.norms(g, rig.segs, rig.mode)
    want_s = G.scales(want_n, c)
    torch.cuda.synchronize()
    nrm, sc = rig.ok.clip_norm.cpu().double(), rig.ok.clip_scale.cpu().double()
    assert nrm.shape == want_n.shape and sc.shape == want_s.shape
    for i in range(len(want_n)):
        en = abs(nrm[i].item() - want_n[i].item()) / max(want_n[i].item(), 1e-300)
        es = abs(sc[i].item() - want_s[i].item()) / want_s[i].item()
        print(f"[{tag}] {i}: norm {nrm[i].item()!r} float64 {want_n[i].item()!r} rel {en / 2.0 ** -24:.3g} x 2^-24; "
              f"scale rel {es / 2.0 ** -24:.3g} x 2^-24 (allowed {G.NORM_TOL / 2.0 ** -24:.3g})")
        assert en <= G.NORM_TOL and es <= G.NORM_TOL, (tag, i, en, es)
        if want_n[i].item() <= c * (1.0 - G.NORM_TOL):
            assert sc[i].item() == 1.0, (tag, i)


@pytest.mark.parametrize("mode", NORM_MODES)
def test_norms_bit_exact_on_a_dyadic_gradient(mode):
    c = 0.5
    rig = Rig("sgd", mode, c)
    g, want = G.dyadic_gradient(rig.store.n_trainable, rig.segs, mode, OO.W_SENTINEL)
    assert torch.equal(G.norms(torch.where(rig.mask, g, torch.zeros(())), rig.segs, mode), want)   # the construction
    assert all(float(np.log2(x)).is_integer() for x in want.tolist())
    rig.store.g.copy_(g)                                            # the gaps hold the sentinel
    assert int((rig.store.g == OO.W_SENTINEL).sum()) == int((~rig.mask).sum()) > 0
    assert rig.norm_launches() == 0
    torch.cuda.synchronize()
    nrm, sc = rig.ok.clip_norm.cpu(), rig.ok.clip_scale.cpu()
    want32 = want.float()
    d = OO.first_diff(nrm, want32)
    assert not d, f"{mode} norm: {d}"
    d = OO.first_diff(sc, torch.tensor(c, dtype=torch.float32) / torch.clamp(want32, min=c))
    assert not d, f"{mode} scale: {d}"
    assert float(sc.min()) < 1.0 and (mode == "global_clipnorm" or float(sc.max()) == 1.0)


@pytest.mark.parametrize("mode", NORM_MODES)
def test_norms_against_float64_and_bitwise_repeatable(mode):
    c = 1.0
    rig = Rig("sgd", mode, c)
    gen = torch.Generator().manual_seed(7)
    g = torch.randn(rig.store.n_trainable, generator=gen)
    g[rig.store.segments["v10"].offset: rig.store.segments["v10"].offset + 10] *= 0.01     # a norm well below c
    rig.set_grad(g.double())
    assert rig.norm_launches() == 0
    _check_norms(mode, rig, torch.where(rig.mask, g, torch.zeros(())), c)
    first = [b.cpu().clone() for b in (rig.ok.clip_partials, rig.ok.clip_norm, rig.ok.clip_scale)]
    for b in (rig.ok.clip_partials, rig.ok.clip_norm, rig.ok.clip_scale):
        b.fill_(-3.0)
    assert rig.norm_launches() == 0
    torch.cuda.synchronize()
    for a, b, what in zip(first, (rig.ok.clip_partials, rig.ok.clip_norm, rig.ok.clip_scale), ("partials", "norm", "scale")):
        d = OO.first_diff(b, a)
        assert not d, f"{mode} second run, {what}: {d}"
    assert not OO.first_diff(rig.store.g, torch.where(rig.mask, g, torch.tensor(OO.W_SENTINEL)))   # g only read


@pytest.mark.parametrize("mode", NORM_MODES)
def test_norm_of_300_chunks_and_3(mode):
    """301 partials of one segment: past the 64 lanes (clipnorm) and the 256 threads (global) of the scale launch."""
    c = 100.0
    rig = Rig("sgd", mode, c, [G.LONG_SEGMENT])
    assert rig.ok.clip_nent == 301
    gen = torch.Generator().manual_seed(9)
    g = torch.randn(rig.store.n_trainable, generator=gen)
    rig.set_grad(g.double())
    assert rig.norm_launches() == 0
    _check_norms(f"long {mode}", rig, torch.where(rig.mask, g, torch.zeros(())), c)
    assert rig.ok.clip_scale.item() < 0.1
    # and on +-1/2: 1228803 elements, every partial 1024 exactly but the last (3/4): the norm is sqrt(307200.75)
    rig.set_grad(torch.where(rig.idx % 2 == 0, 0.5, -0.5).double())
    assert rig.norm_launches() == 0
    torch.cuda.synchronize()
    assert rig.ok.clip_partials.cpu().tolist() == [1024.0] * 300 + [0.75]
    assert rig.ok.clip_norm.item() == float(np.sqrt(np.float32(307200.75)))


# ------------------------------------------------------------------------------------- 2. the clipped apply
@pytest.mark.parametrize("mode", NORM_MODES)
@pytest.mark.parametrize("kind", ALL_KINDS)
def test_clipped_apply_against_the_oracles(kind, mode):
    """Two steps, grad_scale 0.5 then 1 (with zero_grad off, then on): the device's own scale read back, the
    effective gradient formed on the host in the kernel's order, the optimizer oracles stepped with it."""
    c = 8.0
    rig = Rig(kind, mode, c)
    state = rig.start()
    fails = []
    for t, (gs, zg) in enumerate(((0.5, 0), (1.0, 1)), start=1):
        g = OO.grid_g(rig.idx, t)
        rig.set_grad(g)
        g_before = rig.store.g.cpu().clone()
        rig.it += 1
        assert rig.norm_launches() == 0
        assert rig.raw_apply(grad_scale=gs, zero_grad=zg) == 0
        torch.cuda.synchronize()
        _check_norms(f"{kind} {mode} t={t}", rig, torch.where(rig.mask, g.float(), torch.zeros(())), c)
        sc = rig.scale_per_element()
        assert float(sc.min()) < 1.0
        if mode == "clipnorm":
            assert rig.ok.clip_scale[rig.names.index("v1")].item() == 1.0      # |g| < 4 < c: not clipped
        g_eff = (g.float() * torch.tensor(gs, dtype=torch.float32)) * sc
        state = rig.step_and_compare(f"{kind} {mode} t={t}", state, g_eff, t, fails)
        rig.check_layout(f"{kind} {mode} t={t}", grad_zero=bool(zg))
        if not zg:
            assert not OO.first_diff(rig.store.g, g_before), "zero_grad = 0 changed g"
        # the device state becomes the next step's start: the comparison is per step
        state = [rig.store.w.cpu().double()] + [b.cpu().double() for b in rig.slots] + [None] * (2 - len(rig.slots))
    assert not fails, fails


@pytest.mark.parametrize("kind", ALL_KINDS)
def test_scale_one_is_bitwise_the_unclipped_launch(kind):
    """norm <= c: the scale is exactly 1 and w, the slots, the shadows and g equal tde_optim_apply's bit for bit.
    (A workgroup whose segment's scale is 1 runs the unclipped kernel's program text: with the multiply by 1
    left in, the compiler contracted the RMSprop step differently and 226 / 170 of 36544 weights came out
    one bit off.)"""
    outs = []
    for clip in (True, False):
        rig = Rig(kind, "global_clipnorm", 1e6)
        rig.start(exact_grid=False, seed=3)
        gen = torch.Generator().manual_seed(5)
        rig.set_grad(torch.randn(rig.store.n_trainable, generator=gen).double())
        rig.it += 1
        if clip:
            assert rig.norm_launches() == 0
        assert rig.raw_apply(clip=clip, grad_scale=0.25) == 0
        torch.cuda.synchronize()
        if clip:
            assert rig.ok.clip_scale.item() == 1.0 and 0 < rig.ok.clip_norm.item() < 1e6
        outs.append([b.cpu().clone() for b in [rig.store.w, rig.store.g, rig.ok.shadow] + rig.slots])
    for a, b in zip(*outs):
        d = OO.first_diff(a, b)
        assert not d, f"{kind}: {d}"


@pytest.mark.parametrize("kind", ["sgd", "momentum", "adam", "rmsprop_momentum"])
def test_clipvalue_is_bit_exact(kind):
    """clipvalue launches no norm kernel; the clamp is exact, so kinds 0..2 on the grid equal the oracle bit for
    bit (c = 1.5 on the 2^-6 grid, grad_scale 0.5: values at +-c, beyond and inside), the others their rules."""
    c = 1.5
    rig = Rig(kind, "clipvalue", c)
    assert rig.ok.clip_scale is None and rig.ok.clip_partials is None
    state = rig.start()
    g = OO.grid_g(rig.idx, 0)
    o = rig.store.segments["v2049"].offset
    g[o: o + 6] = torch.tensor([3.0, -3.0, -0.0, 0.0, 3.984375, -3.984375], dtype=torch.float64)    # +-c after 0.5 x
    rig.set_grad(g)
    rig.it += 1
    assert rig.raw_apply(grad_scale=0.5) == 0
    g_eff = (g.float() * 0.5).clamp(-c, c)
    assert g_eff[o: o + 6].tolist() == [1.5, -1.5, -0.0, 0.0, 1.5, -1.5] and bool(torch.signbit(g_eff[o + 2]))
    assert int((g_eff.abs() == c).sum()) > 100 and int((g_eff.abs() < c).sum()) > 100
    fails = []
    new = rig.step_and_compare(f"clipvalue {kind}", state, g_eff, 1, fails)
    assert not fails, fails
    if kind in ("sgd", "momentum"):
        dev = [rig.store.w.cpu()] + [b.cpu() for b in rig.slots]
        for name in rig.names:
            for d, w in zip(dev, new):
                diff = OO.first_diff(rig.seg(name, d).double(), rig.seg(name, w), bitwise=False)
                assert not diff, f"clipvalue {kind} {name}: {diff}"
    rig.check_layout(f"clipvalue {kind}")


@pytest.mark.parametrize("mode", NORM_MODES)
def test_zero_gradient_gives_scale_one(mode):
    rig = Rig("adam", mode, 0.5)
    state = rig.start()
    rig.set_grad(torch.zeros(rig.store.n_trainable, dtype=torch.float64))
    rig.it += 1
    rig.ok.apply()
    torch.cuda.synchronize()
    assert torch.all(rig.ok.clip_norm == 0) and torch.all(rig.ok.clip_scale == 1.0)
    fails = []
    rig.step_and_compare(f"zero gradient {mode}", state, torch.zeros(rig.store.n_trainable), 1, fails)
    assert not fails, fails
    rig.check_layout(f"zero gradient {mode}")


def test_schedule_and_clip_read_both_words():
    """lr_ptr and the scale in one launch: SGD on the grid with the rate 0.25 from a device word."""
    rig = Rig("sgd", "global_clipnorm", 8.0)
    state = rig.start()
    g = OO.grid_g(rig.idx, 0)
    rig.set_grad(g)
    lr_dev = torch.tensor([0.25], dtype=torch.float32, device=DEV)
    assert rig.norm_launches() == 0 and rig.raw_apply(lr_ptr=lr_dev) == 0
    torch.cuda.synchronize()
    sc = rig.ok.clip_scale.item()
    assert 0 < sc < 1
    rig.hyper = dict(rig.hyper, lr=0.25)
    fails = []
    rig.step_and_compare("lr_ptr + clip", state, g.float() * torch.tensor(sc, dtype=torch.float32), 1, fails)
    assert not fails, fails
    assert float((rig.store.w.cpu().double() - state[0])[rig.mask].abs().max()) > 0
    rig.check_layout("lr_ptr + clip")


def test_refusals_write_nothing():
    rig = Rig("momentum", "clipnorm", 0.5)
    rig.start()
    rig.set_grad(OO.grid_g(rig.idx, 0))
    assert rig.norm_launches() == 0
    snap = rig.snapshot()
    assert rig.raw_apply(mode=0) == -3 and rig.raw_apply(mode=4) == -3 and rig.raw_apply(mode=-1) == -3     # unknown mode
    assert rig.raw_apply(mode=1, c=0.0) == -3 and rig.raw_apply(mode=1, c=-1.0) == -3                     # c <= 0
    assert rig.raw_apply(mode=1, c=float("nan")) == -3 and rig.raw_apply(mode=1, c=float("inf")) == -3
    assert rig.raw_apply(scale=None) == -3 and rig.raw_apply(mode=3, scale=None) == -3                  # null scale
    assert rig.raw_apply(w_off=4) == -1                                                                 # misaligned
    assert rig.raw_apply(kind_id=6) == -2
    assert rig.norm_launches(mode=1) == -3 and rig.norm_launches(mode=0) == -3 and rig.norm_launches(mode=7) == -3
    assert rig.norm_launches(c=0.0) == -3 and rig.norm_launches(c=-2.0) == -3 and rig.norm_launches(c=float("nan")) == -3
    N, ok, st = _N(), rig.ok, rig.store
    assert N.hip().tde_clip_sumsq(st.g.data_ptr() + 4, ok.segs_dev.data_ptr(), ok.clip_ents_dev.data_ptr(), ok.clip_nent,
                                  ok.clip_partials.data_ptr(), N.stream_ptr()) == -1
    assert N.hip().tde_clip_sumsq(None, ok.segs_dev.data_ptr(), ok.clip_ents_dev.data_ptr(), ok.clip_nent,
                                  ok.clip_partials.data_ptr(), N.stream_ptr()) == -1
    rig.assert_unchanged(snap, "a refused call")
    assert rig.raw_apply() == 0                                  # and the same arguments do update when accepted
    torch.cuda.synchronize()
    assert float((rig.store.w.cpu() - snap[0])[rig.mask].abs().max()) > 0


# ------------------------------------------------------------------------------------- 3. the small-net plan
def _model(tde, which, opt):
    m = tde.zoo.lenet5() if which == "lenet5" else tde.zoo.mnist_mlp()
    m.compile(loss=tde.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=opt, metrics=["accuracy"])
    m.build()
    return m


def _batch(m, n, seed):
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.standard_normal((n,) + tuple(m.input_shape[1:])).astype(np.float32))
    y = torch.from_numpy(rng.integers(0, 10, n).astype(np.int32))
    return x, y


BPLAN = 8
C_FRACTION = {"clipvalue": 0.9, "clipnorm": 0.5, "global_clipnorm": 0.5}
STEP_B = (8, 8, 1)        # the third step sees one image of the global batch of 8: a gradient of about 1/8 the size


def _size(g, mode):
    """What the clip compares with c, per mode, from {name: gradient}: the largest of them."""
    if mode == "clipvalue":
        return max(float(t.abs().max()) for t in g.values())
    sq = [float(t.double().square().sum()) for t in g.values()]
    return max(sq) ** 0.5 if mode == "clipnorm" else sum(sq) ** 0.5


def _trajectory(m, st, batches, opt, kind, mode, c, dtype):
    """The float64 (or torch float32) trajectory from the store's weights: gradients of smallnet_oracle.oracle,
    clipped in float64 by grad_clip_oracle, the update of optim_oracle.  -> (weights, [size of every step])."""
    W = {n: w.detach().clone() for n, w in O._weights(m, st, dtype, False).items()}
    z = {n: torch.zeros_like(w) for n, w in W.items()}
    s0, s1 = dict(z), {n: t.clone() for n, t in z.items()}
    hp = opt.hparams()
    sizes = []
    for k, ((x, y), B) in enumerate(zip(batches, STEP_B)):
        g = O.oracle(m, st, x, y, B, BPLAN, None, dtype, weights=W)["grads"]
        sizes.append(_size(g, mode))
        g = G.clip_named(g, mode, c)
        h = dict(lr=opt.lr_at(k), **hp)
        step = OO.oracle_step if dtype == torch.float64 else OO.fp32_step
        for n in g:
            W[n], a, b = step(kind, h, W[n], g[n].to(dtype), s0[n], s1[n], k + 1)
            s0[n], s1[n] = (a if a is not None else s0[n]), (b if b is not None else s1[n])
    return W, sizes


def _first_size(m, st, batch, mode):
    return _size(O.oracle(m, st, batch[0], batch[1], STEP_B[0], BPLAN)["grads"], mode)


@pytest.mark.parametrize("mode", G.MODES)
@pytest.mark.parametrize("kind", ["sgd", "adam"])
@pytest.mark.parametrize("model", ["lenet5", "mnist_mlp"])
def test_smallnet_plan_three_steps_against_float64(model, kind, mode):
    """c is a fraction of the first step's size (half the largest variable norm or the global norm, 0.9 of the
    largest |g|, which the output bias holds and one image of eight lowers least): the first step clips; the
    third step's gradient (one image of eight) lies below c: it does not.  Both asserted from the oracle."""
    tde, PG = _tde()
    tde.backend.set_random_seed(3)
    probe = _model(tde, model, tde.optimizers.SGD(0.05))
    batches = [_batch(probe, BPLAN, 20 + s) for s in range(3)]
    c = OO.f32(C_FRACTION[mode] * _first_size(probe, probe._store, batches[0], mode))
    w_init = probe.get_weights()
    tde.backend.clear_session()
    opt = tde.optimizers.SGD(0.05, **{mode: c}) if kind == "sgd" else tde.optimizers.Adam(1e-3, **{mode: c})
    m = _model(tde, model, opt)
    m.set_weights(w_init)
    st = m._store
    w0 = {n: st.view(n).detach().cpu().double().clone() for n in st.names(trainable=True)}
    w64, sizes = _trajectory(m, st, batches, opt, kind, mode, c, torch.float64)
    w32, _ = _trajectory(m, st, batches, opt, kind, mode, c, torch.float32)
    print(f"[{model} {kind} {mode}] c {c!r}, sizes {sizes}")
    assert sizes[0] > c * 1.1 and sizes[2] < c * 0.9, (sizes, c)
    plan = PG.make_plan(m, st, DEV, BPLAN, BPLAN, m.optimizer, m.loss)
    assert plan.kind == "fused_smallnet" and plan.step_mode == "plain"
    assert not plan.supports_step_mode("local") and not plan.supports_step_mode("xgmi") and not plan._opt_fused()
    scales = []
    for (x, y), B in zip(batches, STEP_B):
        plan.train_step(x.to(DEV), y.to(DEV), B)
        plan.apply()
        if mode != "clipvalue":
            scales.append(plan.opt.clip_scale.cpu().clone())
    torch.cuda.synchronize()
    assert plan.iterations.item() == 3
    if mode != "clipvalue":
        assert float(scales[0].min()) < 0.75 and torch.all(scales[2] == 1.0), scales
    for n in w0:
        d = st.view(n).detach().cpu().double() - w0[n]
        e, ref = O.rel(d, w64[n] - w0[n]), O.rel(w32[n].double() - w0[n], w64[n] - w0[n])
        print(f"[{model} {kind} {mode}] {n}: vs float64 {e:.3g}  torch-fp32 {ref:.3g}  bound {O.bound(ref):.3g}")
        assert float(d.abs().max()) > 0
        assert e <= O.bound(ref), (n, e, ref)


def _graph_run(tde, monkeypatch, graph, opt):
    monkeypatch.setenv("TDE_GRAPH", "1" if graph else "0")
    tde.backend.clear_session()
    tde.backend.set_random_seed(3)
    m = tde.zoo.lenet5()
    m.compile(loss=tde.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=opt, metrics=["accuracy"],
              steps_per_execution=4)
    prog = m._program("train", BPLAN)
    plan = prog.plans[0]
    assert prog.plan_kind == "fused_smallnet" and plan.step_mode == "plain" and bool(prog.use_graph) == graph and prog.S == 4
    prog.enable_trace()
    gen = torch.Generator().manual_seed(11)
    x = torch.randn((4, BPLAN) + tuple(prog.x_shape), generator=gen)
    x[2:] *= 0.02                                         # steps 2 and 3: small gradients, below c
    y = torch.randint(0, 10, (4, BPLAN), generator=gen).to(torch.int32)
    for _ in range(2):
        prog.stage([(x.to(DEV, plan.input_dtype).contiguous(), y.to(DEV).contiguous())])
        prog.run()
    prog.sync()
    nw = plan.store.w.numel()
    return prog, plan, prog.trace[-1][:, :nw].cpu().clone(), plan.store.w.cpu().clone()


def test_graph_replay_equals_eager_and_the_scale_moves_inside_one_replay(monkeypatch):
    """steps_per_execution = 4 in one hipGraph against TDE_GRAPH=0: bitwise equal weights after every step of the
    second execution.  Under SGD + a schedule + global_clipnorm: all three device words are read per step."""
    tde, _ = _tde()

    def mk():
        sch = tde.optimizers.schedules.ExponentialDecay(0.05, 2, 0.5)
        return tde.optimizers.SGD(sch, global_clipnorm=1.0)
    pg, plan_g, tr_g, w_g = _graph_run(tde, monkeypatch, True, mk())
    assert len(pg.graphs) >= 1
    sc_last = plan_g.opt.clip_scale.item()
    n_last = plan_g.opt.clip_norm.item()
    pe, plan_e, tr_e, w_e = _graph_run(tde, monkeypatch, False, mk())
    assert not OO.first_diff(tr_g, tr_e) and not OO.first_diff(w_g, w_e)
    assert plan_g.iterations.item() == plan_e.iterations.item() == 8
    assert plan_e.opt.clip_scale.item() == sc_last == 1.0 and 0 < n_last < 1.0     # the last step did not clip
    assert all(not torch.equal(tr_g[i], tr_g[i + 1]) for i in range(3))
    # ... and an earlier step of the same replay did: with c large the trajectory is another one
    big = tde.optimizers.SGD(tde.optimizers.schedules.ExponentialDecay(0.05, 2, 0.5), global_clipnorm=1e6)
    _, _, tr_b, _ = _graph_run(tde, monkeypatch, True, big)
    assert not torch.equal(tr_b[0], tr_g[0])


# ------------------------------------------------------------------------------------- 4. fused plans fall back
def test_fused_cnn_runs_plain_under_clipping():
    """zoo.mnist_cnn + SGD(global_clipnorm): the fused CNN plan in step mode "plain"; one train_step, then
    ``apply()`` on the gradient it left against the float64 oracle applied to that same gradient, clipped."""
    tde, _ = _tde()
    tde.backend.set_random_seed(0)
    m = tde.zoo.mnist_cnn()
    c = 0.05
    opt = tde.optimizers.SGD(0.05, global_clipnorm=c)
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
    g, w = st.g.cpu().clone(), st.w.cpu().clone()
    segs = G.store_segments(st)
    n64 = G.norms(g, segs, "global_clipnorm")[0].item()
    assert n64 > 2 * c
    plan.apply()
    torch.cuda.synchronize()
    nd, sd = plan.opt.clip_norm.item(), plan.opt.clip_scale.item()
    print(f"[mnist_cnn plain] norm {nd!r} float64 {n64!r}, scale {sd!r}")
    assert abs(nd - n64) <= G.NORM_TOL * n64 and abs(sd - c / n64) <= G.NORM_TOL * c / n64
    hyper = dict(lr=0.05, **opt.hparams())
    ow = OO.oracle_step("sgd", hyper, w.double(), G.clip(g, segs, "global_clipnorm", c), None, None, 2)[0]
    hw = OO.fp32_step("sgd", hyper, w, g * torch.tensor(sd, dtype=torch.float32), None, None, 2)[0]
    dw = st.w.cpu()
    fails = []
    for o, n in segs:
        R.compare("mnist_cnn plain", "w", str(o), dw[o: o + n], hw[o: o + n], ow[o: o + n], fails)
        assert float((dw[o: o + n] - w[o: o + n]).abs().max()) > 0
    assert not fails, fails
    assert float(st.g.abs().max()) == 0.0


@pytest.mark.parametrize("zoo", ["generic", "bn_cnn"])
def test_generic_and_bn_cnn_plans_report_plain(zoo):
    tde, _ = _tde()
    m = tde.zoo.mnist_cnn(filters=16, units=32) if zoo == "generic" else tde.zoo.mnist_bn_cnn()
    loss = tde.losses.SparseCategoricalCrossentropy(from_logits=True) if zoo == "generic" else "sparse_categorical_crossentropy"
    m.compile(loss=loss, optimizer=tde.optimizers.Adam(1e-3, clipnorm=1.0), metrics=["accuracy"])
    prog = m._program("train", 64)
    plan = prog.plans[0]
    assert prog.plan_kind == ("fused_convnet_generic" if zoo == "generic" else "fused_bncnn")
    assert plan.step_mode == "plain" and not plan.supports_step_mode("local") and not plan.supports_step_mode("xgmi")
    assert plan.opt.clip_scale is not None and plan.opt.clip_scale.numel() == len(plan.store.names(trainable=True))
    if zoo == "generic":
        m.compile(loss=loss, optimizer=tde.optimizers.Adam(1e-3), metrics=["accuracy"])     # the unclipped twin fuses
        assert m._program("train", 64).plans[0].step_mode == "local"


# ------------------------------------------------------------------------------------- 5. mirrored
CHILD_TIMEOUT = 90


def _child(mode, c):
    env = dict(os.environ, TDE_HEARTBEAT="0", OMP_NUM_THREADS="2", TDE_XGMI_TIMEOUT="20")
    p = subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "grad_clip_mirrored_child.py"), mode, repr(c)],
                         env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         text=True, start_new_session=True)
    try:
        out, _ = p.communicate(timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        os.killpg(p.pid, signal.SIGKILL)
        out, _ = p.communicate()
        raise AssertionError(f"timed out:\n{out[-3000:]}")
    assert p.returncode == 0, out[-4000:]
    return json.loads([l for l in out.splitlines() if l.startswith("RESULT ")][0][7:])


def test_mirrored_replicas_clip_the_reduced_gradient():
    """Two Mirrored replicas rehearsed on cuda:0 and, in the same child, one replica at the same global batch:
    a plain all-reduce, every replica's own norm launches and clipped apply, the replicas bit-identical and
    equal to the one-replica run within the tolerance of tests/test_mirrored_gpu.py (rtol 1e-4, atol 1e-5)."""
    res = _child("global_clipnorm", 0.05)
    print(res)
    assert res["plan"] == "fused_smallnet" and res["step_modes"] == ["plain", "plain"], res
    assert res["comm_applies"] is False and res["iterations"] == [3, 3], res
    assert res["w_identical"] and res["words_identical"], res
    assert res["scale_max"] < 0.75 and res["w_moved"] > 0, res           # every step clipped
    assert res["one_step_mode"] == "plain" and res["worst_excess"] <= 0.0, res
