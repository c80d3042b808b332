"""The float32 step kernels' prologues (csrc/kernels/convnet_f32.hip) issue every global load up front with
indices clamped into the buffers.  The entry points are called directly at the smallest shapes where those
loads can go wrong (a lone row, ragged chunks, a 1-row tail, three chunks; the smallest image; few and many
classes; every replica-count path) and compared with a float64 numpy oracle of the same math at the
tolerance of tests/test_fp32_gpu.py (1e-5 relative, norm-wise; the conv itself exact on quantized operands).
Every buffer the clamped loads touch lies between guard pages of sentinel values that must stay untouched."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("fp32_policy")]

DEV = "cuda"
TOL = 1e-5            # tests/test_fp32_gpu.py: TOL of test_convnet_fwd_f32 / test_convnet_bwd_f32
GUARD = 1024          # elements of sentinel on each side of a guarded buffer
SGD, MOMENTUM, ADAM = 0, 1, 3
HP = {SGD: dict(lr=1.0, mom=0.0, b1=0.0, b2=0.0, eps=0.0), MOMENTUM: dict(lr=1.0, mom=0.9, b1=0.0, b2=0.0, eps=0.0),
      ADAM: dict(lr=2e-3, mom=0.0, b1=0.9, b2=0.999, eps=1e-7)}


class Guarded:
    """A device tensor between two guard pages of a sentinel value."""

    def __init__(self, shape, dtype=torch.float32, fill=None):
        n = int(np.prod(shape))
        self.sent = {torch.float32: 12345.5, torch.int32: 0x5A5A5A5A, torch.int64: 0x5A5A5A5A5A5A5A5A}[dtype]
        self.flat = torch.full((n + 2 * GUARD,), self.sent, dtype=dtype, device=DEV)
        self.t = self.flat[GUARD:GUARD + n].view(*shape)
        if fill is not None:
            self.t.copy_(torch.as_tensor(fill).to(dtype).reshape(shape))
        self.n = n

    def intact(self):
        return bool((self.flat[:GUARD] == self.sent).all() and (self.flat[GUARD + self.n:] == self.sent).all())


def _rel(got, ref):
    got = got.detach().double().cpu().numpy() if torch.is_tensor(got) else np.asarray(got, np.float64)
    return float(np.linalg.norm(got - ref) / (np.linalg.norm(ref) + 1e-30))


# ---------------------------------------------------------------- float64 oracle

def conv_pool(x, w, b):
    """x [B,H,W], w [3,3,32], b [32] -> pooled [B,P,32], window values [B,Hp,Wp,4,32] (slot q = 2*dy + dx)."""
    B, H, W = x.shape
    Ho, Wo = H - 2, W - 2
    z = np.zeros((B, Ho, Wo, 32)) + b
    for ky in range(3):
        for kx in range(3):
            z += x[:, ky:ky + Ho, kx:kx + Wo, None] * w[ky, kx]
    Hp, Wp = Ho // 2, Wo // 2
    zw = z[:, :2 * Hp, :2 * Wp].reshape(B, Hp, 2, Wp, 2, 32).transpose(0, 1, 3, 2, 4, 5).reshape(B, Hp, Wp, 4, 32)
    return np.maximum(zw.max(3), 0).reshape(B, Hp * Wp, 32), zw


def conv_pool_bwd(x, zw, dP):
    """Gradients of the conv kernel / bias for dP [B,P,32] (first maximum of the window, ReLU mask)."""
    B, H, W = x.shape
    _, Hp, Wp, _, C = zw.shape
    arg, best = zw.argmax(3), zw.max(3)
    dzw = (np.arange(4)[None, None, None, :, None] == arg[:, :, :, None, :]) * (best > 0)[:, :, :, None, :] * \
        dP.reshape(B, Hp, Wp, 1, C)
    dz = np.zeros((B, H - 2, W - 2, C))
    dz[:, :2 * Hp, :2 * Wp] = dzw.reshape(B, Hp, Wp, 2, 2, C).transpose(0, 1, 3, 2, 4, 5).reshape(B, 2 * Hp, 2 * Wp, C)
    dw = np.zeros((3, 3, C))
    for ky in range(3):
        for kx in range(3):
            dw[ky, kx] = np.einsum("bij,bijc->c", x[:, ky:ky + H - 2, kx:kx + W - 2], dz)
    return dw, dz.sum((0, 1, 2))


def head(hsum, b1, W2, b2, lab, scale):
    h = np.maximum(hsum + (b1 if b1 is not None else 0.0), 0)
    logits = h @ W2 + b2
    e = np.exp(logits - logits.max(1, keepdims=True))
    pr = e / e.sum(1, keepdims=True)
    onehot = np.eye(W2.shape[1])[lab]
    dl = (pr - onehot) * scale
    dH = (dl @ W2.T) * (h > 0)
    loss = -(np.log(pr) * onehot).sum()
    return h, dl, dH, loss, int((logits.argmax(1) == lab).sum())


def opt_step(kind, w, g, m, v, t):
    hp = HP[kind]
    if kind == SGD:
        return w - hp["lr"] * g, m, v
    if kind == MOMENTUM:
        nv = hp["mom"] * m - hp["lr"] * g
        return w + nv, nv, v
    m2 = hp["b1"] * m + (1 - hp["b1"]) * g
    v2 = hp["b2"] * v + (1 - hp["b2"]) * g * g
    lr_t = hp["lr"] * np.sqrt(1 - hp["b2"] ** t) / (1 - hp["b1"] ** t)
    return w - lr_t * m2 / (np.sqrt(v2) + hp["eps"]), m2, v2


def _f64(t):
    return t.detach().double().cpu().numpy()


def _hyper(kind):
    from tensorflow_distributed_example_amd.ops import kernels as Kk
    hp = HP[kind]
    return Kk.OptHyper(kind, hp["lr"], hp["mom"], hp["b1"], hp["b2"], hp["eps"])


def _data(B, HW, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randint(0, 17, (B, HW, HW, 1), generator=g).float() / 16.0
    w = torch.randint(-32, 33, (3, 3, 1, 32), generator=g).float() / 64
    b = torch.randint(-8, 9, (32,), generator=g).float() / 64
    return g, x, w, b


# ---------------------------------------------------------------- backward

BWD_CASES = [
    # B, image, classes, hpre replicas, Dense(64) bias, optimizer (None: plain backward, MODE 0)
    (1, 12, 3, 1, False, None),
    (50, 28, 10, 2, True, SGD),
    (64, 28, 10, 4, True, SGD),
    (65, 12, 16, 3, False, MOMENTUM),
    (130, 28, 10, 8, True, ADAM),
    (65, 28, 3, 9, True, None),
    (130, 12, 16, 9, True, SGD),
    (64, 12, 10, 8, False, ADAM),
]


@pytest.mark.parametrize("B,HW,C,hrep,bias,kind", BWD_CASES)
def test_bwd_prologue(B, HW, C, hrep, bias, kind):
    from tensorflow_distributed_example_amd.ops import kernels as Kk
    g, x0, wc, bc = _data(B, HW, 100 + B + HW + C + hrep)
    Pn = ((HW - 2) // 2) ** 2
    Kf, Hd = Pn * 32, 64
    Bp = (B + 7) // 8 * 8
    rn = lambda *s, k=1.0: torch.randn(*s, generator=g) * k   # noqa: E731
    x = Guarded((B, HW, HW, 1), fill=x0)
    lab = Guarded((B,), torch.int32, fill=torch.randint(0, C, (B,), generator=g))
    hpre = Guarded((hrep, B, Hd), fill=rn(hrep, B, Hd, k=0.5 / hrep ** 0.5))
    hzero = Guarded((hrep, B, Hd), fill=torch.full((hrep, B, Hd), 7.0))
    Pt = Guarded((Kf, Bp), fill=torch.zeros(Kf, Bp))
    amax = Guarded((Pn, 4, Bp), torch.int64, fill=torch.zeros(Pn, 4, Bp, dtype=torch.int64))
    # flat variable buffer [W1 | W2 | b2 (padded to 16) | b1] with its slots; the trunk reads the head from copies
    off_w2, off_b2, off_b1 = Kf * Hd, Kf * Hd + Hd * C, Kf * Hd + Hd * C + 16
    nflat = off_b1 + Hd
    wflat = torch.zeros(nflat)
    wflat[:off_w2] = rn(Kf * Hd, k=0.02)
    wflat[off_w2:off_b2] = rn(Hd * C, k=0.3)
    wflat[off_b2:off_b2 + C] = rn(C, k=0.1)
    wflat[off_b1:] = rn(Hd, k=0.1)
    mflat, vflat = rn(nflat, k=1e-3), torch.rand(nflat, generator=g) * 1e-6
    wd, md, vd = wflat.to(DEV), mflat.to(DEV), vflat.to(DEV)
    W1 = wd[:off_w2].view(Kf, Hd)
    W2s, b2s = wd[off_w2:off_b2].view(Hd, C).clone(), wd[off_b2:off_b2 + C].clone()
    b1s = wd[off_b1:].clone() if bias else None
    scale = 1.0 / 256
    xd, wcd, bcd = x.t, wc.to(DEV), bc.to(DEV)
    Kk.convnet_fwd(xd, wcd, bcd, W1, torch.zeros(B, Hd, device=DEV), Pt.t, amax.t)
    dW1 = torch.full((Kf, Hd), 9.0, device=DEV)
    dw, db = torch.zeros(3, 3, 1, 32, device=DEV), torch.zeros(32, device=DEV)
    dW2, db2, db1 = torch.zeros(Hd, C, device=DEV), torch.zeros(C, device=DEV), torch.zeros(Hd, device=DEV)
    met = torch.zeros(4, device=DEV)
    t_now = 3
    iters = torch.full((1,), t_now, dtype=torch.int64, device=DEV)
    iprev = torch.zeros(1, dtype=torch.int64, device=DEV)
    pend = torch.zeros(1, dtype=torch.int32, device=DEV)
    opt = None
    if kind is not None:
        opt = Kk.BwdOpt(_hyper(kind), wd.data_ptr(),
                        md.data_ptr() if kind != SGD else None, vd.data_ptr() if kind == ADAM else None,
                        0, off_w2, off_b2, off_b1 if bias else -1, None, 0, iters.data_ptr(), iprev.data_ptr(),
                        Kk.FlatApply(), pend.data_ptr(), 1, 0)
    W1_0 = _f64(W1)
    Kk.convnet_bwd(xd, amax.t, hpre.t, hzero.t, b1s, W2s, b2s, lab.t, scale=scale, pre_relu=True, metrics=met,
                   W1row=W1, Pt=Pt.t, dW1=dW1, dwc=dw, dbc=db, dW2=dW2, db2=db2, db1=db1, B=B, opt=opt)
    torch.cuda.synchronize()

    xn = _f64(x0)[..., 0]
    pooled, zw = conv_pool(xn, _f64(wc)[:, :, 0], _f64(bc))
    h, dl, dH, loss, correct = head(_f64(hpre.t).sum(0), _f64(b1s) if bias else None, _f64(W2s), _f64(b2s),
                                    lab.t.cpu().numpy(), scale)
    dW1_ref = pooled.reshape(B, Kf).T @ dH
    dw_ref, db_ref = conv_pool_bwd(xn, zw, (dH @ W1_0.T).reshape(B, Pn, 32))
    figs = {"dconv_w": _rel(dw.view(3, 3, 32), dw_ref), "dconv_b": _rel(db, db_ref)}
    assert np.array_equal(_f64(Pt.t)[:, :B].T, pooled.reshape(B, Kf))   # the operands the backward read
    upd_tol = TOL
    if kind is None:
        figs.update(dW1=_rel(dW1, dW1_ref), dW2=_rel(dW2, h.T @ dl), db2=_rel(db2, dl.sum(0)))
        if bias:
            figs["db1"] = _rel(db1, dH.sum(0))
    else:
        m0, v0 = _f64(mflat[:off_w2]).reshape(Kf, Hd), _f64(vflat[:off_w2]).reshape(Kf, Hd)
        w_ref, m_ref, v_ref = opt_step(kind, W1_0, dW1_ref, m0, v0, t_now)
        figs["W1"] = _rel(W1, w_ref)
        # SGD / momentum: the update itself (lr = 1: the gradient), at TOL plus what the new weights' own
        # float32 rounding (<= 2^-24 |w| per element, twice for w + v) puts between it and the oracle's
        upd = np.linalg.norm(w_ref - W1_0)
        upd_tol = TOL + 2.0 ** -23 * np.linalg.norm(w_ref) / upd
        if kind != ADAM:
            figs["W1 update"] = float(np.linalg.norm(_f64(W1) - w_ref) / upd)
        if kind != SGD:
            figs["m1"] = _rel(md[:off_w2].view(Kf, Hd), m_ref)
        if kind == ADAM:
            figs["v1"] = _rel(vd[:off_w2].view(Kf, Hd), v_ref)
        assert int(iprev.item()) == t_now and int(pend.item()) == 1 and int(iters.item()) == t_now
    print("bwd", (B, HW, C, hrep, bias, kind), {k: f"{v:.2e}" for k, v in figs.items()})
    for name, v in figs.items():
        assert v < (upd_tol if name == "W1 update" else TOL), (name, v)
    assert abs(met[0].item() - loss) < 1e-5 * abs(loss)
    assert met[1].item() == correct and met[2].item() == B
    assert bool((hzero.t == 0).all()), "the other-parity hpre buffer must be all zero"
    for name, gb in [("x", x), ("labels", lab), ("hpre", hpre), ("hzero", hzero), ("Pt", Pt), ("amax", amax)]:
        assert gb.intact(), f"guard page of {name} overwritten"


# ---------------------------------------------------------------- forward

FWD_CASES = [
    # B, image, optimizer (None: plain), pend, grep, snapshot classes (0: none), snapshot b1, fly_count
    (37, 12, None, 0, 1, 0, False, False),
    (37, 28, SGD, 1, 1, 10, True, True),
    (16, 12, MOMENTUM, 1, 3, 16, False, False),
    (20, 12, ADAM, 1, 8, 0, False, True),
    (20, 12, ADAM, 0, 8, 3, True, True),
    (37, 28, SGD, 0, 3, 0, False, False),
]


@pytest.mark.parametrize("B,HW,kind,pend,grep,snapC,snapb1,fly", FWD_CASES)
def test_fwd_prologue(B, HW, kind, pend, grep, snapC, snapb1, fly):
    from tensorflow_distributed_example_amd.ops import kernels as Kk
    g, x0, wc, bc = _data(B, HW, 200 + B + HW + grep + snapC)
    Pn = ((HW - 2) // 2) ** 2
    Kf, Hd = Pn * 32, 64
    Bp = (B + 7) // 8 * 8
    x = Guarded((B, HW, HW, 1), fill=x0)
    hpre = Guarded((B, Hd), fill=torch.zeros(B, Hd))
    Pt = Guarded((Kf, Bp), fill=torch.full((Kf, Bp), 5.0))
    amax = Guarded((Pn, 4, Bp), torch.int64, fill=torch.zeros(Pn, 4, Bp, dtype=torch.int64))
    W1 = (torch.randn(Kf, Hd, generator=g) * 0.02).to(DEV)
    # flat buffers [conv kernel 288 | conv bias 32]; the gradient in grep replicas of stride 512
    off_wc, off_bc, stride = 0, 288, 512
    wflat = Guarded((320,), fill=torch.cat([wc.reshape(-1), bc]))
    gflat = Guarded((grep * stride,), fill=torch.randn(grep * stride, generator=g) * (0.02 if kind != ADAM else 1e-3))
    mflat = Guarded((320,), fill=torch.randn(320, generator=g) * 1e-3)
    vflat = Guarded((320,), fill=torch.rand(320, generator=g) * 1e-6)
    t_prev = 4
    iters = torch.full((1,), t_prev, dtype=torch.int64, device=DEV)
    counter = torch.full((1,), 11, dtype=torch.int64, device=DEV)
    pendt = torch.full((1,), pend, dtype=torch.int32, device=DEV)
    flyt = torch.zeros(1, dtype=torch.int64, device=DEV)
    n_snap = 64 + 64 * snapC + snapC
    snap = Guarded((max(n_snap, 4),), fill=torch.full((max(n_snap, 4),), -3.0))
    s_w2 = Guarded((64, max(snapC, 1)), fill=torch.randn(64, max(snapC, 1), generator=g))
    s_b2 = Guarded((max(snapC, 1),), fill=torch.randn(max(snapC, 1), generator=g))
    s_b1 = Guarded((64,), fill=torch.randn(64, generator=g))
    opt = None
    if kind is not None:
        opt = Kk.StepOpt(_hyper(kind), wflat.t.data_ptr(),
                         gflat.t.data_ptr(), mflat.t.data_ptr() if kind != SGD else None,
                         vflat.t.data_ptr() if kind == ADAM else None, iters.data_ptr(), pendt.data_ptr(), grep, stride,
                         flyt.data_ptr() if fly else None)
        if snapC:
            opt.hsrc_w2, opt.hsrc_b2 = s_w2.t.data_ptr(), s_b2.t.data_ptr()
            opt.hsrc_b1 = s_b1.t.data_ptr() if snapb1 else None
            opt.hsnap, opt.hC = snap.t.data_ptr(), snapC
    keep = {n: b.t.clone() for n, b in [("w", wflat), ("g", gflat), ("m", mflat), ("v", vflat)]}
    Kk.convnet_fwd(x.t, wflat.t[:288].view(3, 3, 1, 32), wflat.t[288:], W1, hpre.t, Pt.t, amax.t, opt=opt,
                   off_wc=off_wc, off_bc=off_bc, inc_iter=counter)
    torch.cuda.synchronize()

    w_eff = _f64(keep["w"])
    if kind is not None and pend:
        gsum = _f64(keep["g"]).reshape(grep, stride)[0, :320].copy()
        for r in range(1, grep):   # replica order
            gsum = gsum + _f64(keep["g"]).reshape(grep, stride)[r, :320]
        w_eff, _, _ = opt_step(kind, w_eff, gsum, _f64(keep["m"]), _f64(keep["v"]), t_prev)
    pooled, zw = conv_pool(_f64(x0)[..., 0], w_eff[:288].reshape(3, 3, 32), w_eff[288:])
    pooled = pooled.reshape(B, Kf)
    figs = {"Pt": _rel(_f64(Pt.t)[:, :B].T, pooled), "hpre": _rel(hpre.t, pooled @ _f64(W1))}
    print("fwd", (B, HW, kind, pend, grep, snapC, snapb1, fly), {k: f"{v:.2e}" for k, v in figs.items()})
    if kind is None or not pend:
        assert np.array_equal(_f64(Pt.t)[:, :B].T, pooled)   # exact conv (quantized operands)
    for name, v in figs.items():
        assert v < TOL, (name, v)
    assert bool((Pt.t[:, B:] == 0).all())
    am = amax.t.view(torch.uint8).view(Pn, 4, Bp, 8).permute(2, 0, 1, 3).reshape(Bp, Kf)[:B].cpu().numpy()
    decided = np.abs(zw.max(3).reshape(B, Kf)) > 1e-6     # away from the ReLU edge the mask is the oracle's
    assert np.array_equal((am != 255)[decided], (pooled > 0)[decided])
    assert int(counter.item()) == 12 and int(pendt.item()) == pend and int(iters.item()) == t_prev
    assert int(flyt.item()) == (1 if (fly and pend and kind is not None) else 0)
    for n, b in [("w", wflat), ("g", gflat), ("m", mflat), ("v", vflat)]:
        assert torch.equal(b.t, keep[n]), f"the forward must not write {n}"
    if kind is not None and snapC:
        want = torch.cat([s_b1.t if snapb1 else torch.zeros(64, device=DEV), s_w2.t.reshape(-1), s_b2.t])
        assert torch.equal(snap.t[:n_snap], want), "the snapshot must equal its sources bitwise"
    else:
        assert bool((snap.t == -3.0).all())
    for name, gb in [("x", x), ("hpre", hpre), ("Pt", Pt), ("amax", amax), ("w", wflat), ("g", gflat), ("m", mflat),
                     ("v", vflat), ("hsnap", snap), ("hsrc_w2", s_w2), ("hsrc_b2", s_b2), ("hsrc_b1", s_b1)]:
        assert gb.intact(), f"guard page of {name} overwritten"
