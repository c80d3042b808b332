"""The float32 backward's head chain (csrc/include/tde_convnet.h: head_logits_ce16) runs the softmax-CE on all
16 waves, the trunk workgroups skip the metrics, and the backward of 28 x 28 images takes kernels with compile-time
geometry (csrc/kernels/convnet_f32.hip: Geo<28, 28>) while every other shape keeps the runtime form.  The entry points
are called directly at the smallest shapes where that code can go wrong (a lone row, a ragged chunk, a full
chunk, a 1-row tail, three chunks; 28 x 28 and 12 x 12; 3 / 10 / 16 classes; 1 / 2 / 4 replicas and the
deterministic layout; plain, fused SGD and fused Adam) and compared with the float64 numpy oracle of
tests/test_prologue_gpu.py at the bound of tests/test_fp32_gpu.py (1e-5 relative, norm-wise); the counts are
exact.  Every buffer lies between guard pages of sentinels."""
import numpy as np
import pytest
import torch

from test_prologue_gpu import (ADAM, DEV, SGD, TOL, Guarded, _data, _f64, _hyper, _rel, conv_pool, conv_pool_bwd,
                               head, opt_step)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("fp32_policy")]

DET = "det"   # the deterministic layout: one hpre replica per pooled position, conv partials per workgroup


class runtime_geometry:
    """Forces the runtime-geometry kernels for every shape while active."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from tensorflow_distributed_example_amd import _native as N
        self.fn = N.hip().tde_convnet_f32_runtime_geom
        self.prev = self.fn(1 if self.on else 0)

    def __exit__(self, *exc):
        self.fn(self.prev)


def _inputs(B, HW, C, hrep, bias, seed):
    """Host-side inputs of one case (shared by the runs that are compared with each other)."""
    g, x0, wc, bc = _data(B, HW, seed)
    Pn = ((HW - 2) // 2) ** 2
    Kf, Hd = Pn * 32, 64
    R = Pn if hrep == DET else hrep
    rn = lambda *s, k=1.0: torch.randn(*s, generator=g) * k   # noqa: E731
    d = dict(B=B, HW=HW, C=C, R=R, det=hrep == DET, bias=bias, Pn=Pn, Kf=Kf, x0=x0, wc=wc, bc=bc)
    d["lab"] = torch.randint(0, C, (B,), generator=g)
    d["hpre"] = rn(R, B, Hd, k=0.5 / R ** 0.5)
    off_w2, off_b2, off_b1 = Kf * Hd, Kf * Hd + Hd * C, Kf * Hd + Hd * C + 16
    wflat = torch.zeros(off_b1 + Hd)
    wflat[:off_w2] = rn(Kf * Hd, k=0.02)
    wflat[off_w2:off_b2] = rn(Hd * C, k=0.3)
    wflat[off_b2:off_b2 + C] = rn(C, k=0.1)
    wflat[off_b1:] = rn(Hd, k=0.1)
    d.update(offs=(off_w2, off_b2, off_b1), wflat=wflat, mflat=rn(off_b1 + Hd, k=1e-3),
             vflat=torch.rand(off_b1 + Hd, generator=g) * 1e-6)
    return d


def _run(d, kind, fallback=False):
    """One forward (for Pt / amax) and one backward through the entry points; returns the device results."""
    from tensorflow_distributed_example_amd.ops import kernels as Kk
    B, HW, C, R, Pn, Kf, Hd = d["B"], d["HW"], d["C"], d["R"], d["Pn"], d["Kf"], 64
    off_w2, off_b2, off_b1 = d["offs"]
    Bp = (B + 7) // 8 * 8
    x = Guarded((B, HW, HW, 1), fill=d["x0"])
    lab = Guarded((B,), torch.int32, fill=d["lab"])
    hpre = Guarded((R, B, Hd), fill=d["hpre"])
    hzero = Guarded((R, B, Hd), fill=torch.full((R, B, Hd), 7.0))
    Pt = Guarded((Kf, Bp), fill=torch.zeros(Kf, Bp))
    amax = Guarded((Pn, 4, Bp), torch.int64, fill=torch.zeros(Pn, 4, Bp, dtype=torch.int64))
    cpart = Guarded(((Pn + 1) * 320,), fill=torch.zeros((Pn + 1) * 320)) if d["det"] else None
    wd, md, vd = d["wflat"].to(DEV), d["mflat"].to(DEV), d["vflat"].to(DEV)
    W1 = wd[:off_w2].view(Kf, Hd)
    W2s, b2s = wd[off_w2:off_b2].view(Hd, C).clone(), wd[off_b2:off_b2 + C].clone()
    b1s = wd[off_b1:].clone() if d["bias"] else None
    fwd_h = Guarded((B, Hd), fill=torch.zeros(B, Hd))
    dW1 = torch.full((Kf, Hd), 9.0, device=DEV)
    dw, db = torch.zeros(3, 3, 1, 32, device=DEV), torch.zeros(32, device=DEV)
    dW2, db2, db1 = torch.zeros(Hd, C, device=DEV), torch.zeros(C, device=DEV), torch.zeros(Hd, device=DEV)
    met = torch.zeros(4, device=DEV)
    iters = torch.full((1,), 3, dtype=torch.int64, device=DEV)
    iprev = torch.zeros(1, dtype=torch.int64, device=DEV)
    pend = torch.zeros(1, dtype=torch.int32, device=DEV)
    opt = None
    if kind is not None:
        opt = Kk.BwdOpt(_hyper(kind), wd.data_ptr(), md.data_ptr() if kind != SGD else None,
                        vd.data_ptr() if kind == ADAM else None, 0, off_w2, off_b2, off_b1 if d["bias"] else -1, None, 0,
                        iters.data_ptr(), iprev.data_ptr(), Kk.FlatApply(), pend.data_ptr(), 1, 0)
    with runtime_geometry(fallback):
        Kk.convnet_fwd(x.t, d["wc"].to(DEV), d["bc"].to(DEV), W1, fwd_h.t, Pt.t, amax.t)
        fwd_hpre = fwd_h.t.clone()
        Kk.convnet_bwd(x.t, amax.t, hpre.t, hzero.t, b1s, W2s, b2s, lab.t, scale=1.0 / 256, pre_relu=True, metrics=met,
                       W1row=W1, Pt=Pt.t, dW1=dW1, dwc=dw, dbc=db, dW2=dW2, db2=db2, db1=db1, B=B, opt=opt,
                       cpart=cpart.t if cpart else None)
        if cpart:
            Kk.convnet_cgrad_reduce(cpart.t, Pn, dw, db)
    torch.cuda.synchronize()
    assert bool((hzero.t == 0).all()), "the other-parity hpre buffer must be all zero"
    guards = [("x", x), ("labels", lab), ("hpre", hpre), ("hzero", hzero), ("Pt", Pt), ("amax", amax), ("fwd hpre", fwd_h)]
    for name, gb in guards + ([("cpart", cpart)] if cpart else []):
        assert gb.intact(), f"guard page of {name} overwritten"
    if kind is not None:
        assert int(iprev.item()) == 3 and int(pend.item()) == 1 and int(iters.item()) == 3
    return dict(Pt=Pt.t[:, :B].clone(), fwd_hpre=fwd_hpre, dW1=dW1, dwc=dw.view(3, 3, 32), dbc=db, dW2=dW2, db2=db2,
                db1=db1, met=met, w=wd, m=md, v=vd)


def _oracle(d, kind):
    """float64 results of one case, in the names of _run's dictionary (computed once per case)."""
    B, C, Pn, Kf, Hd = d["B"], d["C"], d["Pn"], d["Kf"], 64
    off_w2, off_b2, off_b1 = d["offs"]
    w0 = _f64(d["wflat"])
    W1_0, W2, b2 = w0[:off_w2].reshape(Kf, Hd), w0[off_w2:off_b2].reshape(Hd, C), w0[off_b2:off_b2 + C]
    b1 = w0[off_b1:] if d["bias"] else None
    xn = _f64(d["x0"])[..., 0]
    pooled, zw = conv_pool(xn, _f64(d["wc"])[:, :, 0], _f64(d["bc"]))
    hsum = _f64(d["hpre"])[0].copy()
    for r in range(1, d["R"]):   # replica order
        hsum = hsum + _f64(d["hpre"])[r]
    h, dl, dH, loss, correct = head(hsum, b1, W2, b2, d["lab"].numpy(), 1.0 / 256)
    pooled = pooled.reshape(B, Kf)
    dwc, dbc = conv_pool_bwd(xn, zw, (dH @ W1_0.T).reshape(B, Pn, 32))
    ref = dict(pooled=pooled, fwd_hpre=pooled @ W1_0, dwc=dwc, dbc=dbc, loss=loss, correct=correct)
    grads = {"W1": (0, off_w2, pooled.T @ dH), "W2": (off_w2, off_b2, h.T @ dl), "b2": (off_b2, off_b2 + C, dl.sum(0))}
    if d["bias"]:
        grads["b1"] = (off_b1, off_b1 + Hd, dH.sum(0))
    ref["grads"] = grads
    if kind is not None:
        m0, v0 = _f64(d["mflat"]), _f64(d["vflat"])
        ref["upd"] = {n: opt_step(kind, w0[lo:hi], g.reshape(-1), m0[lo:hi], v0[lo:hi], 3) for n, (lo, hi, g) in grads.items()}
    return ref


def _check(d, kind, got, ref, tag):
    figs = {"fwd hpre": _rel(got["fwd_hpre"], ref["fwd_hpre"]), "dconv_w": _rel(got["dwc"], ref["dwc"]),
            "dconv_b": _rel(got["dbc"], ref["dbc"])}
    assert np.array_equal(_f64(got["Pt"]).T, ref["pooled"])   # exact conv on quantized operands: what the backward read
    tol = {}
    for n, (lo, hi, g) in ref["grads"].items():
        if kind is None:
            figs["d" + n] = _rel({"W1": got["dW1"], "W2": got["dW2"], "b2": got["db2"], "b1": got["db1"]}[n].reshape(-1),
                                 g.reshape(-1))
            continue
        w_ref, m_ref, v_ref = ref["upd"][n]
        figs[n] = _rel(got["w"][lo:hi], w_ref)
        if kind == SGD:
            # lr = 1: the update is the gradient; at TOL plus what the new weights' own float32 rounding
            # (<= 2^-24 |w| per element) puts between it and the oracle's
            w0 = _f64(d["wflat"])[lo:hi]
            upd = np.linalg.norm(w_ref - w0)
            figs[n + " update"] = float(np.linalg.norm(_f64(got["w"][lo:hi]) - w_ref) / upd)
            tol[n + " update"] = TOL + 2.0 ** -23 * np.linalg.norm(w_ref) / upd
        if kind == ADAM:
            figs["m " + n] = _rel(got["m"][lo:hi], m_ref)
            figs["v " + n] = _rel(got["v"][lo:hi], v_ref)
    met = got["met"].cpu().numpy()
    print(tag, {k: f"{v:.2e}" for k, v in figs.items()}, "loss", met[0], ref["loss"], "correct", met[1], "count", met[2])
    for name, v in figs.items():
        assert v < tol.get(name, TOL), (name, v)
    assert abs(float(met[0]) - ref["loss"]) < 1e-5 * abs(ref["loss"])
    assert met[1] == ref["correct"] and met[2] == d["B"]   # exact: summed over 16 waves


CASES = [
    # B, image, classes, hpre replicas, Dense(64) bias, optimizer (None: plain backward, MODE 0)
    (1, 28, 10, 1, True, None),
    (1, 12, 3, 2, False, ADAM),
    (17, 28, 3, 2, True, SGD),
    (17, 12, 16, DET, True, None),
    (17, 28, 16, 4, True, ADAM),
    (64, 28, 10, 4, True, SGD),
    (64, 28, 10, 2, True, ADAM),
    (64, 12, 10, 1, True, SGD),
    (65, 28, 16, DET, False, SGD),
    (65, 12, 3, 4, True, None),
    (65, 28, 10, 1, True, None),
    (130, 28, 10, DET, True, ADAM),
    (130, 12, 16, 2, False, SGD),
    (130, 28, 3, 4, True, None),
]


@pytest.mark.parametrize("B,HW,C,hrep,bias,kind", CASES)
def test_bwd_head(B, HW, C, hrep, bias, kind):
    d = _inputs(B, HW, C, hrep, bias, 300 + B + HW + C)
    ref = _oracle(d, kind)
    got = _run(d, kind)
    _check(d, kind, got, ref, ("bwd_head", B, HW, C, hrep, bias, kind))
    if hrep == DET:   # deterministic layout: a second run of the same case is bitwise equal, metrics included
        again = _run(d, kind)
        for n in (k for k in got if k != "fwd_hpre"):   # the plain forward's split-K adds are float atomics
            assert torch.equal(got[n], again[n]), f"deterministic layout: {n} differs between two runs"


@pytest.mark.parametrize("B,C,hrep,kind", [(65, 10, 4, None), (17, 16, 2, SGD), (130, 3, DET, ADAM)])
def test_runtime_form_at_28(B, C, hrep, kind):
    """The runtime-geometry kernels forced at 28 x 28, against the oracle and against the specialised ones."""
    d = _inputs(B, 28, C, hrep, True, 400 + B + C)
    ref = _oracle(d, kind)
    spec, fall = _run(d, kind), _run(d, kind, fallback=True)
    _check(d, kind, spec, ref, ("specialised", B, C, hrep, kind))
    _check(d, kind, fall, ref, ("runtime form", B, C, hrep, kind))
    assert torch.equal(spec["Pt"], fall["Pt"])
    names = ["fwd_hpre", "dwc", "dbc"] + (["dW1", "dW2", "db2", "db1"] if kind is None else ["w"] + (["m", "v"] if kind == ADAM else []))
    for n in names:
        assert _rel(fall[n], _f64(spec[n])) < TOL, n
    assert torch.equal(spec["met"][1:3], fall["met"][1:3])
