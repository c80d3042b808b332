"""The float32 step kernels place their workgroups by the maps of csrc/include/tde_convnet.h (fwd_slot, bwd_slot:
the workgroups that hand W1 rows, Pt rows and argmax words to each other between the two launches get ids of one
class mod 8).  A map changes which workgroup does a piece of the step, never what the piece is: with
tde_convnet_f32_identity_slots(1) as the reference on the same inputs, everything that does not go through float
atomics is bit-identical (Pt, argmax, hpre in the deterministic layout; dW1 / dW2 / db2 / db1, the updated weights,
Adam's slots, the metrics, and the conv gradients from the deterministic partials), the split-K atomics of hpre
stay within the 1e-5 of tests/test_fwd_group_gpu.py, and two fused SGD steps in a row (both hpre parities) match
the float64 oracle of tests/test_prologue_gpu.py at its tolerance."""
import numpy as np
import pytest
import torch

from test_bwd_head_gpu import DET, _inputs, _run
from test_fwd_group_gpu import _buffers, _case, _check_trunk
from test_prologue_gpu import ADAM, DEV, SGD, TOL, _f64, _hyper, _rel, conv_pool, conv_pool_bwd, head
from test_step_forms_gpu import _same

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("fp32_policy")]

HD = 64


class identity_slots:
    """Forces the identity maps in both kernels while active."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from tensorflow_distributed_example_amd import _native as N
        self.fn = N.hip().tde_convnet_f32_identity_slots
        self.prev = self.fn(1 if self.on else 0)

    def __exit__(self, *exc):
        self.fn(self.prev)


# ---------------------------------------------------------------- forward

def _fwd(c, hrep, ident):
    from tensorflow_distributed_example_amd.ops import kernels as Kk
    Pt, amax, Bp = _buffers(c)
    hpre = torch.zeros(hrep, c["B"], HD, device=DEV)
    with identity_slots(ident):
        Kk.convnet_fwd(c["x"], c["w"], c["b"], c["W1"], hpre, Pt, amax, hrep=hrep)
    torch.cuda.synchronize()
    _check_trunk(c, Pt, amax, Bp)
    return hpre, Pt, amax


# 28 x 28: P = 169, 43 groups (5 full runs of 8, a partial run of 3); 12 x 12: Wp = 5, P = 25, 7 groups (the last one
# holds one position) at one tile, a ragged second tile and five tiles
@pytest.mark.parametrize("B,HW", [(64, 28), (16, 12), (17, 12), (80, 12)])
def test_forward_maps_against_identity(B, HW):
    c = _case(B, HW, HW)
    for hrep in (c["P"], 1, 4):   # the deterministic layout (one replica per group), one replica, the step's four
        new, ref = _fwd(c, hrep, False), _fwd(c, hrep, True)
        assert torch.equal(new[1], ref[1]), "Pt differs"
        assert torch.equal(new[2], ref[2]), "amax differs"
        e = _rel(new[0].double().sum(0), _f64(ref[0].double().sum(0)))
        eo = _rel(new[0].double().sum(0), _f64(c["ref"]))
        print(f"B={B} {HW}x{HW} hrep={hrep}: hpre against identity {e:.3e}, against the oracle {eo:.3e}")
        if hrep == c["P"]:
            assert torch.equal(new[0], ref[0]), "hpre differs in the deterministic layout"
        else:
            # every replica receives the same addends under both maps (the replica is the group's): each replica
            # within the atomics' order bound
            for r in range(hrep):
                assert _rel(new[0][r], _f64(ref[0][r])) < TOL, (hrep, r)
        assert e < TOL and eo < TOL, (e, eo)


# ---------------------------------------------------------------- backward

def _bwd_pair(d, kind, fallback):
    with identity_slots(False):
        new = _run(d, kind, fallback=fallback)
    with identity_slots(True):
        ref = _run(d, kind, fallback=fallback)
    assert torch.equal(new["Pt"], ref["Pt"])
    return new, ref


@pytest.mark.parametrize("kind", [None, SGD, ADAM])
@pytest.mark.parametrize("B", [64, 128])
def test_production_backward_maps_against_identity(B, kind):
    d = _inputs(B, 28, 10, 4, True, 800 + B)
    new, ref = _bwd_pair(d, kind, False)
    _same(new, ref, kind, False, "maps against identity, production form")


@pytest.mark.parametrize("B,HW,hrep,kind", [(17, 12, 2, ADAM), (17, 28, 2, SGD), (65, 28, 4, None)])
def test_general_backward_maps_against_identity(B, HW, hrep, kind):
    """12 x 12 (P = 25: no full run of 32 positions, the 1-D forward grid alone) and, so that the general form's map
    moves positions too, 28 x 28 at ragged batches."""
    d = _inputs(B, HW, 10, hrep, True, 810 + B + HW)
    new, ref = _bwd_pair(d, kind, True)
    _same(new, ref, kind, False, "maps against identity, general form")


@pytest.mark.parametrize("B,hrep,kind,fallback", [(64, 4, SGD, False), (128, 4, None, False), (17, DET, ADAM, True)])
def test_conv_gradients_from_deterministic_partials(B, hrep, kind, fallback):
    """The partials are stored by position and summed in position order: bit-identical conv gradients."""
    d = _inputs(B, 28, 10, hrep, True, 820 + B)
    if hrep != DET:
        d = dict(d, det=True)
    new, ref = _bwd_pair(d, kind, fallback)
    _same(new, ref, kind, True, "maps against identity, deterministic partials")


# ---------------------------------------------------------------- one fused step, twice

def test_two_fused_sgd_steps_against_the_oracle():
    """Forward then backward with the SGD update inside (MODE 1), twice in a row from seeded weights: the second step
    reads the W1 rows the first backward wrote and the other hpre parity.  float64 oracle of the same two steps."""
    from tensorflow_distributed_example_amd.ops import kernels as Kk
    B, HWi, C, R = 64, 28, 10, 4
    d = _inputs(B, HWi, C, R, True, 830)
    Pn, Kf = d["Pn"], d["Kf"]
    off_w2, off_b2, off_b1 = d["offs"]
    x, lab = d["x0"].to(DEV), d["lab"].to(DEV).int()
    wd = d["wflat"].to(DEV)
    W1 = wd[:off_w2].view(Kf, HD)
    hpre2 = torch.zeros(2, R, B, HD, device=DEV)
    Pt = torch.zeros(Kf, B, device=DEV)
    amax = torch.zeros(Pn, 4, B, dtype=torch.int64, device=DEV)
    dW1 = torch.zeros(Kf, HD, device=DEV)
    dw, db = torch.zeros(3, 3, 1, 32, device=DEV), torch.zeros(32, device=DEV)
    met = torch.zeros(4, device=DEV)
    iters = torch.full((1,), 3, dtype=torch.int64, device=DEV)
    iprev = torch.zeros(1, dtype=torch.int64, device=DEV)
    pend = torch.zeros(1, dtype=torch.int32, device=DEV)
    opt = Kk.BwdOpt(_hyper(SGD), wd.data_ptr(), None, None, 0, off_w2, off_b2, off_b1, None, 0, iters.data_ptr(),
                    iprev.data_ptr(), Kk.FlatApply(), pend.data_ptr(), 1, 0)
    wc, bc = d["wc"].to(DEV), d["bc"].to(DEV)
    for q in (0, 1):
        # the head variables as of this step's forward (the trunk reads the copy, the head workgroup updates wd)
        W2s, b2s, b1s = wd[off_w2:off_b2].view(HD, C).clone(), wd[off_b2:off_b2 + C].clone(), wd[off_b1:].clone()
        Kk.convnet_fwd(x, wc, bc, W1, hpre2[q], Pt, amax, hrep=R)
        Kk.convnet_bwd(x, amax, hpre2[q], hpre2[1 - q], b1s, W2s, b2s, lab, scale=1.0 / 256, pre_relu=True,
                       metrics=met, W1row=W1, Pt=Pt, dW1=dW1, dwc=dw, dbc=db, B=B, opt=opt)
    torch.cuda.synchronize()

    w = _f64(d["wflat"])
    w0 = w.copy()
    xn = _f64(d["x0"])[..., 0]
    pooled, zw = conv_pool(xn, _f64(d["wc"])[:, :, 0], _f64(d["bc"]))
    pooled = pooled.reshape(B, Kf)
    dwc_ref, dbc_ref, loss_ref, correct_ref = 0.0, 0.0, 0.0, 0
    for _ in (0, 1):
        W1r, W2r = w[:off_w2].reshape(Kf, HD), w[off_w2:off_b2].reshape(HD, C)
        h, dl, dH, loss, correct = head(pooled @ W1r, w[off_b1:], W2r, w[off_b2:off_b2 + C], d["lab"].numpy(), 1.0 / 256)
        gc, gb = conv_pool_bwd(xn, zw, (dH @ W1r.T).reshape(B, Pn, 32))
        dwc_ref, dbc_ref, loss_ref, correct_ref = dwc_ref + gc, dbc_ref + gb, loss_ref + loss, correct_ref + correct
        w = w.copy()   # lr = 1
        w[:off_w2] -= (pooled.T @ dH).reshape(-1)
        w[off_w2:off_b2] -= (h.T @ dl).reshape(-1)
        w[off_b2:off_b2 + C] -= dl.sum(0)
        w[off_b1:] -= dH.sum(0)
    assert np.array_equal(_f64(Pt).T, pooled)
    figs, tol = {"dconv_w": _rel(dw.view(3, 3, 32), dwc_ref), "dconv_b": _rel(db, dbc_ref)}, {}
    for n, (lo, hi) in {"W1": (0, off_w2), "W2": (off_w2, off_b2), "b2": (off_b2, off_b2 + C),
                        "b1": (off_b1, off_b1 + HD)}.items():
        figs[n] = _rel(wd[lo:hi], w[lo:hi])
        # the two steps' update itself, at TOL plus the two float32 roundings of the stored weights
        # (<= 2^-24 |w| per element and step) that lie between it and the oracle's
        upd = np.linalg.norm(w[lo:hi] - w0[lo:hi])
        figs[n + " update"] = float(np.linalg.norm(_f64(wd[lo:hi]) - w[lo:hi]) / upd)
        tol[n + " update"] = TOL + 2.0 ** -23 * np.linalg.norm(w[lo:hi]) / upd
    m = met.cpu().numpy()
    print("two fused steps", {k: f"{v:.2e}" for k, v in figs.items()}, "loss", m[0], loss_ref, "correct", m[1], correct_ref)
    for name, v in figs.items():
        assert v < tol.get(name, TOL), (name, v)
    assert abs(float(m[0]) - loss_ref) < 1e-5 * abs(loss_ref)
    assert m[1] == correct_ref and m[2] == 2 * B
    assert int(iprev.item()) == 3 and int(pend.item()) == 1
    assert bool((hpre2[0] == 0).all()), "the second backward zeroes the first parity's buffer"
