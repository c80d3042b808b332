"""Float32 fused forward at eight waves per workgroup (csrc/kernels/convnet_f32.hip): wave w computes conv
channels 4w..4w+3, so a position's 8-byte argmax word is stored as two 32-bit halves by two waves, each wave writes
4 rows of Pt and one float4 of the pooled tile, the prologue runs over 512 threads, and waves 0-3 alone issue the
Dense(64) MFMAs.

The entry point is called directly, as tests/test_fwd_group_gpu.py does, at the smallest shapes where this can go
wrong: an 8x12 image (Hp = 3, Wp = 5, P = 15: the last group holds 3 positions, so lanes and waves run past the
data) at B = 1, 15 (image tile not full) and 17 (second tile almost empty; ldPt = 24 > B: the padding columns of Pt
are written as zeros), 16x16 at B = 64 (P = 49, 13 groups: one full run of the slot map, a partial run and a last
group of one position) and the model's 28x28 at a ragged B = 17.

Operands are unquantized float32, so the conv is not exact.  Bounds, all from the arithmetic and none from the
kernel: a conv output is bias + 9 fused multiply-adds in f32, one rounding each, so it differs from the float64
oracle by at most gamma_9 * S < 10 u S with u = 2^-24 and S = |b| + sum |x||w| of that output (Higham, Accuracy
and Stability, eq. 3.4); the pooled value is a maximum of four such outputs clamped at zero, so the same bound with
the window's largest S holds for Pt.  An argmax byte can differ from the oracle's only where the window's two
largest values lie within twice that bound of each other, or its maximum within the bound of zero: those entries
are exempt, at most 0.5 % of them.  hpre follows tests/test_fwd_group_gpu.py: 1e-5 norm-wise."""
import functools

import numpy as np
import pytest
import torch

DEV = "cuda"
TOL = 1e-5
HD = 64
U = 2.0 ** -24
EXEMPT_CAP = 0.005
SHAPES = [(1, 8, 12), (15, 8, 12), (17, 8, 12), (64, 16, 16), (17, 28, 28)]


# ---------------------------------------------------------------- oracle (NumPy float64) and its inputs

def _inputs(B, H, W):
    g = np.random.default_rng(1000 * H + 10 * W + B)
    P = ((H - 2) // 2) * ((W - 2) // 2)
    x = g.random((B, H, W), dtype=np.float32)
    w = (g.standard_normal((3, 3, 32)) * 0.3).astype(np.float32)
    b = (g.standard_normal(32) * 0.1).astype(np.float32)
    W1 = (g.standard_normal((P * 32, HD)) * 0.02).astype(np.float32)
    return x, w, b, W1


def _windows(z):
    """[B, Ho, Wo, 32] -> [B, P, 4, 32], window slot q = 2 * dy + dx."""
    B, Ho, Wo, C = z.shape
    Hp, Wp = Ho // 2, Wo // 2
    return z[:, :2 * Hp, :2 * Wp].reshape(B, Hp, 2, Wp, 2, C).transpose(0, 1, 3, 2, 4, 5).reshape(B, Hp * Wp, 4, C)


def conv_windows(x, w, b, dtype=np.float64):
    """Conv 3x3 VALID + bias per pool-window slot, bias first and taps in (ky, kx) order.  float64: the oracle;
    float32: every step one rounding, like the kernel's fmaf chain (the product is exact in float64)."""
    B, H, W = x.shape
    Ho, Wo = H - 2, W - 2
    z = np.broadcast_to(b.astype(dtype), (B, Ho, Wo, 32)).copy()
    for ky in range(3):
        for kx in range(3):
            prod = x[:, ky:ky + Ho, kx:kx + Wo, None].astype(np.float64) * w[ky, kx].astype(np.float64)
            z = (prod + z.astype(np.float64)).astype(dtype)
    return _windows(z)


def oracle(x, w, b):
    """pooled [B, P, 32], expected argmax byte [B, P, 32] (0xFF: ReLU zeroed), error bound of a pooled value
    [B, P, 32], exempt entries [B, P, 32]."""
    zw = conv_windows(x, w, b)
    S = conv_windows(np.abs(x), np.abs(w), np.abs(b)).max(2)
    bound = 10 * U * S
    top = np.sort(zw, axis=2)
    best, second = top[:, :, 3], top[:, :, 2]
    arg = np.where(best > 0, zw.argmax(2), 255).astype(np.uint8)   # argmax: the first maximum, as the kernel's >
    exempt = (best - second <= 2 * bound) | (np.abs(best) <= bound)
    return np.maximum(best, 0), arg, bound, exempt


@functools.lru_cache(maxsize=None)
def _case(B, H, W):
    """Inputs on the device and the oracle, computed once per shape and shared, never modified."""
    x, w, b, W1 = _inputs(B, H, W)
    pooled, arg, bound, exempt = oracle(x, w, b)
    P = pooled.shape[1]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return dict(B=B, H=H, W=W, P=P, Kf=P * 32, xn=x, wn=w, bn=b, x=t(x[..., None]), w=t(w[:, :, None, :]), b=t(b),
                W1=t(W1), pooled=pooled, arg=arg, bound=bound, exempt=exempt, ref=pooled.reshape(B, -1) @ W1.astype(np.float64))


def _rel(got, ref):
    got = got.detach().double().cpu().numpy() if torch.is_tensor(got) else np.asarray(got, np.float64)
    return float(np.linalg.norm(got - ref) / (np.linalg.norm(ref) + 1e-30))


def _buffers(c):
    Bp = (c["B"] + 7) // 8 * 8
    Pt = torch.full((c["Kf"], Bp), 5.0, device=DEV)
    amax = torch.full((c["P"], 4, Bp), 0x7777777777777777, dtype=torch.int64, device=DEV)
    return Pt, amax, Bp


def _check_trunk(c, Pt, amax, Bp, pooled=None, arg=None, bound=None, exempt=None):
    """Pt element-wise within the chain's bound, padding columns zero; both halves of every argmax word."""
    B, P = c["B"], c["P"]
    pooled = c["pooled"] if pooled is None else pooled
    arg, bound, exempt = (c["arg"], c["bound"], c["exempt"]) if arg is None else (arg, bound, exempt)
    got = Pt.double().cpu().numpy().reshape(P, 32, Bp).transpose(2, 0, 1)            # [Bp, P, 32]
    err = np.abs(got[:B] - pooled)
    print(f"Pt: largest error / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all(), float((err / bound).max())
    assert (got[B:] == 0).all(), "padding columns of Pt must be zero"
    am = amax.view(torch.uint8).view(P, 4, Bp, 8).permute(2, 0, 1, 3).cpu().numpy()[:B]   # [B, P, word, byte]
    want, ex = arg.reshape(B, P, 4, 8), exempt.reshape(B, P, 4, 8)
    frac = float(ex.mean())
    print(f"amax: exempt {frac:.2e} of {ex.size}")
    assert frac <= EXEMPT_CAP, frac
    for half, name in [(slice(0, 4), "low half (channels 8cg..8cg+3)"), (slice(4, 8), "high half (channels 8cg+4..8cg+7)")]:
        bad = (am[..., half] != want[..., half]) & ~ex[..., half]
        assert not bad.any(), (name, int(bad.sum()), np.argwhere(bad)[:4].tolist())


# ---------------------------------------------------------------- CPU: the exemption rule alone

@pytest.mark.parametrize("B,H,W", SHAPES)
def test_f32_chain_stays_within_bounds_on_these_seeds(B, H, W):
    """The same conv in NumPy float32 (one rounding per step) against float64, on the seeds the GPU tests use:
    every value within the bound, every non-exempt argmax byte equal, exempt entries under the cap."""
    x, w, b, _ = _inputs(B, H, W)
    pooled, arg, bound, exempt = oracle(x, w, b)
    zw = conv_windows(x, w, b, np.float32)
    best = zw.max(2)
    assert (np.abs(np.maximum(best, 0).astype(np.float64) - pooled) <= bound).all()
    arg32 = np.where(best > 0, zw.argmax(2), 255).astype(np.uint8)
    assert ((arg32 == arg) | exempt).all()
    assert exempt.mean() <= EXEMPT_CAP, exempt.mean()


# ---------------------------------------------------------------- GPU

@pytest.mark.gpu
@pytest.mark.usefixtures("fp32_policy")
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_fwd_waves_shapes(B, H, W):
    from tensorflow_distributed_example_amd.ops import kernels as Kk
    c = _case(B, H, W)
    Pt, amax, Bp = _buffers(c)
    hpre = torch.zeros(B, HD, device=DEV)
    Kk.convnet_fwd(c["x"], c["w"], c["b"], c["W1"], hpre, Pt, amax)
    torch.cuda.synchronize()
    _check_trunk(c, Pt, amax, Bp)
    e = _rel(hpre, c["ref"])
    print(f"B={B} {H}x{W}: hpre rel err {e:.3e}")
    assert e < TOL, e


@pytest.mark.gpu
@pytest.mark.usefixtures("fp32_policy")
@pytest.mark.parametrize("hrep", [1, 4])
def test_fwd_waves_replicas_accumulate(hrep):
    """hpre is +=: the replicas start from non-zero values and end at those values plus the oracle's product."""
    from tensorflow_distributed_example_amd.ops import kernels as Kk
    c = _case(17, 8, 12)
    Pt, amax, Bp = _buffers(c)
    h0 = torch.randn(hrep, c["B"], HD, generator=torch.Generator().manual_seed(hrep)).mul(0.1).to(DEV)
    hpre = h0.clone()
    Kk.convnet_fwd(c["x"], c["w"], c["b"], c["W1"], hpre, Pt, amax, hrep=hrep)
    torch.cuda.synchronize()
    _check_trunk(c, Pt, amax, Bp)
    e = _rel(hpre.double().sum(0), c["ref"] + h0.double().sum(0).cpu().numpy())
    print(f"hrep={hrep}: hpre rel err {e:.3e}")
    assert e < TOL, e
    if hrep == 4:   # groups 0..3 -> replicas 0..3: every replica received a share
        assert all(bool((hpre[r] != h0[r]).any()) for r in range(4))


def _run_det(Kk, c, stamps=None):
    """One launch in the deterministic layout (hrep = P) from zeroed buffers."""
    Pt, amax, Bp = _buffers(c)
    hpre = torch.zeros(c["P"], c["B"], HD, device=DEV)
    Kk.convnet_fwd(c["x"], c["w"], c["b"], c["W1"], hpre, Pt, amax, stamps=stamps, hrep=c["P"])
    torch.cuda.synchronize()
    return hpre, Pt, amax


@pytest.mark.gpu
@pytest.mark.usefixtures("fp32_policy")
@pytest.mark.parametrize("B,H,W", [(17, 8, 12), (64, 16, 16)])
def test_fwd_waves_deterministic_layout(B, H, W):
    """hrep = P: replica g receives one add per address, from group g alone, so two runs are bit-identical, the
    replicas past the group count stay zero, and the replicas summed in order give the oracle's product."""
    from tensorflow_distributed_example_amd.ops import kernels as Kk
    c = _case(B, H, W)
    ngroups = (c["P"] + 3) // 4
    (h1, Pt1, am1), (h2, Pt2, am2) = _run_det(Kk, c), _run_det(Kk, c)
    assert torch.equal(h1, h2) and torch.equal(Pt1, Pt2) and torch.equal(am1, am2)
    assert torch.all(h1[ngroups:] == 0)
    s = torch.zeros(B, HD, device=DEV)
    for r in range(ngroups):
        s = s + h1[r]
    e = _rel(s, c["ref"])
    assert e < TOL, e


@pytest.mark.gpu
@pytest.mark.usefixtures("fp32_policy")
@pytest.mark.parametrize("B,H,W", [(17, 8, 12), (64, 16, 16)])
def test_fwd_waves_diagnostic_form(B, H, W):
    """A launch with a stamp buffer computes the same bits, and every workgroup writes stamps 0-4 in order."""
    from tensorflow_distributed_example_amd.ops import kernels as Kk
    c = _case(B, H, W)
    Bp = (B + 7) // 8 * 8
    nwg = ((c["P"] + 3) // 4) * ((max(Bp, B) + 15) // 16)
    st = torch.zeros(nwg + 4, 8, dtype=torch.int64, device=DEV)
    plain, diag = _run_det(Kk, c), _run_det(Kk, c, stamps=st)
    for a, b, name in zip(plain, diag, ("hpre", "Pt", "amax")):
        assert torch.equal(a, b), name
    s = st.cpu().numpy()
    assert (s[:nwg, :5] > 0).all(), "a workgroup left one of the stamps 0-4 unwritten"
    assert (np.diff(s[:nwg, :5], axis=1) >= 0).all(), "stamps out of order"
    assert (s[nwg:] == 0).all(), "stamps written past the last workgroup"


@pytest.mark.gpu
@pytest.mark.usefixtures("fp32_policy")
@pytest.mark.parametrize("pend,hC,with_b1", [(1, 10, True), (0, 16, True), (1, 16, False), (0, 10, False)])
def test_fwd_waves_fused_step_path(pend, hC, with_b1):
    """While *pend the conv weights used are the SGD step of the stored ones (lr = 1: w - g, one rounding, the
    same value in torch float32), otherwise the stored ones; the counters advance by one per launch; the head
    snapshot equals its sources over 512 threads (3 elements per thread) and its b1 slots are zero without b1."""
    from tensorflow_distributed_example_amd.ops import kernels as Kk
    c = _case(17, 8, 12)
    g = torch.Generator().manual_seed(100 * hC + pend)
    wflat = torch.cat([c["w"].reshape(-1), c["b"]]).contiguous()
    gflat = (torch.randn(320, generator=g) * 0.05).to(DEV)
    w_eff = (wflat - gflat if pend else wflat).cpu().numpy()
    pooled, arg, bound, exempt = oracle(c["xn"], w_eff[:288].reshape(3, 3, 32), w_eff[288:])
    assert exempt.mean() <= EXEMPT_CAP
    iters = torch.full((1,), 4, dtype=torch.int64, device=DEV)
    counter = torch.full((1,), 11, dtype=torch.int64, device=DEV)
    pendt = torch.full((1,), pend, dtype=torch.int32, device=DEV)
    fly = torch.zeros(1, dtype=torch.int64, device=DEV)
    n_snap = 64 + 64 * hC + hC
    snap = torch.full((n_snap + 64,), -3.0, device=DEV)
    s_w2, s_b2, s_b1 = (torch.randn(n, generator=g).to(DEV) for n in (64 * hC, hC, 64))
    opt = Kk.StepOpt(Kk.OptHyper(0, 1.0, 0.0, 0.0, 0.0, 0.0), wflat.data_ptr(), gflat.data_ptr(), None, None,
                     iters.data_ptr(), pendt.data_ptr(), 1, 0, fly.data_ptr())
    opt.hsrc_w2, opt.hsrc_b2, opt.hsrc_b1 = s_w2.data_ptr(), s_b2.data_ptr(), s_b1.data_ptr() if with_b1 else None
    opt.hsnap, opt.hC = snap.data_ptr(), hC
    keep = wflat.clone()
    for launch in (1, 2):
        Pt, amax, Bp = _buffers(c)
        hpre = torch.zeros(c["B"], HD, device=DEV)
        Kk.convnet_fwd(c["x"], wflat[:288].view(3, 3, 1, 32), wflat[288:], c["W1"], hpre, Pt, amax, opt=opt,
                       off_wc=0, off_bc=288, inc_iter=counter)
        torch.cuda.synchronize()
        _check_trunk(c, Pt, amax, Bp, pooled, arg, bound, exempt)
        e = _rel(hpre, pooled.reshape(c["B"], -1) @ c["W1"].double().cpu().numpy())
        assert e < TOL, e
        assert int(counter.item()) == 11 + launch and int(fly.item()) == (launch if pend else 0)
        assert int(pendt.item()) == pend and int(iters.item()) == 4
    assert torch.equal(wflat, keep), "the forward must not write the stored weights"
    want = torch.cat([s_b1 if with_b1 else torch.zeros(64, device=DEV), s_w2, s_b2])
    assert torch.equal(snap[:n_snap], want), "the snapshot must equal its sources bitwise"
    assert bool((snap[n_snap:] == -3.0).all()), "the snapshot was written past its end"
