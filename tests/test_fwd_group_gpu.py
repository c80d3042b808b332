"""Float32 fused forward, grouped geometry (csrc/kernels/convnet_f32.hip): a workgroup owns 4 consecutive
pooled positions x one 16-image tile and sums the 4 positions' Dense(64) partial products in the MFMA's K
dimension before the split-K adds into hpre.

Shapes are the smallest at which the group / tile indexing can go wrong: an 8x12 image (Hp = 3, Wp = 5,
P = 15: the groups {0-3}, {4-7}, {8-11}, {12-14} all straddle a pooled row and the last is partial) at
B = 1, 16, 17, 37 (one image, one exact tile, a tile plus a row, a ragged tile count whose padding reaches
past the last tile's images), and 28x28 (P = 169: the last group is a single position) at B = 17.
Recipe of tests/test_fp32_gpu.py::test_convnet_fwd_f32: inputs in sixteenths and conv weights in
sixty-fourths, so the conv is exact in f32 and Pt / the argmax mask compare exactly with a float64 oracle;
hpre within that test's 1e-5 norm-wise."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("fp32_policy")]

DEV = "cuda"
TOL = 1e-5
HD = 64


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


@functools.lru_cache(maxsize=None)
def _case(B, H, W):
    """Inputs (on the device) and the float64 oracle (pooled [B, Kf], hpre [B, 64]); computed once per shape
    and shared, never modified."""
    g = torch.Generator(device="cpu").manual_seed(1000 * H + 10 * W + B)
    P = ((H - 2) // 2) * ((W - 2) // 2)
    Kf = P * 32
    x = torch.randint(0, 17, (B, H, W, 1), generator=g).float() / 16.0
    w = torch.randint(-32, 33, (3, 3, 1, 32), generator=g).float() / 64
    b = torch.randint(-8, 9, (32,), generator=g).float() / 64
    W1 = torch.randn(Kf, HD, generator=g) * 0.02
    y = F.conv2d(x.double().permute(0, 3, 1, 2), w.double().permute(3, 2, 0, 1), b.double())
    pooled = F.max_pool2d(F.relu(y), 2).permute(0, 2, 3, 1).reshape(B, Kf)
    ref = pooled @ W1.double()
    return dict(B=B, P=P, Kf=Kf, x=x.to(DEV), w=w.to(DEV), b=b.to(DEV), W1=W1.to(DEV), pooled=pooled.to(DEV),
                ref=ref.to(DEV))


def _buffers(c):
    Bp = (c["B"] + 7) // 8 * 8
    Pt = torch.full((c["Kf"], Bp), 5.0, device=DEV)
    amax = torch.zeros(c["P"], 4, Bp, dtype=torch.int64, device=DEV)
    return Pt, amax, Bp


def _check_trunk(c, Pt, amax, Bp):
    B, Kf, pooled = c["B"], c["Kf"], c["pooled"]
    assert torch.equal(Pt[:, :B].double().T, pooled)           # exact conv (quantized operands)
    assert torch.all(Pt[:, B:] == 0)
    amax_b = amax.view(torch.uint8).view(c["P"], 4, Bp, 8).permute(2, 0, 1, 3).reshape(Bp, Kf)[:B]
    assert torch.equal(amax_b != 255, pooled > 0)


@pytest.mark.parametrize("B,H,W", [(1, 8, 12), (16, 8, 12), (17, 8, 12), (37, 8, 12), (17, 28, 28)])
def test_fwd_group_shapes(B, H, W):
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


@pytest.mark.parametrize("hrep", [1, 4])
def test_fwd_group_replicas(hrep):
    from tensorflow_distributed_example_amd.ops import kernels as Kk
    c = _case(17, 8, 12)
    Pt, amax, Bp = _buffers(c)
    hpre = torch.zeros(hrep, c["B"], HD, device=DEV)
    Kk.convnet_fwd(c["x"], c["w"], c["b"], c["W1"], hpre, Pt, amax, hrep=hrep)
    torch.cuda.synchronize()
    _check_trunk(c, Pt, amax, Bp)
    e = _rel(hpre.double().sum(0), c["ref"])
    print(f"hrep={hrep}: hpre rel err {e:.3e}")
    assert e < TOL, e
    if hrep == 4:   # groups 0..3 -> replicas 0..3: every replica received a share
        assert all(bool(hpre[r].abs().sum() > 0) for r in range(4))


@pytest.mark.parametrize("H,W", [(8, 12), (28, 28)])
def test_fwd_group_deterministic_layout(H, W):
    """hrep = P (the deterministic mode's layout): replica g receives exactly one add per address from
    group g, the replicas past the group count stay zero, and two runs from zeroed buffers are bit-identical."""
    from tensorflow_distributed_example_amd.ops import kernels as Kk
    c = _case(17, H, W)
    P, ngroups = c["P"], (c["P"] + 3) // 4
    runs = []
    for _ in range(2):
        hpre = torch.zeros(P, c["B"], HD, device=DEV)
        Kk.convnet_fwd(c["x"], c["w"], c["b"], c["W1"], hpre, None, None, hrep=P)
        torch.cuda.synchronize()
        runs.append(hpre)
    assert torch.equal(runs[0], runs[1])
    assert torch.all(runs[0][ngroups:] == 0)
    e = _rel(runs[0].double().sum(0), c["ref"])
    assert e < TOL, e


def test_fwd_group_predict_path():
    """Pt = None, amax = None (the predict path): hpre alone."""
    from tensorflow_distributed_example_amd.ops import kernels as Kk
    c = _case(37, 8, 12)
    hpre = torch.zeros(c["B"], HD, device=DEV)
    Kk.convnet_fwd(c["x"], c["w"], c["b"], c["W1"], hpre, None, None)
    torch.cuda.synchronize()
    e = _rel(hpre, c["ref"])
    assert e < TOL, e


def test_fwd_group_accumulates():
    """hpre is +=: two calls into the same buffer give twice the reference."""
    from tensorflow_distributed_example_amd.ops import kernels as Kk
    c = _case(17, 8, 12)
    Pt, amax, Bp = _buffers(c)
    hpre = torch.zeros(c["B"], HD, device=DEV)
    for _ in range(2):
        Kk.convnet_fwd(c["x"], c["w"], c["b"], c["W1"], hpre, Pt, amax)
    torch.cuda.synchronize()
    _check_trunk(c, Pt, amax, Bp)
    e = _rel(hpre, 2 * c["ref"])
    assert e < TOL, e
