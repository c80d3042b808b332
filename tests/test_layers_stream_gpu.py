"""The streaming kernels of csrc/kernels/layers.hip (BatchNorm forward / backward, max pooling, the fused
BN + ReLU + MaxPool pair, act_bwd, GAP, pad, column statistics, cast, softmax cross-entropy) against the float64
host oracle of tests/layers_oracle.py, element by element within its derived bounds; every case is named by the
kernel / launch branch it must reach (the branch rules are restated in layers_oracle and checked against the case
table in tests/test_layers_oracle.py)."""
import numpy as np
import pytest
import torch

import layers_oracle as LO

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("bf16_policy")]
DEV = "cuda"
bf = torch.bfloat16
SLOTS = LO.STAT_SLOTS


def T(a, dtype=bf):
    """host float64 array (of values the dtype holds exactly) -> device tensor"""
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def N(t):
    return t.detach().double().cpu().numpy()


def nan_bf(*shape):
    return torch.full(shape, float("nan"), device=DEV).to(bf)


def assert_close(out, ref, bound, ambiguous=None, name="", path=""):
    """|out - ref| <= bound for every element outside ``ambiguous`` (at most LO.AMBIGUOUS_CAP of the tensor); a NaN
    fails.  Reports the worst element's index, the shape and the dispatch path."""
    ref = np.asarray(ref, np.float64)
    o = (N(out) if torch.is_tensor(out) else np.asarray(out, np.float64)).reshape(ref.shape)
    bound = np.broadcast_to(np.asarray(bound, np.float64), ref.shape)
    skip = np.zeros(ref.shape, bool) if ambiguous is None else np.broadcast_to(ambiguous, ref.shape)
    assert skip.mean() <= LO.AMBIGUOUS_CAP, (name, path, skip.mean())
    with np.errstate(invalid="ignore"):
        err = np.abs(o - ref)
        bad = ~(err <= bound) & ~skip
    if bad.any():
        excess = np.where(bad, np.where(np.isfinite(err), err - bound, np.inf), -1.0)
        i = np.unravel_index(int(np.argmax(excess)), ref.shape) if ref.ndim else ()
        raise AssertionError(f"{name} [{path}] shape {ref.shape}: {int(bad.sum())} of {bad.size} elements out of bound; "
                             f"worst at {i}: got {o[i]!r}, want {ref[i]!r} +- {bound[i]!r} (error {err[i]!r})")


def check(out, entry, name, path):
    assert_close(out, entry[0], entry[1], entry[2] if len(entry) > 2 else None, name=name, path=path)


class deterministic:
    def __init__(self, on):
        from tensorflow_distributed_example_amd import _native
        self.lib, self.on = _native.hip(), int(bool(on))

    def __enter__(self):
        self.before = self.lib.tde_layers_is_deterministic()
        self.lib.tde_layers_deterministic(self.on)

    def __exit__(self, *exc):
        self.lib.tde_layers_deterministic(self.before)


def _stats(C, fill=0.0):
    return torch.full((2 * SLOTS * C,), fill, dtype=torch.float64, device=DEV)


def _kernel_stats(y, R, C, det, path):
    """tde_colstats of y, checked against the oracle; returns the kernel's slots (the BN oracle's input)."""
    from tensorflow_distributed_example_amd.ops import layer_ops as O
    st = _stats(C)
    O.colstats(y, R, C, st)
    torch.cuda.synchronize()
    slots = N(st).reshape(SLOTS, 2, C)
    ref, bound = LO.colstats(N(y).reshape(R, C), det=det)
    assert_close(slots.sum(0), ref, bound, name="colstats", path=path)
    return st, slots


def _drop_mask(O, d, R, C):
    """the keep mask the kernels draw for (seed, step, layer): dropout over ones normalised by (0, 1)"""
    ones = torch.ones(R, C, dtype=bf, device=DEV)
    o = torch.zeros(R, C, dtype=bf, device=DEV)
    O.bn_fwd(ones, o, R, C, mode=2, eps=0.0, mmean=torch.zeros(C, device=DEV), mvar=torch.ones(C, device=DEV),
             relu=True, drop=d, iter_offset=0)
    torch.cuda.synchronize()
    keep = N(o) > 0
    assert 0.4 < keep.mean() < 0.95
    return keep


@pytest.mark.parametrize("case", LO.BN_CASES, ids=lambda c: c.id)
def test_bn_fwd_bwd(case):
    from tensorflow_distributed_example_amd.ops import layer_ops as O
    c, R, C = case, case.R, case.C
    assert LO.bn_fwd_path(R, C) == c.fwd and LO.bn_reduce_path(R, C, c.mode, c.drop, c.det) == c.reduce
    path = f"fwd {c.fwd}, reduce {c.reduce}"
    inp = LO.bn_inputs(c)
    f32 = torch.float32
    with deterministic(c.det):
        y = T(inp["y"])
        res = T(inp["res"]) if c.res else None
        gamma, beta = T(inp["gamma"], f32), T(inp["beta"], f32)
        stats, slots = _kernel_stats(y, R, C, c.det, path)
        saved = torch.full((2 * C,), float("nan"), device=DEV)
        mm, mv = T(inp["mmean"], f32), T(inp["mvar"], f32)
        zb = torch.full((2 * SLOTS * C,), 7.0, device=DEV)
        out = nan_bf(R, C)
        d, keep = O.DropSpec(), None
        if c.drop:
            d = O.DropSpec(c.drop, 1234, torch.zeros(1, dtype=torch.int64, device=DEV), 3)
            keep = _drop_mask(O, d, R, C)
        O.bn_fwd(y, out, R, C, mode=c.mode, stats=stats if c.mode == 1 else None, saved=saved if c.mode == 1 else None,
                 gamma=gamma, beta=beta, eps=1e-3, mmean=mm, mvar=mv, momentum=0.9, bessel=inp["bessel"],
                 zero_buf=zb if c.mode == 1 else None, res=res, relu=c.relu, drop=d, iter_offset=0)
        torch.cuda.synchronize()
        sv = N(saved).reshape(2, C)
        f, b = LO.bn_oracle(c, inp, stats=slots, saved=(sv[0], sv[1]), keep=keep)
        check(out, f["out"], "out", path)
        if c.mode == 1:
            check(sv[0], f["saved_mean"], "saved mean", path)
            check(sv[1], f["saved_rstd"], "saved rstd", path)
            check(mm, f["mmean"], "moving mean", path)
            check(mv, f["mvar"], "moving variance", path)
            assert zb.abs().max().item() == 0.0
        else:
            assert torch.equal(mm, T(inp["mmean"], f32)) and torch.equal(mv, T(inp["mvar"], f32))
        if c.mode == 2:
            return
        dx = T(inp["dx_prev"]) if c.accum else nan_bf(R, C)
        dres = None
        if c.res:
            dres = T(inp["dres_prev"]) if c.accum else nan_bf(R, C)
        dg, db = T(inp["dgamma_prev"], f32), T(inp["dbeta_prev"], f32)
        O.bn_bwd(T(inp["dout"]), y, R, C, mode=c.mode, saved=saved if c.mode == 1 else None, gamma=gamma, beta=beta,
                 res=res, relu=c.relu, drop=d, iter_offset=0, dstats=zb if c.mode == 1 else None, dx=dx,
                 dx_accum=c.accum, dres=dres, dres_accum=c.accum, dgamma=dg if c.mode == 1 else None,
                 dbeta=db if c.mode == 1 else None, zero_fwd=stats if c.mode == 1 else None)
        torch.cuda.synchronize()
        check(dx, b["dx"], "dx", path)
        if c.res:
            check(dres, b["dres"], "dres", path)
        if c.mode == 1:
            check(dg, b["dgamma"], "dgamma", path)
            check(db, b["dbeta"], "dbeta", path)
            assert stats.abs().max().item() == 0.0     # the forward statistics re-armed


def _geom(O, g):
    return O.ConvGeom(g.B, g.H, g.W, g.C, g.Ho, g.Wo, g.C, g.KH, g.KW, g.sh, g.sw, g.pt, g.pl)


@pytest.mark.parametrize("case", LO.POOL_CASES, ids=lambda c: c.id)
def test_maxpool_fwd_bwd_bit_exact(case):
    from tensorflow_distributed_example_amd.ops import layer_ops as O
    g = case.geo
    assert LO.pool_bwd_path(g) == case.bwd
    path = f"{LO.pool_fwd_path(g)}, backward {case.bwd}"
    x, dy, prev = LO.pool_inputs(g, LO.POOL_CASES.index(case))
    og = _geom(O, g)
    n = g.B * g.Ho * g.Wo * g.C
    y = nan_bf(g.B, g.Ho, g.Wo, g.C)
    idx = torch.full((n,), 77, dtype=torch.uint8, device=DEV)
    O.maxpool_fwd(T(x), y, idx, og)
    dx = nan_bf(g.B, g.H, g.W, g.C)
    dxa = T(prev)
    O.maxpool_bwd(T(dy), idx, dx, og)
    O.maxpool_bwd(T(dy), idx, dxa, og, accum=True)
    torch.cuda.synchronize()
    f = LO.maxpool_fwd(x, g)
    check(y, f["y"], "y", path)
    check(idx, f["idx"], "argmax byte", path)
    ref, bound = LO.maxpool_bwd(dy, f["idx"][0], g)
    assert not bound.any()
    assert_close(dx, ref, bound, name="dx", path=path)
    ref, bound = LO.maxpool_bwd(dy, f["idx"][0], g, prev)
    assert not bound.any()
    assert_close(dxa, ref, bound, name="dx accumulate", path=path)


@pytest.mark.parametrize("case", LO.FUSED_CASES, ids=lambda c: c.id)
def test_bn_relu_maxpool_fused_fwd_bwd(case):
    from tensorflow_distributed_example_amd.ops import layer_ops as O
    c, g = case, case.geo
    assert LO.fused_ok(g) and O.bn_pool_ok(_geom(O, g))
    R, C = g.B * g.H * g.W, g.C
    path = f"fused C={C} rows={g.B * g.H} mode={c.mode}"
    f32 = torch.float32
    inp = LO.fused_inputs(c)
    y, gamma, beta = T(inp["y"]), T(inp["gamma"], f32), T(inp["beta"], f32)
    stats, slots = _kernel_stats(y, R, C, False, path)
    saved = torch.full((2 * C,), float("nan"), device=DEV)
    mm, mv = T(inp["mmean"], f32), T(inp["mvar"], f32)
    zb = torch.full((2 * SLOTS * C,), 3.0, device=DEV)
    n = g.B * g.Ho * g.Wo * C
    pooled = nan_bf(n)
    idx = torch.full((n,), 77, dtype=torch.uint8, device=DEV)
    og = _geom(O, g)
    O.bn_relu_maxpool_fwd(y, R, C, pooled, idx, og, mode=c.mode, stats=stats if c.mode == 1 else None,
                          saved=saved if c.mode == 1 else None, gamma=gamma, beta=beta, eps=1e-5, mmean=mm, mvar=mv,
                          momentum=0.9, bessel=inp["bessel"], zero_buf=zb if c.mode == 1 else None)
    torch.cuda.synchronize()
    f = LO.fused_fwd_oracle(c, inp, stats=slots)
    check(pooled, f["y"], "pooled", path)
    check(idx, f["idx"], "argmax byte", path)
    if c.mode != 1:
        return
    sv = N(saved).reshape(2, C)
    check(sv[0], f["saved_mean"], "saved mean", path)
    check(sv[1], f["saved_rstd"], "saved rstd", path)
    check(mm, f["mmean"], "moving mean", path)
    check(mv, f["mvar"], "moving variance", path)
    assert zb.abs().max().item() == 0.0
    dx = T(inp["dx_prev"]) if c.accum else nan_bf(R, C)
    dg, db = T(inp["dgamma_prev"], f32), T(inp["dbeta_prev"], f32)
    O.bn_pool_bwd(T(inp["dpool"]), idx, y, R, C, og, saved=saved, dstats=zb, dx=dx, gamma=gamma, beta=beta, relu=True,
                  dx_accum=c.accum, dgamma=dg, dbeta=db, zero_fwd=stats)
    torch.cuda.synchronize()
    idx_k = N(idx).astype(np.uint8).reshape(g.B, g.Ho, g.Wo, C)
    b = LO.fused_bwd_oracle(c, inp, idx_k, (sv[0], sv[1]), f["idx"][2])
    assert b["gather_exact"]
    check(dx, b["dx"], "dx", path)
    check(dg, b["dgamma"], "dgamma", path)
    check(db, b["dbeta"], "dbeta", path)
    assert stats.abs().max().item() == 0.0


@pytest.mark.parametrize("det", [False, True], ids=["atomic", "deterministic"])
@pytest.mark.parametrize("R,C", LO.ACT_CASES)
def test_act_bwd(R, C, det):
    from tensorflow_distributed_example_amd.ops import layer_ops as O
    path = "colsum_det" if det else "act_bwd"
    dout, outv, bprev = LO.act_inputs(R, C)
    assert (outv == 0).mean() > 0.3
    ref = LO.act_bwd(dout, outv, True, bprev, det=det)
    ref0 = LO.act_bwd(dout, outv, False, bprev, det=det)
    with deterministic(det):
        for want_dz, want_db in ((True, False), (False, True), (True, True)):
            for relu, r in ((True, ref), (False, ref0)):
                dz = nan_bf(R, C) if want_dz else None
                dbias = T(bprev, torch.float32) if want_db else None
                O.act_bwd(T(dout), T(outv), R, C, relu=relu, dz=dz, dbias=dbias)
                torch.cuda.synchronize()
                if want_dz:
                    check(dz, r["dz"], f"dz relu={relu}", path)
                if want_db:
                    check(dbias, r["dbias"], f"dbias relu={relu} dz={want_dz}", path)


@pytest.mark.parametrize("det", [False, True], ids=["atomic", "deterministic"])
@pytest.mark.parametrize("R,C", LO.COLSTATS_CASES)
def test_colstats(R, C, det):
    x = LO.normal_bf16(np.random.default_rng(7000 + R), (R, C), 2.0, 0.5)
    with deterministic(det):
        _kernel_stats(T(x), R, C, det, "colstats_det" if det else "colstats")


def test_colstats_det_row_stride():
    """colstats_det_kernel with a row stride larger than C: the statistics pass of a deterministic-mode GEMM whose bf16
    output rows are 32 apart for 24 columns; the gap columns (never written: 7.0) must not be counted.  tde_colstats
    takes no stride, and outside deterministic mode a GEMM takes its statistics in its own epilogue, so the atomic
    colstats_kernel has no strided form to cover."""
    from tensorflow_distributed_example_amd.ops import layer_ops as O
    B, fin, out, ld = 37, 16, 24, 32
    rng = np.random.default_rng(8)
    x, w = T(LO.normal_bf16(rng, (B, fin))), T(LO.normal_bf16(rng, (out, fin), 0.3))
    yb = torch.full((B * ld,), 7.0, dtype=bf, device=DEV)
    st = _stats(out)
    with deterministic(True):
        O._igemm(x, fin, O.A_ROWK, w, fin, O.B_NK, B, out, fin, cb=yb, ldcb=ld, colstats=st)
        torch.cuda.synchronize()
    stored = N(yb).reshape(B, ld)
    assert (stored[:, out:] == 7.0).all() and (stored[:, :out] != 7.0).any()
    ref, bound = LO.colstats(stored, C=out, det=True)
    assert_close(N(st).reshape(SLOTS, 2, out).sum(0), ref, bound, name="strided colstats", path="colstats_det ld=32")


@pytest.mark.parametrize("name,B,HW,C", LO.GAP_CASES, ids=[c[0] for c in LO.GAP_CASES])
def test_gap(name, B, HW, C):
    from tensorflow_distributed_example_amd.ops import layer_ops as O
    assert (C % 64 == 0) == name.endswith("vec")
    x, dy, prev = LO.gap_inputs(B, HW, C)
    y = nan_bf(B, C)
    O.gap_fwd(T(x), y, B, HW, C)
    dx, dxa = nan_bf(B, HW, C), T(prev)
    O.gap_bwd(T(dy), dx, B, HW, C)
    O.gap_bwd(T(dy), dxa, B, HW, C, accum=True)
    torch.cuda.synchronize()
    check(y, LO.gap_fwd(x), "gap", name)
    check(dx, LO.gap_bwd(dy, HW), "gap dx", name)
    check(dxa, LO.gap_bwd(dy, HW, prev), "gap dx accumulate", name)


@pytest.mark.parametrize("pads", [(1, 2, 0, 3), (0, 1, 2, 0), (2, 0, 1, 1)], ids=str)
def test_pad(pads):
    from tensorflow_distributed_example_amd.ops import layer_ops as O
    pt, pb, pl, pr = pads
    B, H, W, C = 3, 7, 5, 12
    rng = np.random.default_rng(9)
    x = LO.grid(rng, (B, H, W, C), 0.125, 2.0)
    dy = LO.grid(rng, (B, H + pt + pb, W + pl + pr, C), 0.125, 2.0)
    g = O.ConvGeom(B, H, W, C, H + pt + pb, W + pl + pr, C, 1, 1, 1, 1, pt, pl)
    yp = nan_bf(B, H + pt + pb, W + pl + pr, C)
    O.pad_fwd(T(x), yp, g)
    dx, dxa = nan_bf(B, H, W, C), T(x)
    O.pad_bwd(T(dy), dx, g)
    O.pad_bwd(T(dy), dxa, g, accum=True)
    torch.cuda.synchronize()
    check(yp, LO.pad_fwd(x, pt, pb, pl, pr), "pad", str(pads))
    check(dx, LO.pad_bwd(dy, pt, pl, H, W), "pad dx", str(pads))
    ref, bound = LO.pad_bwd(dy, pt, pl, H, W, x)
    assert not bound.any()
    assert_close(dxa, ref, bound, name="pad dx accumulate", path=str(pads))


@pytest.mark.parametrize("n", [4096, 1025, 7, 3])     # n % 4 in {0, 1, 3}
def test_cast(n):
    from tensorflow_distributed_example_amd.ops import layer_ops as O
    rng = np.random.default_rng(n)
    x = (rng.standard_normal(n) * np.exp(rng.uniform(-30, 30, n))).astype(np.float32)
    x[:3] = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -0.0], np.float32)[:min(3, n)]     # ties to even, -0
    y = nan_bf(n + 5)
    O.cast_bf16(torch.from_numpy(x).to(DEV), y[:n])
    torch.cuda.synchronize()
    ref, bound = LO.cast_bf16(x)
    assert_close(y[:n], ref, bound, name="cast", path=f"n % 4 = {n % 4}")
    assert torch.isnan(y[n:].float()).all()               # nothing past the end


@pytest.mark.parametrize("B", LO.XENT_B)
@pytest.mark.parametrize("C", LO.XENT_C)
def test_xent(C, B):
    from tensorflow_distributed_example_amd.ops import layer_ops as O
    path = LO.xent_path(C)
    assert path == ("xent<16>" if C <= 64 * 16 else "xent<0>")
    x, lab = LO.xent_inputs(B, C)
    logits, labels = torch.from_numpy(x.astype(np.float32)).to(DEV), torch.from_numpy(lab).to(DEV)
    m0 = [1.0, 2.0, 3.0]
    ref = LO.xent(x, lab, 0.5, metrics_prev=m0)
    dl = nan_bf(B, C)
    met = torch.tensor(m0 + [0.0], device=DEV)
    it = torch.full((1,), 41, dtype=torch.int64, device=DEV)
    O.xent(logits, labels, B, C, scale=0.5, dlogits=dl, metrics=met, iterations=it)
    torch.cuda.synchronize()
    assert it.item() == 42                                 # advanced by exactly one, whatever the grid
    check(dl, ref["dlogits"], "dlogits", path)
    check(met[0], ref["loss"], "loss sum", path)
    check(met[1], ref["correct"], "correct", path)
    check(met[2], ref["count"], "count", path)
    assert met[3].item() == 0.0
    probs = torch.full((B, C), float("nan"), device=DEV)
    O.xent(logits, labels, B, C, probs=probs)
    cp = torch.full((B, C), float("nan"), device=DEV)
    O.xent(logits, labels, B, C, probs=cp, probs_are_logits=True, iterations=it)
    torch.cuda.synchronize()
    check(probs, ref["probs"], "probs", path)
    assert torch.equal(cp, logits) and it.item() == 43
