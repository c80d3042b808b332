"""The float64 oracle of the streaming layer kernels (tests/layers_oracle.py) against torch float64 on the host
(autograd, F.max_pool2d, F.cross_entropy) with its bf16 rounding switched off, its rounding helper against
torch's bfloat16 cast, the pooling tie rule on a hand-written window, the launch-path predicates against the case
table, the measured summation constant, and the 0.5 % ambiguity cap of every GPU case.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import layers_oracle as LO

f64 = torch.float64


def _t(a, grad=False):
    return torch.tensor(np.asarray(a, np.float64), dtype=f64, requires_grad=grad)


def _close(a, b, tol=1e-11):
    a, b = np.asarray(a, np.float64), np.asarray(b.detach().numpy() if torch.is_tensor(b) else b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.abs(a - b).max() <= tol * (1 + np.abs(b).max()), np.abs(a - b).max()


def test_bf16_round_matches_torch_cast():
    rng = np.random.default_rng(0)
    x = np.concatenate([np.atleast_1d(np.asarray(v, np.float64)) for v in (
        rng.standard_normal(20000) * np.exp(rng.uniform(-80, 80, 20000)),
        [0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, 3.3895313892515355e38, 3.4e38, -3.4e38],
        # halfway cases: 1 + (2k+1) * 2^-8 ties to even, and just beside them
        1.0 + (2 * np.arange(8) + 1) * 2.0 ** -8, -(1.0 + (2 * np.arange(8) + 1) * 2.0 ** -8),
        [1.0 + 2.0 ** -8 + 2.0 ** -20, 1.0 + 2.0 ** -8 - 2.0 ** -20],
        # subnormals of bf16 (spacing 2^-133), their halfway points, the smallest normal, below half the smallest
        np.arange(0, 260) * 2.0 ** -134, -np.arange(0, 260) * 2.0 ** -134, [2.0 ** -126, 2.0 ** -135, 2.0 ** -140])])
    x = x.astype(np.float32).astype(np.float64)      # torch casts from fp32; every value above is an fp32 value
    got = LO.bf16_round(x)
    want = torch.tensor(x, dtype=torch.float32).to(torch.bfloat16).double().numpy()
    assert np.array_equal(got, want)
    assert np.array_equal(np.signbit(got), np.signbit(want))      # -0 stays -0
    with LO.no_rounding():
        assert np.array_equal(LO.bf16_round(x), x)
    # a float64 value is rounded once, not through fp32: 1 + 2^-8 + 2^-40 is above the tie, fp32 would put it on it
    assert LO.bf16_round(np.array([1 + 2.0 ** -8 + 2.0 ** -40]))[0] == 1 + 2.0 ** -7
    ref, bound = LO.cast_bf16(x[np.isfinite(x)].astype(np.float32))
    assert np.array_equal(ref, want[np.isfinite(x)]) and not bound.any()


@pytest.mark.parametrize("mode,relu,res,accum", [(1, True, True, True), (1, False, False, False), (1, True, False, False),
                                                 (0, True, True, False), (2, True, True, False)])
def test_bn_oracle_matches_float64_autograd(mode, relu, res, accum):
    rng = np.random.default_rng(3)
    R, C, eps, mom = 37, 10, 1e-3, 0.9
    y, r, dout = rng.standard_normal((R, C)) * 2 + 0.5, rng.standard_normal((R, C)), rng.standard_normal((R, C))
    gamma, beta = rng.random(C) + 0.5, rng.standard_normal(C) * 0.1
    mm, mv = rng.standard_normal(C) * 0.2, rng.random(C) + 0.5
    keep = rng.random((R, C)) < 0.7
    prev = [rng.standard_normal((R, C)) if accum else None for _ in range(2)]
    gprev = [rng.standard_normal(C) for _ in range(2)]
    bessel = R / (R - 1)
    with LO.no_rounding():
        st = LO.stats_slots(LO.colstats(y)[0], C)
        st[3], st[0] = st[0] * 0.25, st[0] * 0.75           # spread over two slots
        f = LO.bn_fwd(y, mode=mode, stats=st, gamma=gamma, beta=beta, eps=eps, mmean=mm, mvar=mv, momentum=mom,
                      bessel=bessel, res=r if res else None, relu=relu, keep=keep, drop_rate=0.3)
        b = None
        if mode != 2:
            b = LO.bn_bwd(dout, y, mode=mode, mean=f["saved_mean"][0] if mode == 1 else None,
                          rstd=f["saved_rstd"][0] if mode == 1 else None, gamma=gamma, beta=beta,
                          res=r if res else None, relu=relu, keep=keep, drop_rate=0.3, dx_prev=prev[0],
                          dres_prev=prev[1] if res else None, dgamma_prev=gprev[0], dbeta_prev=gprev[1], want_dres=res)
    yt, rt, gt, bt = _t(y, True), _t(r, True), _t(gamma, True), _t(beta, True)
    if mode == 1:
        mean, var = yt.mean(0), yt.var(0, unbiased=False)
    elif mode == 2:
        mean, var = _t(mm), _t(mv)
    z = (yt - mean) * torch.rsqrt(var + float(np.float32(eps))) * gt + bt if mode else yt * 1.0
    if res:
        z = z + rt
    if relu:
        z = F.relu(z)
    z = z * _t(keep) / 0.7
    _close(f["out"][0], z)
    if mode == 1:
        _close(f["saved_mean"][0], mean)
        _close(f["saved_rstd"][0], torch.rsqrt(var + float(np.float32(eps))))
        m32 = float(np.float32(mom))
        _close(f["mmean"][0], _t(mm) * m32 + mean * (1 - m32), 1e-7)     # 1 - momentum is taken in fp32
        _close(f["mvar"][0], _t(mv) * m32 + var * bessel * (1 - m32), 1e-6)
    if b is None:
        return
    z.backward(_t(dout))
    _close(b["dx"][0], yt.grad + (0 if prev[0] is None else _t(prev[0])))
    if res:
        _close(b["dres"][0], rt.grad + (0 if prev[1] is None else _t(prev[1])))
    if mode == 1:
        _close(b["dgamma"][0], gt.grad + _t(gprev[0]))
        _close(b["dbeta"][0], bt.grad + _t(gprev[1]))
    assert all((v[1] >= 0).all() for k, v in b.items() if isinstance(v, tuple))


def test_bn_degenerate_variance_is_clamped():
    y = np.full((7, 3), 1.5)
    y[:, 2] = [1, 2, 3, 4, 5, 6, 7]
    f = LO.bn_fwd(y, mode=1, stats=LO.stats_slots(LO.colstats(y)[0], 3), eps=1e-3)
    assert f["saved_rstd"][0][0] == 1 / np.sqrt(float(np.float32(1e-3))) and (f["out"][0][:, :2] == 0).all()
    st = LO.stats_slots(LO.colstats(y)[0], 3)
    st[0, 1, 0] -= 1e-9                                        # E[y^2] a hair below mean^2: max(.., 0)
    assert LO.bn_fwd(y, mode=1, stats=st, eps=1e-3)["saved_rstd"][0][0] == f["saved_rstd"][0][0]


def test_act_bwd_colstats_gap_pad_oracles_match_float64_autograd():
    rng = np.random.default_rng(4)
    R, C = 23, 7
    pre, dout, bprev = rng.standard_normal((R, C)), rng.standard_normal((R, C)), rng.standard_normal(C)
    bias = _t(np.zeros(C), True)
    xt = _t(pre, True)
    out = F.relu(xt + bias)
    out.backward(_t(dout))
    a = LO.act_bwd(dout, out.detach().numpy(), True, bprev)
    _close(a["dz"][0], xt.grad)
    _close(a["dbias"][0], bias.grad + _t(bprev))
    a = LO.act_bwd(dout, None, False)
    _close(a["dz"][0], dout)
    _close(a["dbias"][0], dout.sum(0))
    x = rng.standard_normal((R, C + 5))
    s, _ = LO.colstats(x, C)
    _close(s, torch.stack([_t(x)[:, :C].sum(0), (_t(x)[:, :C] ** 2).sum(0)]))
    B, HW = 3, 11
    with LO.no_rounding():
        g, dy, prev = rng.standard_normal((B, HW, C)), rng.standard_normal((B, C)), rng.standard_normal((B, HW, C))
        gt = _t(g, True)
        m = gt.mean(1)
        m.backward(_t(dy))
        _close(LO.gap_fwd(g)[0], m)
        _close(LO.gap_bwd(dy, HW)[0], gt.grad)
        _close(LO.gap_bwd(dy, HW, prev)[0], gt.grad + _t(prev))
        p = rng.standard_normal((2, 5, 4, 3))
        pt_, pb, pl, pr = 1, 2, 0, 3
        ptn = _t(p, True)
        padded = F.pad(ptn, (0, 0, pl, pr, pt_, pb))
        dyp = rng.standard_normal(tuple(padded.shape))
        padded.backward(_t(dyp))
        _close(LO.pad_fwd(p, pt_, pb, pl, pr)[0], padded)
        _close(LO.pad_bwd(dyp, pt_, pl, 5, 4)[0], ptn.grad)
        _close(LO.pad_bwd(dyp, pt_, pl, 5, 4, p)[0], ptn.grad + _t(p))


def _torch_pool(xt, g):
    H2, W2 = (g.Ho - 1) * g.sh + g.KH, (g.Wo - 1) * g.sw + g.KW
    pb, pr = max(H2 - g.H - g.pt, 0), max(W2 - g.W - g.pl, 0)
    xp = F.pad(xt.permute(0, 3, 1, 2), (g.pl, pr, g.pt, pb), value=float("-inf"))
    return F.max_pool2d(xp, (g.KH, g.KW), (g.sh, g.sw)).permute(0, 2, 3, 1)


@pytest.mark.parametrize("case", [c for c in LO.POOL_CASES if c.geo.B * c.geo.H < 1000], ids=lambda c: c.id)
def test_maxpool_oracle_matches_torch(case):
    g = case.geo
    rng = np.random.default_rng(5)
    x = rng.standard_normal((g.B, g.H, g.W, g.C))           # no ties: autograd's choice is the only one
    dy = rng.standard_normal((g.B, g.Ho, g.Wo, g.C))
    prev = rng.standard_normal(x.shape)
    xt = _t(x, True)
    ref = _torch_pool(xt, g)
    ref.backward(_t(dy))
    with LO.no_rounding():
        f = LO.maxpool_fwd(x, g)
        _close(f["y"][0], ref, 0)
        _close(LO.maxpool_bwd(dy, f["idx"][0], g)[0], xt.grad)
        _close(LO.maxpool_bwd(dy, f["idx"][0], g, prev)[0], xt.grad + _t(prev))
    # values on the tie grid: the value still matches; the byte names an in-bounds tap holding that value
    xg, _, _ = LO.pool_inputs(g, 0)
    f = LO.maxpool_fwd(xg, g)
    _close(f["y"][0], _torch_pool(_t(xg), g), 0)
    idx = f["idx"][0].astype(int)
    oh, ow = np.meshgrid(np.arange(g.Ho), np.arange(g.Wo), indexing="ij")
    ih = oh[None, :, :, None] * g.sh - g.pt + idx // g.KW
    iw = ow[None, :, :, None] * g.sw - g.pl + idx % g.KW
    assert (ih >= 0).all() and (ih < g.H).all() and (iw >= 0).all() and (iw < g.W).all()
    b, c = np.arange(g.B)[:, None, None, None], np.arange(g.C)[None, None, None, :]
    assert np.array_equal(xg[b, ih, iw, c], f["y"][0])
    # exact sums of grid values: bound 0 everywhere
    _, dyg, pg = LO.pool_inputs(g, 0)
    assert not LO.maxpool_bwd(dyg, f["idx"][0], g, pg)[1].any()


def test_pool_tie_rule_first_maximum_in_row_major_order():
    w = np.array([[1.0, 2.0, 2.0],
                  [2.0, 0.5, 2.0],
                  [-1.0, 2.0, 1.0]]).reshape(1, 3, 3, 1)
    g = LO.pool_geo(1, 3, 3, 1, 3, 1, "valid")
    f = LO.maxpool_fwd(w, g)
    assert f["y"][0].item() == 2.0 and f["idx"][0].item() == 1           # (0, 1), not (0, 2), (1, 0), (1, 2), (2, 1)
    g = LO.pool_geo(1, 3, 3, 1, 3, 1, "same")                            # every window clipped by the border
    f = LO.maxpool_fwd(w, g)
    # output (0, 0): taps (1..2, 1..2) -> pixels (0..1, 0..1) = [[1, 2], [2, .5]]: first max at pixel (0, 1) = byte 1*3+2
    assert f["idx"][0][0, 0, 0, 0] == 5 and f["y"][0][0, 0, 0, 0] == 2.0
    # output (2, 2): pixels (1..2, 1..2) = [[.5, 2], [2, 1]]: first max at pixel (1, 2) = tap (0, 1)
    assert f["idx"][0][0, 2, 2, 0] == 1
    # all equal: the first IN-BOUNDS tap wins, not byte 0
    f = LO.maxpool_fwd(np.zeros((1, 3, 3, 1)), g)
    assert f["idx"][0][0, :, :, 0].tolist() == [[4, 3, 3], [1, 0, 0], [1, 0, 0]]
    dx, bound = LO.maxpool_bwd(np.ones((1, 3, 3, 1)), f["idx"][0], g)
    assert dx[0, :, :, 0].tolist() == [[4, 2, 0], [2, 1, 0], [0, 0, 0]] and not bound.any()


def test_fused_bn_relu_maxpool_oracle_matches_float64_autograd():
    rng = np.random.default_rng(6)
    g = LO.pool_geo(2, 7, 6, 8, 3, 2, "same")
    R = g.B * g.H * g.W
    y, gamma, beta = rng.standard_normal((R, g.C)) * 2 + 0.2, rng.random(g.C) + 0.5, rng.standard_normal(g.C) * 0.3
    dpool, prev = rng.standard_normal((g.B, g.Ho, g.Wo, g.C)), rng.standard_normal((R, g.C))
    yt, gt, bt = _t(y, True), _t(gamma, True), _t(beta, True)
    mean, var = yt.mean(0), yt.var(0, unbiased=False)
    z = F.relu((yt - mean) * torch.rsqrt(var + float(np.float32(1e-5))) * gt + bt)
    ref = _torch_pool(z.view(g.B, g.H, g.W, g.C), g)
    ref.backward(_t(dpool))
    with LO.no_rounding():
        f = LO.bn_relu_maxpool_fwd(y, g, mode=1, stats=LO.stats_slots(LO.colstats(y)[0], g.C), gamma=gamma,
                                   beta=beta, eps=1e-5)
        _close(f["y"][0], ref)
        b = LO.bn_pool_bwd(dpool, f["idx"][0], y, g, mean=f["saved_mean"][0], rstd=f["saved_rstd"][0], gamma=gamma,
                           beta=beta, dx_prev=prev)
    _close(b["dx"][0], yt.grad + _t(prev))
    _close(b["dgamma"][0], gt.grad)
    _close(b["dbeta"][0], bt.grad)


@pytest.mark.parametrize("B,C", [(5, 10), (37, 1025), (1, 1)])
def test_xent_oracle_matches_torch(B, C):
    x, lab = LO.xent_inputs(B, C)
    xt = _t(x, True)
    loss = F.cross_entropy(xt, torch.tensor(lab, dtype=torch.long), reduction="sum")
    (loss * 0.5).backward()
    o = LO.xent(x, lab, 0.5, metrics_prev=[1.0, 2.0, 3.0])
    _close(o["loss"][0], loss + 1.0)
    _close(o["probs"][0], torch.softmax(xt, 1))
    _close(o["dlogits"][0], xt.grad)
    assert o["count"][0] == B + 3
    first = np.array([int(np.flatnonzero(r == r.max())[0]) for r in x])
    assert o["correct"][0] == (first == lab).sum() + 2
    if B == 37:   # the duplicated maxima: row 2's label is the first occurrence (correct), row 3's the second (not)
        assert first[2] == lab[2] and first[3] != lab[3] and x[3, lab[3]] == x[3].max()


def test_case_table_paths_restate_the_launchers():
    for c in LO.BN_CASES:
        assert LO.bn_fwd_path(c.R, c.C) == c.fwd, c.id
        assert LO.bn_reduce_path(c.R, c.C, c.mode, c.drop, c.det) == c.reduce, c.id
    loop = next(c for c in LO.BN_CASES if c.id.startswith("tiled_loop"))
    assert LO.bn_tiled_loops(loop.R, loop.C, 16384, 512, 4096) and LO.bn_tiled_loops(loop.R, loop.C, 32768, 256, 1024)
    assert not LO.bn_tiled_loops(130, 128, 16384, 512, 4096)
    assert {c.reduce for c in LO.BN_CASES} >= {"cols", "rows8", "rows16", "generic", "tiled", "det"}
    assert {c.fwd for c in LO.BN_CASES} == {"flat_scalar", "flat_vec", "tiled"}
    assert any(256 % (c.C // 8) for c in LO.BN_CASES if c.fwd == "tiled")       # 24, 40, 56
    for c in LO.POOL_CASES:
        assert LO.pool_bwd_path(c.geo) == c.bwd, c.id
    assert {c.bwd for c in LO.POOL_CASES} == {"bwd", "bwd8", "w2", "w2p"}
    fb = next(c for c in LO.POOL_CASES if "fallback" in c.id).geo
    assert fb.B * fb.H == 65536
    combos = {(c.geo.W % 2, c.geo.pl) for c in LO.POOL_CASES if c.bwd == "w2p" and c.geo.W > 2}
    assert combos == {(0, 0), (0, 1), (1, 0), (1, 1)}, combos      # even / odd W with pl = 0 / 1, all four
    assert [LO.xent_path(C) for C in LO.XENT_C] == ["xent<16>"] * 4 + ["xent<0>"] * 2
    for c in LO.FUSED_CASES:
        assert LO.fused_ok(c.geo), c.id
    assert {c.geo.C for c in LO.FUSED_CASES} >= {8, 16, 64, 512}
    assert any(c.geo.B * c.geo.H > 1024 for c in LO.FUSED_CASES)


def test_sum_constant_is_the_measured_one():
    m = LO.measure_sum_constant()
    print("measured SUM_C ratio", m)
    assert 4 * m <= LO.SUM_C <= 4.2 * m, m


@pytest.mark.parametrize("case", LO.BN_CASES, ids=lambda c: c.id)
def test_bn_cases_stay_under_the_ambiguity_cap(case):
    f, b = LO.bn_oracle(case, LO.bn_inputs(case))
    assert f["out"][2].mean() <= LO.AMBIGUOUS_CAP
    if case.zeros:
        z = f["z"]
        assert 0.05 < (z == 0).mean() < 0.2 and not b["dx"][2].any() and (b["dx"][0][z == 0] == 0).all()
    if b is not None:
        assert b["dx"][2].mean() <= LO.AMBIGUOUS_CAP
        assert all(np.isfinite(v[0]).all() and np.isfinite(v[1]).all() for v in b.values() if isinstance(v, tuple))


@pytest.mark.parametrize("case", LO.FUSED_CASES, ids=lambda c: c.id)
def test_fused_cases_stay_under_the_ambiguity_cap(case):
    inp = LO.fused_inputs(case)
    f = LO.fused_fwd_oracle(case, inp)
    amb = f["idx"][2]
    assert amb.mean() <= LO.AMBIGUOUS_CAP
    ties = (f["y"][0] == 0).mean()
    if "zero-ties" in case.id:
        assert 0.3 < ties < 0.8, ties                        # about half the windows are all-zero ties
    if case.mode == 1:
        saved = (LO.f32_round(f["saved_mean"][0]), LO.f32_round(f["saved_rstd"][0]))
        b = LO.fused_bwd_oracle(case, inp, f["idx"][0], saved, amb)
        assert b["dx"][2].mean() <= LO.AMBIGUOUS_CAP and b["gather_exact"]
