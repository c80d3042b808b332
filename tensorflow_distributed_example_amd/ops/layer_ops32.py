"""Host wrappers for the float32 layer-wise kernel library (csrc/kernels/layers_f32.hip).

The float32 twin of ``layer_ops``: activations, activation gradients and logits are f32, the GEMMs read
the f32 master kernels in their Keras layouts (HWIO conv kernels, [in, out] dense kernels) on the
exact-f32 MFMA, BN statistics / backward sums are f64.  Every wrapper validates operand sizes on the host
against the geometry it hands the kernel, so a kernel never indexes outside its buffers.
"""
from __future__ import annotations

import ctypes as C

import torch

from .. import _native as N
from .layer_ops import (A_COLM, A_CONV, A_DGRAD, A_ROWK, A_WGRAD, B_DGRADW, B_KN, B_NK, STAT_SLOTS, ConvGeom, DropSpec,
                        dgrad_phases)

_P = N.ptr
_vp, _i, _i64, _f, _u64 = C.c_void_p, C.c_int, C.c_longlong, C.c_float, C.c_ulonglong
N.register_hip({
    # a, lda, akind, b, ldb, bkind, M, N, K, geo, c, ldc, accum, bias, relu, colstats, splits, part, phase, stream
    "tde_igemm32": (_i, [_vp, _i64, _i, _vp, _i64, _i, _i, _i, _i, _vp, _vp, _i64, _i, _vp, _i, _vp, _i, _vp, _vp,
                         _vp]),
    "tde_colstats32": (_i, [_vp, _i64, _i, _vp, _vp]),
    "tde_bn_fwd32": (_i, [_vp, _vp, _vp, _i64, _i, _i, _vp, _vp, _vp, _vp, _f, _vp, _vp, _f, _f, _vp, _i, _f, _u64,
                          _vp, _i, _i, _vp]),
    "tde_bn_bwd32": (_i, [_vp, _vp, _vp, _i64, _i, _i, _vp, _vp, _vp, _i, _f, _u64, _vp, _i, _i, _vp, _vp, _i, _vp,
                          _i, _vp, _vp, _vp, _vp]),
    "tde_act_bwd32": (_i, [_vp, _vp, _i64, _i, _i, _vp, _vp, _vp]),
    "tde_maxpool32": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp]),
    "tde_maxpool32_bwd_relu": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "tde_gap32": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "tde_pad32": (_i, [_vp, _vp, _vp, _i, _i, _vp]),
    "tde_xent32": (_i, [_vp, _vp, _i, _i, _f, _vp, _vp, _vp, _i, _vp, _vp]),
    # csrc/kernels/depthwise.hip
    "tde_dwconv32_fwd": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp]),          # x, w, bias, relu, y, geo, stream
    "tde_dwconv32_dgrad": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp]),        # dy, y, w, dx, accum, geo, stream
    "tde_dwconv32_wgrad": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),  # x, dy, y, dW, db, part, geo, stream
    "tde_dwconv32_splits": (_i, [_vp]),
    # csrc/kernels/groupnorm.hip
    "tde_gn32_plan": (_i, [_i, _i, _i, _i, _vp]),                                       # R, S, C, G, out[7]
    "tde_gn32_fwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp]),      # x, gamma, beta, y, mean, rstd
    # dy, x, gamma, mean, rstd, dx, accum, dgamma, dbeta, part, R, S, C, G, stream
    "tde_gn32_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    # csrc/kernels/attention.hip
    "tde_mha32_fwd": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),         # q, k, v, o, lse, B, H, T, dk, dv
    # q, k, v, o, lse, dO, dq, accum, dk, dv, B, H, T, dk, dv, stream
    "tde_mha32_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    # csrc/kernels/lstm.hip
    "tde_lstm32_fwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),   # z, U, hseq, hprev, gates, cseq, hlast, B, T, u
    "tde_lstm32_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),         # gates, cseq, U, dh, dz, B, T, u, last_only
    # csrc/kernels/gru.hip
    "tde_gru32_fwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),   # x, U, rb, hseq, hprev, acts, hlast, B, T, u
    "tde_gru32_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),    # acts, hprev, U, dh, dx, dr, B, T, u, last_only
    # both directions of a Bidirectional in one launch: operand pairs (direction 0, direction 1), then out / dh
    # z, U, hseq, hprev, gates, cseq pairs, out, B, T, u, seq
    "tde_lstm32_bi_fwd": (_i, [_vp] * 13 + [_i, _i, _i, _i, _vp]),
    "tde_lstm32_bi_bwd": (_i, [_vp] * 9 + [_i, _i, _i, _i, _vp]),    # gates, cseq, U pairs, dh, dz pair, B, T, u, last_only
    # x, U, rb, hseq, hprev, acts pairs, out, B, T, u, seq
    "tde_gru32_bi_fwd": (_i, [_vp] * 13 + [_i, _i, _i, _i, _vp]),
    # acts, hprev, U pairs, dh, dx pair, dr pair, B, T, u, last_only
    "tde_gru32_bi_bwd": (_i, [_vp] * 11 + [_i, _i, _i, _i, _vp]),
    # csrc/kernels/embedding.hip
    "tde_embed32_fwd": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),   # ids, table, out, n, V, D, ids_are_int
    "tde_embed32_bwd": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),   # ids, dy, dtable, n, V, D, ids_are_int
})

_NODROP = DropSpec()


def _s():
    return N.stream_ptr()


def _req(cond, msg):
    if not cond:
        raise ValueError(msg)


def _f32(t, n, what):
    _req(t is not None and t.dtype == torch.float32 and t.is_contiguous() and t.numel() >= n,
         f"{what}: f32 [{n}] expected")


def _f64(t, n, what):
    _req(t is not None and t.dtype == torch.float64 and t.is_contiguous() and t.numel() >= n,
         f"{what}: f64 [{n}] expected")


def tiles(M, N_):
    """Output tiles of an igemm32 launch (64 x 64 by default: layers_f32.hip tile_n)."""
    return -(-M // 64) * -(-N_ // 64)


def wgrad_splits(M, N_, K, target=256):
    """Split-K factor of a weight-gradient GEMM: its output tiles alone rarely fill the 256 CUs while its
    K (= pixels x batch) is long; the partials are summed in split order (deterministic)."""
    tiles_ = tiles(M, N_)
    chunks = -(-K // 16)
    if tiles_ >= target or chunks < 16:
        return 1
    return max(1, min(-(-target // tiles_), chunks // 8))


def wgrad_part_elems(M, N_, K):
    s = wgrad_splits(M, N_, K)
    return s * M * N_ if s > 1 else 0


def fd_splits(M, N_, K, target=256):
    """Split-K factor of a forward / input-gradient GEMM whose output tiles are too few to fill the chip
    while K is long (a Dense layer on a wide flattened input: M = batch, K = 10,816); the partials are
    summed in split order by the reduce launch, which then applies bias / ReLU / BN statistics."""
    tiles_ = tiles(M, N_)
    chunks = -(-K // 16)
    if tiles_ >= 128 or chunks < 32:
        return 1
    return max(1, min(-(-target // tiles_), chunks // 8))


def fd_part_elems(M, N_, K):
    s = fd_splits(M, N_, K)
    return s * M * N_ if s > 1 else 0


def _fd(M, N_, K, part):
    s = fd_splits(M, N_, K) if part is not None else 1
    return (s, part) if s > 1 and part.numel() >= s * M * N_ else (1, None)


def igemm32(a, lda, ak, b, ldb, bk, M, N_, K, c, ldc, *, geo=None, accum=False, bias=None, relu=False,
            colstats=None, splits=1, part=None, phase=None):
    if splits > 1:
        _f32(part, splits * M * N_, "igemm32 split-K partials")
    if colstats is not None:
        _f64(colstats, 2 * STAT_SLOTS * N_, "igemm32 colstats")
    ph = (C.c_int * len(phase))(*phase) if phase is not None else None
    rc = N.hip().tde_igemm32(_P(a), int(lda), ak, _P(b), int(ldb), bk, int(M), int(N_), int(K),
                             geo.carray() if geo is not None else None, _P(c), int(ldc), int(accum), _P(bias),
                             int(relu), _P(colstats), int(splits), _P(part), ph, _s())
    N.check(rc, "tde_igemm32")


# ---------------------------------------------------------------- Conv2D / Dense
def conv_fwd(x, W, y, g: ConvGeom, bias=None, relu=False, colstats=None, part=None):
    """y[B*Ho*Wo, Co] = conv(x, W) (+bias, ReLU, BN statistics); W the HWIO f32 master kernel."""
    _f32(x, g.B * g.H * g.W * g.C, "conv_fwd x")
    _f32(W, g.K * g.Co, "conv_fwd W")
    _f32(y, g.B * g.Ho * g.Wo * g.Co, "conv_fwd y")
    M = g.B * g.Ho * g.Wo
    s, pt = _fd(M, g.Co, g.K, part)
    igemm32(x, 0, A_CONV, W, g.Co, B_KN, M, g.Co, g.K, y, g.Co, geo=g, bias=bias, relu=relu,
            colstats=colstats, splits=s, part=pt)


def conv_dgrad(dy, W, dx, g: ConvGeom, accum=False, part=None):
    """dx = conv input gradient.  Strided convs run every stride phase in ONE launch, each phase over only
    the taps that reach its pixels (the other (s^2-1)/s^2 of the implicit-GEMM K would multiply zeros)."""
    _f32(dy, g.B * g.Ho * g.Wo * g.Co, "conv_dgrad dy")
    _f32(W, g.K * g.Co, "conv_dgrad W")
    _f32(dx, g.B * g.H * g.W * g.C, "conv_dgrad dx")
    if g.sh > 1 or g.sw > 1:
        phases = dgrad_phases(g)
        if 1 <= len(phases) <= 4 and len(phases) == g.sh * g.sw:
            table = [len(phases)] + [v for ph in phases for v in ph]
            Mx = max(g.B * ph[2] * ph[3] for ph in phases)
            Kx = max(ph[6] * ph[7] * g.Co for ph in phases)
            igemm32(dy, 0, A_DGRAD, W, 0, B_DGRADW, Mx, g.C, Kx, dx, g.C, geo=g, accum=accum, phase=table)
            return
    M, K = g.B * g.H * g.W, g.KH * g.KW * g.Co
    s, pt = _fd(M, g.C, K, part)
    igemm32(dy, 0, A_DGRAD, W, 0, B_DGRADW, M, g.C, K, dx, g.C, geo=g, accum=accum, splits=s, part=pt)


def conv_wgrad(x, dy, dW, g: ConvGeom, part=None):
    """dW[KH*KW*C, Co] = sum over pixels x (patch) . dy (stored)."""
    _f32(x, g.B * g.H * g.W * g.C, "conv_wgrad x")
    _f32(dy, g.B * g.Ho * g.Wo * g.Co, "conv_wgrad dy")
    _f32(dW, g.K * g.Co, "conv_wgrad dW")
    K = g.B * g.Ho * g.Wo
    s = wgrad_splits(g.K, g.Co, K) if part is not None else 1
    igemm32(x, 0, A_WGRAD, dy, g.Co, B_KN, g.K, g.Co, K, dW, g.Co, geo=g, splits=s, part=part)


def dense_fwd(x, W, rows, y, bias=None, relu=False, colstats=None, part=None):
    fin, fout = W.shape
    _f32(x, rows * fin, "dense_fwd x")
    _f32(y, rows * fout, "dense_fwd y")
    s, pt = _fd(rows, fout, fin, part)
    igemm32(x, fin, A_ROWK, W, fout, B_KN, rows, fout, fin, y, fout, bias=bias, relu=relu, colstats=colstats,
            splits=s, part=pt)


def dense_dgrad(dy, W, dx, rows, accum=False, part=None):
    fin, fout = W.shape
    _f32(dy, rows * fout, "dense_dgrad dy")
    _f32(dx, rows * fin, "dense_dgrad dx")
    s, pt = _fd(rows, fin, fout, part)
    igemm32(dy, fout, A_ROWK, W, fout, B_NK, rows, fin, fout, dx, fin, accum=accum, splits=s, part=pt)


def dense_wgrad(x, dy, dW, rows, part=None):
    fin, fout = dW.shape
    _f32(x, rows * fin, "dense_wgrad x")
    _f32(dy, rows * fout, "dense_wgrad dy")
    s = wgrad_splits(fin, fout, rows) if part is not None else 1
    igemm32(x, fin, A_COLM, dy, fout, B_KN, fin, fout, rows, dW, fout, splits=s, part=part)


# ---------------------------------------------------------------- DepthwiseConv2D (csrc/kernels/depthwise.hip)
DW_MAX_K, DW_MAX_STRIDE, DW_MAX_DM = 7, 4, 8


def dw_check(g: ConvGeom, what):
    """The supported range of the depthwise kernels; returns (x, y, w) element counts.  Co = C * dm."""
    _req(min(g.B, g.H, g.W, g.C, g.Ho, g.Wo, g.Co) >= 1, f"{what}: empty geometry {g}")
    _req(1 <= g.KH <= DW_MAX_K and 1 <= g.KW <= DW_MAX_K, f"{what}: kernel {g.KH}x{g.KW} (at most 7x7)")
    _req(1 <= g.sh <= DW_MAX_STRIDE and 1 <= g.sw <= DW_MAX_STRIDE, f"{what}: strides ({g.sh}, {g.sw}) (at most 4)")
    _req(g.Co % g.C == 0 and g.Co // g.C <= DW_MAX_DM, f"{what}: depth multiplier {g.Co / g.C:g} (an integer <= 8)")
    _req(0 <= g.pt < g.KH and 0 <= g.pl < g.KW, f"{what}: pads ({g.pt}, {g.pl})")
    _req((g.Ho - 1) * g.sh - g.pt < g.H and (g.Wo - 1) * g.sw - g.pl < g.W, f"{what}: output extent past the input")
    return g.B * g.H * g.W * g.C, g.B * g.Ho * g.Wo * g.Co, g.KH * g.KW * g.Co


def dw_splits(g: ConvGeom):
    """Pixel splits of the depthwise weight gradient (the kernel library's own rule: one source of truth)."""
    dw_check(g, "dw_splits")
    return int(N.hip().tde_dwconv32_splits(g.carray()))


def dw_part_elems(g: ConvGeom):
    """f32 elements of the per-split partial rows [splits][KH*KW*Co + Co] of ``dw_wgrad``."""
    return dw_splits(g) * (g.KH * g.KW * g.Co + g.Co)


def dw_fwd(x, w, y, g: ConvGeom, bias=None, relu=False):
    """y[B,Ho,Wo,C*dm] = act(bias + depthwise_conv(x, w)); w the Keras depthwise_kernel [KH,KW,C,dm] master."""
    nx, ny, nw = dw_check(g, "dw_fwd")
    _f32(x, nx, "dw_fwd x")
    _f32(w, nw, "dw_fwd w")
    _f32(y, ny, "dw_fwd y")
    if bias is not None:
        _f32(bias, g.Co, "dw_fwd bias")
    N.check(N.hip().tde_dwconv32_fwd(_P(x), _P(w), _P(bias), int(relu), _P(y), g.carray(), _s()), "tde_dwconv32_fwd")


def dw_dgrad(dy, w, dx, g: ConvGeom, y=None, accum=False):
    """dx (+)= the input gradient of dy * (y > 0) (``y``: the layer's ReLU output; None: linear)."""
    nx, ny, nw = dw_check(g, "dw_dgrad")
    _f32(dy, ny, "dw_dgrad dy")
    _f32(w, nw, "dw_dgrad w")
    _f32(dx, nx, "dw_dgrad dx")
    if y is not None:
        _f32(y, ny, "dw_dgrad y")
    N.check(N.hip().tde_dwconv32_dgrad(_P(dy), _P(y), _P(w), _P(dx), int(accum), g.carray(), _s()),
            "tde_dwconv32_dgrad")


def dw_wgrad(x, dy, dW, g: ConvGeom, part, y=None, db=None):
    """dW[KH,KW,C,dm] = sum over pixels x . dy * (y > 0), db[Co] = sum of that dy; per-split partials in ``part``
    (``dw_part_elems``), summed in split order: bitwise reproducible."""
    nx, ny, nw = dw_check(g, "dw_wgrad")
    _f32(x, nx, "dw_wgrad x")
    _f32(dy, ny, "dw_wgrad dy")
    _f32(dW, nw, "dw_wgrad dW")
    _f32(part, dw_part_elems(g), "dw_wgrad partials")
    if y is not None:
        _f32(y, ny, "dw_wgrad y")
    if db is not None:
        _f32(db, g.Co, "dw_wgrad db")
    N.check(N.hip().tde_dwconv32_wgrad(_P(x), _P(dy), _P(y), _P(dW), _P(db), _P(part), g.carray(), _s()),
            "tde_dwconv32_wgrad")


# ---------------------------------------------------------------- GroupNormalization / LayerNormalization
GN_MAX_C = 2048


def gn_check(R, S, C, G, what):
    """The supported range of csrc/kernels/groupnorm.hip: R rows of S positions x C channels in G groups (group
    (r, g): for each s the C // G floats at ((r*S + s)*C + g*(C // G))).  Returns (elements, groups)."""
    _req(min(R, S, C, G) >= 1, f"{what}: empty geometry R={R} S={S} C={C} G={G}")
    _req(C <= GN_MAX_C, f"{what}: {C} channels (at most {GN_MAX_C})")
    _req(C % G == 0, f"{what}: {G} groups do not divide {C} channels")
    _req(R * G < 2 ** 31 and R * S < 2 ** 31, f"{what}: R={R} S={S} G={G} past the 32-bit row range")
    return R * S * C, R * G


def gn_plan(R, S, C, G):
    """How the kernel library splits a geometry (its own rule: one source of truth): dict(slab, parts, strip,
    group_block, blocks, staged_fwd, staged_bwd); ``parts`` partial rows [2][C] feed the ordered reduction."""
    gn_check(R, S, C, G, "gn_plan")
    out = (_i * 7)()
    N.check(min(N.hip().tde_gn32_plan(R, S, C, G, out), 0), "tde_gn32_plan")
    return dict(zip(("slab", "parts", "strip", "group_block", "blocks", "staged_fwd", "staged_bwd"), out))


def gn_part_elems(R, S, C, G):
    """f32 elements of the partial rows [parts][2][C] of ``gn_bwd``."""
    return gn_plan(R, S, C, G)["parts"] * 2 * C


def gn_fwd(x, y, mean, rstd, R, S, C, G, eps, gamma=None, beta=None):
    """y = (x - mean) * rstd * gamma + beta per (row, group); mean, rstd f32 [R*G] are saved for ``gn_bwd``."""
    n, ng = gn_check(R, S, C, G, "gn_fwd")
    _f32(x, n, "gn_fwd x")
    _f32(y, n, "gn_fwd y")
    _f32(mean, ng, "gn_fwd mean")
    _f32(rstd, ng, "gn_fwd rstd")
    if gamma is not None:
        _f32(gamma, C, "gn_fwd gamma")
    if beta is not None:
        _f32(beta, C, "gn_fwd beta")
    N.check(N.hip().tde_gn32_fwd(_P(x), _P(gamma), _P(beta), _P(y), _P(mean), _P(rstd), R, S, C, G, float(eps), _s()),
            "tde_gn32_fwd")


def gn_bwd(dy, x, mean, rstd, R, S, C, G, part, gamma=None, dx=None, accum=False, dgamma=None, dbeta=None):
    """dx (+)= rstd * (g - mean_grp(g) - xh * mean_grp(g * xh)) with xh = (x - mean) * rstd, g = dy * gamma (dx
    None: skipped); dgamma = sum dy * xh, dbeta = sum dy from per-workgroup partials in ``part``
    (``gn_part_elems``), summed in a fixed order: bitwise reproducible."""
    n, ng = gn_check(R, S, C, G, "gn_bwd")
    _f32(dy, n, "gn_bwd dy")
    _f32(x, n, "gn_bwd x")
    _f32(mean, ng, "gn_bwd mean")
    _f32(rstd, ng, "gn_bwd rstd")
    _f32(part, gn_part_elems(R, S, C, G), "gn_bwd partials")
    for t, m, what in ((gamma, C, "gamma"), (dx, n, "dx"), (dgamma, C, "dgamma"), (dbeta, C, "dbeta")):
        if t is not None:
            _f32(t, m, f"gn_bwd {what}")
    N.check(N.hip().tde_gn32_bwd(_P(dy), _P(x), _P(gamma), _P(mean), _P(rstd), _P(dx), int(accum), _P(dgamma),
                                 _P(dbeta), _P(part), R, S, C, G, _s()), "tde_gn32_bwd")


# ---------------------------------------------------------------- MultiHeadAttention core (csrc/kernels/attention.hip)
MHA_MAX_T, MHA_MAX_D = 256, 64


def mha_check(B, H, T, dk, dv, what):
    """The supported range of csrc/kernels/attention.hip: B samples, H heads, T tokens, head sizes dk (query /
    key) and dv (value).  Returns the element counts of (Q or K, V or O, lse)."""
    _req(min(B, H, T) >= 1, f"{what}: empty geometry B={B} heads={H} T={T}")
    _req(T <= MHA_MAX_T, f"{what}: {T} tokens (at most {MHA_MAX_T})")
    for d, n in ((dk, "key_dim"), (dv, "value_dim")):
        _req(4 <= d <= MHA_MAX_D and d % 4 == 0, f"{what}: {n}={d} (a multiple of 4, at most {MHA_MAX_D})")
    _req(B * H * -(-T // 64) < 2 ** 31, f"{what}: B={B} heads={H} past the 32-bit workgroup range")
    return B * T * H * dk, B * T * H * dv, B * H * T


def _mha_f32(t, n, what):
    _f32(t, n, what)
    _req(t.data_ptr() % 16 == 0, f"{what}: a 16-byte aligned base expected")


def mha_fwd(q, k, v, o, lse, B, H, T, dk, dv):
    """o [B,T,H*dv] = softmax(q k^T / sqrt(dk)) v per (sample, head), q / k [B,T,H*dk] and v [B,T,H*dv] head-major
    in the last axis; lse f32 [B,H,T] (the row log-sum-exp of the scaled scores) is saved for ``mha_bwd``."""
    nk, nv, nl = mha_check(B, H, T, dk, dv, "mha_fwd")
    for t, n, what in ((q, nk, "q"), (k, nk, "k"), (v, nv, "v"), (o, nv, "o")):
        _mha_f32(t, n, f"mha_fwd {what}")
    _f32(lse, nl, "mha_fwd lse")
    N.check(N.hip().tde_mha32_fwd(_P(q), _P(k), _P(v), _P(o), _P(lse), B, H, T, dk, dv, _s()), "tde_mha32_fwd")


def mha_bwd(q, k, v, o, lse, do, dq, dk_, dv_, B, H, T, dk, dv, accum=False):
    """dq (+)= , dk_ = , dv_ = the gradients of ``mha_fwd`` under ``do``; ``accum`` adds onto dq.  Two launches
    (dK / dV per key block, dQ per query block), no atomics: bitwise reproducible."""
    nk, nv, nl = mha_check(B, H, T, dk, dv, "mha_bwd")
    for t, n, what in ((q, nk, "q"), (k, nk, "k"), (v, nv, "v"), (o, nv, "o"), (do, nv, "do"), (dq, nk, "dq"),
                       (dk_, nk, "dk"), (dv_, nv, "dv")):
        _mha_f32(t, n, f"mha_bwd {what}")
    _f32(lse, nl, "mha_bwd lse")
    N.check(N.hip().tde_mha32_bwd(_P(q), _P(k), _P(v), _P(o), _P(lse), _P(do), _P(dq), int(accum), _P(dk_), _P(dv_),
                                  B, H, T, dk, dv, _s()), "tde_mha32_bwd")


# ---------------------------------------------------------------- LSTM recurrence (csrc/kernels/lstm.hip)
LSTM_MIN_UNITS, LSTM_MAX_UNITS = 16, 128


def lstm_check(B, T, units, what):
    """The supported range of csrc/kernels/lstm.hip: B sequences of T steps, ``units`` hidden units.  Returns the
    element count of a [B, T, units] tensor."""
    _req(min(B, T) >= 1, f"{what}: empty geometry B={B} T={T}")
    _req(LSTM_MIN_UNITS <= units <= LSTM_MAX_UNITS and units % 16 == 0,
         f"{what}: units={units} (a multiple of 16 from {LSTM_MIN_UNITS} to {LSTM_MAX_UNITS})")
    _req(T * units < 2 ** 24, f"{what}: T={T} x units={units} (a workgroup's 16 sequences are addressed by 32-bit "
                              "byte offsets: T * units below 2^24)")
    return B * T * units


def lstm_fwd(z, rk, hseq, hprev, gates, cseq, B, T, units, hlast=None):
    """The forward sweep over z = x W + b [B, T, 4 units] (gate order i, f, c, o) with the recurrent kernel rk
    [units, 4 units] from a zero state: hseq (h_t), hprev (h_{t-1}, zeros at t = 0) and cseq [B, T, units], the
    four gate activations ``gates`` [B, T, 4 units], and the last h into ``hlast`` [B, units] when given."""
    n = lstm_check(B, T, units, "lstm_fwd")
    for t, k, what in ((z, 4 * n, "z"), (rk, 4 * units * units, "recurrent kernel"), (hseq, n, "hseq"),
                       (hprev, n, "hprev"), (gates, 4 * n, "gates"), (cseq, n, "cseq")):
        _f32(t, k, f"lstm_fwd {what}")
    if hlast is not None:
        _f32(hlast, B * units, "lstm_fwd hlast")
    N.check(N.hip().tde_lstm32_fwd(_P(z), _P(rk), _P(hseq), _P(hprev), _P(gates), _P(cseq), _P(hlast), B, T, units,
                                   _s()), "tde_lstm32_fwd")


def lstm_bwd(gates, cseq, rk, dh, dz, B, T, units, last_only):
    """dz [B, T, 4 units] = the gradient of ``lstm_fwd``'s z under dh, the gradient of hseq [B, T, units] or, with
    ``last_only``, of the last h alone [B, units].  One launch, no atomics: bitwise reproducible."""
    n = lstm_check(B, T, units, "lstm_bwd")
    for t, k, what in ((gates, 4 * n, "gates"), (cseq, n, "cseq"), (rk, 4 * units * units, "recurrent kernel"),
                       (dh, B * units if last_only else n, "dh"), (dz, 4 * n, "dz")):
        _f32(t, k, f"lstm_bwd {what}")
    N.check(N.hip().tde_lstm32_bwd(_P(gates), _P(cseq), _P(rk), _P(dh), _P(dz), B, T, units, int(bool(last_only)),
                                   _s()), "tde_lstm32_bwd")


# ---------------------------------------------------------------- GRU recurrence (csrc/kernels/gru.hip)
def gru_check(B, T, units, what):
    """The supported range of csrc/kernels/gru.hip, which is that of the LSTM sweeps: B sequences of T steps,
    ``units`` hidden units.  Returns the element count of a [B, T, units] tensor."""
    return lstm_check(B, T, units, what)


def gru_fwd(x, rk, rb, hseq, hprev, acts, B, T, units, hlast=None):
    """The forward sweep over x = input W + b[0] [B, T, 3 units] (gate order z, r, h) with the recurrent kernel rk
    [units, 3 units] and the recurrent bias rb [3 units] (None: none) from a zero state: hseq (h_t) and hprev
    (h_{t-1}, zeros at t = 0) [B, T, units], ``acts`` [B, T, 4 units] in the order z, r, hh, R_h (the candidate's
    recurrent pre-activation h_{t-1} U_h + rb_h), and the last h into ``hlast`` [B, units] when given."""
    n = gru_check(B, T, units, "gru_fwd")
    for t, k, what in ((x, 3 * n, "x"), (rk, 3 * units * units, "recurrent kernel"), (hseq, n, "hseq"),
                       (hprev, n, "hprev"), (acts, 4 * n, "acts")):
        _f32(t, k, f"gru_fwd {what}")
    if rb is not None:
        _f32(rb, 3 * units, "gru_fwd recurrent bias")
    if hlast is not None:
        _f32(hlast, B * units, "gru_fwd hlast")
    N.check(N.hip().tde_gru32_fwd(_P(x), _P(rk), _P(rb), _P(hseq), _P(hprev), _P(acts), _P(hlast), B, T, units,
                                  _s()), "tde_gru32_fwd")


def gru_bwd(acts, hprev, rk, dh, dx, dr, B, T, units, last_only):
    """dx and dr [B, T, 3 units] = the gradients of ``gru_fwd``'s x and of the recurrent pre-activation
    h_{t-1} rk + rb (they differ in the candidate's block) under dh, the gradient of hseq [B, T, units] or, with
    ``last_only``, of the last h alone [B, units].  One launch, no atomics: bitwise reproducible."""
    n = gru_check(B, T, units, "gru_bwd")
    for t, k, what in ((acts, 4 * n, "acts"), (hprev, n, "hprev"), (rk, 3 * units * units, "recurrent kernel"),
                       (dh, B * units if last_only else n, "dh"), (dx, 3 * n, "dx"), (dr, 3 * n, "dr")):
        _f32(t, k, f"gru_bwd {what}")
    N.check(N.hip().tde_gru32_bwd(_P(acts), _P(hprev), _P(rk), _P(dh), _P(dx), _P(dr), B, T, units,
                                  int(bool(last_only)), _s()), "tde_gru32_bwd")


# ---------------------------------------------------------------- Bidirectional(LSTM | GRU): one launch per sweep
# Every per-direction operand is a pair (direction 0: forward in time, direction 1: backward in time).  ``out`` is the
# layer's output: with ``seq`` [B, T, 2 units], direction d's h of position t in columns d * units .. (original time
# order; the ``hseq`` pair is not used and may be None); otherwise [B, 2 units], direction 0's state after t = T - 1
# and direction 1's after t = 0, with every h into ``hseq[d]`` [B, T, units] when given.  ``hprev[d]`` at position t is
# direction d's state before it processed position t: for direction 1 that is h of position t + 1, zeros at T - 1.
def _pair(ts, n, what, optional=False):
    _req(isinstance(ts, (tuple, list)) and len(ts) == 2, f"{what}: a pair (direction 0, direction 1) expected")
    for d, t in enumerate(ts):
        if t is not None or not optional:
            _f32(t, n, f"{what}[{d}]")
    return _P(ts[0]), _P(ts[1])


def lstm_bi_fwd(z, rk, hseq, hprev, gates, cseq, out, B, T, units, seq):
    """``lstm_fwd`` for both directions at once (grid (ceil(B / 16), 2)): see the section comment."""
    n = lstm_check(B, T, units, "lstm_bi_fwd")
    args = (*_pair(z, 4 * n, "lstm_bi_fwd z"), *_pair(rk, 4 * units * units, "lstm_bi_fwd recurrent kernel"),
            *_pair(hseq or (None, None), n, "lstm_bi_fwd hseq", optional=True), *_pair(hprev, n, "lstm_bi_fwd hprev"),
            *_pair(gates, 4 * n, "lstm_bi_fwd gates"), *_pair(cseq, n, "lstm_bi_fwd cseq"))
    _f32(out, 2 * n if seq else 2 * B * units, "lstm_bi_fwd out")
    N.check(N.hip().tde_lstm32_bi_fwd(*args, _P(out), B, T, units, int(bool(seq)), _s()), "tde_lstm32_bi_fwd")


def lstm_bi_bwd(gates, cseq, rk, dh, dz, B, T, units, last_only):
    """``lstm_bwd`` for both directions at once: dz[d] [B, T, 4 units] under dh [B, T, 2 units], or [B, 2 units]
    with ``last_only`` (the gradient of the two final states).  One launch, no atomics: bitwise reproducible."""
    n = lstm_check(B, T, units, "lstm_bi_bwd")
    args = (*_pair(gates, 4 * n, "lstm_bi_bwd gates"), *_pair(cseq, n, "lstm_bi_bwd cseq"),
            *_pair(rk, 4 * units * units, "lstm_bi_bwd recurrent kernel"))
    _f32(dh, 2 * B * units if last_only else 2 * n, "lstm_bi_bwd dh")
    N.check(N.hip().tde_lstm32_bi_bwd(*args, _P(dh), *_pair(dz, 4 * n, "lstm_bi_bwd dz"), B, T, units,
                                      int(bool(last_only)), _s()), "tde_lstm32_bi_bwd")


def gru_bi_fwd(x, rk, rb, hseq, hprev, acts, out, B, T, units, seq):
    """``gru_fwd`` for both directions at once (grid (ceil(B / 16), 2)): see the section comment.  ``rb``: the pair
    of recurrent biases [3 units], or None for none."""
    n = gru_check(B, T, units, "gru_bi_fwd")
    args = (*_pair(x, 3 * n, "gru_bi_fwd x"), *_pair(rk, 3 * units * units, "gru_bi_fwd recurrent kernel"),
            *_pair(rb or (None, None), 3 * units, "gru_bi_fwd recurrent bias", optional=True),
            *_pair(hseq or (None, None), n, "gru_bi_fwd hseq", optional=True), *_pair(hprev, n, "gru_bi_fwd hprev"),
            *_pair(acts, 4 * n, "gru_bi_fwd acts"))
    _f32(out, 2 * n if seq else 2 * B * units, "gru_bi_fwd out")
    N.check(N.hip().tde_gru32_bi_fwd(*args, _P(out), B, T, units, int(bool(seq)), _s()), "tde_gru32_bi_fwd")


def gru_bi_bwd(acts, hprev, rk, dh, dx, dr, B, T, units, last_only):
    """``gru_bwd`` for both directions at once: dx[d] and dr[d] [B, T, 3 units] under dh [B, T, 2 units], or
    [B, 2 units] with ``last_only``.  One launch, no atomics: bitwise reproducible."""
    n = gru_check(B, T, units, "gru_bi_bwd")
    args = (*_pair(acts, 4 * n, "gru_bi_bwd acts"), *_pair(hprev, n, "gru_bi_bwd hprev"),
            *_pair(rk, 3 * units * units, "gru_bi_bwd recurrent kernel"))
    _f32(dh, 2 * B * units if last_only else 2 * n, "gru_bi_bwd dh")
    N.check(N.hip().tde_gru32_bi_bwd(*args, _P(dh), *_pair(dx, 3 * n, "gru_bi_bwd dx"),
                                     *_pair(dr, 3 * n, "gru_bi_bwd dr"), B, T, units, int(bool(last_only)), _s()),
            "tde_gru32_bi_bwd")


# ---------------------------------------------------------------- Embedding (csrc/kernels/embedding.hip)
EMBED_MAX_V, EMBED_MAX_D = 2 ** 24, 512


def embed_check(n, V, D, what):
    """The supported range of csrc/kernels/embedding.hip: n tokens, a [V, D] table.  Ids travel as float32 (exact up
    to 2^24) and every tensor is indexed by 32-bit element offsets."""
    _req(n >= 1, f"{what}: empty geometry n={n}")
    _req(1 <= V <= EMBED_MAX_V, f"{what}: input_dim={V} (from 1 to 2^24: ids are read as float32)")
    _req(4 <= D <= EMBED_MAX_D and D % 4 == 0, f"{what}: output_dim={D} (a multiple of 4 from 4 to {EMBED_MAX_D})")
    _req(n * D < 2 ** 31, f"{what}: n={n} x output_dim={D} (the output is addressed by 32-bit offsets: below 2^31)")
    _req(V * D < 2 ** 31, f"{what}: input_dim={V} x output_dim={D} (the table is addressed by 32-bit offsets: below "
                          "2^31)")


def _embed_ids(ids, n, what):
    _req(ids is not None and ids.dtype in (torch.float32, torch.int32) and ids.is_contiguous() and ids.numel() >= n,
         f"{what}: f32 or i32 [{n}] expected")
    return int(ids.dtype == torch.int32)


def embed_fwd(ids, table, out, n, V, D):
    """out [n, D] = table[ids]: ids float32 (truncated toward zero) or int32; an id outside [0, V) gives a zero
    row."""
    embed_check(n, V, D, "embed_fwd")
    flag = _embed_ids(ids, n, "embed_fwd ids")
    _f32(table, V * D, "embed_fwd table")
    _f32(out, n * D, "embed_fwd out")
    N.check(N.hip().tde_embed32_fwd(_P(ids), _P(table), _P(out), n, V, D, flag, _s()), "tde_embed32_fwd")


def embed_bwd(ids, dy, dtable, n, V, D):
    """dtable [V, D], written whole: row v is the float32 sum of the dy [n, D] rows whose id is v, added in token
    order from zero (numpy's ``add.at`` bit for bit); ids outside [0, V) take no part.  One launch, no atomics."""
    embed_check(n, V, D, "embed_bwd")
    flag = _embed_ids(ids, n, "embed_bwd ids")
    _f32(dy, n * D, "embed_bwd dy")
    _f32(dtable, V * D, "embed_bwd dtable")
    N.check(N.hip().tde_embed32_bwd(_P(ids), _P(dy), _P(dtable), n, V, D, flag, _s()), "tde_embed32_bwd")


# ---------------------------------------------------------------- BatchNormalization / activations
def colstats(x, R, Cc, stats):
    _f32(x, R * Cc, "colstats32 x")
    _f64(stats, 2 * STAT_SLOTS * Cc, "colstats32 stats")
    N.check(N.hip().tde_colstats32(_P(x), int(R), int(Cc), _P(stats), _s()), "tde_colstats32")


def bn_fwd(y, out, R, Cc, *, mode, stats=None, saved=None, gamma=None, beta=None, eps=1e-3, mmean=None, mvar=None,
           momentum=0.99, bessel=1.0, zero_buf=None, res=None, relu=False, drop: DropSpec = _NODROP, iter_offset=0):
    """out = dropout(relu(bn(y) + res)); mode 0 identity, 1 batch stats (from ``stats``), 2 moving stats."""
    n = R * Cc
    _f32(y, n, "bn_fwd32 y")
    _f32(out, n, "bn_fwd32 out")
    _req(Cc <= 2048, "bn_fwd32: at most 2048 channels")
    if res is not None:
        _f32(res, n, "bn_fwd32 res")
    if mode == 1:
        _f64(stats, 2 * STAT_SLOTS * Cc, "bn_fwd32 stats")
        _f32(saved, 2 * Cc, "bn_fwd32 saved")
    if mode == 2:
        _f32(mmean, Cc, "bn_fwd32 moving_mean")
        _f32(mvar, Cc, "bn_fwd32 moving_variance")
    if zero_buf is not None:
        _f64(zero_buf, 2 * STAT_SLOTS * Cc, "bn_fwd32 zero_buf")
    rc = N.hip().tde_bn_fwd32(_P(y), _P(out), _P(res), int(R), int(Cc), int(mode), _P(stats), _P(saved), _P(gamma),
                              _P(beta), float(eps), _P(mmean), _P(mvar), float(momentum), float(bessel), _P(zero_buf),
                              int(relu), float(drop.rate), int(drop.seed) & (2 ** 64 - 1), _P(drop.iterations),
                              int(iter_offset), int(drop.layer_id), _s())
    N.check(rc, "tde_bn_fwd32")


def bn_bwd(dout, y, R, Cc, *, mode, saved=None, gamma=None, beta=None, res=None, relu=False,
           drop: DropSpec = _NODROP, iter_offset=-1, dstats=None, dx=None, dx_accum=False, dres=None,
           dres_accum=False, dgamma=None, dbeta=None, zero_fwd=None):
    n = R * Cc
    _f32(dout, n, "bn_bwd32 dout")
    _f32(y, n, "bn_bwd32 y")
    _req(Cc <= 2048, "bn_bwd32: at most 2048 channels")
    if mode == 1:
        _f32(saved, 2 * Cc, "bn_bwd32 saved")
        _f64(dstats, 2 * STAT_SLOTS * Cc, "bn_bwd32 dstats")
    if zero_fwd is not None:
        _f64(zero_fwd, 2 * STAT_SLOTS * Cc, "bn_bwd32 zero_fwd")
    for t, what in ((dx, "dx"), (dres, "dres"), (res, "res")):
        if t is not None:
            _f32(t, n, f"bn_bwd32 {what}")
    rc = N.hip().tde_bn_bwd32(_P(dout), _P(y), _P(res), int(R), int(Cc), int(mode), _P(saved), _P(gamma), _P(beta),
                              int(relu), float(drop.rate), int(drop.seed) & (2 ** 64 - 1), _P(drop.iterations),
                              int(iter_offset), int(drop.layer_id), _P(dstats), _P(dx), int(dx_accum), _P(dres),
                              int(dres_accum), _P(dgamma), _P(dbeta), _P(zero_fwd), _s())
    N.check(rc, "tde_bn_bwd32")


def act_bwd(dout, out, R, Cc, *, relu, dz=None, dbias=None):
    n = R * Cc
    _f32(dout, n, "act_bwd32 dout")
    if relu:
        _f32(out, n, "act_bwd32 out")
    if dz is not None:
        _f32(dz, n, "act_bwd32 dz")
    if dbias is not None:
        _f32(dbias, Cc, "act_bwd32 dbias")
    rc = N.hip().tde_act_bwd32(_P(dout), _P(out), int(R), int(Cc), int(relu), _P(dz), _P(dbias), _s())
    N.check(rc, "tde_act_bwd32")


# ---------------------------------------------------------------- pooling / padding / head
def maxpool_fwd(x, y, idx, g: ConvGeom):
    _f32(x, g.B * g.H * g.W * g.C, "maxpool32 x")
    _f32(y, g.B * g.Ho * g.Wo * g.C, "maxpool32 y")
    _req(idx is None or (idx.dtype == torch.uint8 and idx.numel() >= g.B * g.Ho * g.Wo * g.C), "maxpool32 idx")
    N.check(N.hip().tde_maxpool32(_P(x), _P(y), _P(idx), None, None, 0, g.carray(), 0, _s()), "tde_maxpool32")


def maxpool_bwd(dy, idx, dx, g: ConvGeom, accum=False):
    _f32(dy, g.B * g.Ho * g.Wo * g.C, "maxpool32 dy")
    _f32(dx, g.B * g.H * g.W * g.C, "maxpool32 dx")
    _req(idx.dtype == torch.uint8 and idx.numel() >= g.B * g.Ho * g.Wo * g.C, "maxpool32 idx")
    N.check(N.hip().tde_maxpool32(None, None, _P(idx), _P(dy), _P(dx), int(accum), g.carray(), 1, _s()),
            "tde_maxpool32")


def maxpool_bwd_relu(dy, y, idx, dx, g: ConvGeom, dbias=None, accum=False):
    """Max-pool backward fused with the producer's ReLU (+ bias) backward: dx = dy * (y > 0) at each window's
    winner, 0 elsewhere; dbias += the column sums of that over the pooled cells.  Non-overlapping windows."""
    _f32(dy, g.B * g.Ho * g.Wo * g.C, "maxpool_bwd_relu dy")
    _f32(y, g.B * g.Ho * g.Wo * g.C, "maxpool_bwd_relu y")
    _f32(dx, g.B * g.H * g.W * g.C, "maxpool_bwd_relu dx")
    _req(idx.numel() >= g.B * g.Ho * g.Wo * g.C and (dbias is None or dbias.numel() == g.C), "maxpool_bwd_relu")
    N.check(N.hip().tde_maxpool32_bwd_relu(_P(dy), _P(y), _P(idx), _P(dx), _P(dbias), int(accum), g.carray(), _s()),
            "tde_maxpool32_bwd_relu")


def pool_relu_fusable(g: ConvGeom):
    return g.C % 4 == 0 and g.sh >= g.KH and g.sw >= g.KW and g.KH * g.KW <= 255


def gap_fwd(x, y, B, HW, Cc):
    _f32(x, B * HW * Cc, "gap32 x")
    _f32(y, B * Cc, "gap32 y")
    N.check(N.hip().tde_gap32(_P(x), _P(y), int(B), int(HW), int(Cc), 0, 0, _s()), "tde_gap32")


def gap_bwd(dy, dx, B, HW, Cc, accum=False):
    _f32(dy, B * Cc, "gap32 dy")
    _f32(dx, B * HW * Cc, "gap32 dx")
    N.check(N.hip().tde_gap32(_P(dy), _P(dx), int(B), int(HW), int(Cc), 1, int(accum), _s()), "tde_gap32")


def pad_fwd(x, y, g: ConvGeom):
    _f32(x, g.B * g.H * g.W * g.C, "pad32 x")
    _f32(y, g.B * g.Ho * g.Wo * g.C, "pad32 y")
    N.check(N.hip().tde_pad32(_P(x), _P(y), g.carray(), 0, 0, _s()), "tde_pad32")


def pad_bwd(dy, dx, g: ConvGeom, accum=False):
    _f32(dy, g.B * g.Ho * g.Wo * g.C, "pad32 dy")
    _f32(dx, g.B * g.H * g.W * g.C, "pad32 dx")
    N.check(N.hip().tde_pad32(_P(dy), _P(dx), g.carray(), 1, int(accum), _s()), "tde_pad32")


def xent(logits, labels, B, Cc, *, scale=1.0, dlogits=None, metrics=None, probs=None, probs_are_logits=False,
         iterations=None):
    _f32(logits, B * Cc, "xent32 logits")
    _req(labels.dtype == torch.int32 and labels.numel() >= B, "xent32 labels")
    if dlogits is not None:
        _f32(dlogits, B * Cc, "xent32 dlogits")
    if probs is not None:
        _f32(probs, B * Cc, "xent32 probs")
    rc = N.hip().tde_xent32(_P(logits), _P(labels), int(B), int(Cc), float(scale), _P(dlogits), _P(metrics),
                            _P(probs), int(probs_are_logits), _P(iterations), _s())
    N.check(rc, "tde_xent32")
