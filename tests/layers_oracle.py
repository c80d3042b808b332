"""Float64 NumPy oracle of the streaming kernels of csrc/kernels/layers.hip (BatchNorm forward / backward, max
pooling, the fused BN + ReLU + MaxPool pair, act_bwd, GAP, pad, column statistics, the bf16 cast and softmax
cross-entropy), with a per-element absolute bound for every result, and the case table that
tests/test_layers_oracle.py (CPU) and tests/test_layers_stream_gpu.py (GPU) share.  No GPU, no torch.

Every function returns ``(ref, bound)`` or a dict ``name -> (ref, bound)``; ``ref`` of a bf16-stored result is the
float64 value BEFORE the final store, so the store's own rounding is part of the bound (comparing two independently
rounded values would double it).  Where a later stage consumes a stored bf16 tensor the oracle rounds it with
``bf16_round`` (round to nearest even, the kernels' f2bf).

How the bounds are built (u = 2^-24, one fp32 rounding, relative):
  * a bf16 store of v: |bf16(v) - v| <= 2^-8 |v| (half an ulp of an 8-bit significand) + 2^-134 (subnormals);
  * an fp32 expression: u * k * sum|terms|, k = the number of fp32 roundings on the longest path to that element
    (first order: each rounding is relative to a partial result no larger than sum|terms|); an FMA contraction
    only removes roundings.  rsqrtf counts 2 (v_rsq_f32: 1 ulp), __expf / __logf / 1/x count as written below;
  * an fp32 sum over R rows whose order the hardware picks (atomics): u * (SUM_C * sqrt(R) + k_term) * sum|terms|
    with SUM_C measured on the CPU (``measure_sum_constant``), never against a kernel;
  * exact operations (max pooling, pad, cast, sums of grid values) have bound 0.
``ambiguous`` masks mark elements whose ReLU / argmax decision depends on fp32 rounding: |z| below z's own fp32
term, or a pooling window whose winner changes when every candidate moves by its fp32 term.  A test may leave out at
most AMBIGUOUS_CAP of a tensor this way."""
from collections import namedtuple
from contextlib import contextmanager

import numpy as np

U = 2.0 ** -24          # one fp32 rounding (half an ulp, relative)
HB = 2.0 ** -8          # one bf16 rounding (half an ulp, relative)
BF16_TINY = 2.0 ** -134  # half the spacing of bf16 subnormals
FLT_MIN = 2.0 ** -126    # smallest normal fp32: results below it may be flushed to zero
AMBIGUOUS_CAP = 0.005
STAT_SLOTS = 8

# fp32 roundings on the longest path (see the docstrings of the functions that use them)
K_BN_FWD = 8     # var+eps 1, rsqrtf 2, g*rstd 1, mean*scale 1, beta-.. 1, +shift 1 (v*scale is a shorter path), +res 1
K_BN_DROP = 2    # 1/(1-rate) (1-rate is exact for rate <= 0.5: Sterbenz) 1, z*ks 1
K_BN_MOV = 4     # var*bessel 1, *(1-momentum) 1, old*momentum (parallel), + 1, and 1 spare for 1-momentum
K_BN_BWD_Z = 5   # mean*g 1, *rstd 1, beta-.. 1, (v*sc)+sf 1, +res 1   (v*sc: g*rstd 1, v*sc 1 is shorter)
K_BN_TERM = 4    # one term dz*xhat: v-mu 1, *rstd 1, dz*xhat 1, dout*ks 1 (dropout only)
K_BN_SLOTS = 9   # the 8 slot adds of the apply pass and the += into dgamma / dbeta
K_BN_DX = 10     # 1/R 1, sums*invR 1 (k1), xhat 2, xhat*k2 1, two subtractions 2, g*rstd 1, sc*(..) 1, accumulate add 1
K_GAP = 3        # 1/HW 1, s*inv 1, accumulate add 1
# SUM_C: |fp32 sum - exact sum| <= SUM_C * sqrt(R) * u * sum|terms| for the column sums of this file's case table.
# measure_sum_constant() (float32 NumPy: sequential, reversed, and 64 / 256 strided per-thread partials folded in
# order, over the dz, dz*xhat, act_bwd, colstats and GAP terms of every case below) gives 2.2329 as the worst
# ratio; allowed: 4 x that.  tests/test_layers_oracle.py re-measures it and asserts 4 * measured <= SUM_C <= 4.2 *
# measured.
SUM_C_MEASURED = 2.2329
SUM_C = 4 * SUM_C_MEASURED

_ROUND = [True]


@contextmanager
def no_rounding():
    """Inside: bf16_round / f32_round are the identity (the oracle becomes the plain float64 operation that torch's
    float64 autograd computes)."""
    _ROUND[0] = False
    try:
        yield
    finally:
        _ROUND[0] = True


def bf16_round(x, force=False):
    """float64 -> nearest bfloat16 (ties to even), as float64; subnormals (spacing 2^-133), +-0, inf and nan kept."""
    x = np.asarray(x, dtype=np.float64)
    if not (_ROUND[0] or force):
        return x.copy()
    fin = np.isfinite(x)
    ax = np.where(fin, np.abs(x), 1.0)
    _, e = np.frexp(ax)                        # ax = m * 2^e, m in [0.5, 1): floor(log2 ax) = e - 1
    q = np.ldexp(1.0, np.maximum(e - 1, -126) - 7)   # spacing of bf16 in that binade
    r = np.rint(x / q) * q                     # x / q is exact (power of two); rint is half-to-even
    big = (2.0 - 2.0 ** -7) * 2.0 ** 127
    r = np.where(np.abs(r) > big, np.copysign(np.inf, x), r)
    return np.where(fin, r, x)


def f32_round(x):
    x = np.asarray(x, dtype=np.float64)
    return x.astype(np.float32).astype(np.float64) if _ROUND[0] else x.copy()


def store_bound(ref, fp32_term=0.0):
    """|bf16(v32) - ref| for v32 within fp32_term of ref."""
    return HB * np.abs(ref) + BF16_TINY + (1 + HB) * np.asarray(fp32_term, dtype=np.float64)


def sum_bound(abs_terms_sum, R, k_term, det=False):
    """det: the deterministic-mode reductions accumulate in float64 in a fixed order (R * 2^-53) and store one fp32
    value per slot (1 more rounding): no order term."""
    if det:
        return (U * (k_term + 1) + R * 2.0 ** -53) * abs_terms_sum
    return U * (SUM_C * np.sqrt(R) + k_term) * abs_terms_sum


# ----------------------------------------------------------------------------------------------- column statistics
def colstats(x, C=None, det=False):
    """x [R, ld] of stored bf16 values: the first C columns of every row count, the row stride is ld >= C.
    ref [2, C]: sum, sum of squares.  v*v of a bf16 v is exact in fp32 (16-bit product), so both are pure sums:
    per-block fp32 partials met by f64 atomics (SUM_C over the rows), or f64 throughout in deterministic mode
    (R * 2^-53)."""
    R = x.shape[0]
    C = x.shape[1] if C is None else C
    v = x[:, :C]
    ref = np.stack([v.sum(0), (v * v).sum(0)])
    mag = np.stack([np.abs(v).sum(0), (v * v).sum(0)])
    bound = mag * (R * 2.0 ** -53) if det else sum_bound(mag, R, 0)
    return ref, bound


def stats_slots(ref, C):
    """The [slots][2][C] f64 buffer the kernels read, all of it in slot 0."""
    st = np.zeros((STAT_SLOTS, 2, C))
    st[0] = ref
    return st


# ----------------------------------------------------------------------------------------------- BatchNorm forward
def bn_fwd(y, *, mode, stats=None, gamma=None, beta=None, eps=1e-3, mmean=None, mvar=None, momentum=0.99, bessel=1.0,
           res=None, relu=False, keep=None, drop_rate=0.0):
    """out = bf16(relu(y*scale + shift + res) * keep), scale = gamma*rstd, shift = beta - mean*scale.
    mode 0: scale 1, shift 0; 1: mean / var from the f64 slots ``stats`` [slots, 2, C] (summed in slot order, mean
    and var = max(E[y^2] - mean^2, 0) cast to fp32 as the kernel does); 2: moving statistics.  ``keep`` is the
    dropout mask (0 / 1), the kernel's keep-scale is fp32(1 / fp32(1 - rate)).
    Returns a dict: out, saved_mean, saved_rstd, mmean, mvar -> (ref, bound); out also carries ``ambiguous`` (ReLU
    decision within z's fp32 term) as third entry; "z" / "dz_term" are the pre-ReLU value and its fp32 term.
    k: K_BN_FWD roundings on z (listed at the constant), K_BN_DROP more with dropout, K_BN_MOV for the moving
    averages; rstd: var+eps 1, rsqrtf 2, and the f64 cancellation of E[y^2] - mean^2 (4 * 2^-53 * E[y^2])."""
    R, C = y.shape
    gamma = np.ones(C) if gamma is None else np.asarray(gamma, np.float64)
    beta = np.zeros(C) if beta is None else np.asarray(beta, np.float64)
    out = {}
    if mode == 0:
        scale, shift, mean = np.ones(C), np.zeros(C), np.zeros(C)
    else:
        if mode == 1:
            s = np.zeros((2, C))
            for sl in range(STAT_SLOTS):
                s = s + stats[sl]
            md = s[0] / R
            ey2 = s[1] / R
            mean = f32_round(md)
            var = f32_round(np.maximum(ey2 - md * md, 0.0))
        else:
            mean, var, ey2 = np.asarray(mmean, np.float64), np.asarray(mvar, np.float64), None
        ve = var + float(np.float32(eps))
        rstd = 1.0 / np.sqrt(ve)
        scale = gamma * rstd
        shift = beta - mean * scale
        if mode == 1:
            out["saved_mean"] = (mean, U * np.abs(mean) + 4 * 2.0 ** -53 * np.abs(md))
            cancel = 4 * 2.0 ** -53 * ey2 + U * var
            out["saved_rstd"] = (rstd, rstd * (3 * U + 0.5 * cancel / ve))
            if mmean is not None:
                m32 = float(np.float32(momentum))
                one_m = float(np.float32(1.0) - np.float32(momentum))
                b32 = float(np.float32(bessel))
                t0, t1 = np.asarray(mmean, np.float64) * m32, mean * one_m
                out["mmean"] = (t0 + t1, U * K_BN_MOV * (np.abs(t0) + np.abs(t1)))
                t0, t1 = np.asarray(mvar, np.float64) * m32, var * b32 * one_m
                out["mvar"] = (t0 + t1, U * K_BN_MOV * (np.abs(t0) + np.abs(t1)) + b32 * one_m * cancel)
    z = y * scale + shift
    terms = np.abs(y * scale) + np.abs(mean * scale) + np.abs(beta)
    if res is not None:
        z = z + res
        terms = terms + np.abs(res)
    dz_term = U * K_BN_FWD * terms
    if mode == 0:   # scale 1, shift 0: z = y + res is ONE rounding, relative to z itself (an exact 0 stays 0)
        dz_term = U * np.abs(z)
    if mode == 1:   # rstd's own cancellation noise, relative, on the two scale terms
        dz_term = dz_term + (np.abs(y * scale) + np.abs(mean * scale)) * (0.5 * cancel / ve)
    amb = np.zeros(y.shape, dtype=bool)
    o = z
    if relu:
        amb = np.abs(z) < dz_term if mode == 0 else np.abs(z) <= dz_term
        o = np.maximum(z, 0.0)
    term = dz_term
    if keep is not None:
        ks = np.asarray(keep, np.float64)
        if _ROUND[0]:
            ks = ks * float(np.float32(1.0) / (np.float32(1.0) - np.float32(drop_rate)))
        else:
            ks = ks / (1.0 - drop_rate)
        o = o * ks
        term = (dz_term + U * K_BN_DROP * np.abs(z)) * ks
    out["out"] = (o, store_bound(o, term), amb)
    out["z"] = z
    out["dz_term"] = dz_term
    return out


# ----------------------------------------------------------------------------------------------- BatchNorm backward
def bn_bwd(dout, y, *, mode, mean=None, rstd=None, gamma=None, beta=None, res=None, relu=False, keep=None,
           drop_rate=0.0, dx_prev=None, dres_prev=None, dgamma_prev=None, dbeta_prev=None, want_dres=True,
           extra_ambiguous=None, det=False):
    """dz = dout * keep * (z > 0), z = y*sc + sf + res recomputed from the SAVED mean / rstd (fp32 values, the
    kernel's own: bn_fwd's are checked on their own); xhat = (y - mean) * rstd;
    dbeta += sum dz; dgamma += sum dz*xhat; dx (+)= sc * (dz - mean(dz) - xhat * mean(dz*xhat)); dres (+)= dz.
    mode 0: dx = dz, no sums.  Returns dx, dres, dgamma, dbeta -> (ref, bound[, ambiguous]).
    k: K_BN_BWD_Z on z (ambiguous where |z| is within it), K_BN_TERM per summed term, SUM_C * sqrt(R) for the order
    of the R-row fp32 sums, K_BN_SLOTS for the slot adds, K_BN_DX on dx; the sums' own bound (and every ambiguous
    element's |term|, which may or may not be in the kernel's sum) carries into dx through mean(dz), mean(dz*xhat).
    dres without accumulate or dropout stores a value that already is bf16: bound 0.
    det: bn_bwd_reduce_det_kernel sums the fp32 terms in float64, rows in a fixed order, and stores one fp32 value per
    slot: the order term SUM_C * sqrt(R) is replaced by that one rounding (sum_bound(det=True))."""
    R, C = y.shape
    gamma = np.ones(C) if gamma is None else np.asarray(gamma, np.float64)
    beta = np.zeros(C) if beta is None else np.asarray(beta, np.float64)
    if mode == 1:
        mean, rstd = np.asarray(mean, np.float64), np.asarray(rstd, np.float64)
        sc = gamma * rstd
        sf = beta - mean * gamma * rstd
    else:
        mean, rstd, sc, sf = np.zeros(C), np.ones(C), np.ones(C), np.zeros(C)
    z = y * sc + sf
    terms = np.abs(y * sc) + np.abs(mean * sc) + np.abs(beta)
    if res is not None:
        z = z + res
        terms = terms + np.abs(res)
    amb = np.zeros(y.shape, dtype=bool)
    g = np.asarray(dout, np.float64).copy()
    gerr = np.zeros(y.shape)
    if keep is not None:
        inv = float(np.float32(1.0) / (np.float32(1.0) - np.float32(drop_rate))) if _ROUND[0] else 1 / (1 - drop_rate)
        g = g * np.asarray(keep, np.float64) * inv
        gerr = U * K_BN_DROP * np.abs(g)
    if relu:
        # mode 0: z = y + res, one rounding relative to z itself: never ambiguous, and z == 0 exactly masks
        amb = np.abs(z) <= U * K_BN_BWD_Z * terms if mode == 1 else np.zeros(y.shape, dtype=bool)
        g = np.where(z > 0, g, 0.0)
        gerr = np.where(z > 0, gerr, 0.0)
    if extra_ambiguous is not None:
        amb = amb | extra_ambiguous
    dz = g
    out = {}
    if dres_prev is not None:
        r = dz + dres_prev
        out["dres"] = (r, store_bound(r, gerr + U * np.abs(r)), amb)
    elif want_dres:
        out["dres"] = (dz, store_bound(dz, gerr) if keep is not None else np.zeros(y.shape), amb)
    if mode != 1:
        dx = dz
        dxerr = gerr
    else:
        xh = (y - mean) * rstd
        t2 = dz * xh
        amb_g = np.where(amb, np.abs(dout), 0.0)
        a1, a2 = np.abs(dz).sum(0), np.abs(t2).sum(0)
        e1 = sum_bound(a1, R, K_BN_TERM + K_BN_SLOTS, det) + amb_g.sum(0) * (1 + 2 * drop_rate / max(1 - drop_rate, 0.5))
        e2 = sum_bound(a2, R, K_BN_TERM + K_BN_SLOTS, det) + (amb_g * np.abs(xh)).sum(0) * (1 + 2 * drop_rate / max(1 - drop_rate, 0.5))
        s1, s2 = dz.sum(0), t2.sum(0)
        db0 = np.zeros(C) if dbeta_prev is None else np.asarray(dbeta_prev, np.float64)
        dg0 = np.zeros(C) if dgamma_prev is None else np.asarray(dgamma_prev, np.float64)
        out["dbeta"] = (s1 + db0, e1 + U * (np.abs(s1) + np.abs(db0)))
        out["dgamma"] = (s2 + dg0, e2 + U * (np.abs(s2) + np.abs(dg0)))
        k1, k2 = s1 / R, s2 / R
        dx = sc * (dz - k1 - xh * k2)
        mag = np.abs(sc) * (np.abs(dz) + np.abs(k1) + np.abs(xh * k2))
        dxerr = np.abs(sc) * (gerr + e1 / R + np.abs(xh) * e2 / R) + U * K_BN_DX * mag
    if dx_prev is not None:
        dx = dx + dx_prev
        dxerr = dxerr + U * np.abs(dx)
    out["dx"] = (dx, store_bound(dx, dxerr), amb)
    return out


# ----------------------------------------------------------------------------------------------- act_bwd
def act_bwd(dout, outv, relu, dbias_prev=None, det=False):
    """dz = dout * (out > 0) (a bf16 value stored as bf16: exact), dbias += sum over rows of dz (fp32, SUM_C).
    det: colsum_det_kernel adds the rows r, r + 4, ... of each of 4 lanes in order in fp32, folds the lanes with 2
    more adds and adds the result to dbias: a fixed order of ceil(R/4) + 2 roundings on any path, so the worst-case
    bound of sequential summation, u * (ceil(R/4) + 2) * sum|terms|, replaces the measured order term."""
    R, C = dout.shape
    dz = np.where(outv > 0, dout, 0.0) if relu else np.asarray(dout, np.float64).copy()
    s = dz.sum(0)
    p = np.zeros(C) if dbias_prev is None else np.asarray(dbias_prev, np.float64)
    return {"dz": (dz, np.zeros(dz.shape)),
            "dbias": (s + p, (U * (-(-R // 4) + 2) * np.abs(dz).sum(0) if det else sum_bound(np.abs(dz).sum(0), R, 2))
                      + U * (np.abs(s) + np.abs(p)))}


# ----------------------------------------------------------------------------------------------- max pooling
Geo = namedtuple("Geo", "B H W C Ho Wo KH KW sh sw pt pl")


def pool_geo(B, H, W, C, k, s, pad):
    if pad == "same":
        Ho, Wo = -(-H // s), -(-W // s)
        pt = max((Ho - 1) * s + k - H, 0) // 2
        pl = max((Wo - 1) * s + k - W, 0) // 2
    else:
        Ho, Wo, pt, pl = (H - k) // s + 1, (W - k) // s + 1, 0, 0
    return Geo(B, H, W, C, Ho, Wo, k, k, s, s, pt, pl)


def _taps(g):
    """(window byte, output rows, input rows, output cols, input cols) of every tap with an in-bounds pixel."""
    for i in range(g.KH):
        ih = np.arange(g.Ho) * g.sh - g.pt + i
        vh = (ih >= 0) & (ih < g.H)
        for j in range(g.KW):
            iw = np.arange(g.Wo) * g.sw - g.pl + j
            vw = (iw >= 0) & (iw < g.W)
            if vh.any() and vw.any():
                yield i * g.KW + j, np.nonzero(vh)[0], ih[vh], np.nonzero(vw)[0], iw[vw]


def maxpool_fwd(x, g):
    """value and argmax byte i*KW + j of every window: the FIRST maximum in row-major window order over in-bounds
    taps only (strict >, byte 0 when nothing is greater than -inf).  Exact: bound 0."""
    best = np.full((g.B, g.Ho, g.Wo, g.C), -np.inf)
    idx = np.zeros((g.B, g.Ho, g.Wo, g.C), dtype=np.uint8)
    for w, oh, ih, ow, iw in _taps(g):
        cand = x[:, ih[:, None], iw[None, :], :]
        cur = best[:, oh[:, None], ow[None, :], :]
        upd = cand > cur
        best[:, oh[:, None], ow[None, :], :] = np.where(upd, cand, cur)
        ci = idx[:, oh[:, None], ow[None, :], :]
        idx[:, oh[:, None], ow[None, :], :] = np.where(upd, np.uint8(w), ci)
    return {"y": (best, np.zeros(best.shape)), "idx": (idx, np.zeros(idx.shape))}


def maxpool_bwd(dy, idx, g, prev=None):
    """dx[pixel] (+)= sum of dy over the windows whose argmax byte names that pixel (<= 9 fp32 adds, then the bf16
    store).  Where the exact sum is a bf16 value the result is exact (partial sums of grid values are exact in
    fp32): bound 0 there; elsewhere 2^-8 |ref| + 10 u sum|terms|."""
    dx = np.zeros((g.B, g.H, g.W, g.C))
    mag = np.zeros((g.B, g.H, g.W, g.C))
    for w, oh, ih, ow, iw in _taps(g):
        d = np.where(idx[:, oh[:, None], ow[None, :], :] == w, dy[:, oh[:, None], ow[None, :], :], 0.0)
        dx[:, ih[:, None], iw[None, :], :] += d
        mag[:, ih[:, None], iw[None, :], :] += np.abs(d)
    if prev is not None:
        dx = dx + prev
        mag = mag + np.abs(prev)
    exact = bf16_round(dx, force=True) == dx
    return dx, np.where(exact, 0.0, store_bound(dx, 10 * U * mag))


def bn_relu_maxpool_fwd(y, g, **bn):
    """maxpool_fwd over bf16(relu(bn(y))): the fused kernel rounds every candidate to bf16 before the max, so value
    and argmax are exact wherever every candidate's rounded value is certain.  ``ambiguous`` (per window): the
    winner or its value changes between all candidates moved down and all moved up by their fp32 term (rounding is
    monotonic, so in between nothing else can happen).  Returns the bn_fwd dict plus y, idx -> (ref, 0, ambiguous)."""
    f = bn_fwd(y.reshape(-1, g.C), relu=True, **bn)
    z, t = f["z"], f["dz_term"]
    shp = (g.B, g.H, g.W, g.C)
    mid = maxpool_fwd(bf16_round(np.maximum(z, 0)).reshape(shp), g)
    lo = maxpool_fwd(bf16_round(np.maximum(z - t, 0)).reshape(shp), g)
    hi = maxpool_fwd(bf16_round(np.maximum(z + t, 0)).reshape(shp), g)
    amb = (lo["idx"][0] != hi["idx"][0]) | (lo["y"][0] != hi["y"][0])
    f["y"] = (mid["y"][0], np.zeros(amb.shape), amb)
    f["idx"] = (mid["idx"][0], np.zeros(amb.shape), amb)
    return f


def bn_pool_bwd(dpool, idx, y, g, *, mean, rstd, gamma=None, beta=None, dx_prev=None, dgamma_prev=None,
                dbeta_prev=None, idx_ambiguous=None):
    """bn_bwd (batch statistics, ReLU) whose output gradient is bf16(maxpool_bwd(dpool, idx)), the value the pool
    backward would have stored.  idx: the kernel's own argmax bytes; windows that were ambiguous in the forward
    make every pixel they cover ambiguous here."""
    d, db = maxpool_bwd(dpool, idx, g)
    extra = None
    if idx_ambiguous is not None and idx_ambiguous.any():
        cov = np.zeros((g.B, g.H, g.W, g.C))
        for w, oh, ih, ow, iw in _taps(g):
            cov[:, ih[:, None], iw[None, :], :] += idx_ambiguous[:, oh[:, None], ow[None, :], :]
        extra = (cov > 0).reshape(-1, g.C)
    out = bn_bwd(bf16_round(d).reshape(-1, g.C), y.reshape(-1, g.C), mode=1, mean=mean, rstd=rstd, gamma=gamma,
                 beta=beta, relu=True, dx_prev=None if dx_prev is None else dx_prev.reshape(-1, g.C),
                 dgamma_prev=dgamma_prev, dbeta_prev=dbeta_prev, want_dres=False, extra_ambiguous=extra)
    out["gather_exact"] = bool((db == 0).all())
    return out


# ----------------------------------------------------------------------------------------------- GAP, pad, cast
def gap_fwd(x):
    """x [B, HW, C] -> mean over HW: an fp32 sum (sequential, or 32 strided partials folded in order: SUM_C), then
    * fp32(1/HW) and the bf16 store (K_GAP)."""
    B, HW, C = x.shape
    ref = x.sum(1) / HW
    mag = np.abs(x).sum(1) / HW
    return ref, store_bound(ref, sum_bound(mag, HW, K_GAP))


def gap_bwd(dy, HW, prev=None):
    """dx[b, p, c] (+)= dy[b, c] * fp32(1/HW); K_GAP roundings."""
    ref = np.repeat(dy[:, None, :], HW, axis=1) / HW
    mag = np.abs(ref)
    if prev is not None:
        ref = ref + prev
        mag = mag + np.abs(prev)
    return ref, store_bound(ref, U * K_GAP * mag)


def pad_fwd(x, pt, pb, pl, pr):
    ref = np.pad(x, ((0, 0), (pt, pb), (pl, pr), (0, 0)))
    return ref, np.zeros(ref.shape)


def pad_bwd(dy, pt, pl, H, W, prev=None):
    """crop; with accumulate one fp32 add and the bf16 store (bound 0 where the sum is a bf16 value)."""
    ref = dy[:, pt:pt + H, pl:pl + W, :].copy()
    if prev is None:
        return ref, np.zeros(ref.shape)
    ref = ref + prev
    exact = bf16_round(ref, force=True) == ref
    return ref, np.where(exact, 0.0, store_bound(ref, U * np.abs(ref)))


def cast_bf16(x32):
    """fp32 -> bf16, round to nearest even: exact."""
    ref = bf16_round(np.asarray(x32, np.float32).astype(np.float64), force=True)
    return ref, np.zeros(ref.shape)


# ----------------------------------------------------------------------------------------------- cross-entropy
def xent(logits, labels, scale=1.0, metrics_prev=None):
    """Softmax cross-entropy of fp32 logits [B, C], one row per wave: mx = max, d = x - mx, e = __expf(d),
    se = sum e, p = e / se, loss = mx + __logf(se) - x[label], correct = (first index of the max == label),
    dlogits = bf16(scale * (p - onehot)).  Returns loss (sum), correct, count, probs, dlogits -> (ref, bound).
    Roundings: d 1 (absolute u |d|, which the exponential turns into a relative u |d|); __expf = exp2(d * log2e):
    the product's rounding is relative u |d| again, v_exp_f32 1 ulp = 2 -> rel(e) = u (2 |d| + 3).
    se: its terms' errors weighted by p (u (2 D + 3), D = sum p |d|) plus the order of the sum: <= 24 adds per lane
    and 6 butterfly steps -> rel(se) = u (2 D + 33).  p: rel(e) + rel(se) + 1/se 2 + product 1.
    dlogits: p's error, the subtraction and the scaling 2 u |p - onehot|, times |scale|, then the bf16 store.
    loss per row: __logf = v_log_f32 * ln2: 3 u |log se| + rel(se); the add and the subtraction u (|lse| + |loss|);
    the sum over rows (4 per block, then atomics) u (B/4 + 4) sum|loss|.
    fp32 subnormals: v_exp_f32 and the products that follow may flush a result below 2^-126 to zero, so e, and with
    se >= 1 also p = e / se, carry an absolute 2^-126 each (probs 2 * 2^-126; dlogits that times |scale| and one
    more for its own product; se C * 2^-126)."""
    x = np.asarray(logits, np.float64)
    B, C = x.shape
    mx = x.max(1, keepdims=True)
    d = x - mx
    e = np.exp(d)
    se = e.sum(1, keepdims=True)
    p = e / se
    D = (p * np.abs(d)).sum(1, keepdims=True)
    rel_se = U * (2 * D + 33) + C * FLT_MIN / se
    rel_p = U * (2 * np.abs(d) + 3) + rel_se + 3 * U
    onehot = np.zeros((B, C))
    lab = np.asarray(labels)
    onehot[np.arange(B), lab] = 1.0
    lse = mx[:, 0] + np.log(se[:, 0])
    loss = lse - x[np.arange(B), lab]
    eloss = (3 * U * np.abs(np.log(se[:, 0])) + rel_se[:, 0] + U * (np.abs(lse) + np.abs(loss)) + U * np.abs(mx[:, 0]))
    am = x.argmax(1)                 # NumPy: first index of the maximum, the kernel's rule
    m0 = np.zeros(3) if metrics_prev is None else np.asarray(metrics_prev, np.float64)
    dl = float(np.float32(scale)) * (p - onehot)
    edl = abs(scale) * (p * rel_p + 2 * U * np.abs(p - onehot)) + (2 * abs(scale) + 1) * FLT_MIN
    return {"loss": (loss.sum() + m0[0], eloss.sum() + U * (B / 4 + 4) * np.abs(loss).sum() + U * abs(m0[0])),
            "correct": (float((am == lab).sum()) + m0[1], 0.0),
            "count": (float(B) + m0[2], 0.0),
            "probs": (p, p * rel_p + 2 * FLT_MIN),
            "dlogits": (dl, store_bound(dl, edl))}


# ----------------------------------------------------------------------------------------------- inputs
def grid(rng, shape, step, lim):
    """multiples of ``step`` in [-lim, lim], uniformly."""
    n = int(round(lim / step))
    return rng.integers(-n, n + 1, size=shape).astype(np.float64) * step


def normal_bf16(rng, shape, scale=1.0, shift=0.0):
    return bf16_round(rng.standard_normal(shape) * scale + shift, force=True)


def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


# ----------------------------------------------------------------------------------------------- BatchNorm cases
def bn_tiled(C):
    """tde_bn_fwd / tde_bn_bwd: channel-tiled kernels (torch allocations are 16-byte aligned)."""
    return C % 8 == 0 and (C <= 64 or C % 64 == 0)


def bn_fwd_path(R, C):
    if bn_tiled(C):
        return "tiled"
    return "flat_vec" if (R * C) % 8 == 0 else "flat_scalar"


def bn_tiled_loops(R, C, blocks_div, lo, hi):
    """bn_tiled_grid: does the row loop of a thread iterate (more row blocks needed than launched)?"""
    cg = min(C, 64)
    rp, ng = 256 // (cg // 8), C // cg
    blocks = min(max(R * C // blocks_div, lo), hi)
    return -(-R // rp) > -(-blocks // ng)


def bn_reduce_path(R, C, mode, drop, det=False):
    if mode != 1:
        return None
    if det:
        return "det"
    if bn_tiled(C):
        return "tiled"
    if C > 16 and R <= 1024:
        return "cols"
    if C <= 16 and drop == 0:
        return "rows8" if C <= 8 else "rows16"
    return "generic"


BnCase = namedtuple("BnCase", "id R C mode relu res drop bessel accum const_col fwd reduce det seed zeros")


def _bn(id, R, C, fwd, reduce, mode=1, relu=True, res=False, drop=0.0, bessel=False, accum=False, const_col=False,
        det=False, seed=0, zeros=False):
    return BnCase(id, R, C, mode, relu, res, drop, bessel, accum, const_col, fwd, reduce, det, seed, zeros)


BN_CASES = [
    _bn("flat_scalar_tail-rows8-5x6", 5, 6, "flat_scalar", "rows8", seed=1),
    _bn("flat_vec-cols-50x200", 50, 200, "flat_vec", "cols", res=True, bessel=True, seed=2),
    _bn("flat_vec-cols-17x72-norelu", 17, 72, "flat_vec", "cols", relu=False, accum=True, seed=3),
    _bn("tiled-50x24-constcol", 50, 24, "tiled", "tiled", const_col=True, bessel=True, seed=4),
    _bn("tiled-200x40-res", 200, 40, "tiled", "tiled", res=True, accum=True, seed=5),
    _bn("tiled-100x56-norelu", 100, 56, "tiled", "tiled", relu=False, res=True, seed=6),
    _bn("tiled-130x128", 130, 128, "tiled", "tiled", bessel=True, seed=7),
    _bn("tiled_loop-2050x512", 2050, 512, "tiled", "tiled", res=True, bessel=True, seed=8),
    _bn("degenerate-R1-tiled-1x40", 1, 40, "tiled", "tiled", seed=9),
    _bn("degenerate-R1-flat-1x6", 1, 6, "flat_scalar", "rows8", res=True, seed=10),
    _bn("rows8-300x6", 300, 6, "flat_vec", "rows8", bessel=True, seed=11),
    _bn("rows16-300x12", 300, 12, "flat_vec", "rows16", res=True, accum=True, seed=12),
    _bn("generic-1030x72", 1030, 72, "flat_vec", "generic", res=True, seed=13),
    _bn("generic-dropout-64x12", 64, 12, "flat_vec", "generic", drop=0.3, seed=14),
    _bn("mode0-flat-50x200", 50, 200, "flat_vec", None, mode=0, res=True, accum=True, seed=15),
    _bn("mode0-tiled-130x128-norelu", 130, 128, "tiled", None, mode=0, relu=False, res=True, seed=16),
    # y and res on the 0.5 grid: y + res is exactly 0 on about a ninth of the elements, where the gradient is masked
    _bn("mode0-exact-zero-flat-50x200", 50, 200, "flat_vec", None, mode=0, res=True, zeros=True, seed=23),
    _bn("mode0-exact-zero-tiled-130x128", 130, 128, "tiled", None, mode=0, res=True, zeros=True, seed=24),
    _bn("mode2-flat-17x72", 17, 72, "flat_vec", None, mode=2, seed=17),
    _bn("mode2-tiled-50x24", 50, 24, "tiled", None, mode=2, res=True, seed=18),
    # deterministic mode: bn_bwd_reduce_det_kernel + colstats_det_kernel, flat and tiled apply passes
    _bn("det-flat-50x200", 50, 200, "flat_vec", "det", res=True, det=True, seed=19),
    _bn("det-flat_tail-5x6", 5, 6, "flat_scalar", "det", det=True, seed=20),
    _bn("det-tiled-200x40", 200, 40, "tiled", "det", res=True, accum=True, det=True, seed=21),
    _bn("det-tiled-130x128", 130, 128, "tiled", "det", det=True, seed=22),
]


def bn_inputs(c):
    rng = np.random.default_rng(1000 + c.seed)
    y = normal_bf16(rng, (c.R, c.C), 2.0, 0.5)
    if c.const_col:
        y[:, 1] = 1.5
    if c.zeros:
        y = grid(rng, (c.R, c.C), 0.5, 2.0)
    res = grid(rng, (c.R, c.C), 0.5, 2.0) if c.zeros else (normal_bf16(rng, (c.R, c.C)) if c.res else None)
    d = {"y": y, "res": res,
         "gamma": f32(rng.random(c.C) + 0.5), "beta": f32(rng.standard_normal(c.C) * 0.1),
         "dout": normal_bf16(rng, (c.R, c.C)), "mmean": f32(rng.standard_normal(c.C) * 0.2),
         "mvar": f32(rng.random(c.C) + 0.5), "bessel": c.R / (c.R - 1.0) if (c.bessel and c.R > 1) else 1.0,
         "dx_prev": normal_bf16(rng, (c.R, c.C)) if c.accum else None,
         "dres_prev": normal_bf16(rng, (c.R, c.C)) if (c.accum and c.res) else None,
         "dgamma_prev": f32(rng.standard_normal(c.C)), "dbeta_prev": f32(rng.standard_normal(c.C)),
         "keep": (rng.random((c.R, c.C)) < 0.7) if c.drop else None}
    return d


def bn_oracle(c, inp, stats=None, saved=None, keep=None):
    """Forward and backward oracle of one case; ``stats`` / ``saved`` / ``keep`` default to the oracle's own (the GPU
    test passes the kernel's: its slots, its saved mean / rstd, its dropout mask)."""
    if stats is None:
        stats = stats_slots(colstats(inp["y"])[0], c.C)
    keep = inp["keep"] if keep is None else keep
    f = bn_fwd(inp["y"], mode=c.mode, stats=stats, gamma=inp["gamma"], beta=inp["beta"], eps=1e-3,
               mmean=inp["mmean"], mvar=inp["mvar"], momentum=0.9, bessel=inp["bessel"], res=inp["res"], relu=c.relu,
               keep=keep, drop_rate=c.drop)
    b = None
    if c.mode != 2:
        mean, rstd = (None, None)
        if c.mode == 1:
            mean, rstd = saved if saved is not None else (f32_round(f["saved_mean"][0]), f32_round(f["saved_rstd"][0]))
        b = bn_bwd(inp["dout"], inp["y"], mode=c.mode, mean=mean, rstd=rstd, gamma=inp["gamma"], beta=inp["beta"],
                   res=inp["res"], relu=c.relu, keep=keep, drop_rate=c.drop, dx_prev=inp["dx_prev"],
                   dres_prev=inp["dres_prev"], dgamma_prev=inp["dgamma_prev"], dbeta_prev=inp["dbeta_prev"],
                   want_dres=c.res, det=c.det)
    return f, b


# ----------------------------------------------------------------------------------------------- pooling cases
def pool_fwd_path(g):
    return "fwd8" if g.C % 8 == 0 else "fwd"


def pool_bwd_path(g):
    """tde_maxpool's backward dispatch."""
    if g.C % 8:
        return "bwd"
    if -(-g.KH // g.sh) <= 2 and -(-g.KW // g.sw) <= 2 and g.KH * g.KW < 255 and g.B * g.H <= 65535:
        return "w2p" if (g.KW + g.sw) // g.sw <= 2 else "w2"
    return "bwd8"


PoolCase = namedtuple("PoolCase", "id geo bwd")
POOL_CASES = [PoolCase(i, pool_geo(*g), p) for i, g, p in [
    ("scalar-C6", (2, 9, 7, 6, 3, 2, "same"), "bwd"),
    ("fwd8-bwd8-3x3s1", (2, 11, 10, 8, 3, 1, "same"), "bwd8"),
    ("w2-2x2s1-valid", (2, 9, 8, 16, 2, 1, "valid"), "w2"),
    ("w2-4x4s2-same", (2, 10, 9, 8, 4, 2, "same"), "w2"),
    ("w2p-3x3s2-W8-pl0", (2, 8, 8, 8, 3, 2, "same"), "w2p"),
    ("w2p-3x3s2-W9-pl1", (2, 9, 9, 16, 3, 2, "same"), "w2p"),
    ("w2p-3x3s2-W7-pl1", (2, 7, 7, 8, 3, 2, "same"), "w2p"),
    ("w2p-3x3s2-W6-pl0", (2, 6, 6, 24, 3, 2, "same"), "w2p"),
    ("w2p-2x2s2-valid", (2, 26, 26, 32, 2, 2, "valid"), "w2p"),
    # odd W with pl = 0: the last thread owns one column while tx0 is even; even W with pl = 1
    ("w2p-2x2s2-same-W9-pl0", (2, 9, 9, 8, 2, 2, "same"), "w2p"),
    ("w2p-3x3s2-valid-W9-pl0", (2, 9, 9, 16, 3, 2, "valid"), "w2p"),
    ("w2p-3x3s3-same-W10-pl1", (2, 10, 10, 8, 3, 3, "same"), "w2p"),
    ("w2p-W1", (3, 5, 1, 8, 3, 2, "same"), "w2p"),
    ("w2p-H1", (3, 1, 5, 8, 3, 2, "same"), "w2p"),
    ("w2p-W2", (3, 4, 2, 8, 3, 2, "same"), "w2p"),
    ("bwd8-W1-3x3s1", (2, 4, 1, 8, 3, 1, "same"), "bwd8"),
    ("w2p-many-blocks-112", (1, 112, 112, 64, 3, 2, "same"), "w2p"),
    ("bwd8-BH65536-fallback", (8192, 8, 2, 8, 3, 2, "same"), "bwd8"),
]]


def pool_inputs(g, seed):
    """x on a 9-value grid (multiples of 0.5 in [-2, 2]: most windows tie); dy and the accumulate base multiples of
    1/8 in [-2, 2]: every sum of <= 9 + 1 of them is exact in fp32 and in bf16 (|sum| <= 20 = 160 eighths < 2^8)."""
    rng = np.random.default_rng(2000 + seed)
    return (grid(rng, (g.B, g.H, g.W, g.C), 0.5, 2.0), grid(rng, (g.B, g.Ho, g.Wo, g.C), 0.125, 2.0),
            grid(rng, (g.B, g.H, g.W, g.C), 0.125, 2.0))


FusedCase = namedtuple("FusedCase", "id geo mode beta_shift accum seed")
FUSED_CASES = [FusedCase(i, pool_geo(*g), m, bs, a, s) for i, g, m, bs, a, s in [
    ("C8-3x3s2", (3, 15, 4, 8, 3, 2, "same"), 1, 0.0, False, 1),
    ("C16-3x3s2-odd", (3, 15, 13, 16, 3, 2, "same"), 1, 0.0, True, 2),
    ("C64-3x3s2", (2, 16, 16, 64, 3, 2, "same"), 1, 0.0, False, 3),
    ("C512-2x2s2-valid", (2, 6, 8, 512, 2, 2, "valid"), 1, 0.0, False, 4),
    ("BH1040-capped-reduce-grid", (65, 16, 4, 8, 3, 2, "same"), 1, 0.0, False, 5),
    ("negative-beta-zero-ties", (2, 16, 16, 16, 3, 2, "same"), 1, -1.2, True, 6),
    ("mode2-C64", (2, 16, 16, 64, 3, 2, "same"), 2, 0.0, False, 7),
]]


def fused_ok(g):
    """tde_bn_pool_bwd's host checks (layer_ops.bn_pool_ok)."""
    C8 = g.C // 8
    return (g.C % 8 == 0 and g.C <= 512 and 256 % C8 == 0 and -(-g.KH // g.sh) <= 2 and (g.KW + g.sw) // g.sw <= 2
            and g.Wo * g.C <= 4096 and (g.Wo * g.C) % 16 == 0)


def fused_inputs(c):
    g = c.geo
    rng = np.random.default_rng(3000 + c.seed)
    R = g.B * g.H * g.W
    return {"y": normal_bf16(rng, (R, g.C), 2.0, 0.2), "gamma": f32(rng.random(g.C) + 0.5),
            "beta": f32(rng.standard_normal(g.C) * 0.3 + c.beta_shift), "mmean": f32(np.full(g.C, 0.1)),
            "mvar": f32(np.full(g.C, 0.9)), "bessel": R / (R - 1.0),
            "dpool": grid(rng, (g.B, g.Ho, g.Wo, g.C), 0.125, 2.0),
            "dx_prev": normal_bf16(rng, (R, g.C)) if c.accum else None,
            "dgamma_prev": f32(rng.standard_normal(g.C)), "dbeta_prev": f32(rng.standard_normal(g.C))}


def fused_fwd_oracle(c, inp, stats=None):
    g = c.geo
    if stats is None:
        stats = stats_slots(colstats(inp["y"])[0], g.C)
    return bn_relu_maxpool_fwd(inp["y"], g, mode=c.mode, stats=stats, gamma=inp["gamma"], beta=inp["beta"], eps=1e-5,
                               mmean=inp["mmean"], mvar=inp["mvar"], momentum=0.9, bessel=inp["bessel"])


def fused_bwd_oracle(c, inp, idx, saved, idx_ambiguous):
    return bn_pool_bwd(inp["dpool"], idx, inp["y"], c.geo, mean=saved[0], rstd=saved[1], gamma=inp["gamma"],
                       beta=inp["beta"], dx_prev=inp["dx_prev"], dgamma_prev=inp["dgamma_prev"],
                       dbeta_prev=inp["dbeta_prev"], idx_ambiguous=idx_ambiguous)


# ----------------------------------------------------------------------------------------------- other cases
ACT_CASES = [(37, 10), (128, 200), (5, 1000)]
GAP_CASES = [("vec", 3, 49, 128), ("scalar", 2, 25, 40), ("HW1-vec", 4, 1, 64), ("HW1-scalar", 4, 1, 24)]
COLSTATS_CASES = [(50, 200), (300, 6), (2050, 512), (1, 40)]
def xent_path(C):
    """tde_xent: the register-resident form up to 64 * 16 classes, the per-pass form above."""
    return "xent<16>" if C <= 64 * 16 else "xent<0>"


XENT_C = [1, 10, 1000, 1024, 1025, 1500]
XENT_B = [1, 5, 37]


def act_inputs(R, C):
    rng = np.random.default_rng(4000 + R + C)
    out = np.maximum(normal_bf16(rng, (R, C)), 0.0)       # about half the elements are exactly 0
    return normal_bf16(rng, (R, C)), out, f32(rng.standard_normal(C))


def gap_inputs(B, HW, C):
    rng = np.random.default_rng(5000 + HW + C)
    return normal_bf16(rng, (B, HW, C), 1.0, 0.3), normal_bf16(rng, (B, C)), normal_bf16(rng, (B, HW, C))


def xent_inputs(B, C):
    """fp32 logits spanning +-80 (an unshifted exp overflows), labels at 0 and C-1, and rows whose maximum is
    duplicated with the label on its first / second occurrence."""
    rng = np.random.default_rng(6000 + 7 * B + C)
    x = f32(rng.standard_normal((B, C)) * 3)
    x[0] = f32(rng.uniform(-80, 80, C))
    lab = rng.integers(0, C, B)
    lab[0] = 0
    if B > 1:
        lab[1] = C - 1
    if B > 3 and C > 3:
        for r, which in ((2, 0), (3, 1)):
            a, b = sorted(rng.choice(C, 2, replace=False))
            x[r, a] = x[r, b] = x[r].max() + 1.0
            lab[r] = (a, b)[which]
    return x, lab.astype(np.int32)


# ----------------------------------------------------------------------------------------------- SUM_C measurement
def _sum_ratio(t):
    """worst |fp32 sum - exact| / (u sqrt(R) sum|t|) over the columns of t [R, n] in four summation orders."""
    R = t.shape[0]
    if R < 2:
        return 0.0
    t32 = t.astype(np.float32)
    exact = t32.astype(np.float64).sum(0)
    mag = np.abs(t32.astype(np.float64)).sum(0)
    sums = [np.cumsum(t32, 0, dtype=np.float32)[-1], np.cumsum(t32[::-1], 0, dtype=np.float32)[-1]]
    for T in (64, 256):   # per-thread strided partials (row r to thread r % T), folded in thread order
        pad = (-R) % T
        tp = np.concatenate([t32, np.zeros((pad,) + t32.shape[1:], np.float32)]).reshape(-1, T, *t32.shape[1:])
        part = np.cumsum(tp, 0, dtype=np.float32)[-1]
        sums.append(np.cumsum(part, 0, dtype=np.float32)[-1])
    worst = 0.0
    ok = mag > 0
    for s in sums:
        dev = np.abs(s.astype(np.float64) - exact)
        if ok.any():
            worst = max(worst, float((dev[ok] / (U * np.sqrt(R) * mag[ok])).max()))
    return worst


def measure_sum_constant():
    worst = 0.0
    for c in BN_CASES:
        if c.mode != 1:
            continue
        inp = bn_inputs(c)
        _, b = bn_oracle(c, inp)
        f = bn_fwd(inp["y"], mode=1, stats=stats_slots(colstats(inp["y"])[0], c.C), gamma=inp["gamma"],
                   beta=inp["beta"], res=inp["res"], relu=c.relu)
        dz = np.where(f["z"] > 0, inp["dout"], 0.0) if c.relu else inp["dout"]
        xh = (inp["y"] - f["saved_mean"][0]) * f["saved_rstd"][0]
        worst = max(worst, _sum_ratio(dz), _sum_ratio(dz * xh))
    for R, C in ACT_CASES:
        dout, out, _ = act_inputs(R, C)
        worst = max(worst, _sum_ratio(np.where(out > 0, dout, 0.0)))
    for R, C in COLSTATS_CASES:
        x = normal_bf16(np.random.default_rng(7000 + R), (R, C), 2.0, 0.5)
        worst = max(worst, _sum_ratio(x), _sum_ratio(x * x))
    for _, B, HW, C in GAP_CASES:
        x = gap_inputs(B, HW, C)[0]
        worst = max(worst, _sum_ratio(np.moveaxis(x, 1, 0).reshape(HW, -1)))
    return worst
