"""Float64 oracle of the fused classifier head (csrc/kernels/head.hip, tde_head_xent): every output the kernel can
produce from its arguments, a per-element float32 bound for each, the stored (bf16 / transposed) forms of the input
gradient, and the case table and seeded inputs that tests/test_head_oracle.py (CPU) and tests/test_head_gpu.py (GPU)
share.  Host only: NumPy and torch tensors on the CPU, plain formulas (no autograd: autograd checks them).

The operation:  h = hin + pre_bias, relu'd if pre_relu;  logits = h W2 + b2;  probs = softmax(logits);
row_loss = logsumexp(logits) - logits[label];  correct = #(first maximum == label);  count = B;
dlogits = scale (probs - onehot);  dW2 = h^T dlogits;  db2 = column sums of dlogits;
dH = dlogits W2^T masked by h > 0 (pre_relu);  dpre_bias = column sums of dH.

Bounds (u = 2^-24, one fp32 rounding; the convention of tests/layers_oracle.py: |got - ref| <= u k sum|terms| of the
element's own sum, k = the roundings on the longest path to it, first order):
  logits   k = Hp/4 + 4: a wave adds Hp/16 MFMA steps of 4 products each (Hp = H rounded up to 16), 3 adds fold the
           4 waves, 1 adds the bias.  EZ = the largest such bound of a row.
  probs    p_c = e_c / se: a logit error dz moves p_c by p_c (dz_c - sum p dz) -> 2 EZ relative; d = z - m one
           rounding, absolute u |d|, which the exponential makes relative; exp2(d log2e): the product's rounding is
           u |d| relative again, the exponential 1 ulp = 2 u -> rel(e) = u (2 |d| + 3); se: its terms' errors
           weighted by p, u (2 D + 3) with D = sum p |d|, and 4 butterfly adds; the division 2 u:
           rel(p) = 2 EZ + u (2 |d| + 2 D + 12), and 2 * 2^-126 absolute for results flushed to zero.
  row_loss log(se) 3 u |log se| (1 ulp, times ln 2) + rel(se); the add and the subtraction u (|lse| + |loss|); the
           maximum and the label's logit carry EZ each.
  loss_sum the rows' bounds, u (B/4 + 4) sum|loss| for the adds (4 rows per lane group, 4 groups, atomics per
           workgroup) and u |start| for the accumulate.
  dlogits  |scale| (p rel(p) + 2 u |p - onehot|): the subtraction and the scaling.
  dW2, db2, dpre_bias   the operands' own bounds times the other factor, plus u k sum|terms| with k = 16 (rows of a
           workgroup on the MFMA) + the workgroups (atomics) + 1 (the accumulate), |start| among the terms.
  dH       sum_c bound(dlogits) |W2| + 17 u sum|dlogits W2|; the ReLU decision is exact (inputs on a grid).
"""
from functools import lru_cache

import numpy as np

from layers_oracle import FLT_MIN, U, bf16_round

SCALE = 1.0 / 128
ROWS = 16            # rows per workgroup
# (B, H, C) -> the edge it covers
CASES = [
    (1, 4, 1),        # one row, one k-step per wave, one class (p = 1, loss 0, zero gradients)
    (15, 16, 2),      # one row short of a workgroup
    (16, 64, 10),     # an exact workgroup at the reference width
    (17, 60, 10),     # one row into a second workgroup; H % 16 = 12
    (33, 252, 15),    # the widest padded H (Hp = 256), an odd C, three workgroups
    (20, 256, 16),    # both upper limits, no column padding
    (45, 200, 10),    # the Model B shape
    (16, 12, 16),     # H smaller than one MFMA tile, with C at its limit
]
TIE_CASES = {(17, 60, 10): (2, 7), (33, 252, 15): (4, 14)}   # two identical W2 columns with equal b2 entries
STABLE_CASE = (16, 64, 10)                                   # logits reach about +-80
MIN_GAP = 1e-3
EXACT_SUM = 64.0     # sum|h W2| of every logit stays below it (the +-80 case has a grid of its own)
ZERO_SHARE = 0.05
REL_FWD, REL_GRAD = 1e-6, 1e-5     # relative L2: forward outputs, gradients (the project's float32 convention)
FWD_OUTPUTS = ("logits", "probs", "row_loss", "loss_sum")
GRAD_OUTPUTS = ("dW2", "db2", "dpre_bias", "dH")


def _np64(t):
    """a NumPy array or a torch tensor (float32 or bfloat16), taken exactly as stored."""
    if hasattr(t, "detach"):
        return t.detach().cpu().double().numpy()
    return np.asarray(t, dtype=np.float64)


def first_max(z):
    """index of the FIRST maximum of every row (the kernel's accuracy rule), as a plain formula."""
    z = np.asarray(z)
    C = z.shape[1]
    return np.where(z == z.max(1, keepdims=True), np.arange(C)[None, :], C).min(1)


def head_oracle(hin, pre_bias, pre_relu, W2, b2, labels, B, scale, start=None):
    """Every output of one launch, in float64, from the kernel's own arguments (hin [>= B, >= H] f32 or bf16,
    pre_bias [H] or None, W2 [H, C], b2 [C] or None, int labels [>= B]).  ``start``: the values the accumulate
    outputs hold before the launch, {"dW2", "db2", "dpre_bias", "loss_sum"} (for the bounds only; default 0).
    Returns a dict of results and, under "bound", a dict of per-element absolute bounds of the same names."""
    W = _np64(W2)
    H, C = W.shape
    pre = _np64(hin)[:B, :H]
    if pre_bias is not None:
        pre = pre + _np64(pre_bias)[None, :]
    h = np.maximum(pre, 0.0) if pre_relu else pre
    bias = np.zeros(C) if b2 is None else _np64(b2)
    lab = np.asarray(_np64(labels)[:B], dtype=np.int64)
    s32 = float(np.float32(scale))
    start = start or {}
    st = {k: np.abs(_np64(start[k])) if k in start else 0.0 for k in ("dW2", "db2", "dpre_bias", "loss_sum")}

    z = h @ W + bias
    m = z.max(1, keepdims=True)
    d = z - m
    e = np.exp(d)
    se = e.sum(1, keepdims=True)
    p = e / se
    lse = m[:, 0] + np.log(se[:, 0])
    zl = z[np.arange(B), lab]
    row_loss = lse - zl
    am = first_max(z)
    onehot = np.zeros((B, C))
    onehot[np.arange(B), lab] = 1.0
    dl = s32 * (p - onehot)
    dW = h.T @ dl
    db = dl.sum(0)
    dH = dl @ W.T
    if pre_relu:
        dH = np.where(pre > 0, dH, 0.0)
    dpb = dH.sum(0)

    Hp = (H + 15) // 16 * 16
    groups = (B + ROWS - 1) // ROWS
    ez = U * (Hp // 4 + 4) * (np.abs(h) @ np.abs(W) + np.abs(bias))
    EZ = ez.max(1, keepdims=True)
    D = (p * np.abs(d)).sum(1, keepdims=True)
    rel_se = 2 * EZ + U * (2 * D + 7)
    rel_p = 2 * EZ + U * (2 * np.abs(d) + 2 * D + 12)
    ep = p * rel_p + 2 * FLT_MIN
    eloss = (2 * EZ[:, 0] + rel_se[:, 0] + U * (3 * np.abs(np.log(se[:, 0])) + np.abs(lse) + np.abs(row_loss)
                                                  + np.abs(m[:, 0])))
    edl = abs(s32) * (ep + 2 * U * np.abs(p - onehot)) + FLT_MIN
    ka = 16 + groups + 1
    edH = edl @ np.abs(W).T + 17 * U * (np.abs(dl) @ np.abs(W).T)
    if pre_relu:
        edH = np.where(pre > 0, edH, 0.0)
    bound = {
        "logits": ez, "probs": ep, "row_loss": eloss,
        "loss_sum": eloss.sum() + U * (B / 4 + 4) * np.abs(row_loss).sum() + U * (st["loss_sum"] + abs(row_loss.sum())),
        "dlogits": edl,
        "dW2": np.abs(h).T @ edl + ka * U * (np.abs(h).T @ np.abs(dl) + st["dW2"]),
        "db2": edl.sum(0) + ka * U * (np.abs(dl).sum(0) + st["db2"]),
        "dH": edH,
        "dpre_bias": edH.sum(0) + ka * U * (np.abs(dH).sum(0) + st["dpre_bias"]),
    }
    return {"pre": pre, "h": h, "logits": z, "probs": p, "row_loss": row_loss, "loss_sum": float(row_loss.sum()),
            "argmax": am, "correct": int((am == lab).sum()), "count": B, "dlogits": dl, "dW2": dW, "db2": db,
            "dH": dH, "dpre_bias": dpb, "bound": bound}


def stored_forms(dH32, B, ldgt):
    """The stored forms of the input gradient, from its float32 values [B, H]: G = bf16 round-to-nearest-even of
    them [B, H]; Gt [H, ldgt] with Gt[:, :B] = G.T and zero padding columns.  Both as float64 arrays."""
    G = bf16_round(np.asarray(_np64(dH32)[:B], dtype=np.float32).astype(np.float64), force=True)
    Gt = np.zeros((G.shape[1], ldgt))
    Gt[:, :B] = G.T
    return G, Gt


# ------------------------------------------------------------------------------------------------------- inputs
def _grid(rng, shape, lim=4.0, step=2.0 ** -6):
    n = int(round(lim / step))
    return rng.integers(-n, n + 1, size=shape).astype(np.float64) * step


def _gaps(z, tie):
    """per row: the gap between the two largest logits; for a row led by the tied pair, between it and the third."""
    B, C = z.shape
    if C == 1:
        return np.full(B, np.inf), np.zeros(B, dtype=bool)
    s = np.sort(z, 1)[:, ::-1]
    gap = s[:, 0] - s[:, 1]
    led = np.zeros(B, dtype=bool)
    if tie is not None:
        a, b = tie
        led = (z[:, a] == s[:, 0]) & (z[:, b] == s[:, 0])
        third = s[:, 2] if C > 2 else np.full(B, -np.inf)
        gap = np.where(led, s[:, 0] - third, gap)
    return gap, led


def _draw(B, H, C, bias, relu, seed):
    rng = np.random.default_rng(seed)
    full = bias and relu     # the tied columns and the +-80 logits belong to the full form of a case
    tie = TIE_CASES.get((B, H, C)) if full else None
    stable = full and (B, H, C) == STABLE_CASE
    pb = _grid(rng, H) if bias else None
    hin = _grid(rng, (B, H))
    zero = rng.random((B, H)) < 0.08
    zero[0, 0] = True
    hin = np.where(zero, 0.0 if pb is None else -pb[None, :], hin)
    if stable:
        # multiples of 2^-6 in [-3, 3]: every product h W2 is a multiple of 2^-12 below 2^5 and every partial sum
        # of the <= 64 of them stays below 2^11, so the logits are exact in fp32 in any order, up to about +-80
        W = _grid(rng, (H, C), lim=3.0)
        b2 = _grid(rng, C, lim=1.0)
    else:
        # multiples of 2^-12 (10 bits and more: not bf16 values) with deviation 0.5 / sqrt(H), cut at four deviations:
        # logits of order 1.  Every product h W2 is a multiple of 2^-18, and where sum|h W2| <= EXACT_SUM = 64 every
        # partial sum, in any order, is one below 2^6: 24 bits, exact in fp32.  So h W2 has no rounding at all, and
        # neither the order of the kernel's sum nor that of a reference enters the comparison.
        sd = 0.5 / np.sqrt(H)
        W = np.clip(np.rint(rng.standard_normal((H, C)) * sd * 4096), -int(4 * sd * 4096), int(4 * sd * 4096)) / 4096
        b2 = (rng.standard_normal(C) * 0.1).astype(np.float32).astype(np.float64) if bias else None
    if tie is not None:
        a, b = tie
        W[:, b] = W[:, a]
        b2[a] = b2[b] = np.float32(b2.max() + 0.75)      # the pair leads a good share of the rows
    pre = hin if pb is None else hin + pb[None, :]
    h = np.maximum(pre, 0.0) if relu else pre
    z = h @ W + (0.0 if b2 is None else b2)
    gap, led = _gaps(z, tie)
    lab = np.full(B, -1, dtype=np.int64)
    if tie is not None:
        rows = np.nonzero(led)[0][:4]
        lab[rows] = np.array([tie[0], tie[1], tie[0], tie[0]])[: len(rows)]
    rest = np.nonzero(lab < 0)[0]
    lab[rest] = rng.permutation(len(rest)) % C
    ok = (gap >= MIN_GAP).all() and (np.abs(pre) == 0).mean() >= ZERO_SHARE
    ok = ok and (stable or (np.abs(h) @ np.abs(W)).max() <= EXACT_SUM)
    ok = ok and len(set(lab.tolist())) == min(B, C)
    if tie is not None:
        # more rows on the first column than on the second: a last-maximum rule would count differently
        ok = ok and (lab[led] == tie[0]).sum() >= 2 and 1 <= (lab[led] == tie[1]).sum() < (lab[led] == tie[0]).sum()
    if stable:
        ok = ok and z.max() >= 70.0 and z.min() <= -70.0 and np.abs(z).max() <= 100.0
    return ok, {"hin": hin, "pre_bias": pb, "W2": W, "b2": b2, "labels": lab.astype(np.int32), "tie": tie}


@lru_cache(maxsize=None)
def head_inputs(B, H, C, bias=True, relu=True):
    """Seeded float64 inputs of one case (all values exact in float32; hin also in bf16), reseeded until the
    conditions hold that tests/test_head_oracle.py asserts: hin and pre_bias multiples of 2^-6 in [-4, 4], at least
    ZERO_SHARE of the pre-activations exactly 0, every class a label, top-two logit gap >= MIN_GAP outside the
    tied pair, the tied pair leading at least two rows labelled with its first column and fewer, but at least one, with its
    second (so that a last-maximum rule counts a different ``correct``)."""
    for k in range(200):
        ok, inp = _draw(B, H, C, bias, relu, 9000 + 1000 * k + 7 * B + 3 * H + C + 2 * bias + relu)
        if ok:
            return inp
    raise AssertionError(f"no seed satisfies the input conditions of {(B, H, C, bias, relu)}")


@lru_cache(maxsize=None)
def head_start(H, C):
    """Seeded non-zero start values of the accumulate outputs (float32 values).  The gradient buffers start at
    2^-10 .. 2^-8 in magnitude, the size of the smallest increments (dpre_bias at scale 1/128): a larger start would
    put its own ulp, not the kernel's arithmetic, into the relative error of the increment.  correct / count start
    on integers."""
    rng = np.random.default_rng(77 + 5 * H + C)

    def f(lo, hi, *s):
        return (rng.uniform(lo, hi, s) * rng.choice([-1.0, 1.0], s)).astype(np.float32).astype(np.float64)

    g = (2.0 ** -10, 2.0 ** -8)
    return {"dW2": f(*g, H, C), "db2": f(*g, C), "dpre_bias": f(*g, H),
            "metrics": np.array([float(f(0.125, 0.5, 1)[0]), 3.0, 5.0, 0.0])}


@lru_cache(maxsize=None)
def case_oracle(B, H, C, bias=True, relu=True, scale=SCALE):
    inp = head_inputs(B, H, C, bias, relu)
    st = head_start(H, C)
    return head_oracle(inp["hin"], inp["pre_bias"], relu, inp["W2"], inp["b2"], inp["labels"], B, scale,
                       start={"dW2": st["dW2"], "db2": st["db2"], "dpre_bias": st["dpre_bias"],
                              "loss_sum": st["metrics"][0]})


def rel_l2(got, ref):
    """|got - ref| / |ref| in L2; 0 where both vanish (an all-zero reference must be met exactly)."""
    got, ref = _np64(got), _np64(ref)
    num, den = float(np.linalg.norm(got - ref)), float(np.linalg.norm(ref))
    if den == 0.0:
        return 0.0 if num == 0.0 else float("inf")
    return num / den


def bound_ratio(got, ref, bound):
    """the largest |got - ref| / bound over the elements (0 / 0 counts as 0)."""
    err = np.abs(_np64(got) - _np64(ref))
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.max(r)) if r.size else 0.0


START = {"loss_sum": lambda st: st["metrics"][0], "dW2": lambda st: st["dW2"], "db2": lambda st: st["db2"],
         "dpre_bias": lambda st: st["dpre_bias"]}


def figures(got, o, st):
    """name -> (relative L2 error, its cap, worst element's share of its own bound).  Accumulate outputs: the
    relative error is that of got - start against the oracle's increment; the element bound is on got itself."""
    out = {}
    for name in FWD_OUTPUTS + GRAD_OUTPUTS:
        if name not in got:
            continue
        g = _np64(got[name])
        s0 = START[name](st) if name in START else 0.0
        rel = rel_l2(g - s0, o[name])
        out[name] = (rel, REL_FWD if name in FWD_OUTPUTS else REL_GRAD,
                     bound_ratio(g, o[name] + s0, o["bound"][name]))
    return out


def show(tag, fig):
    print(f"{tag}: " + "  ".join(f"{n} {r:.2e} ({e:.3f})" for n, (r, _, e) in fig.items()))
