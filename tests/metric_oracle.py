"""Float64 numpy oracle of the metrics beyond the accuracy (csrc/include/tde_metric.h, metrics.py), for
tests/test_metric_head.py (CPU) and tests/test_metric_head_gpu.py (GPU).  Written from the definitions, row by
row, with no code of the package:

    top-k hit    0 <= y < C, l_y finite, #{c : l_c > l_y} < k
    crossentropy (1 - e)(lse - l_y) + e (lse - mean l); a label outside [0, C): l_y := max
    confusion    cm[y][lowest-index argmax] += 1 for 0 <= y < C
    F-score      p = tp/(tp+fp+eps), r = tp/(tp+fn+eps), f = (1+b^2) p r / (b^2 p + r + eps), eps = 1e-7

``words`` returns every accumulator word in the layout's order, ``logged`` every logged value, ``margins`` the
float64 distance of each row from the decision boundary of each count.
"""
from __future__ import annotations

import math

import numpy as np

EPS = 1e-7


def _lse(row):
    m = row.max()
    if not np.isfinite(m):
        return float(m) if m > 0 else -math.inf
    return float(m + np.log(np.exp(row - m).sum()))


def row_values(l, y, ks, smooths):
    """One row: -> (hits per k, crossentropy per e, lowest-index argmax or None, valid)."""
    l = np.asarray(l, dtype=np.float64)
    C = l.shape[0]
    valid = 0 <= y < C
    ly = l[y] if valid else l.max()
    greater = int((l > ly).sum())
    hits = [int(valid and math.isfinite(ly) and greater < k) for k in ks]
    with np.errstate(all="ignore"):
        lse = _lse(l)
        ces = [float((1.0 - e) * (lse - ly) + (e * (lse - l.mean()) if e else 0.0)) for e in smooths]
    am = None
    if not np.isnan(l).all() and l[~np.isnan(l)].max() > -math.inf:
        am = int(np.flatnonzero(l == l[~np.isnan(l)].max())[0])
    return hits, ces, am, valid


def words(logits, labels, ks=(), smooths=(), cm=False):
    """-> dict(topk [len(ks)], ce [len(smooths)], cm [C, C] or None, correct, rows, flat: the ext buffer)."""
    z = np.asarray(logits, dtype=np.float64)
    C = z.shape[1]
    topk = np.zeros(len(ks))
    ce = np.zeros(len(smooths))
    conf = np.zeros((C, C))
    correct = 0
    for l, y in zip(z, np.asarray(labels).reshape(-1)):
        y = int(y)
        h, c, am, valid = row_values(l, y, ks, smooths)
        topk += h
        with np.errstate(all="ignore"):
            ce += c
        if valid and am is not None:
            conf[y, am] += 1
        correct += int(am == y)
    flat = np.concatenate([topk, ce, conf.reshape(-1) if cm else np.zeros(0)])
    return dict(topk=topk, ce=ce, cm=conf if cm else None, correct=correct, rows=z.shape[0], flat=flat)


def fbeta(cm, beta, average):
    C = cm.shape[0]
    tp = [cm[c, c] for c in range(C)]
    fp = [sum(cm[r, c] for r in range(C) if r != c) for c in range(C)]
    fn = [sum(cm[c, r] for r in range(C) if r != c) for c in range(C)]
    sup = [cm[c].sum() for c in range(C)]
    if average == "micro":
        tp, fp, fn = [sum(tp)], [sum(fp)], [sum(fn)]
    f = []
    for a, b, c in zip(tp, fp, fn):
        p, r = a / (a + b + EPS), a / (a + c + EPS)
        f.append((1 + beta ** 2) * p * r / (beta ** 2 * p + r + EPS))
    if average == "weighted":
        return sum(fi * s for fi, s in zip(f, sup)) / sum(sup)
    return sum(f) / len(f)


def margins(logits, labels, ks):
    """-> (top-k margins [N, len(ks)]: |l_y - k-th largest other| (inf without such a class or a valid label),
    argmax margins [N]: the gap of the two largest logits)."""
    z = np.asarray(logits, dtype=np.float64)
    N, C = z.shape
    mk = np.full((N, len(ks)), np.inf)
    ma = np.full(N, np.inf)
    for i, (l, y) in enumerate(zip(z, np.asarray(labels).reshape(-1))):
        s = np.sort(l)[::-1]
        if C > 1:
            ma[i] = s[0] - s[1]
        if 0 <= y < C:
            others = np.sort(np.delete(l, int(y)))[::-1]
            for j, k in enumerate(ks):
                if k - 1 < len(others):
                    mk[i, j] = abs(l[int(y)] - others[k - 1])
    return mk, ma
