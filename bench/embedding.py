#!/usr/bin/env python
"""Embedding kernels (csrc/kernels/embedding.hip), float32: device-event time of the forward gather and of the
backward scatter-sum (one launch each) at three (n, V, D) under three id distributions -- uniform, Zipf-like, and
half of the tokens on id 0 (the padding id of a text batch: the longest serial add chain the token-order contract
allows) -- with the bytes per second against what each launch must move (forward: the ids, the gathered rows and
the output, 4 n + 8 n D; backward: ``V*D*4 + n*D*4``, the gradient written and dy read), and
``torch.nn.functional.embedding`` in float32 on the same card in the same process (forward under no_grad; backward
as forward + autograd backward minus forward: a zero fill plus an atomic scatter, not bitwise reproducible).
Operand sets rotate launch by launch (as bench/gru.py; at most 64 sets, so the smallest shape's 1.5 MB sets stay
inside the Infinity Cache, as they would in a training step).  Prints a markdown table (``--out FILE`` also writes
it); needs a GPU.

    python bench/embedding.py [--window 0.2] [--repeats 3] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(1, os.path.dirname(os.path.abspath(__file__)))
from attention import _med   # noqa: E402
from depthwise import COLD_BYTES   # noqa: E402

SHAPES = [(128 * 32, 2000, 32), (128 * 80, 20000, 64), (128 * 80, 20000, 128)]   # n, V, D
HBM_PEAK = 8e12   # bytes/s, MI355X


def make_ids(kind, n, V, rng):
    if kind == "uniform":
        return rng.integers(0, V, n)
    if kind == "zipf":
        return np.minimum(rng.zipf(1.3, n) - 1, V - 1)
    ids = rng.integers(1, V, n)          # "half zero"
    ids[rng.permutation(n)[: n // 2]] = 0
    return ids


def kernels(window, repeats):
    from tensorflow_distributed_example_amd.ops import layer_ops32 as O32
    rows = []
    rng = np.random.default_rng(0)
    for n, V, D in SHAPES:
        nbuf = min(64, max(2, -(-COLD_BYTES // (4 * (2 * V * D + 2 * n * D)))))   # table, dtable, out, dy
        table, dy = torch.randn(nbuf, V, D, device="cuda"), torch.randn(nbuf, n, D, device="cuda")
        out, dtable = torch.empty_like(dy), torch.empty_like(table)
        tw = [table[i].clone().requires_grad_(True) for i in range(nbuf)]
        for kind in ("uniform", "zipf", "half zero"):
            ids_np = make_ids(kind, n, V, rng)
            ids, idl = torch.from_numpy(ids_np.astype(np.float32)).cuda(), torch.from_numpy(ids_np).cuda()
            hot = int(np.bincount(ids_np).max())

            def fwd(i):
                O32.embed_fwd(ids, table[i], out[i], n, V, D)

            def bwd(i):
                O32.embed_bwd(ids, dy[i], dtable[i], n, V, D)

            def tnograd(i):
                with torch.no_grad():
                    F.embedding(idl, tw[i])

            def tboth(i):
                tw[i].grad = None
                F.embedding(idl, tw[i]).backward(dy[i])

            fwd(0), bwd(0), tboth(0)
            same = torch.equal(out[0], F.embedding(idl, table[0]))   # the two sides compute the same thing
            err = ((dtable[0] - tw[0].grad).norm() / tw[0].grad.norm()).item()
            t_f, _ = _med(tnograd, nbuf, window, repeats)
            t_fb, _ = _med(tboth, nbuf, window, repeats)
            for name, fn, nbytes, t_torch in (("fwd", fwd, 4 * n + 8 * n * D, t_f),
                                              ("bwd", bwd, 4 * (V * D + n * D), t_fb - t_f)):
                t, spread = _med(fn, nbuf, window, repeats)
                rows.append((f"{n}, {V}, {D}", kind, hot, name, nbuf, t * 1e6, spread, nbytes / t / 1e9,
                             nbytes / t / HBM_PEAK, t_torch * 1e6, f"{same}, {err:.1e}"))
        del table, dy, out, dtable, tw
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.2, help="least seconds of launches in a timed window")
    ap.add_argument("--repeats", type=int, default=3, help="windows per figure (median and spread)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench/embedding.py needs a GPU: nothing measured")
    lines = ["| n, V, D | ids | tokens on the hottest id | launch | operand sets | time us | spread | achieved GB/s "
             "| share of the HBM roof (8 TB/s) | torch F.embedding f32 us (bwd: fwd+bwd minus fwd) "
             "| out equal to torch, dtable vs torch rel |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    lines += [f"| {s} | {k} | {h} | {l} | {nb} | {t:.1f} | {100 * sp:.1f} % | {bw:.0f} | {100 * sh:.2f} % | {tt:.1f} | "
              f"{e} |" for s, k, h, l, nb, t, sp, bw, sh, tt, e in kernels(a.window, a.repeats)]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
