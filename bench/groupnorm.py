#!/usr/bin/env python
"""Group-norm kernels (csrc/kernels/groupnorm.hip) at batch 64, float32: device-event time of the forward and the
backward (dx + dgamma + dbeta), achieved bytes/s against the bytes each shape needs (every operand crossing HBM
once), the share of the HBM peak BASELINE.md's roofline table uses, and ``torch.nn.functional.group_norm`` /
``layer_norm`` (forward, and forward + autograd backward, channels-last input) in the same process; then a training
step of ``zoo.mnist_gn_cnn`` under ``fit``.  Prints a markdown table (``--out FILE`` also writes it); needs a GPU.

    python bench/groupnorm.py [--window 0.2] [--repeats 3] [--out FILE]

Every timed window lasts at least ``--window`` seconds of back-to-back launches, and the launches rotate over
operand sets that together exceed the Infinity Cache four times, so the bytes/s are HBM figures.  Each figure is
the median of ``--repeats`` windows; the spread is (max - min) / median.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(1, os.path.dirname(os.path.abspath(__file__)))
from depthwise import COLD_BYTES, HBM_PEAK, _time   # noqa: E402  (bench/depthwise.py: the same window and rotation)

BATCH = 64
SHAPES = [  # name, R, S, C, G, torch form
    ("GN 112x112x32 G=8", BATCH, 112 * 112, 32, 8, "gn"), ("GN 56x56x128 G=32", BATCH, 56 * 56, 128, 32, "gn"),
    ("GN 14x14x512 G=32", BATCH, 14 * 14, 512, 32, "gn"), ("GN 7x7x1024 G=32", BATCH, 7 * 7, 1024, 32, "gn"),
    ("instance norm 56x56x64", BATCH, 56 * 56, 64, 64, "gn"), ("LN 3136x128 rows", BATCH * 3136, 1, 128, 1, "ln"),
    ("LN [64, 128]", BATCH, 1, 128, 1, "ln")]


def _med(fn, nbuf, window, repeats):
    ts = sorted(_time(fn, nbuf, window) for _ in range(repeats))
    return ts[len(ts) // 2], (ts[-1] - ts[0]) / ts[len(ts) // 2]


def kernels(window, repeats):
    from tensorflow_distributed_example_amd.ops import layer_ops32 as O32
    rows = []
    for name, R, S, C, G, form in SHAPES:
        n = R * S * C
        nbuf = max(2, -(-COLD_BYTES // (4 * 4 * n)))   # x, y, dy, dx per set
        x = [torch.randn(R, S, C, device="cuda") + 1.0 for _ in range(nbuf)]
        y, dx = [torch.empty_like(t) for t in x], [torch.empty_like(t) for t in x]
        dy = [torch.randn_like(t) for t in x]
        gamma, beta = torch.rand(C, device="cuda") + 0.5, torch.randn(C, device="cuda")
        dg, db = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
        mean, rstd = torch.zeros(R * G, device="cuda"), torch.zeros(R * G, device="cuda")
        part = torch.empty(O32.gn_part_elems(R, S, C, G), device="cuda")
        plan = O32.gn_plan(R, S, C, G)
        O32.gn_fwd(x[0], y[0], mean, rstd, R, S, C, G, 1e-3, gamma=gamma, beta=beta)
        # torch: the same NHWC storage as a channels_last [N, C, H, W] tensor; leaves that require gradients
        h = int(round(S ** 0.5))

        def view(t):
            return t.view(R, h, h, C).permute(0, 3, 1, 2) if form == "gn" else t.view(R, C)

        xt = [view(u.clone()).requires_grad_(True) for u in x]
        gt, bt = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        dyt = [view(t) for t in dy]

        def tfwd(i):
            return F.group_norm(xt[i], G, gt, bt, 1e-3) if form == "gn" else F.layer_norm(xt[i], (C,), gt, bt, 1e-3)

        def tboth(i):
            for t in (xt[i], gt, bt):
                t.grad = None
            tfwd(i).backward(dyt[i])

        def tnograd(i):
            with torch.no_grad():
                tfwd(i)

        runs = {   # kernel: (ours on operand set i, floats crossing HBM once)
            "fwd": (lambda i: O32.gn_fwd(x[i], y[i], mean, rstd, R, S, C, G, 1e-3, gamma=gamma, beta=beta),
                    2 * n + 2 * C + 2 * R * G),
            "bwd": (lambda i: O32.gn_bwd(dy[i], x[i], mean, rstd, R, S, C, G, part, gamma=gamma, dx=dx[i], dgamma=dg,
                                         dbeta=db), 3 * n + 3 * C + 2 * R * G),
        }
        t_f, _ = _med(tnograd, nbuf, window, repeats)
        t_fb, _ = _med(tboth, nbuf, window, repeats)
        for k, (fn, floats) in runs.items():
            t, spread = _med(fn, nbuf, window, repeats)
            t_torch = t_f if k == "fwd" else t_fb - t_f
            form_ = ("row" if not plan["slab"] else "slab, LDS" if plan["staged_" + k] else "slab, two sweeps")
            rows.append((name, k, form_, nbuf, t * 1e6, spread, 4 * floats / t / 1e12, 4 * floats / t / HBM_PEAK,
                         t_torch * 1e6))
        del x, y, dx, dy, xt, dyt
        torch.cuda.empty_cache()
    return rows


def fit_step(steps=64):
    import tensorflow_distributed_example_amd as tde
    tde.backend.set_global_policy("float32")
    tde.backend.set_random_seed(0)
    m = tde.zoo.mnist_gn_cnn()
    m.compile(loss=tde.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=tde.optimizers.SGD(0.05),
              metrics=["accuracy"], steps_per_execution=16)
    rng = np.random.default_rng(0)
    x, y = rng.random((BATCH * steps, 28, 28, 1), dtype=np.float32), rng.integers(0, 10, BATCH * steps)
    m.fit(x, y, batch_size=BATCH, epochs=1, verbose=0)   # builds the program, captures the graph
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m.fit(x, y, batch_size=BATCH, epochs=3, verbose=0)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (3 * steps), m._program("train", BATCH).plan_kind


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.2, help="least seconds of launches in a timed window")
    ap.add_argument("--repeats", type=int, default=3, help="windows per figure (median and spread)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench/groupnorm.py needs a GPU: nothing measured")
    rows = kernels(a.window, a.repeats)
    lines = ["| shape (batch 64) | kernel | form | operand sets | time us | spread | achieved TB/s | share of HBM peak "
             "(8 TB/s) | torch us (bwd: fwd+bwd minus fwd) |", "|---|---|---|---|---|---|---|---|---|"]
    lines += [f"| {s} | {k} | {f} | {n} | {t:.1f} | {100 * sp:.1f} % | {bw:.2f} | {100 * sh:.1f} % | {tt:.1f} |"
              for s, k, f, n, t, sp, bw, sh, tt in rows]
    worst = min((r for r in rows if r[4] > 20), key=lambda r: r[7])   # launches of a few us are latency, not bytes
    lines.append(f"\nFurthest from its byte bound: {worst[1]} at {worst[0]} ({100 * worst[7]:.1f} % of the HBM peak).")
    t, kind = fit_step()
    lines.append(f"\nzoo.mnist_gn_cnn under fit (batch 64, {kind} plan, 16 steps per execution): "
                 f"{t * 1e6:.0f} us per step, {BATCH / t:,.0f} img/s (host clock around synchronised epochs).")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
