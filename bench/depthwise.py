#!/usr/bin/env python
"""Depthwise kernels (csrc/kernels/depthwise.hip) at MobileNet-sized shapes, batch 64, float32: device-event time
of the forward, the input gradient and the weight gradient, achieved bytes/s against the bytes each shape needs
(every operand crossing HBM once) and the share of the HBM peak BASELINE.md's roofline table uses; then a
training step of ``zoo.mnist_separable_cnn`` under ``fit``.  Prints a markdown table (``--out FILE`` also writes
it); needs a GPU — there is no CPU fallback for a timing.

    python bench/depthwise.py [--window 0.25] [--out FILE]

Every timed window lasts at least ``--window`` seconds of back-to-back launches, and the launches rotate over
operand sets that together exceed the Infinity Cache four times, so the bytes/s are HBM figures.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12   # bytes/s, the HBM roof of BASELINE.md
SHAPES = [  # H, C, k, stride
    (112, 32, 3, 1), (56, 128, 3, 2), (14, 512, 3, 1), (7, 1024, 3, 1), (14, 256, 7, 1)]
BATCH = 64
COLD_BYTES = 1 << 30   # bytes of x, y, dy, dx over the rotated operand sets of a shape (4x the Infinity Cache)


def _time(fn, nbuf, window):
    """Seconds per launch of fn(i), i rotating over the nbuf operand sets, over a window of at least ``window`` s."""
    for i in range(max(3, nbuf)):
        fn(i % nbuf)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    iters, t = 20, 0.0
    while True:
        t0.record()
        for i in range(iters):
            fn(i % nbuf)
        t1.record()
        torch.cuda.synchronize()
        t = t0.elapsed_time(t1) * 1e-3
        if t >= window:
            return t / iters
        iters = int(iters * max(2.0, 1.2 * window / max(t, 1e-6)))


def kernels(window):
    from tensorflow_distributed_example_amd.models.layers import tf_same_pads
    from tensorflow_distributed_example_amd.ops import layer_ops32 as O32
    from tensorflow_distributed_example_amd.ops.layer_ops import ConvGeom
    rows = []
    for H, C, k, s in SHAPES:
        Ho = -(-H // s)
        p = tf_same_pads(H, k, s)[0]
        g = ConvGeom(BATCH, H, H, C, Ho, Ho, C, k, k, s, s, p, p)
        nx, ny, nw = BATCH * H * H * C, BATCH * Ho * Ho * C, k * k * C
        # operand sets rotated launch by launch so that no launch finds its operands in the 256 MB Infinity
        # Cache: together the sets hold COLD_BYTES
        nbuf = max(2, -(-COLD_BYTES // (4 * 2 * (nx + ny))))
        x = [torch.randn(BATCH, H, H, C, device="cuda") for _ in range(nbuf)]
        y = [torch.randn(BATCH, Ho, Ho, C, device="cuda") for _ in range(nbuf)]
        dy, dx = [torch.randn_like(t) for t in y], [torch.zeros_like(t) for t in x]
        w, b = torch.randn(k, k, C, 1, device="cuda") * 0.1, torch.zeros(C, device="cuda")
        dW, db = torch.zeros_like(w), torch.zeros_like(b)
        part = torch.empty(O32.dw_part_elems(g), device="cuda")
        runs = {   # kernel: (launch on operand set i, floats that must cross HBM once)
            "fwd": (lambda i: O32.dw_fwd(x[i], w, y[i], g, bias=b, relu=True), nx + ny + nw + C),
            "wgrad": (lambda i: O32.dw_wgrad(x[i], dy[i], dW, g, part, y=y[i], db=db), nx + 2 * ny + nw + C),
            "dgrad": (lambda i: O32.dw_dgrad(dy[i], w, dx[i], g, y=y[i]), 2 * ny + nx + nw),
        }
        for name, (fn, floats) in runs.items():
            t = _time(fn, nbuf, window)
            rows.append((f"{H}x{H}x{C} {k}x{k}/{s}", name, nbuf, t * 1e6, 4 * floats / t / 1e12,
                         4 * floats / t / HBM_PEAK))
    return rows


def fit_step(steps=64):
    import tensorflow_distributed_example_amd as tde
    tde.backend.set_global_policy("float32")
    tde.backend.set_random_seed(0)
    m = tde.zoo.mnist_separable_cnn()
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
    ap.add_argument("--window", type=float, default=0.25, help="least seconds of launches in a timed window")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench/depthwise.py needs a GPU: nothing measured")
    rows = kernels(a.window)
    lines = ["| shape (batch 64) | kernel | operand sets | time us | achieved TB/s | share of HBM peak (8 TB/s) |",
             "|---|---|---|---|---|---|"]
    lines += [f"| {s} | {k} | {n} | {t:.1f} | {bw:.2f} | {100 * sh:.1f} % |" for s, k, n, t, bw, sh in rows]
    worst = min(rows, key=lambda r: r[5])
    lines.append(f"\nFurthest from its byte bound: {worst[1]} at {worst[0]} ({100 * worst[5]:.1f} % of the HBM peak).")
    t, kind = fit_step()
    lines.append(f"\nzoo.mnist_separable_cnn under fit (batch 64, {kind} plan, hipGraph, 16 steps per execution): "
                 f"{t * 1e6:.0f} us per step, {BATCH / t:,.0f} img/s (host clock around synchronised epochs).")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
