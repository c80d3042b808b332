#!/usr/bin/env python
"""Attention kernels (csrc/kernels/attention.hip), float32: device-event time of the core forward and backward
(dQ + dK + dV, two launches), the achieved f32 MFMA rate against the FLOPs the algorithm needs (forward: Q K^T and
P V; backward: S, dP, dV, dK, dQ -- the recomputation of S and dP by the dQ sweep is not counted as useful work),
its share of the 157 TFLOP/s f32 matrix roof, and ``torch.nn.functional.scaled_dot_product_attention`` in float32
on the same storage (forward under no_grad, and forward + autograd backward minus forward) in the same process; then
a training step of ``zoo.mnist_attn_cnn`` under ``fit``.  Prints a markdown table (``--out FILE`` also writes it);
needs a GPU.

    python bench/attention.py [--window 0.2] [--repeats 3] [--out FILE]

Every timed window lasts at least ``--window`` seconds of back-to-back launches, and the launches rotate over
operand sets that together exceed the Infinity Cache four times, so the operands come from HBM.  Each figure is the
median of ``--repeats`` windows; the spread is (max - min) / median.
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
from depthwise import COLD_BYTES, _time   # noqa: E402  (bench/depthwise.py: the same window and rotation)

MFMA_F32_PEAK = 157e12   # FLOP/s, v_mfma_f32_16x16x4_f32 on an MI355X
SHAPES = [(64, 4, 49, 8), (64, 4, 196, 16), (64, 8, 256, 64), (256, 4, 49, 32)]   # B, heads, T, d (dk = dv)
BATCH = 64


def _med(fn, nbuf, window, repeats):
    ts = sorted(_time(fn, nbuf, window) for _ in range(repeats))
    return ts[len(ts) // 2], (ts[-1] - ts[0]) / ts[len(ts) // 2]


def kernels(window, repeats):
    from tensorflow_distributed_example_amd.ops import layer_ops32 as O32
    rows = []
    for B, h, T, d in SHAPES:
        n = B * T * h * d
        nbuf = max(2, -(-COLD_BYTES // (4 * 8 * n)))   # q, k, v, o, do, dq, dk, dv per set
        q, k, v, do = (torch.randn(nbuf, B, T, h * d, device="cuda") for _ in range(4))
        o, dq, dk, dv = (torch.empty_like(q) for _ in range(4))
        lse = torch.zeros(nbuf, B, h, T, device="cuda")
        for i in range(nbuf):
            O32.mha_fwd(q[i], k[i], v[i], o[i], lse[i], B, h, T, d, d)

        def heads(t):   # torch's [B, heads, T, d] view of one operand set's storage
            return t.view(B, T, h, d).transpose(1, 2)

        qt, kt, vt = ([heads(t[i].clone()).requires_grad_(True) for i in range(nbuf)] for t in (q, k, v))
        dot = [heads(do[i]) for i in range(nbuf)]

        def tfwd(i):
            return F.scaled_dot_product_attention(qt[i], kt[i], vt[i])

        def tboth(i):
            for t in (qt[i], kt[i], vt[i]):
                t.grad = None
            tfwd(i).backward(dot[i])

        def tnograd(i):
            with torch.no_grad():
                tfwd(i)

        # the check that the two sides compute the same thing at the timed size
        with torch.no_grad():
            err = ((heads(o[0]) - tfwd(0)).norm() / tfwd(0).norm()).item()
        runs = {
            "fwd": (lambda i: O32.mha_fwd(q[i], k[i], v[i], o[i], lse[i], B, h, T, d, d), 2 * 2 * B * h * T * T * d),
            "bwd": (lambda i: O32.mha_bwd(q[i], k[i], v[i], o[i], lse[i], do[i], dq[i], dk[i], dv[i], B, h, T, d, d),
                    5 * 2 * B * h * T * T * d),
        }
        t_f, _ = _med(tnograd, nbuf, window, repeats)
        t_fb, _ = _med(tboth, nbuf, window, repeats)
        for name, (fn, flops) in runs.items():
            t, spread = _med(fn, nbuf, window, repeats)
            t_torch = t_f if name == "fwd" else t_fb - t_f
            rows.append((f"{B}, {h}, {T}, {d}", name, nbuf, t * 1e6, spread, flops / t / 1e12,
                         flops / t / MFMA_F32_PEAK, t_torch * 1e6, err))
        del q, k, v, do, o, dq, dk, dv, qt, kt, vt, dot
        torch.cuda.empty_cache()
    return rows


def fit_step(steps=64):
    import tensorflow_distributed_example_amd as tde
    tde.backend.set_global_policy("float32")
    tde.backend.set_random_seed(0)
    m = tde.zoo.mnist_attn_cnn()
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
        sys.exit("bench/attention.py needs a GPU: nothing measured")
    rows = kernels(a.window, a.repeats)
    lines = ["| B, heads, T, d | kernel | operand sets | time us | spread | achieved TFLOP/s | share of the f32 MFMA "
             "roof (157 TFLOP/s) | torch SDPA f32 us (bwd: fwd+bwd minus fwd) | O vs torch rel |",
             "|---|---|---|---|---|---|---|---|---|"]
    lines += [f"| {s} | {k} | {n} | {t:.1f} | {100 * sp:.1f} % | {fl:.2f} | {100 * sh:.1f} % | {tt:.1f} | {e:.1e} |"
              for s, k, n, t, sp, fl, sh, tt, e in rows]
    t, kind = fit_step()
    lines.append(f"\nzoo.mnist_attn_cnn under fit (batch 64, {kind} plan, 16 steps per execution): "
                 f"{t * 1e6:.0f} us per step, {BATCH / t:,.0f} img/s (host clock around synchronised epochs).")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
