#!/usr/bin/env python
"""GRU sweeps (csrc/kernels/gru.hip), float32: device-event time of the forward and the backward sweep (one launch
each; the input projection, the dU GEMM and the bias column sum are not part of them), per sweep and per time step,
the f32 MFMA rate against the FLOPs of the recurrent product (2 * N * T * u * 3u each way), and ``torch.nn.GRU`` in
float32 on the same card in the same process (forward under no_grad, and forward + autograd backward minus forward;
torch's figures include its input projection from D = 28 features and its weight gradients, ours do not); then a
training step of ``zoo.mnist_gru`` under ``fit``.  Prints a markdown table (``--out FILE`` also writes it); needs a
GPU.  The shapes, windows, operand rotation and the median / spread are those of bench/lstm.py, so the two tables
of one session compare line by line.

    python bench/gru.py [--window 0.2] [--repeats 3] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(1, os.path.dirname(os.path.abspath(__file__)))
from attention import MFMA_F32_PEAK, _med   # noqa: E402
from depthwise import COLD_BYTES   # noqa: E402
from lstm import BATCH, D, SHAPES   # noqa: E402


def to_torch(w, u):
    """Our gate blocks z, r, h along the last axis as torch's r, z, n rows."""
    z, r, h = w.split(u, dim=-1)
    return torch.cat([r, z, h], -1).t()


def kernels(window, repeats):
    from tensorflow_distributed_example_amd.ops import layer_ops32 as O32
    rows = []
    for N, T, u in SHAPES:
        n = N * T * u
        nbuf = max(2, -(-COLD_BYTES // (4 * 17 * n)))   # x, dx, dr (3n each), acts (4n), hseq, hprev, dh (n each)
        inp = torch.randn(nbuf, N, T, D, device="cuda")
        W, U = torch.randn(D, 3 * u, device="cuda") / D ** 0.5, torch.randn(u, 3 * u, device="cuda") / u ** 0.5
        b = 0.5 * torch.randn(2, 3 * u, device="cuda")
        x = inp @ W + b[0]
        dh = torch.randn(nbuf, N, T, u, device="cuda")
        hseq, hprev = torch.empty_like(dh), torch.empty_like(dh)
        acts = torch.empty(nbuf, N, T, 4 * u, device="cuda")
        dx, dr = torch.empty_like(x), torch.empty_like(x)

        def fwd(i):
            O32.gru_fwd(x[i], U, b[1], hseq[i], hprev[i], acts[i], N, T, u)

        for i in range(nbuf):
            fwd(i)
        ref = torch.nn.GRU(D, u, batch_first=True).cuda()
        with torch.no_grad():
            ref.weight_ih_l0.copy_(to_torch(W, u))
            ref.weight_hh_l0.copy_(to_torch(U, u))
            ref.bias_ih_l0.copy_(to_torch(b[0], u))
            ref.bias_hh_l0.copy_(to_torch(b[1], u))
            want = ref(inp[0])[0]
            err = ((hseq[0] - want).norm() / want.norm()).item()   # the two sides compute the same thing

        def tnograd(i):
            with torch.no_grad():
                ref(inp[i])

        def tboth(i):
            ref.zero_grad(set_to_none=True)
            ref(inp[i])[0].backward(dh[i])

        t_f, _ = _med(tnograd, nbuf, window, repeats)
        t_fb, _ = _med(tboth, nbuf, window, repeats)
        flops = 2 * N * T * u * 3 * u
        for name, fn, t_torch in (("fwd", fwd, t_f),
                                  ("bwd", lambda i: O32.gru_bwd(acts[i], hprev[i], U, dh[i], dx[i], dr[i], N, T, u,
                                                                False), t_fb - t_f)):
            t, spread = _med(fn, nbuf, window, repeats)
            rows.append((f"{N}, {T}, {u}", name, nbuf, -(-N // 16), t * 1e6, spread, t / T * 1e6, flops / t / 1e12,
                         flops / t / MFMA_F32_PEAK, t_torch * 1e6, err))
        del inp, x, dh, hseq, hprev, acts, dx, dr
        torch.cuda.empty_cache()
    return rows


def fit_step(steps=64):
    import tensorflow_distributed_example_amd as tde
    tde.backend.set_global_policy("float32")
    tde.backend.set_random_seed(0)
    m = tde.zoo.mnist_gru()
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
        sys.exit("bench/gru.py needs a GPU: nothing measured")
    rows = kernels(a.window, a.repeats)
    lines = ["| N, T, units | sweep | operand sets | workgroups | time us | spread | us per time step | achieved TFLOP/s "
             "| share of the f32 MFMA roof (157 TFLOP/s) | torch.nn.GRU f32 us (with x W and, bwd, the weight "
             "gradients; bwd: fwd+bwd minus fwd) | hseq vs torch rel |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    lines += [f"| {s} | {k} | {n} | {wg} | {t:.1f} | {100 * sp:.1f} % | {ts:.2f} | {fl:.2f} | {100 * sh:.2f} % | "
              f"{tt:.1f} | {e:.1e} |" for s, k, n, wg, t, sp, ts, fl, sh, tt, e in rows]
    t, kind = fit_step()
    lines.append(f"\nzoo.mnist_gru under fit (batch 64, {kind} plan, 16 steps per execution): "
                 f"{t * 1e6:.0f} us per step, {BATCH / t:,.0f} img/s (host clock around synchronised epochs).")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
