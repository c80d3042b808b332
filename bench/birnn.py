#!/usr/bin/env python
"""Bidirectional sweeps (the BI kernels of csrc/kernels/lstm.hip and gru.hip), float32, ``return_sequences`` form:
device-event time of the ONE forward and the ONE backward launch for both directions, against what the same result
costs without them: one unidirectional sweep (the yardstick for "two directions in the time of one"), the two
unidirectional launches alone, and the two launches with the torch copies they need around them (forward: flip X_1,
flip h_1 back, concatenate; backward: split dh, flip its second half, flip dX_1 back — and dR_1 for a GRU).  The
composed result is compared with the bidirectional one bit for bit.  Shapes: the zoo's (``text_bilstm`` at batch 64)
and N = T = units = 128.  Prints a markdown table (``--out FILE`` also writes it); needs a GPU.  Windows, operand
rotation and the median / spread are those of bench/gru.py.

    python bench/birnn.py [--window 0.2] [--repeats 3] [--out FILE]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(1, os.path.dirname(os.path.abspath(__file__)))
from attention import _med   # noqa: E402
from depthwise import COLD_BYTES   # noqa: E402

SHAPES = [(64, 32, 64), (128, 128, 128)]   # N, T, units


def kernels(window, repeats):
    from tensorflow_distributed_example_amd.ops import layer_ops32 as O32
    rows = []
    for cell in ("lstm", "gru"):
        gru = cell == "gru"
        G = 3 if gru else 4
        for N, T, u in SHAPES:
            n = N * T * u
            # per set and direction: x, dx (G n each; a GRU's dr too), acts (4n), hprev, cseq, h, dh (n each)
            nbuf = max(2, -(-COLD_BYTES // (4 * 2 * (3 * G + 8) * n)))

            def rnd(*s):
                return torch.randn(nbuf, *s, device="cuda")

            x = [rnd(N, T, G * u) for _ in range(2)]
            U = [torch.randn(u, G * u, device="cuda") / u ** 0.5 for _ in range(2)]
            rb = [0.5 * torch.randn(3 * u, device="cuda") for _ in range(2)]
            dh, out = rnd(N, T, 2 * u), torch.empty(nbuf, N, T, 2 * u, device="cuda")
            hprev, cseq, hs = ([torch.empty(nbuf, N, T, u, device="cuda") for _ in range(2)] for _ in range(3))
            acts = [torch.empty(nbuf, N, T, 4 * u, device="cuda") for _ in range(2)]
            dx, dr = ([torch.empty_like(x[0]) for _ in range(2)] for _ in range(2))

            def at(ts, i):
                return [t[i] for t in ts]

            def bi_fwd(i):
                if gru:
                    O32.gru_bi_fwd(at(x, i), U, rb, None, at(hprev, i), at(acts, i), out[i], N, T, u, seq=True)
                else:
                    O32.lstm_bi_fwd(at(x, i), U, None, at(hprev, i), at(acts, i), at(cseq, i), out[i], N, T, u,
                                    seq=True)

            def bi_bwd(i):
                if gru:
                    O32.gru_bi_bwd(at(acts, i), at(hprev, i), U, dh[i], at(dx, i), at(dr, i), N, T, u, False)
                else:
                    O32.lstm_bi_bwd(at(acts, i), at(cseq, i), U, dh[i], at(dx, i), N, T, u, False)

            def uni_fwd(i, d, xd):   # one direction's sweep over xd in its own time order
                if gru:
                    O32.gru_fwd(xd, U[d], rb[d], hs[d][i], hprev[d][i], acts[d][i], N, T, u)
                else:
                    O32.lstm_fwd(xd, U[d], hs[d][i], hprev[d][i], acts[d][i], cseq[d][i], N, T, u)

            def uni_bwd(i, d, dhd):
                if gru:
                    O32.gru_bwd(acts[d][i], hprev[d][i], U[d], dhd, dx[d][i], dr[d][i], N, T, u, False)
                else:
                    O32.lstm_bwd(acts[d][i], cseq[d][i], U[d], dhd, dx[d][i], N, T, u, False)

            def two_fwd(i):
                uni_fwd(i, 0, x[0][i])
                uni_fwd(i, 1, x[1][i])

            def composed_fwd(i):
                uni_fwd(i, 0, x[0][i])
                uni_fwd(i, 1, torch.flip(x[1][i], [1]))
                return torch.cat([hs[0][i], torch.flip(hs[1][i], [1])], -1)

            def two_bwd(i):
                uni_bwd(i, 0, hs[0][i])   # any dense [N, T, u] operand: the time is what counts here
                uni_bwd(i, 1, hs[1][i])

            def composed_bwd(i):
                uni_bwd(i, 0, dh[i][..., :u].contiguous())
                uni_bwd(i, 1, torch.flip(dh[i][..., u:], [1]))
                back = [torch.flip(dx[1][i], [1])] + ([torch.flip(dr[1][i], [1])] if gru else [])
                return [dx[0][i]] + back

            # the two routes give the same bits (the composed one last: its saved tensors are direction 1's flipped)
            bi_fwd(0)
            bi_bwd(0)
            want = [out[0].clone(), dx[0][0].clone(), dx[1][0].clone()] + ([dr[1][0].clone()] if gru else [])
            got = [composed_fwd(0)] + composed_bwd(0)
            same = all(torch.equal(a, b) for a, b in zip(want, got))
            for name, one, bi, two, comp in (("fwd", lambda i: uni_fwd(i, 0, x[0][i]), bi_fwd, two_fwd, composed_fwd),
                                             ("bwd", lambda i: uni_bwd(i, 0, hs[0][i]), bi_bwd, two_bwd, composed_bwd)):
                for i in range(nbuf):   # every set's h and saved tensors are some forward's before a backward is timed
                    composed_fwd(i)     # (direction 1's in one order or the other: the sweeps' time does not depend
                    bi_fwd(i)           # on the values)
                t1, _ = _med(one, nbuf, window, repeats)
                t2, _ = _med(two, nbuf, window, repeats)
                tc, _ = _med(comp, nbuf, window, repeats)
                tb, sp = _med(bi, nbuf, window, repeats)
                rows.append((cell, f"{N}, {T}, {u}", name, nbuf, 2 * -(-N // 16), tb * 1e6, sp, t1 * 1e6, t2 * 1e6,
                             tc * 1e6, tb / t1, tc / tb, same))
            del x, dh, out, hprev, cseq, hs, acts, dx, dr
            torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.2, help="least seconds of launches in a timed window")
    ap.add_argument("--repeats", type=int, default=3, help="windows per figure (median and spread)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench/birnn.py needs a GPU: nothing measured")
    rows = kernels(a.window, a.repeats)
    lines = ["| cell | N, T, units | sweep | operand sets | workgroups | bidirectional launch us | spread | one "
             "unidirectional sweep us | two unidirectional launches us | two launches + flip / concat / split copies us"
             " | bidirectional / one sweep | composed / bidirectional | same bits |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    lines += [f"| {c} | {s} | {k} | {n} | {wg} | {tb:.1f} | {100 * sp:.1f} % | {t1:.1f} | {t2:.1f} | {tc:.1f} | "
              f"{r1:.2f} | {rc:.2f} | {same} |" for c, s, k, n, wg, tb, sp, t1, t2, tc, r1, rc, same in rows]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
