"""Float64 oracle of gradient clipping (csrc/include/tde_clip.h) over a segment list, and the fixtures of
tests/test_grad_clip.py (CPU) and tests/test_grad_clip_gpu.py (GPU).

``segments`` is a list of (offset, numel) into a flat gradient; what lies between the segments (the alignment
gaps of ``store.g``) takes no part.  Semantics (TF 2.4+: the aggregated gradient is clipped):

  clipvalue        g <- min(max(g, -c), c)
  clipnorm         g <- g * (c / max(||g||_2, c)), one norm per segment
  global_clipnorm  the same with one norm over all segments

The error bound of the device's norm and scale follows the kernel's summation order (csrc/kernels/gradclip.hip):
16 fmaf + 6 wave levels + 3 adds = 25 float32 roundings on the longest path of a partial, the float64 sums
over the partials add nothing at that scale, then the cast to float32, the root and the divide: ROUNDINGS = 28.
The tests allow twice that count of 2^-24, halved for the root.
"""
from __future__ import annotations

import numpy as np
import torch

MODES = ("clipvalue", "clipnorm", "global_clipnorm")
MODE_ID = {"clipvalue": 1, "clipnorm": 2, "global_clipnorm": 3}
CHUNK = 4096            # kClipChunk: elements per sum-of-squares workgroup
ROUNDINGS = 28
NORM_TOL = 2 * ROUNDINGS * 2.0 ** -24 / 2     # relative, norm and scale alike

# the three extra segments of the issue and the long one for the strided loop of the scale kernel
EXTRA_SEGMENTS = [("c1", (1,), None), ("cchunk", (CHUNK,), None), ("cchunk5", (CHUNK + 5,), None)]
LONG_SEGMENT = ("c300", (300 * CHUNK + 3,), None)


def store_segments(store):
    """[(offset, numel)] of the trainable variables of a ``ParamStore``, in the optimizer kernel's order."""
    return [(store.segments[n].offset, store.segments[n].numel) for n in store.names(trainable=True)]


def norms(g, segments, mode):
    """float64 tensor: one norm per segment (``clipnorm``) or one in all (``global_clipnorm``)."""
    g = g.detach().cpu().double()
    sq = torch.stack([g[o: o + n].square().sum() for o, n in segments])
    return sq.sqrt() if mode == "clipnorm" else sq.sum().sqrt().reshape(1)


def scales(nrm, c):
    """c / max(norm, c) in float64: exactly 1 where norm <= c (a zero gradient included)."""
    return float(c) / torch.clamp(nrm, min=float(c))


def clip(g, segments, mode, c):
    """The clipped flat gradient in float64; elements outside the segments are returned unchanged."""
    out = g.detach().cpu().double().clone()
    if mode == "clipvalue":
        for o, n in segments:
            out[o: o + n] = out[o: o + n].clamp(-float(c), float(c))
        return out
    s = scales(norms(g, segments, mode), c)
    for i, (o, n) in enumerate(segments):
        out[o: o + n] = out[o: o + n] * s[i if mode == "clipnorm" else 0]
    return out


def clip_named(grads, mode, c):
    """The same over {name: tensor} (the gradients of tests/smallnet_oracle.py), in float64."""
    names = list(grads)
    flat = torch.cat([grads[n].detach().double().reshape(-1) for n in names])
    segs, o = [], 0
    for n in names:
        segs.append((o, grads[n].numel()))
        o += grads[n].numel()
    out = clip(flat, segs, mode, c)
    return {n: out[o: o + k].view(grads[n].shape) for n, (o, k) in zip(names, segs)}


def chunks(numel):
    return (numel + CHUNK - 1) // CHUNK


def table(segments):
    """What tde_clip_build_table has to produce: ([(seg, chunk)], [(first, count)])."""
    ents, ranges = [], []
    for i, (_, n) in enumerate(segments):
        ranges.append((len(ents), chunks(n)))
        ents += [(i, c) for c in range(chunks(n))]
    return ents, ranges


def dyadic_gradient(n_flat, segments, mode, sentinel):
    """A flat float32 gradient whose sums of squares and norms are exact powers of two whatever the order:
    every segment holds 4^a nonzero elements of value 2^b (so ||seg||^2 = 4^(a + b), every partial sum an
    integer multiple of 4^b below 2^24 of them); under ``global_clipnorm`` the segment sums are then made to
    add up to a power of four as well.  The gaps hold ``sentinel``.  -> (g, float64 norms)."""
    g = torch.full((n_flat,), float(sentinel), dtype=torch.float32)
    sq = []
    if mode == "global_clipnorm":
        # 1024 elements of +-1/2 in all: the last element of every segment, the rest in the largest segment
        big = max(range(len(segments)), key=lambda i: segments[i][1])
        assert len(segments) <= 512 and segments[big][1] >= 2048
        for i, (o, n) in enumerate(segments):
            seg = torch.zeros(n, dtype=torch.float32)
            seg[n - 1] = 0.5
            if i == big:
                k = 1024 - len(segments)
                seg[torch.arange(k) * ((n - 1) // k)] = 0.5 * (1.0 - 2.0 * (torch.arange(k) % 2))
            g[o: o + n] = seg
        assert int((g == 0.5).sum() + (g == -0.5).sum()) == 1024
        return g, torch.tensor([16.0], dtype=torch.float64)
    for i, (o, n) in enumerate(segments):
        a = min(int(np.log2(n) // 2), 5)
        k, b = 4 ** a, (i % 5) - 2
        seg = torch.zeros(n, dtype=torch.float32)
        idx = torch.arange(k) * (n // k)
        if k > 1:
            idx[-1] = n - 1       # the last element of the segment takes part: the ragged tail
        seg[idx] = (2.0 ** b) * (1.0 - 2.0 * (torch.arange(k) % 2))
        g[o: o + n] = seg
        sq.append(float(k) * 4.0 ** b)
    return g, torch.tensor(sq, dtype=torch.float64).sqrt()
