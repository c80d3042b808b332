"""Float64 oracle of the optimizer update (csrc/include/tde_optim.h) and the fixtures of the optimizer
kernel tests (tests/test_optim_oracle.py on the CPU, tests/test_optim_gpu.py on the GPU).

``oracle_step`` is the header's formulas in float64 on the float32-rounded hyper-parameters: the kernels
receive floats, so this is the exact result of the operation they are asked to do.  ``fp32_step`` is
``opt_step``'s operation order in torch float32 on the host (one sample of what fp32 arithmetic loses).

The exact grid: lr = 2^-3, mom = 2^-1 and every weight, gradient and initial slot a multiple of 2^-6 below
4 in magnitude (gradient replicas: up to 8 of them, a sum below 32; grad_scale 2^-2).  After three steps every
product and sum is a multiple of 2^-14 below 2^7, 21 bits (tests/test_optim_oracle.py checks it), so each
fp32 operation is exact whether or not the compiler contracts a multiply and an add, and the kernel has to
equal the oracle bit for bit.  The values of element
i are ((a i + c) mod p - p // 2) / 64 with a different prime p < 512 for w, g and the slot: w alone is
distinct over any 509 consecutive elements and the triple (w, g, slot) over 509 * 503 * 499, so an element
written to a wrong place, skipped or updated twice gives a different number.
"""
from __future__ import annotations

import types

import numpy as np
import torch

KINDS = ("sgd", "momentum", "nesterov", "adam")
KIND_ID = {"sgd": 0, "momentum": 1, "nesterov": 2, "adam": 3}
GRID_HYPER = dict(lr=0.125, mom=0.5, b1=0.9, b2=0.999, eps=1e-7)

# Every awkward segment in one store: (name, shape, shadows).  Shadowed with "col" -> the 16 x 64 tile path
# (2-D view [prod(shape[:-1]), shape[-1]], a 1-D shape is one row); everything else -> the 1-D path in
# 2048-element chunks of two 1024-element sub-iterations.  The small-row tiles come first and the two
# largest shadows last, so no shadow of a small tensor ends the shadow buffer.
SEGMENTS = [
    ("v1", (1,), None),                      # scalar tail only
    ("t5x130", (5, 130), ("row", "col")),    # three column tiles, cols % 4 != 0, last tile 2 wide
    ("v10", (10,), ("row",)),                # two float4 and a 2-element scalar tail, row shadow both ways
    ("t1x4", (1, 4), ("row", "col")),        # rows = 1
    ("t70", (70,), ("col",)),                # 1-D shape on the tile path: rows = 1, two column tiles, scalar
    ("v1023", (1023,), ("row",)),            # ends 1 short of a sub-iteration: 3-element scalar tail
    ("t15x60", (15, 60), ("row", "col")),    # row tail, one partial column tile, float4 branch
    ("v1027", (1027,), None),                # crosses a sub-iteration by 3
    ("t16x64", (16, 64), ("row", "col")),    # exactly one tile
    ("v2047", (2047,), None),                # 1 short of a chunk
    ("t17x64", (17, 64), ("row", "col")),    # second row tile of one row
    ("conv3x3x1x6", (3, 3, 1, 6), None),     # conv kernel without a shadow: 54 elements, 1-D path
    ("t64x10", (64, 10), ("row", "col")),    # cols % 4 != 0, one column tile
    ("v2049", (2049,), ("row",)),            # crosses a chunk by 1: a chunk of one scalar element
    ("t33x65", (33, 65), ("row", "col")),    # cols % 4 != 0, second column tile 1 wide, row tail of 1
    ("t20x68", (20, 68), ("col",)),          # cols % 4 == 0 with a partial second tile, no row shadow
    ("v4100", (4100,), ("row",)),            # three chunks, the last one float4 only
    ("t147x64", (147, 64), ("col",)),        # ten row tiles with a tail of 3, no row shadow
]
SHAPES = [(n, s) for n, s, _ in SEGMENTS]
SHADOWS = {n: sh for n, _, sh in SEGMENTS if sh}

W_SENTINEL = -7777.25     # fp32 value of the alignment gaps of w / g / the slots
SH_SENTINEL = -7776.0     # bf16 value of the round-to-8 gaps of the shadow buffer


def f32(x) -> float:
    """x rounded to float32, as a Python float."""
    return float(np.float32(x))


def hyper32(hyper: dict) -> dict:
    return {k: f32(v) for k, v in hyper.items()}


def lr_t64(hyper: dict, t) -> float:
    """Adam's bias-corrected step size in float64 on the float32 hyper-parameters; t < 1 is treated as 1."""
    h = hyper32(hyper)
    t = max(int(t), 1)
    return h["lr"] * np.sqrt(1.0 - h["b2"] ** t) / (1.0 - h["b1"] ** t)


def oracle_step(kind, hyper, w, g, m, v, t, grad_scale=1.0):
    """One update on float64 tensors; returns the new (w, m, v) and modifies nothing.  ``m`` is the momentum
    slot of momentum / nesterov and Adam's first moment; slots a kind does not use come back unchanged."""
    assert all(x is None or x.dtype == torch.float64 for x in (w, g, m, v))
    h = hyper32(hyper)
    g = g * f32(grad_scale)
    if kind == "sgd":
        return w - h["lr"] * g, m, v
    if kind in ("momentum", "nesterov"):
        nv = h["mom"] * m - h["lr"] * g
        return (w + h["mom"] * nv - h["lr"] * g if kind == "nesterov" else w + nv), nv, v
    assert kind == "adam"
    m = h["b1"] * m + (1.0 - h["b1"]) * g
    v = h["b2"] * v + (1.0 - h["b2"]) * g * g
    return w - lr_t64(hyper, t) * m / (v.sqrt() + h["eps"]), m, v


def fp32_step(kind, hyper, w, g, m, v, t, grad_scale=1.0):
    """``opt_step`` operation by operation in torch float32 (no contraction); lr_t is the float64 value
    rounded once, so what the kernel's own ``opt_lr_t`` loses is not part of this sample."""
    assert all(x is None or x.dtype == torch.float32 for x in (w, g, m, v))
    h = {k: torch.tensor(x, dtype=torch.float32) for k, x in hyper.items()}
    one = torch.tensor(1.0, dtype=torch.float32)
    g = g * torch.tensor(grad_scale, dtype=torch.float32)
    if kind == "sgd":
        return w - h["lr"] * g, m, v
    if kind in ("momentum", "nesterov"):
        nv = h["mom"] * m - h["lr"] * g
        return (w + h["mom"] * nv - h["lr"] * g if kind == "nesterov" else w + nv), nv, v
    assert kind == "adam"
    m = h["b1"] * m + (one - h["b1"]) * g
    v = h["b2"] * v + (one - h["b2"]) * g * g
    lr_t = torch.tensor(lr_t64(hyper, t), dtype=torch.float32)
    return w - lr_t * m / (v.sqrt() + h["eps"]), m, v


def grid(idx, p, a, c):
    """Exact-grid values of the elements ``idx`` (int64 tensor): multiples of 2^-6 in (-4, 4), float64."""
    assert p < 512
    return ((idx * a + c) % p - p // 2).double() / 64.0


def grid_w(idx):
    return grid(idx, 509, 101, 7)


def grid_slot(idx):
    return grid(idx, 499, 211, 3)


def grid_g(idx, step, rep=0):
    return grid(idx, 503, 157, 11 + 37 * step + 101 * rep)


# ------------------------------------------------------------------------------------------- store
def _zeros(shape, gen=None):
    return np.zeros(shape, dtype=np.float32)


def make_store(shapes, device):
    """A ``ParamStore`` of trainable, zero-initialised variables from (name, shape) pairs."""
    from tensorflow_distributed_example_amd.train.params import ParamStore
    specs = [types.SimpleNamespace(full_name=n, shape=tuple(s), trainable=True, aggregation="none",
                                   initializer=_zeros) for n, s in shapes]
    return ParamStore(specs, device)


def seg_mask(store):
    """bool[n_trainable]: True inside a segment, False in the alignment gaps."""
    mask = torch.zeros(store.n_trainable, dtype=torch.bool)
    for name in store.names(trainable=True):
        s = store.segments[name]
        mask[s.offset: s.offset + s.numel] = True
    return mask


def view2d(store, name, flat):
    """The segment of the flat tensor ``flat`` in the optimizer kernel's 2-D view."""
    s = store.segments[name]
    rows, cols = (int(np.prod(s.shape[:-1])), s.shape[-1]) if len(s.shape) >= 2 else (1, s.numel)
    return flat[s.offset: s.offset + s.numel].view(rows, cols)


def _bits(t):
    return t.detach().cpu().contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def fill_store_gaps(store):
    """Writes the sentinel into the alignment gaps of w, g and every slot buffer; returns the snapshot
    ``assert_store_gaps`` compares with."""
    gap = (~seg_mask(store)).to(store.device)
    assert int(gap.sum()) > 0
    bufs = {"w": store.w, "g": store.g, **{f"slot {k}": b for k, b in store.slots.items()}}
    for b in bufs.values():
        b[gap] = W_SENTINEL
    return {k: _bits(b[gap]) for k, b in bufs.items()}


def assert_store_gaps(store, snap):
    gap = (~seg_mask(store)).to(store.device)
    bufs = {"w": store.w, "g": store.g, **{f"slot {k}": b for k, b in store.slots.items()}}
    assert set(bufs) == set(snap)
    for k, b in bufs.items():
        assert torch.equal(_bits(b[gap]), snap[k]), f"alignment gap of {k} written"


def shadow_mask(ok):
    """bool over ``OptimizerKernel.shadow``: True inside a shadow view."""
    mask = torch.zeros(ok.shadow.numel(), dtype=torch.bool)
    for view in ok.shadow_views.values():
        off = view.storage_offset() - ok.shadow.storage_offset()
        assert not mask[off: off + view.numel()].any()
        mask[off: off + view.numel()] = True
    return mask


def fill_shadow_gaps(ok):
    gap = (~shadow_mask(ok)).to(ok.shadow.device)
    assert int(gap.sum()) > 0
    ok.shadow[gap] = SH_SENTINEL
    return _bits(ok.shadow[gap])


def assert_shadow_gaps(ok, snap):
    gap = (~shadow_mask(ok)).to(ok.shadow.device)
    assert torch.equal(_bits(ok.shadow[gap]), snap), "gap of the shadow buffer written"


def first_diff(a, b, bitwise=True):
    """'' when the tensors are equal (bit for bit, or value for value: -0 == +0), else a description of the
    first differing element."""
    a, b = a.detach().cpu().reshape(-1), b.detach().cpu().reshape(-1)
    if a.shape != b.shape or a.dtype != b.dtype:
        return f"{a.dtype} {tuple(a.shape)} != {b.dtype} {tuple(b.shape)}"
    ne = ((_bits(a) != _bits(b)) if bitwise else (a != b)).nonzero().reshape(-1)
    if ne.numel() == 0:
        return ""
    i = int(ne[0])
    return f"{ne.numel()} of {a.numel()} differ, first at {i}: {a[i].item()!r} != {b[i].item()!r}"
