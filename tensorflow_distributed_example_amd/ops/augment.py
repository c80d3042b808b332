"""Host (numpy float32) twin of the input stage (``csrc/include/tde_augment.h``, ``csrc/kernels/augment.hip``):
Keras ``RandomFlip`` / ``RandomTranslation`` as a pure function of (layer seed, global step t, input-stage index j,
local row r).

One Philox4x32-10 block per (row, step, layer): counter = (r, t >> 32, t, j), key = the layer's seed;
``u_q = (word_q >> 8) * 2**-24``.  A flip is horizontal iff its mode allows it and ``u0 < 0.5``, vertical iff its
mode allows it and ``u1 < 0.5``; a translation moves by ``dy = (lo_h + u2 (hi_h - lo_h)) H`` and
``dx = (lo_w + u3 (hi_w - lo_w)) W``, every operation rounded to float32 on its own, so ``row_params`` equals the
device's bit for bit.  Flips and ``"nearest"`` translations move whole pixels and equal the device's rows bit for
bit; ``"bilinear"`` sums the four neighbours in the device's order in float32, where the device may contract a
multiply-add (compared with a tolerance).

``AugLayer`` / ``AugSpec`` are the ctypes twins of the header's structs; ``stage_spec`` builds them from a model's
input-stage layers, ``apply`` is the transform of a batch group and ``stage_rows`` the device launch.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import philox

MAX_LAYERS = 4
FLIP, TRANSLATE = 0, 1
FILL_MODES = {"constant": 0, "nearest": 1, "reflect": 2, "wrap": 3}
FLIP_MODES = {"horizontal": 1, "vertical": 2, "horizontal_and_vertical": 3}
DTYPES = {"float32": 0, "bfloat16": 1}

_f = np.float32


class AugLayer(C.Structure):
    _fields_ = [("kind", C.c_int), ("mode", C.c_int), ("bilinear", C.c_int), ("j", C.c_int),
                ("seed", C.c_ulonglong), ("lo_h", C.c_float), ("hi_h", C.c_float), ("lo_w", C.c_float),
                ("hi_w", C.c_float), ("fill_value", C.c_float), ("pad_", C.c_int)]


class AugSpec(C.Structure):
    _fields_ = [("n", C.c_int), ("pad_", C.c_int), ("layer", AugLayer * MAX_LAYERS)]


def flip_layer(mode, j, seed):
    return AugLayer(FLIP, FLIP_MODES[mode], 0, int(j), int(seed) & (2 ** 64 - 1), 0.0, 0.0, 0.0, 0.0, 0.0, 0)


def translate_layer(height, width, fill_mode, interpolation, fill_value, j, seed):
    """``height`` / ``width``: the (lo, hi) factor ranges."""
    return AugLayer(TRANSLATE, FILL_MODES[fill_mode], 1 if interpolation == "bilinear" else 0, int(j),
                    int(seed) & (2 ** 64 - 1), height[0], height[1], width[0], width[1], fill_value, 0)


def make_spec(layers):
    layers = list(layers)
    if len(layers) > MAX_LAYERS:
        raise ValueError(f"an input stage holds at most {MAX_LAYERS} layers (got {len(layers)})")
    if sum(l.kind == TRANSLATE and l.bilinear for l in layers) > 1:
        raise ValueError("an input stage holds at most one RandomTranslation with interpolation='bilinear'")
    s = AugSpec()
    s.n = len(layers)
    for k, l in enumerate(layers):
        s.layer[k] = l
    return s


def stage_spec(stage):
    """The ``AugSpec`` of a model's input-stage layers (``Model.input_stage``), seeds resolved."""
    return make_spec(l.aug_layer(j) for j, l in enumerate(stage))


# ------------------------------------------------------------------------------------ the draws
def units(seed, t, j, rows):
    """``u[rows, 4]`` float32 of local rows 0..rows-1 at step ``t`` of input-stage layer ``j``."""
    r = np.arange(rows, dtype=np.uint64)
    t = int(t) & (2 ** 64 - 1)
    ctr = np.stack([r.astype(np.uint32), np.full(rows, t >> 32, np.uint32), np.full(rows, t & 0xFFFFFFFF, np.uint32),
                    np.full(rows, j & 0xFFFFFFFF, np.uint32)], axis=-1)
    key = np.broadcast_to(np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], np.uint32), (rows, 2))
    w = philox.philox4x32_10(ctr, key)
    return (w >> np.uint32(8)).astype(np.float32) * _f(1.0 / 16777216.0)


def _draw(lo, hi, u, n):
    lo, hi = _f(lo), _f(hi)
    return ((lo + (u * (hi - lo)).astype(_f)).astype(_f) * _f(n)).astype(_f)


def layer_rows(layer, t, rows, H, W):
    """One layer's draws for local rows 0..rows-1 at step ``t``: dict(hflip, vflip) of bool arrays for a flip,
    dict(dy, dx) of float32 arrays for a translation."""
    u = units(int(layer.seed), t, int(layer.j), rows)
    if layer.kind == FLIP:
        return dict(hflip=bool(layer.mode & 1) & (u[:, 0] < _f(0.5)), vflip=bool(layer.mode & 2) & (u[:, 1] < _f(0.5)))
    return dict(dy=_draw(layer.lo_h, layer.hi_h, u[:, 2], H), dx=_draw(layer.lo_w, layer.hi_w, u[:, 3], W))


def row_params(spec, t, rows, H, W):
    """The composed ``(hflip, vflip, dy, dx)`` float32 [rows, 4] the device writes to ``params``."""
    hf = np.zeros(rows, bool)
    vf = np.zeros(rows, bool)
    dy = np.zeros(rows, _f)
    dx = np.zeros(rows, _f)
    for k in range(spec.n):
        d = layer_rows(spec.layer[k], t, rows, H, W)
        if spec.layer[k].kind == FLIP:
            hf ^= d["hflip"]
            vf ^= d["vflip"]
        else:
            dy = (dy + d["dy"]).astype(_f)
            dx = (dx + d["dx"]).astype(_f)
    return np.stack([hf.astype(_f), vf.astype(_f), dy, dx], axis=-1)


# ------------------------------------------------------------------------------------ the transform
def _index(fill, n, i):
    """Source indices ``i`` (int array) of an axis of ``n`` entries through the fill mode -> (indices, inside)."""
    i = np.asarray(i, dtype=np.int64)
    ok = (i >= 0) & (i < n)
    if fill == FILL_MODES["constant"]:
        return np.where(ok, i, 0), ok
    if fill == FILL_MODES["nearest"]:
        return np.clip(i, 0, n - 1), np.ones_like(ok)
    if fill == FILL_MODES["reflect"]:
        m = np.mod(i, 2 * n)
        return np.where(m < n, m, 2 * n - 1 - m), np.ones_like(ok)
    return np.mod(i, n), np.ones_like(ok)


def _take(img, fill, cval, sy, sx):
    """img[H, W, C] at rows ``arange(H) + sy`` / columns ``arange(W) + sx`` through the fill mode."""
    H, W = img.shape[0], img.shape[1]
    iy, oky = _index(fill, H, np.arange(H) + sy)
    ix, okx = _index(fill, W, np.arange(W) + sx)
    out = img[iy][:, ix]
    inside = oky[:, None] & okx[None, :]
    return np.where(inside[:, :, None], out, _f(cval)).astype(_f)


def _split(d):
    """Shift and fraction of one axis of a bilinear translation by float32 ``d`` (tde_augment.h aug_split)."""
    di = np.floor(d).astype(_f)
    a = _f(d - di)
    if a > 0:
        return -int(di) - 1, _f(_f(1.0) - a)
    return -int(di), _f(0.0)


def translate_row(img, layer, dy, dx):
    """One RandomTranslation of img[H, W, C] float32 by float32 (dy, dx)."""
    dy, dx = _f(dy), _f(dx)
    cval = layer.fill_value
    if not layer.bilinear:
        return _take(img, layer.mode, cval, int(np.floor(_f(_f(0.5) - dy))), int(np.floor(_f(_f(0.5) - dx))))
    sy, fy = _split(dy)
    sx, fx = _split(dx)
    if fy == 0 and fx == 0:
        return _take(img, layer.mode, cval, sy, sx)
    wy = (_f(_f(1.0) - fy), fy)
    wx = (_f(_f(1.0) - fx), fx)
    acc = None
    for tap in range(4):
        v = _take(img, layer.mode, cval, sy + (tap >> 1), sx + (tap & 1))
        term = (_f(wy[tap >> 1] * wx[tap & 1]) * v).astype(_f)
        acc = term if acc is None else (acc + term).astype(_f)
    return acc


def apply(spec, x, B, step0):
    """``out[i] = T_{r = i mod B, t = step0 + i // B}(x[i])`` for x[n, H, W, C]; float32 in and out."""
    x = np.asarray(x, dtype=_f)
    n, H, W = x.shape[0], x.shape[1], x.shape[2]
    out = x.copy()
    if n == 0 or spec.n == 0:
        return out
    rows = min(B, n)
    for s in range((n + B - 1) // B):
        lo, hi = s * B, min(n, (s + 1) * B)
        for k in range(spec.n):
            layer = spec.layer[k]
            d = layer_rows(layer, step0 + s, rows, H, W)
            for i in range(lo, hi):
                r = i - lo
                if layer.kind == FLIP:
                    if d["vflip"][r]:
                        out[i] = out[i][::-1]
                    if d["hflip"][r]:
                        out[i] = out[i][:, ::-1]
                else:
                    out[i] = translate_row(out[i], layer, d["dy"][r], d["dx"][r])
    return out


# ------------------------------------------------------------------------------------ the device launch
def check_abi(lib):
    out = (C.c_longlong * 3)()
    if lib.tde_augment_abi(out, 3) != 3 or list(out) != [C.sizeof(AugSpec), C.sizeof(AugLayer), MAX_LAYERS]:
        raise RuntimeError(f"AugSpec ABI mismatch: library {list(out)}, host "
                           f"{[C.sizeof(AugSpec), C.sizeof(AugLayer), MAX_LAYERS]}")


def stage_rows(src, nrows, idx, n, B, shape, dst, spec, step0, bad, params=None):
    """Launch ``tde_stage_rows_aug`` on the current stream: torch device tensors ``src`` (the cache, or a staged
    group for ``idx=None``), ``dst`` (the ring) of one dtype, ``idx`` int32 or None, ``bad`` int32 [1]."""
    import torch
    from .. import _native as N
    if src.dtype != dst.dtype or src.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"tde_stage_rows_aug: float32 or bfloat16 rows of one dtype (got {src.dtype}, {dst.dtype})")
    H, W, Cc = (int(v) for v in shape)
    if src.numel() < int(nrows) * H * W * Cc or dst.numel() < int(n) * H * W * Cc:
        raise ValueError("tde_stage_rows_aug: a buffer is smaller than its rows")
    rc = N.hip().tde_stage_rows_aug(src.data_ptr(), 1 if src.dtype == torch.bfloat16 else 0, int(nrows), N.ptr(idx),
                                    int(n), int(B), H, W, Cc, dst.data_ptr(), C.byref(spec), int(step0),
                                    N.ptr(params), bad.data_ptr(), N.stream_ptr())
    N.check(rc, "tde_stage_rows_aug")
