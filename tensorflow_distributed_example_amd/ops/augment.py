"""Host (numpy float32) twin of the input stage (``csrc/include/tde_augment.h``, ``csrc/kernels/augment.hip``):
Keras ``RandomFlip`` / ``RandomTranslation`` / ``RandomRotation`` / ``RandomZoom`` as a pure function of (layer
seed, global step t, input-stage index j, local row r).

One Philox4x32-10 block per (row, step, layer): counter = (r, t >> 32, t, j), key = the layer's seed;
``u_q = (word_q >> 8) * 2**-24``.  A flip is horizontal iff its mode allows it and ``u0 < 0.5``, vertical iff its
mode allows it and ``u1 < 0.5``; a translation moves by ``dy = (lo_h + u2 (hi_h - lo_h)) H`` and
``dx = (lo_w + u3 (hi_w - lo_w)) W``, every operation rounded to float32 on its own, so ``row_params`` equals the
device's bit for bit.  Flips and ``"nearest"`` translations move whole pixels and equal the device's rows bit for
bit; ``"bilinear"`` sums the four neighbours in the device's order in float32, where the device may contract a
multiply-add (compared with a tolerance).

A rotation draws ``f = lo + u0 (hi - lo)`` turns and a zoom ``zh = 1 + (lo_h + u2 (hi_h - lo_h))``,
``zw = 1 + (lo_w + u3 (hi_w - lo_w))`` (``zw = zh`` when the width follows the height).  Both are the header's
general source-coordinate map ``sx = cx + (ax vx - bx vy)``, ``sy = cy + (ay vx + by vy)`` about the image centre,
with ``ax = by = c``, ``bx = ay = s`` for a rotation (``sincos``: the header's own polynomials, bit for bit) and
``ax = zw``, ``by = zh``, ``bx = ay = 0`` for a zoom.  Draws, c, s and every source coordinate equal the device's bit
for bit, so ``"nearest"`` rows do too; ``"bilinear"`` rows are compared with the translation's tolerance.

``AugLayer`` / ``AugSpec`` are the ctypes twins of the header's structs; ``stage_spec`` builds them from a model's
input-stage layers, ``apply`` is the transform of a batch group and ``stage_rows`` the device launch.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import philox

MAX_LAYERS = 4
FLIP, TRANSLATE, ROTATE, ZOOM = 0, 1, 2, 3
KIND_NAMES = {FLIP: "RandomFlip", TRANSLATE: "RandomTranslation", ROTATE: "RandomRotation", ZOOM: "RandomZoom"}
AFFINE_MAX_DIM = 1 << 20   # kAugAffineMaxDim
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


def rotate_layer(factor, fill_mode, interpolation, fill_value, j, seed):
    """``factor``: the (lo, hi) range in turns."""
    return AugLayer(ROTATE, FILL_MODES[fill_mode], 1 if interpolation == "bilinear" else 0, int(j),
                    int(seed) & (2 ** 64 - 1), factor[0], factor[1], 0.0, 0.0, fill_value, 0)


def zoom_layer(height, width, fill_mode, interpolation, fill_value, j, seed):
    """``height`` / ``width``: the (lo, hi) factor ranges; ``width=None``: the width zooms by the height's draw."""
    w = (0.0, 0.0) if width is None else width
    return AugLayer(ZOOM, FILL_MODES[fill_mode], 1 if interpolation == "bilinear" else 0, int(j),
                    int(seed) & (2 ** 64 - 1), height[0], height[1], w[0], w[1], fill_value, 1 if width is None else 0)


def interpolating(layers):
    """Indices of the layers that interpolate."""
    return [k for k, l in enumerate(layers) if l.kind != FLIP and l.bilinear]


def is_affine(spec):
    """The spec holds a rotation or a zoom: the device runs its general source-coordinate map."""
    return any(spec.layer[k].kind in (ROTATE, ZOOM) for k in range(spec.n))


def _one_interpolating(layers, names=None):
    ks = interpolating(layers)
    if len(ks) > 1:
        who = ", ".join(f"{names[k]!r} ({KIND_NAMES[layers[k].kind]})" if names else
                        f"layer {k} ({KIND_NAMES[layers[k].kind]})" for k in ks)
        raise ValueError(f"an input stage holds at most one interpolating layer (interpolation='bilinear'), got "
                         f"{len(ks)}: {who}; layers with interpolation='nearest' chain freely")


def make_spec(layers, names=None):
    layers = list(layers)
    if len(layers) > MAX_LAYERS:
        raise ValueError(f"an input stage holds at most {MAX_LAYERS} layers (got {len(layers)})")
    if sum(l.kind == TRANSLATE and l.bilinear for l in layers) > 1:
        raise ValueError("an input stage holds at most one RandomTranslation with interpolation='bilinear'")
    _one_interpolating(layers, names)
    s = AugSpec()
    s.n = len(layers)
    for k, l in enumerate(layers):
        s.layer[k] = l
    return s


def stage_spec(stage):
    """The ``AugSpec`` of a model's input-stage layers (``Model.input_stage``), seeds resolved."""
    stage = list(stage)
    return make_spec((l.aug_layer(j) for j, l in enumerate(stage)), [l.name for l in stage])


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


def _draw1(lo, hi, u):
    lo, hi = _f(lo), _f(hi)
    return (lo + (u * (hi - lo)).astype(_f)).astype(_f)


# aug_sincos's Taylor coefficients of sin(pi r / 2) / r and cos(pi r / 2) in r^2, highest first
_SIN = [_f(float.fromhex(h)) for h in ("0x1.507834p-13", "-0x1.32d2ccp-8", "0x1.466bc6p-4", "-0x1.4abbcep-1",
                                       "0x1.921fb6p+0")]
_COS = [_f(float.fromhex(h)) for h in ("-0x1.a6d1f2p-16", "0x1.e1f506p-11", "-0x1.55d3c8p-6", "0x1.03c1fp-2",
                                       "-0x1.3bd3ccp+0")]


def sincos(f):
    """(cos(2 pi f), sin(2 pi f)) of float32 turns ``f``, |f| <= 1, as tde_augment.h aug_sincos computes them."""
    f = np.asarray(f, dtype=_f)
    f4 = (_f(4.0) * f).astype(_f)
    q = np.rint(f4).astype(_f)
    r = (f4 - q).astype(_f)
    r2 = (r * r).astype(_f)
    ps = np.full_like(r, _SIN[0])
    for c in _SIN[1:]:
        ps = (c + (r2 * ps).astype(_f)).astype(_f)
    sr = (r * ps).astype(_f)
    pc = np.full_like(r, _COS[0])
    for c in _COS[1:]:
        pc = (c + (r2 * pc).astype(_f)).astype(_f)
    cr = (_f(1.0) + (r2 * pc).astype(_f)).astype(_f)
    qi = q.astype(np.int64) & 3
    zero = _f(0.0)
    c = np.select([qi == 0, qi == 1, qi == 2], [cr, zero - sr, zero - cr], sr).astype(_f)
    s = np.select([qi == 0, qi == 1, qi == 2], [sr, cr, zero - sr], zero - cr).astype(_f)
    return c, s


def layer_rows(layer, t, rows, H, W):
    """One layer's draws for local rows 0..rows-1 at step ``t``: dict(hflip, vflip) of bool arrays for a flip,
    dict(dy, dx) of float32 arrays for a translation, dict(f, c, s) for a rotation, dict(zh, zw) for a zoom."""
    u = units(int(layer.seed), t, int(layer.j), rows)
    if layer.kind == FLIP:
        return dict(hflip=bool(layer.mode & 1) & (u[:, 0] < _f(0.5)), vflip=bool(layer.mode & 2) & (u[:, 1] < _f(0.5)))
    if layer.kind == ROTATE:
        f = _draw1(layer.lo_h, layer.hi_h, u[:, 0])
        c, s = sincos(f)
        return dict(f=f, c=c, s=s)
    if layer.kind == ZOOM:
        zh = (_f(1.0) + _draw1(layer.lo_h, layer.hi_h, u[:, 2])).astype(_f)
        zw = zh if layer.pad_ else (_f(1.0) + _draw1(layer.lo_w, layer.hi_w, u[:, 3])).astype(_f)
        return dict(zh=zh, zw=zw)
    return dict(dy=_draw(layer.lo_h, layer.hi_h, u[:, 2], H), dx=_draw(layer.lo_w, layer.hi_w, u[:, 3], W))


def params_width(spec):
    """Floats per row of the device's ``params``: 4, or 4 per layer slot for a spec with a rotation or a zoom."""
    return 4 * MAX_LAYERS if is_affine(spec) else 4


def row_params(spec, t, rows, H, W):
    """What the device writes to ``params``, float32 [rows, params_width(spec)]: the composed ``(hflip, vflip, dy,
    dx)``, or for a spec with a rotation or a zoom each layer's own draws, [rows][MAX_LAYERS][4]: flip
    ``(hflip, vflip, 0, 0)``, translation ``(dy, dx, 0, 0)``, rotation ``(f, c, s, 0)``, zoom ``(zh, zw, 0, 0)``."""
    if is_affine(spec):
        out = np.zeros((rows, MAX_LAYERS, 4), _f)
        keys = {FLIP: ("hflip", "vflip"), TRANSLATE: ("dy", "dx"), ROTATE: ("f", "c", "s"), ZOOM: ("zh", "zw")}
        for k in range(spec.n):
            d = layer_rows(spec.layer[k], t, rows, H, W)
            for q, name in enumerate(keys[spec.layer[k].kind]):
                out[:, k, q] = d[name]
        return out.reshape(rows, 4 * MAX_LAYERS)
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


def affine_row(img, layer, ax, bx, ay, by):
    """One RandomRotation / RandomZoom of img[H, W, C] float32: the source-coordinate map
    ``sx = cx + (ax vx - bx vy)``, ``sy = cy + (ay vx + by vy)`` in float32, operation by operation."""
    H, W = img.shape[0], img.shape[1]
    if max(H, W) > AFFINE_MAX_DIM:
        raise ValueError(f"a rotation or zoom takes images of at most {AFFINE_MAX_DIM} rows and columns")
    ax, bx, ay, by = _f(ax), _f(bx), _f(ay), _f(by)
    cy, cx = _f(_f(H - 1) * _f(0.5)), _f(_f(W - 1) * _f(0.5))
    vy = (np.arange(H, dtype=_f) - cy).astype(_f)[:, None]
    vx = (np.arange(W, dtype=_f) - cx).astype(_f)[None, :]
    sx = (cx + ((ax * vx).astype(_f) - (bx * vy).astype(_f)).astype(_f)).astype(_f)
    sy = (cy + ((ay * vx).astype(_f) + (by * vy).astype(_f)).astype(_f)).astype(_f)
    fill, cval = layer.mode, _f(layer.fill_value)

    def at(iy, ix):
        iy, oky = _index(fill, H, iy)
        ix, okx = _index(fill, W, ix)
        return np.where((oky & okx)[:, :, None], img[iy, ix], cval).astype(_f)

    if not layer.bilinear:
        return at(np.floor((sy + _f(0.5)).astype(_f)).astype(np.int64),
                  np.floor((sx + _f(0.5)).astype(_f)).astype(np.int64))
    y0, x0 = np.floor(sy), np.floor(sx)
    fy, fx = (sy - y0).astype(_f), (sx - x0).astype(_f)
    y0, x0 = y0.astype(np.int64), x0.astype(np.int64)
    wy = ((_f(1.0) - fy).astype(_f), fy)
    wx = ((_f(1.0) - fx).astype(_f), fx)
    acc = None
    for tap in range(4):
        v = at(y0 + (tap >> 1), x0 + (tap & 1))
        term = ((wy[tap >> 1] * wx[tap & 1]).astype(_f)[:, :, None] * v).astype(_f)
        acc = term if acc is None else (acc + term).astype(_f)
    return np.where(((fy == 0) & (fx == 0))[:, :, None], at(y0, x0), acc).astype(_f)   # no fraction: the pixel copied


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
                elif layer.kind == ROTATE:
                    out[i] = affine_row(out[i], layer, d["c"][r], d["s"][r], d["s"][r], d["c"][r])
                elif layer.kind == ZOOM:
                    out[i] = affine_row(out[i], layer, d["zw"][r], 0.0, 0.0, d["zh"][r])
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
