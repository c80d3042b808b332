"""Float64 oracle of the input stage (RandomFlip / RandomTranslation), written from the definition in
csrc/include/tde_augment.h with per-pixel loops.  A plain helper module: tests/test_augment.py and
tests/test_augment_gpu.py import it.  It shares no code with ops/augment.py; the Philox block itself comes
from ops/philox.py, which tests/test_augment.py pins to the published known answers.

A layer is a dict: ``dict(kind="flip", mode=..., seed=, j=)`` or ``dict(kind="translate", height=(lo, hi),
width=(lo, hi), fill_mode=, interpolation=, fill_value=, seed=, j=)``.  A draw is what the layer does to one
row: ``dict(hflip=, vflip=)`` or ``dict(dy=, dx=)``.  ``draws`` derives them from (seed, t, j, r);
``transform`` evaluates a row of the stage's output pixel by pixel in float64 for given draws, so that a test
can also feed it the parameters a device reported.  ``transform_grid`` is the same evaluation with the pixel
loops run as array operations (tests/test_augment.py holds the two equal bit for bit), for tests that check
every row of many launches.
"""
import math
import struct

import numpy as np


def f32(v):
    """Round a Python float to float32 (one rounded operation of the definition)."""
    return struct.unpack("f", struct.pack("f", v))[0]


def layer_of(l, j, seed):
    """The oracle's description of a ``RandomFlip`` / ``RandomTranslation`` layer object."""
    if type(l).__name__ == "RandomFlip":
        return dict(kind="flip", mode=l.mode, seed=seed, j=j)
    return dict(kind="translate", height=l.height_range, width=l.width_range, fill_mode=l.fill_mode,
                interpolation=l.interpolation, fill_value=l.fill_value, seed=seed, j=j)


def draws(layer, r, t, H, W):
    from tensorflow_distributed_example_amd.ops.philox import philox4x32_10
    seed = layer["seed"]
    w = philox4x32_10(np.array([r, (t >> 32) & 0xFFFFFFFF, t & 0xFFFFFFFF, layer["j"]], dtype=np.uint32),
                      np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint32))
    u = [(int(v) >> 8) / 16777216.0 for v in w]          # 24 bits: exact in float32 and float64
    if layer["kind"] == "flip":
        m = layer["mode"]
        return dict(hflip=m in ("horizontal", "horizontal_and_vertical") and u[0] < 0.5,
                    vflip=m in ("vertical", "horizontal_and_vertical") and u[1] < 0.5)

    def draw(rng, uq, n):
        lo, hi = f32(rng[0]), f32(rng[1])
        return f32(f32(lo + f32(uq * f32(hi - lo))) * n)

    return dict(dy=draw(layer["height"], u[2], H), dx=draw(layer["width"], u[3], W))


def _fill(mode, n, i):
    """Index i of an axis of n entries through the fill mode, applied as often as needed; None: the constant."""
    if 0 <= i < n:
        return i
    if mode == "constant":
        return None
    if mode == "nearest":
        return 0 if i < 0 else n - 1
    while i < 0 or i >= n:
        if mode == "reflect":          # d c b a | a b c d | d c b a
            i = -1 - i if i < 0 else 2 * n - 1 - i
        else:                          # wrap
            i = i + n if i < 0 else i - n
    return i


def _pixel(img, layers, dr, k, y, x, c):
    """Channel c of pixel (y, x) of the output of layers 0..k (k = -1: the image)."""
    if k < 0:
        return float(img[y, x, c])
    H, W = img.shape[0], img.shape[1]
    l, d = layers[k], dr[k]
    if l["kind"] == "flip":
        return _pixel(img, layers, dr, k - 1, H - 1 - y if d["vflip"] else y, W - 1 - x if d["hflip"] else x, c)
    sy, sx = y - float(d["dy"]), x - float(d["dx"])
    mode, cval = l["fill_mode"], float(f32(l["fill_value"]))

    def at(iy, ix):
        iy, ix = _fill(mode, H, iy), _fill(mode, W, ix)
        return cval if iy is None or ix is None else _pixel(img, layers, dr, k - 1, iy, ix, c)

    if l["interpolation"] == "nearest":
        return at(math.floor(sy + 0.5), math.floor(sx + 0.5))
    y0, x0 = math.floor(sy), math.floor(sx)
    fy, fx = sy - y0, sx - x0
    return ((1 - fy) * (1 - fx) * at(y0, x0) + (1 - fy) * fx * at(y0, x0 + 1) + fy * (1 - fx) * at(y0 + 1, x0)
            + fy * fx * at(y0 + 1, x0 + 1))


def transform(img, layers, dr):
    """img[H, W, C] through ``layers`` with the draws ``dr`` (one per layer), float64."""
    img = np.asarray(img, dtype=np.float64)
    out = np.empty_like(img)
    for y in range(img.shape[0]):
        for x in range(img.shape[1]):
            for c in range(img.shape[2]):
                out[y, x, c] = _pixel(img, layers, dr, len(layers) - 1, y, x, c)
    return out


def _fill_grid(mode, n, i):
    """``_fill`` over an integer array -> (indices, inside): ``inside`` is False where the constant applies."""
    i = np.array(i, dtype=np.int64)
    inside = (i >= 0) & (i < n)
    if mode == "constant":
        return np.where(inside, i, 0), inside
    if mode == "nearest":
        return np.where(i < 0, 0, np.where(i >= n, n - 1, i)), np.ones_like(inside)
    while True:
        lo, hi = i < 0, i >= n
        if not (lo.any() or hi.any()):
            return i, np.ones_like(inside)
        if mode == "reflect":
            i = np.where(lo, -1 - i, np.where(hi, 2 * n - 1 - i, i))
        else:
            i = np.where(lo, i + n, np.where(hi, i - n, i))


def _grid(img, layers, dr, k, y, x):
    """``_pixel`` for integer arrays y, x of one shape -> values [..., C]: the same float64 operations in the
    same order, over all pixels at once."""
    if k < 0:
        return img[y, x]
    H, W = img.shape[0], img.shape[1]
    l, d = layers[k], dr[k]
    if l["kind"] == "flip":
        return _grid(img, layers, dr, k - 1, H - 1 - y if d["vflip"] else y, W - 1 - x if d["hflip"] else x)
    sy, sx = y - float(d["dy"]), x - float(d["dx"])
    mode, cval = l["fill_mode"], float(f32(l["fill_value"]))

    def at(iy, ix):
        iy, oky = _fill_grid(mode, H, iy)
        ix, okx = _fill_grid(mode, W, ix)
        return np.where((oky & okx)[..., None], _grid(img, layers, dr, k - 1, iy, ix), cval)

    if l["interpolation"] == "nearest":
        return at(np.floor(sy + 0.5).astype(np.int64), np.floor(sx + 0.5).astype(np.int64))
    y0, x0 = np.floor(sy), np.floor(sx)
    fy, fx = (sy - y0)[..., None], (sx - x0)[..., None]
    y0, x0 = y0.astype(np.int64), x0.astype(np.int64)
    return ((1 - fy) * (1 - fx) * at(y0, x0) + (1 - fy) * fx * at(y0, x0 + 1) + fy * (1 - fx) * at(y0 + 1, x0)
            + fy * fx * at(y0 + 1, x0 + 1))


def transform_grid(img, layers, dr):
    """``transform`` with the pixel loops run as array operations (tests/test_augment.py holds the two equal):
    what the GPU tests can afford on every row."""
    img = np.asarray(img, dtype=np.float64)
    y, x = np.meshgrid(np.arange(img.shape[0]), np.arange(img.shape[1]), indexing="ij")
    return _grid(img, layers, dr, len(layers) - 1, y, x)


def apply(layers, x, B, step0):
    """out[i] = T_{r = i mod B, t = step0 + i // B}(x[i]) for x[n, H, W, C], float64."""
    x = np.asarray(x, dtype=np.float64)
    H, W = x.shape[1], x.shape[2]
    return np.stack([transform(x[i], layers, [draws(l, i % B, step0 + i // B, H, W) for l in layers])
                     for i in range(x.shape[0])]) if len(x) else x.copy()


BILINEAR_BOUND = 6 * 2.0 ** -24   # x max|x|: four f32 weights, four products, three adds
