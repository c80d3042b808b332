"""Float64 oracle of the input stage with RandomRotation / RandomZoom layers, written from the definition in
csrc/include/tde_augment.h with plain per-pixel loops.  A plain helper module: tests/test_augment_affine.py and
tests/test_augment_affine_gpu.py import it.  It shares no code with ops/augment.py.

A layer is a dict with ``kind`` in ("flip", "translate", "rotate", "zoom"); all but the flip carry ``fill_mode``,
``interpolation`` and ``fill_value``.  A draw is what the layer does to one row, taken from the twin (or from what
a device reported): ``dict(hflip=, vflip=)``, ``dict(dy=, dx=)``, ``dict(f=)`` (turns) or ``dict(zh=, zw=)``.  The
oracle evaluates the drawn transform in float64 with the true cosine and sine: it knows nothing of the header's
polynomials or of float32 rounding.

``transform`` returns the image; ``coords`` the float64 source coordinates of a single rotation or zoom layer's
output pixels, from which a test finds the pixels that sit on a nearest-neighbour tie.
"""
import math

import numpy as np


def layer_of(l):
    """The oracle's description of a layer object of the input stage."""
    name = type(l).__name__
    if name == "RandomFlip":
        return dict(kind="flip")
    kind = {"RandomTranslation": "translate", "RandomRotation": "rotate", "RandomZoom": "zoom"}[name]
    return dict(kind=kind, fill_mode=l.fill_mode, interpolation=l.interpolation, fill_value=l.fill_value)


def _fill(mode, n, i):
    """Index i of an axis of n entries through the fill mode; None: the constant."""
    if 0 <= i < n:
        return i
    if mode == "constant":
        return None
    if mode == "nearest":
        return 0 if i < 0 else n - 1
    if mode == "reflect":          # d c b a | a b c d | d c b a: period 2n
        m = i % (2 * n)
        return m if m < n else 2 * n - 1 - m
    return i % n                   # wrap


def source(layer, d, H, W, y, x):
    """Float64 source coordinate (sy, sx) of output pixel (y, x) of a translate / rotate / zoom layer."""
    if layer["kind"] == "translate":
        return y - float(d["dy"]), x - float(d["dx"])
    cy, cx = (H - 1) / 2.0, (W - 1) / 2.0
    vy, vx = y - cy, x - cx
    if layer["kind"] == "rotate":
        a = 2.0 * math.pi * float(d["f"])
        c, s = math.cos(a), math.sin(a)
        return cy + (s * vx + c * vy), cx + (c * vx - s * vy)
    return cy + float(d["zh"]) * vy, cx + float(d["zw"]) * vx


def _pixel(img, layers, dr, k, y, x, c):
    """Channel c of pixel (y, x) of the output of layers 0..k (k = -1: the image)."""
    if k < 0:
        return float(img[y, x, c])
    H, W = img.shape[0], img.shape[1]
    l, d = layers[k], dr[k]
    if l["kind"] == "flip":
        return _pixel(img, layers, dr, k - 1, H - 1 - y if d["vflip"] else y, W - 1 - x if d["hflip"] else x, c)
    sy, sx = source(l, d, H, W, y, x)
    mode, cval = l["fill_mode"], float(np.float32(l["fill_value"]))

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


def coords(layer, d, H, W):
    """(sy[H, W], sx[H, W]) float64 of one layer."""
    sy, sx = np.empty((H, W)), np.empty((H, W))
    for y in range(H):
        for x in range(W):
            sy[y, x], sx[y, x] = source(layer, d, H, W, y, x)
    return sy, sx


def near_tie(sy, sx, delta):
    """Pixels one of whose source coordinates lies within ``delta`` of a half-integer: where a coordinate error of
    ``delta`` may move the nearest neighbour."""
    def tie(v):
        return np.abs(v - np.floor(v) - 0.5) <= delta
    return tie(sy) | tie(sx)


# The bounds of the tests (derived in tests/test_augment_affine.py's docstring).
U = 2.0 ** -24                     # the relative error of one rounded f32 operation
SINCOS_MEASURED = 8.82e-8          # max |c - cos|, |s - sin| over all 2^24 draws of [-1, 1], measured by the sweep
SINCOS_BOUND = 2 * SINCOS_MEASURED


def coord_bound(ext, rotation=True):
    """The error of an f32 source coordinate of an image of max(H, W) = ext."""
    return ((SINCOS_BOUND if rotation else 0.0) + 6 * U) * ext


def bilinear_bound(ext, M, rotation=True):
    """The error of a bilinear pixel of an image with max(|x|, |fill_value|) = M."""
    return (4 * coord_bound(ext, rotation) + 6 * U) * M
