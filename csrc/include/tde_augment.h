// The input stage (Keras RandomFlip / RandomTranslation in front of a model), defined once for the staging
// kernel (csrc/kernels/augment.hip) and its host twin (tensorflow_distributed_example_amd/ops/augment.py).
//
// The transform of an image row is a pure function of (layer seed, global step t, input-stage index j, local
// row r), like the dropout masks: one Philox4x32-10 block per (row, step, layer),
//
//   words = philox(counter = (r, t >> 32, t, j), key = (seed, seed >> 32)),   u_q = (word_q >> 8) 2^-24.
//
// RandomFlip:         horizontal iff mode allows it and u0 < 0.5; vertical iff mode allows it and u1 < 0.5.
// RandomTranslation:  dy = (lo_h + u2 (hi_h - lo_h)) H,  dx = (lo_w + u3 (hi_w - lo_w)) W, every operation rounded
//                     to f32 on its own (no contraction): the numpy twin reproduces dy, dx bit for bit.
//                     Output pixel (y, x) samples its input at (y - dy, x - dx).
//   Both interpolations are defined by what this header computes per row in f32 (the twin computes the same):
//   nearest:   the source index is y + floor(fl(0.5 - dy)): an integer shift of the whole row.  It is
//              floor(y - dy + 0.5) except where the one rounding of 0.5 - dy reaches an integer the exact value
//              lies just below (dy = -0.5 + 2^-25 gives 1.0): a tie between two pixels half a unit away.
//   bilinear:  di = floor(dy), a = fl(dy - di), source row y - di - (a > 0), fy = a > 0 ? fl(1 - a) : 0.  The
//              subtraction is exact for dy >= 0; for dy < 0 it may round, by 2^-25 of a pixel at most (a tiny
//              negative dy gives a = 1.0, which stands for shift 0, fy = 0: the image unmoved), and so may
//              fl(1 - a): both inside the bilinear bound.  The four neighbours weigh (1-fy)(1-fx), (1-fy)fx, fy(1-fx), fy fx and
//              are summed in that order in f32.  fy = fx = 0 is the integer shift and copies the pixel.
//   A source index outside [0, n) maps by the fill mode, per axis: constant -> fill_value, nearest -> clamp,
//   reflect -> d c b a | a b c d | d c b a (period 2n), wrap -> modulo n.
//
// Layers apply in model order, in f32; the result is rounded once, at the store.  An output pixel walks the
// layers backwards: flips and integer shifts are maps of the source coordinate, a bilinear layer fans out into
// its four neighbours, each of which walks the layers in front of it.  At most one layer of a row may
// interpolate (aug_spec_ok), so a pixel reads one or four source pixels and nothing is staged in between.
#pragma once
#include "tde_common.h"
#include "tde_philox.h"

namespace tde {

constexpr int kAugLayers = 4;   // layers of one input stage

enum AugKind { kAugFlip = 0, kAugTranslate = 1 };
enum AugFill { kAugConstant = 0, kAugNearest = 1, kAugReflect = 2, kAugWrap = 3 };

// Passed by pointer from the host (ctypes: ops/augment.py AugLayer / AugSpec).
struct AugLayer {
  int kind;                 // AugKind
  int mode;                 // flip: bit 0 horizontal, bit 1 vertical; translation: AugFill
  int bilinear;             // translation: 0 nearest, 1 bilinear
  int j;                    // index in the input stage: the Philox counter's layer word
  unsigned long long seed;  // Philox key
  float lo_h, hi_h, lo_w, hi_w;
  float fill_value;
  int pad_;
};

struct AugSpec {
  int n;
  int pad_;
  AugLayer layer[kAugLayers];
};

inline bool aug_spec_ok(const AugSpec& s) {
  if (s.n < 0 || s.n > kAugLayers) return false;
  int interp = 0;
  for (int k = 0; k < s.n; ++k) {
    const AugLayer& l = s.layer[k];
    if (l.kind == kAugFlip) {
      if (l.mode < 1 || l.mode > 3) return false;
    } else if (l.kind == kAugTranslate) {
      if (l.mode < 0 || l.mode > 3 || (l.bilinear != 0 && l.bilinear != 1)) return false;
      if (!(l.lo_h >= -1.f && l.lo_h <= l.hi_h && l.hi_h <= 1.f)) return false;
      if (!(l.lo_w >= -1.f && l.lo_w <= l.hi_w && l.hi_w <= 1.f)) return false;
      interp += l.bilinear;
    } else {
      return false;
    }
  }
  return interp <= 1;
}

// One layer's transform of one image row, as the pixel loop reads it (LDS, workgroup-uniform).
enum AugRowKind { kRowFlip = 0, kRowShift = 1, kRowBilinear = 2 };
struct AugRow {
  int kind;      // AugRowKind
  int fill;      // AugFill of a shift / bilinear row
  int a, b;      // flip: vertical, horizontal (0 / 1); else the shifts sy, sx: source index = output index + shift
  float fy, fx;  // bilinear fractions
  float cval;    // fill_value
  float dy, dx;  // the drawn translation (params)
};

__device__ __forceinline__ float aug_unit(unsigned w) { return (float)(w >> 8) * (1.f / 16777216.f); }

// One f32 operation, rounded on its own.  HIP's __fmul_rn / __fadd_rn / __fsub_rn are plain operators compiled
// under the default contraction, which fused lo + u * span into a multiply-add here: these are the same
// operators with contraction switched off where they are written.
__device__ __forceinline__ float aug_mul(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float aug_add(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
__device__ __forceinline__ float aug_sub(float a, float b) {
#pragma clang fp contract(off)
  return a - b;
}

// (lo + u (hi - lo)) n: four rounded operations.
__device__ __forceinline__ float aug_draw(float lo, float hi, float u, int n) {
  return aug_mul(aug_add(lo, aug_mul(u, aug_sub(hi, lo))), (float)n);
}

// The shift and fraction of one axis of a bilinear translation by d.
__device__ __forceinline__ void aug_split(float d, int* shift, float* frac) {
  const float di = floorf(d);
  const float a = aug_sub(d, di);
  *shift = -(int)di - (a > 0.f ? 1 : 0);
  *frac = a > 0.f ? aug_sub(1.f, a) : 0.f;
}

__device__ __forceinline__ AugRow aug_row(const AugLayer& l, int r, long long t, int H, int W) {
  const uint2 key{(unsigned)l.seed, (unsigned)(l.seed >> 32)};
  const unsigned long long tt = (unsigned long long)t;
  const uint4 w = philox(uint4{(unsigned)r, (unsigned)(tt >> 32), (unsigned)tt, (unsigned)l.j}, key);
  AugRow o{};
  if (l.kind == kAugFlip) {
    o.kind = kRowFlip;
    o.b = ((l.mode & 1) && aug_unit(w.x) < 0.5f) ? 1 : 0;
    o.a = ((l.mode & 2) && aug_unit(w.y) < 0.5f) ? 1 : 0;
    return o;
  }
  o.fill = l.mode;
  o.cval = l.fill_value;
  o.dy = aug_draw(l.lo_h, l.hi_h, aug_unit(w.z), H);
  o.dx = aug_draw(l.lo_w, l.hi_w, aug_unit(w.w), W);
  if (l.bilinear) {
    aug_split(o.dy, &o.a, &o.fy);
    aug_split(o.dx, &o.b, &o.fx);
    o.kind = (o.fy == 0.f && o.fx == 0.f) ? kRowShift : kRowBilinear;
  } else {
    o.kind = kRowShift;
    o.a = (int)floorf(aug_sub(0.5f, o.dy));
    o.b = (int)floorf(aug_sub(0.5f, o.dx));
  }
  return o;
}

// Index i of an axis of n entries through the fill mode; false: the constant.
__device__ __forceinline__ bool aug_index(int fill, int n, int* i) {
  int v = *i;
  if ((unsigned)v < (unsigned)n) return true;
  if (fill == kAugConstant) return false;
  if (fill == kAugNearest) {
    v = v < 0 ? 0 : n - 1;
  } else if (fill == kAugReflect) {
    const int p = 2 * n;
    int m = v % p;
    m = m < 0 ? m + p : m;
    v = m < n ? m : p - 1 - m;
  } else {
    const int m = v % n;
    v = m < 0 ? m + n : m;
  }
  *i = v;
  return true;
}

// Walk layers k, k-1, .. 0 of flips and shifts from pixel (y, x) of layer k's output to the source pixel.
// Returns -1 at the source (y, x updated), the layer whose constant the pixel takes, or -2 - k when layer k
// interpolates (y, x then are that layer's output pixel).
__device__ __forceinline__ int aug_walk(const AugRow* rows, int k, int H, int W, int* y, int* x) {
  for (; k >= 0; --k) {
    const AugRow& l = rows[k];
    if (l.kind == kRowFlip) {
      if (l.a) *y = H - 1 - *y;
      if (l.b) *x = W - 1 - *x;
    } else if (l.kind == kRowShift) {
      *y += l.a;
      *x += l.b;
      if (!aug_index(l.fill, H, y) || !aug_index(l.fill, W, x)) return k;
    } else {
      return -2 - k;
    }
  }
  return -1;
}

}  // namespace tde
