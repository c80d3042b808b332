// The input stage (Keras RandomFlip / RandomTranslation / RandomRotation / RandomZoom in front of a model),
// defined once for the staging kernels (csrc/kernels/augment.hip) and their host twin
// (tensorflow_distributed_example_amd/ops/augment.py).
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
// RandomRotation:     f = lo_h + u0 (hi_h - lo_h) turns, counter-clockwise as displayed for f > 0.
// RandomZoom:         zh = 1 + (lo_h + u2 (hi_h - lo_h)), zw = 1 + (lo_w + u3 (hi_w - lo_w)), or zw = zh when
//                     pad_ = 1 (Keras's width_factor=None: the aspect ratio kept).  z > 1 zooms out.
//   Both are one general source-coordinate map (AugAffine).  With cy = (H-1)/2, cx = (W-1)/2, vy = y - cy,
//   vx = x - cx (all exact in f32), output pixel (y, x) samples its input at
//     sx = cx + (ax vx - bx vy),   sy = cy + (ay vx + by vy),
//   every operation rounded to f32 on its own; rotation: ax = by = c, bx = ay = s; zoom: ax = zw, by = zh,
//   bx = ay = 0 (the products with 0 change no value: sx = cx + zw vx, sy = cy + zh vy).
//   c = cos(2 pi f), s = sin(2 pi f) by this header's own evaluation (aug_sincos; the device's sinf / cosf have
//   no bitwise host twin): q = rint(4 f), r = 4 f - q (both exact, |r| <= 0.5), sin(pi r / 2) the odd and
//   cos(pi r / 2) the even Taylor polynomial (degrees 9 and 10, constant term exactly 1) in Horner form over
//   aug_mul / aug_add, then the quadrant swap of q mod 4.  Every multiple of a quarter turn gives c, s in
//   {0, 1, -1} exactly: right-angle rotations are exact pixel permutations (f = 0.25 on a square image is
//   np.rot90(img, 1)).  The error against float64 over all 2^24 draws: profiles/augment_affine/NOTES.md.
//   nearest:   the source index is floor(fl(s + 0.5)) per axis: a point map, like a flip or a shift.
//   bilinear:  i0 = floor(s), fr = fl(s - i0), neighbours i0 and i0 + 1, weighted and summed as the translation's
//              four; a pixel with fy = fx = 0 is a point map too and copies the pixel.
//   Every index goes through the fill mode, per neighbour and per axis, as for the translation.
//
// Layers apply in model order, in f32; the result is rounded once, at the store.  An output pixel walks the
// layers backwards: flips, integer shifts and point maps are maps of the source coordinate, a bilinear layer
// fans out into its four neighbours, each of which walks the layers in front of it.  At most one layer of a
// row may interpolate (aug_spec_ok), whatever its kind, so a pixel reads one or four source pixels and nothing
// is staged in between.
#pragma once
#include "tde_common.h"
#include "tde_philox.h"

namespace tde {

constexpr int kAugLayers = 4;   // layers of one input stage

enum AugKind { kAugFlip = 0, kAugTranslate = 1, kAugRotate = 2, kAugZoom = 3 };
enum AugFill { kAugConstant = 0, kAugNearest = 1, kAugReflect = 2, kAugWrap = 3 };

// Passed by pointer from the host (ctypes: ops/augment.py AugLayer / AugSpec).
struct AugLayer {
  int kind;                 // AugKind
  int mode;                 // flip: bit 0 horizontal, bit 1 vertical; translation, rotation, zoom: AugFill
  int bilinear;             // translation, rotation, zoom: 0 nearest, 1 bilinear
  int j;                    // index in the input stage: the Philox counter's layer word
  unsigned long long seed;  // Philox key
  float lo_h, hi_h, lo_w, hi_w;   // factor ranges; rotation: lo_h, hi_h the turn range, lo_w, hi_w unused
  float fill_value;
  int pad_;                 // zoom: 1 when the width follows the height's draw; else 0
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
    } else if (l.kind == kAugRotate || l.kind == kAugZoom) {
      if (l.mode < 0 || l.mode > 3 || (l.bilinear != 0 && l.bilinear != 1)) return false;
      if (!(l.lo_h >= -1.f && l.lo_h <= l.hi_h && l.hi_h <= 1.f)) return false;
      if (l.kind == kAugZoom) {
        if (l.pad_ != 0 && l.pad_ != 1) return false;
        if (l.pad_ == 0 && !(l.lo_w >= -1.f && l.lo_w <= l.hi_w && l.hi_w <= 1.f)) return false;
      }
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

// ---------------------------------------------------------------------------- rotation and zoom
// A spec that holds a rotation or a zoom runs the general source-coordinate map (augment.hip's second kernel).
inline bool aug_spec_affine(const AugSpec& s) {
  for (int k = 0; k < s.n && k < kAugLayers; ++k)
    if (s.layer[k].kind == kAugRotate || s.layer[k].kind == kAugZoom) return true;
  return false;
}

// The largest H or W of the general map: |source coordinate| < 2 max(H, W) + 1 for a valid spec, so half-integer
// coordinates stay exact in f32 and every float-to-int conversion stays far inside int.
constexpr int kAugAffineMaxDim = 1 << 20;

// lo + u (hi - lo): three rounded operations.
__device__ __forceinline__ float aug_draw1(float lo, float hi, float u) {
  return aug_add(lo, aug_mul(u, aug_sub(hi, lo)));
}

// c = cos(2 pi f), s = sin(2 pi f) for f turns, |f| <= 1.
__device__ __forceinline__ void aug_sincos(float f, float* c, float* s) {
  const float f4 = aug_mul(4.f, f);   // exact
  const float q = rintf(f4);
  const float r = aug_sub(f4, q);     // exact, |r| <= 0.5
  const float r2 = aug_mul(r, r);
  // sin(pi r / 2) = r (S0 + r2 (S1 + ..)), cos(pi r / 2) = 1 + r2 (C1 + r2 (C2 + ..)): Taylor, rounded to f32
  float ps = 0x1.507834p-13f;
  ps = aug_add(-0x1.32d2ccp-8f, aug_mul(r2, ps));
  ps = aug_add(0x1.466bc6p-4f, aug_mul(r2, ps));
  ps = aug_add(-0x1.4abbcep-1f, aug_mul(r2, ps));
  ps = aug_add(0x1.921fb6p+0f, aug_mul(r2, ps));
  const float sr = aug_mul(r, ps);
  float pc = -0x1.a6d1f2p-16f;
  pc = aug_add(0x1.e1f506p-11f, aug_mul(r2, pc));
  pc = aug_add(-0x1.55d3c8p-6f, aug_mul(r2, pc));
  pc = aug_add(0x1.03c1fp-2f, aug_mul(r2, pc));
  pc = aug_add(-0x1.3bd3ccp+0f, aug_mul(r2, pc));
  const float cr = aug_add(1.f, aug_mul(r2, pc));
  const int qi = (int)q & 3;          // |q| <= 4; two's complement: q mod 4
  // 0 - v, not -v: a zero stays +0
  if (qi == 0) {
    *c = cr;
    *s = sr;
  } else if (qi == 1) {
    *c = aug_sub(0.f, sr);
    *s = cr;
  } else if (qi == 2) {
    *c = aug_sub(0.f, cr);
    *s = aug_sub(0.f, sr);
  } else {
    *c = sr;
    *s = aug_sub(0.f, cr);
  }
}

// One layer's transform of one image row in the general kernel: the AugRow of a flip or a translation, or the
// source-coordinate map of a rotation or a zoom.
constexpr int kRowAffine = 3;
struct AugAffine {
  AugRow row;            // kind kRowAffine: fill and cval hold the layer's, a = 1 for bilinear, the rest unused
  float ax, bx, ay, by;  // sx = cx + (ax vx - bx vy), sy = cy + (ay vx + by vy)
  float p0, p1, p2;      // what params exports for the layer (augment.hip)
};

__device__ __forceinline__ AugAffine aug_affine_row(const AugLayer& l, int r, long long t, int H, int W) {
  AugAffine o{};
  if (l.kind == kAugFlip || l.kind == kAugTranslate) {
    o.row = aug_row(l, r, t, H, W);
    if (l.kind == kAugFlip) {
      o.p0 = (float)o.row.b;
      o.p1 = (float)o.row.a;
    } else {
      o.p0 = o.row.dy;
      o.p1 = o.row.dx;
    }
    return o;
  }
  const uint2 key{(unsigned)l.seed, (unsigned)(l.seed >> 32)};
  const unsigned long long tt = (unsigned long long)t;
  const uint4 w = philox(uint4{(unsigned)r, (unsigned)(tt >> 32), (unsigned)tt, (unsigned)l.j}, key);
  o.row.kind = kRowAffine;
  o.row.fill = l.mode;
  o.row.cval = l.fill_value;
  o.row.a = l.bilinear;
  if (l.kind == kAugRotate) {
    const float f = aug_draw1(l.lo_h, l.hi_h, aug_unit(w.x));
    float c, s;
    aug_sincos(f, &c, &s);
    o.ax = c, o.bx = s, o.ay = s, o.by = c;
    o.p0 = f, o.p1 = c, o.p2 = s;
  } else {
    const float zh = aug_add(1.f, aug_draw1(l.lo_h, l.hi_h, aug_unit(w.z)));
    const float zw = l.pad_ ? zh : aug_add(1.f, aug_draw1(l.lo_w, l.hi_w, aug_unit(w.w)));
    o.ax = zw, o.by = zh;
    o.p0 = zh, o.p1 = zw;
  }
  return o;
}

// The source coordinate of output pixel (y, x) of a kRowAffine layer; cy = (H-1)/2, cx = (W-1)/2.
__device__ __forceinline__ void aug_affine_at(const AugAffine& l, float cy, float cx, int y, int x, float* sy,
                                              float* sx) {
  const float vy = aug_sub((float)y, cy), vx = aug_sub((float)x, cx);
  *sx = aug_add(cx, aug_sub(aug_mul(l.ax, vx), aug_mul(l.bx, vy)));
  *sy = aug_add(cy, aug_add(aug_mul(l.ay, vx), aug_mul(l.by, vy)));
}

// floor of a source coordinate as an int.  The clamp changes nothing for a valid spec within kAugAffineMaxDim
// (|v| < 2^22); it keeps the conversion defined whatever the operand (fmaxf drops a NaN).
__device__ __forceinline__ int aug_floor_int(float v) {
  return (int)floorf(fminf(fmaxf(v, -8388608.f), 8388608.f));
}

// aug_walk over AugAffine rows.  A kRowAffine layer that reads nearest, or whose pixel has no fraction, is a
// point map.  -2 - k: layer k interpolates at its output pixel (y, x); *y0, *x0 then are the first neighbour's
// (unfilled) indices and *fy, *fx the fractions.
__device__ __forceinline__ int aug_affine_walk(const AugAffine* rows, int k, int H, int W, float cy, float cx, int* y,
                                               int* x, int* y0, int* x0, float* fy, float* fx) {
  for (; k >= 0; --k) {
    const AugRow& l = rows[k].row;
    if (l.kind == kRowFlip) {
      if (l.a) *y = H - 1 - *y;
      if (l.b) *x = W - 1 - *x;
    } else if (l.kind == kRowShift) {
      *y += l.a;
      *x += l.b;
      if (!aug_index(l.fill, H, y) || !aug_index(l.fill, W, x)) return k;
    } else if (l.kind == kRowAffine) {
      float sy, sx;
      aug_affine_at(rows[k], cy, cx, *y, *x, &sy, &sx);
      if (l.a) {
        const int iy = aug_floor_int(sy), ix = aug_floor_int(sx);
        const float ry = aug_sub(sy, (float)iy), rx = aug_sub(sx, (float)ix);
        if (ry != 0.f || rx != 0.f) {
          *y0 = iy, *x0 = ix, *fy = ry, *fx = rx;
          return -2 - k;
        }
        *y = iy, *x = ix;
      } else {
        *y = aug_floor_int(aug_add(sy, 0.5f));
        *x = aug_floor_int(aug_add(sx, 0.5f));
      }
      if (!aug_index(l.fill, H, y) || !aug_index(l.fill, W, x)) return k;
    } else {
      *y0 = *y + l.a, *x0 = *x + l.b, *fy = l.fy, *fx = l.fx;
      return -2 - k;
    }
  }
  return -1;
}

}  // namespace tde
