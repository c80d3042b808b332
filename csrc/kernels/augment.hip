// The input stage applied where the input rows are already touched once per step: the launch that fills the
// training program's input ring.  dst[i] = T_{r = i mod B, t = step0 + i / B}(src[idx[i]]) with T the model's
// RandomFlip / RandomTranslation / RandomRotation / RandomZoom layers (csrc/include/tde_augment.h); a null idx
// stages src[i].  A stage of flips and translations runs stage_rows_aug_kernel; one that holds a rotation or a
// zoom runs stage_rows_affine_kernel, the general source-coordinate map.
//
// One or more workgroups per image row.  Lanes 0 .. n-1 of the first wave draw the row's Philox block per layer
// and leave the layer's flips / shifts / fractions in LDS; the pixel loop behind the barrier is index
// arithmetic plus loads.  A unit of the loop is the widest vector that stays inside one pixel's C contiguous
// channel elements: 16 bytes, else 4 bytes, else one element.  A pixel reads one source pixel (flips, integer
// shifts), none (the constant fill) or four (the bilinear layer); f32 arithmetic, one rounding at the store.
#include "tde_augment.h"

namespace tde {

template <typename U, bool BF>
struct AugUnit {
  static constexpr int E = (int)sizeof(U) / (BF ? 2 : 4);   // elements of a unit
  __device__ static __forceinline__ void unpack(const U& u, float* v) {
    if constexpr (BF) {
      unsigned short h[E];
      __builtin_memcpy(h, &u, sizeof(U));
#pragma unroll
      for (int e = 0; e < E; ++e) v[e] = __uint_as_float((unsigned)h[e] << 16);
    } else {
      __builtin_memcpy(v, &u, sizeof(U));
    }
  }
  __device__ static __forceinline__ U pack(const float* v) {
    U u;
    if constexpr (BF) {
      bf16 h[E];
#pragma unroll
      for (int e = 0; e < E; ++e) h[e] = f2bf(v[e]);
      __builtin_memcpy(&u, h, sizeof(U));
    } else {
      __builtin_memcpy(&u, v, sizeof(U));
    }
    return u;
  }
  __device__ static __forceinline__ U splat(float c) {
    float v[E];
#pragma unroll
    for (int e = 0; e < E; ++e) v[e] = c;
    return pack(v);
  }
};

template <typename U, bool BF>
__global__ __launch_bounds__(256) void stage_rows_aug_kernel(const U* __restrict__ src, long long nrows,
                                                             const int* __restrict__ idx, int B, int H, int W, int upp,
                                                             int bpr, U* __restrict__ dst, AugSpec spec,
                                                             long long step0, float* __restrict__ params,
                                                             int* __restrict__ bad) {
  using A = AugUnit<U, BF>;
  constexpr int E = A::E;
  __shared__ AugRow rows[kAugLayers];
  const int i = blockIdx.x / bpr;            // destination row
  const int chunk = blockIdx.x - i * bpr;
  const long long s = idx ? (long long)idx[i] : (long long)i;
  if ((unsigned long long)s >= (unsigned long long)nrows) {   // never read out of the cache (uniform exit)
    if (chunk == 0 && threadIdx.x == 0) atomicOr(bad, 1);
    return;
  }
  const int nl = spec.n;
#pragma unroll
  for (int k = 0; k < kAugLayers; ++k)
    if (k < nl && (int)threadIdx.x == k) rows[k] = aug_row(spec.layer[k], i % B, step0 + i / B, H, W);
  __syncthreads();
  if (params && chunk == 0 && threadIdx.x == 0) {   // the composed (hflip, vflip, dy, dx) of the row
    int hf = 0, vf = 0;
    float dy = 0.f, dx = 0.f;
    for (int k = 0; k < nl; ++k) {
      if (rows[k].kind == kRowFlip) {
        vf ^= rows[k].a;
        hf ^= rows[k].b;
      } else {
        dy = aug_add(dy, rows[k].dy);
        dx = aug_add(dx, rows[k].dx);
      }
    }
    float* p = params + (long long)i * 4;
    p[0] = (float)hf;
    p[1] = (float)vf;
    p[2] = dy;
    p[3] = dx;
  }
  const unsigned rowu = (unsigned)H * (unsigned)W * (unsigned)upp;
  const U* __restrict__ srow = src + s * (long long)rowu;
  U* __restrict__ drow = dst + (long long)i * (long long)rowu;
  for (unsigned u = (unsigned)chunk * 256u + threadIdx.x; u < rowu; u += (unsigned)bpr * 256u) {
    const unsigned pix = u / (unsigned)upp;
    const unsigned q = u - pix * (unsigned)upp;
    int y = (int)(pix / (unsigned)W);
    int x = (int)(pix - (unsigned)y * (unsigned)W);
    const int st = aug_walk(rows, nl - 1, H, W, &y, &x);
    U out;
    if (st == -1) {
      out = srow[((unsigned)y * (unsigned)W + (unsigned)x) * (unsigned)upp + q];
    } else if (st >= 0) {
      out = A::splat(rows[st].cval);
    } else {
      const int k = -2 - st;
      const int fill = rows[k].fill, sy = rows[k].a, sx = rows[k].b;
      const float fy = rows[k].fy, fx = rows[k].fx, cval = rows[k].cval;
      const float wy[2] = {1.f - fy, fy}, wx[2] = {1.f - fx, fx};
      float acc[E];
#pragma unroll
      for (int tap = 0; tap < 4; ++tap) {
        int ty = y + sy + (tap >> 1), tx = x + sx + (tap & 1);
        float v[E];
        int at = k;   // the layer whose constant the neighbour takes, or -1: a source pixel
        if (aug_index(fill, H, &ty) && aug_index(fill, W, &tx)) at = aug_walk(rows, k - 1, H, W, &ty, &tx);
        if (at == -1) {
          A::unpack(srow[((unsigned)ty * (unsigned)W + (unsigned)tx) * (unsigned)upp + q], v);
        } else {
          const float c = at >= 0 ? rows[at].cval : cval;   // (no second interpolating layer: aug_spec_ok)
#pragma unroll
          for (int e = 0; e < E; ++e) v[e] = c;
        }
        const float w = wy[tap >> 1] * wx[tap & 1];
#pragma unroll
        for (int e = 0; e < E; ++e) acc[e] = tap == 0 ? w * v[e] : acc[e] + w * v[e];
      }
      out = A::pack(acc);
    }
    drow[u] = out;
  }
}

template <typename U, bool BF>
static int launch_aug(const void* src, long long nrows, const int* idx, long long n, int B, int H, int W, int upp,
                      void* dst, const AugSpec& spec, long long step0, float* params, int* bad, hipStream_t stream) {
  const long long rowu = (long long)H * W * upp;
  if (rowu >= (1LL << 31)) return -2;
  long long bpr = (rowu + 1023) / 1024;
  bpr = bpr > 64 ? 64 : bpr;
  if (n * bpr >= (1LL << 31)) return -2;
  stage_rows_aug_kernel<U, BF><<<(unsigned)(n * bpr), 256, 0, stream>>>((const U*)src, nrows, idx, B, H, W, upp,
                                                                         (int)bpr, (U*)dst, spec, step0, params, bad);
  TDE_LAUNCH_CHECK();
  return 0;
}

// The stage of a spec that holds a RandomRotation or a RandomZoom (aug_spec_affine): the same grid, units and
// bad-index rule, with every layer as an AugAffine record.  A pixel does the layers' coordinate arithmetic in
// f32 (aug_affine_walk) and reads one or four source pixels in whole units straight from global memory: a
// workgroup reads only its own source row (3 KB for 28x28x1 f32), each pixel of it a handful of times, so after
// the first touch the loads hit the CU's 32 KiB vector L1; a copy staged in LDS would add a pass over the row and
// a barrier in front of gathers that then cost an LDS read where they now cost an L1 hit, and would bound H x W x C
// by the LDS.
template <typename U, bool BF>
__global__ __launch_bounds__(256) void stage_rows_affine_kernel(const U* __restrict__ src, long long nrows,
                                                                const int* __restrict__ idx, int B, int H, int W,
                                                                int upp, int bpr, U* __restrict__ dst, AugSpec spec,
                                                                long long step0, float* __restrict__ params,
                                                                int* __restrict__ bad) {
  using A = AugUnit<U, BF>;
  constexpr int E = A::E;
  __shared__ AugAffine rows[kAugLayers];
  const int i = blockIdx.x / bpr;            // destination row
  const int chunk = blockIdx.x - i * bpr;
  const long long s = idx ? (long long)idx[i] : (long long)i;
  if ((unsigned long long)s >= (unsigned long long)nrows) {   // never read out of the cache (uniform exit)
    if (chunk == 0 && threadIdx.x == 0) atomicOr(bad, 1);
    return;
  }
  const int nl = spec.n;
#pragma unroll
  for (int k = 0; k < kAugLayers; ++k)
    if (k < nl && (int)threadIdx.x == k) rows[k] = aug_affine_row(spec.layer[k], i % B, step0 + i / B, H, W);
  __syncthreads();
  if (params && chunk == 0 && threadIdx.x < 4 * kAugLayers) {   // [kAugLayers][4]: each layer's drawn values
    const int k = (int)threadIdx.x >> 2, q = (int)threadIdx.x & 3;
    float v = 0.f;
    if (k < nl) v = q == 0 ? rows[k].p0 : q == 1 ? rows[k].p1 : q == 2 ? rows[k].p2 : 0.f;
    params[(long long)i * (4 * kAugLayers) + threadIdx.x] = v;
  }
  const float cy = aug_mul((float)(H - 1), 0.5f), cx = aug_mul((float)(W - 1), 0.5f);
  const unsigned rowu = (unsigned)H * (unsigned)W * (unsigned)upp;
  const U* __restrict__ srow = src + s * (long long)rowu;
  U* __restrict__ drow = dst + (long long)i * (long long)rowu;
  for (unsigned u = (unsigned)chunk * 256u + threadIdx.x; u < rowu; u += (unsigned)bpr * 256u) {
    const unsigned pix = u / (unsigned)upp;
    const unsigned q = u - pix * (unsigned)upp;
    int y = (int)(pix / (unsigned)W);
    int x = (int)(pix - (unsigned)y * (unsigned)W);
    int y0 = 0, x0 = 0;
    float fy = 0.f, fx = 0.f;
    const int st = aug_affine_walk(rows, nl - 1, H, W, cy, cx, &y, &x, &y0, &x0, &fy, &fx);
    U out;
    if (st == -1) {
      out = srow[((unsigned)y * (unsigned)W + (unsigned)x) * (unsigned)upp + q];
    } else if (st >= 0) {
      out = A::splat(rows[st].row.cval);
    } else {
      const int k = -2 - st;
      const int fill = rows[k].row.fill;
      const float cval = rows[k].row.cval;
      const float wy[2] = {1.f - fy, fy}, wx[2] = {1.f - fx, fx};
      float acc[E];
#pragma unroll
      for (int tap = 0; tap < 4; ++tap) {
        int ty = y0 + (tap >> 1), tx = x0 + (tap & 1);
        float v[E];
        int at = k;   // the layer whose constant the neighbour takes, or -1: a source pixel
        if (aug_index(fill, H, &ty) && aug_index(fill, W, &tx)) {
          int uy, ux;
          float gy, gx;
          at = aug_affine_walk(rows, k - 1, H, W, cy, cx, &ty, &tx, &uy, &ux, &gy, &gx);
        }
        if (at == -1) {
          A::unpack(srow[((unsigned)ty * (unsigned)W + (unsigned)tx) * (unsigned)upp + q], v);
        } else {
          const float c = at >= 0 ? rows[at].row.cval : cval;   // (no second interpolating layer: aug_spec_ok)
#pragma unroll
          for (int e = 0; e < E; ++e) v[e] = c;
        }
        const float w = wy[tap >> 1] * wx[tap & 1];
#pragma unroll
        for (int e = 0; e < E; ++e) acc[e] = tap == 0 ? w * v[e] : acc[e] + w * v[e];
      }
      out = A::pack(acc);
    }
    drow[u] = out;
  }
}

template <typename U, bool BF>
static int launch_affine(const void* src, long long nrows, const int* idx, long long n, int B, int H, int W, int upp,
                         void* dst, const AugSpec& spec, long long step0, float* params, int* bad,
                         hipStream_t stream) {
  if (H > kAugAffineMaxDim || W > kAugAffineMaxDim) return -2;
  const long long rowu = (long long)H * W * upp;
  if (rowu >= (1LL << 31)) return -2;
  long long bpr = (rowu + 1023) / 1024;
  bpr = bpr > 64 ? 64 : bpr;
  if (n * bpr >= (1LL << 31)) return -2;
  stage_rows_affine_kernel<U, BF><<<(unsigned)(n * bpr), 256, 0, stream>>>((const U*)src, nrows, idx, B, H, W, upp,
                                                                            (int)bpr, (U*)dst, spec, step0, params,
                                                                            bad);
  TDE_LAUNCH_CHECK();
  return 0;
}

}  // namespace tde

using namespace tde;

// dst[i] = T_{i mod B, step0 + i / B}(src[idx[i]]) for i < n rows of H x W x C elements; src_dtype 0: float32,
// 1: bfloat16, of src and dst alike.  idx (device int32, may be null: src[i]); `spec` is a host pointer, taken
// by value; `params` (device float, may be null) receives each row's draws; `bad` gets bit 0 set for an index
// outside [0, nrows), whose destination row (and its params) stays as it was.
// params of a spec of flips and translations: [n][4], the composed (hflip, vflip, dy, dx).
// params of a spec that holds a rotation or a zoom (aug_spec_affine): [n][kAugLayers][4], layer k's own draws --
// flip (hflip, vflip, 0, 0), translation (dy, dx, 0, 0), rotation (f in turns, c, s, 0), zoom (zh, zw, 0, 0),
// and zeros for k >= spec.n.  Such a spec needs H, W <= kAugAffineMaxDim (-2 otherwise).
TDE_API int tde_stage_rows_aug(const void* src, int src_dtype, long long nrows, const int* idx, long long n, int B,
                               int H, int W, int C, void* dst, const AugSpec* spec, long long step0, float* params,
                               int* bad, hipStream_t stream) {
  if (!src || !dst || !spec || !bad || !aug_spec_ok(*spec)) return -1;
  if ((src_dtype != 0 && src_dtype != 1) || B < 1 || H < 1 || W < 1 || C < 1 || nrows < 0) return -1;
  if (n <= 0) return 0;
  const bool bf = src_dtype == 1;
  const long long pb = (long long)C * (bf ? 2 : 4);   // bytes of a pixel
  const uintptr_t al = (uintptr_t)src | (uintptr_t)dst;
  if (aug_spec_affine(*spec)) {   // a rotation or a zoom: the general map, the same unit widths
    if (pb % 16 == 0 && (al & 15) == 0) {
      const int upp = (int)(pb / 16);
      return bf ? launch_affine<uint4, true>(src, nrows, idx, n, B, H, W, upp, dst, *spec, step0, params, bad, stream)
                : launch_affine<uint4, false>(src, nrows, idx, n, B, H, W, upp, dst, *spec, step0, params, bad, stream);
    }
    if (pb % 4 == 0 && (al & 3) == 0) {
      const int upp = (int)(pb / 4);
      return bf ? launch_affine<unsigned, true>(src, nrows, idx, n, B, H, W, upp, dst, *spec, step0, params, bad,
                                                stream)
                : launch_affine<unsigned, false>(src, nrows, idx, n, B, H, W, upp, dst, *spec, step0, params, bad,
                                                 stream);
    }
    if (!bf || (al & 1)) return -2;
    return launch_affine<unsigned short, true>(src, nrows, idx, n, B, H, W, C, dst, *spec, step0, params, bad,
                                               stream);
  }
  if (pb % 16 == 0 && (al & 15) == 0) {
    const int upp = (int)(pb / 16);
    return bf ? launch_aug<uint4, true>(src, nrows, idx, n, B, H, W, upp, dst, *spec, step0, params, bad, stream)
              : launch_aug<uint4, false>(src, nrows, idx, n, B, H, W, upp, dst, *spec, step0, params, bad, stream);
  }
  if (pb % 4 == 0 && (al & 3) == 0) {
    const int upp = (int)(pb / 4);
    return bf ? launch_aug<unsigned, true>(src, nrows, idx, n, B, H, W, upp, dst, *spec, step0, params, bad, stream)
              : launch_aug<unsigned, false>(src, nrows, idx, n, B, H, W, upp, dst, *spec, step0, params, bad, stream);
  }
  if (!bf || (al & 1)) return -2;
  return launch_aug<unsigned short, true>(src, nrows, idx, n, B, H, W, C, dst, *spec, step0, params, bad, stream);
}

// {sizeof(AugSpec), sizeof(AugLayer), kAugLayers}: the host checks its ctypes twin against them.
TDE_API int tde_augment_abi(long long* out, int n) {
  const long long v[3] = {(long long)sizeof(AugSpec), (long long)sizeof(AugLayer), kAugLayers};
  for (int i = 0; i < n && i < 3; ++i) out[i] = v[i];
  return 3;
}
