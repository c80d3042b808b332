// Multi-tensor optimizer apply over the flat parameter buffer: SGD (optionally
// momentum / Nesterov, Keras form) and Adam (Keras/TF form, epsilon added to
// sqrt(v_hat)), in ONE launch for all variables (SURVEY.md §2.5 A14/B17,
// reference: distributed_with_keras.py:42, mnist_keras_distributed.py:111,
// tf2_mnist_distributed.py:137).
//
// The same pass (a) zeroes the gradient buffer for the next step's atomic /
// split-K accumulation and (b) refreshes the bf16 compute copies ("shadows") of
// the weights in the layouts the MFMA kernels read — row-major and, through an
// LDS 16x64 transpose, column-major.  The step counter (`iterations`, Keras
// optimizer.iterations / Estimator global_step) lives on the device and is
// advanced by the step's loss kernel before this launch, so Adam's bias
// correction reads t = iterations with no host round trip and no in-kernel
// cross-workgroup protocol.
//
// Vectorised: float4 loads/stores everywhere (segments are 256-byte aligned).
//
// CLIP variants (tde_optim_apply_clip): the gradient clipped (tde_clip.h) before the step, by value with c
// in the arguments or by the scale the norm launches (gradclip.hip) left on the device.
//
// WD variants (tde_optim_apply_wd): decoupled weight decay (tde_reg.h) in front of the step, with or without
// a clip: the step starts from w - (w * wd[seg]) * lr, lr the rate in effect (lr_ptr applied; never Adam's lr_t).
#include "tde_clip.h"
#include "tde_optim.h"
#include "tde_reg.h"

namespace tde {

struct OptArgs {
  float* w; float* g; float* m; float* v;
  bf16* shadow;
  const OptSeg* segs;
  const int4* table;        // per block: {seg, kind(0=1d,1=tile), a, b}
  const long long* iterations;
  OptHyper h;
  float grad_scale;
  int zero_grad;
  const float* lr_ptr;      // optional device-resident lr (schedules): replaces h.lr
};

constexpr int kChunk = 2048;
constexpr int kTileR = 16;  // rows per transposed-shadow tile (tile = kTileR x 64)

// What a CLIP variant adds to OptArgs.
struct ClipArgs {
  const float* scale;   // norm modes: scale[seg] (kClipNorm) or scale[0] (kClipGlobalNorm)
  float c;              // kClipValue: the bound
  int mode;
};

// What a WD variant adds to OptArgs.
struct WdArgs {
  const float* wd;      // wd[seg]: the segment's decay, 0 for a variable excluded from it
};

// The hyper-parameters in effect (lr_ptr applied) and the step size; CLIP variants: the clip in effect for
// this workgroup's segment (cs: the scale of a norm mode, else 1; cv: the bound of kClipValue, else +inf);
// WD variants: the segment's decay.
struct Hyper {
  OptHyper oh;
  float lr_t;
  float cs, cv;
  float wd;
};

// The weight a WD variant's step starts from: three roundings, product, product, difference, never
// contracted into an fma (the host form f32(w - f32(f32(w * wd) * lr)) is what the tests feed the oracles).
__device__ __forceinline__ float wd_start(float w, const Hyper& h) {
#pragma clang fp contract(off)
  const float d = w * h.wd;
  const float e = d * h.oh.lr;
  return w - e;
}

// The gradient the step sees: g * grad_scale; CLIP: (g * grad_scale) * scale, or clamped to [-c, c], in one
// straight line for both modes (the scale is 1 under kClipValue, the bound infinite under a norm mode, both
// exact; the compares leave a NaN as the formulas do).
template <bool CLIP>
__device__ __forceinline__ float grad_eff(const OptArgs& a, float g, const Hyper& h) {
  const float x = g * a.grad_scale;
  if constexpr (CLIP) {
    const float y = x * h.cs;
    return y < -h.cv ? -h.cv : (y > h.cv ? h.cv : y);
  }
  return x;
}

// EXT = false: kinds 0..3 (the instruction stream these kinds always had).  EXT = true: the RMSprop kinds,
// launched for kinds 4 / 5 only: rms is `m`, the momentum accumulator `v` (kind 5 alone reads or writes it).
template <bool EXT, bool CLIP>
__device__ __forceinline__ float upd1(const OptArgs& a, float w, float g, float& m, float& v, const Hyper& h) {
  return opt_step<EXT>(h.oh, h.lr_t, w, grad_eff<CLIP>(a, g, h), m, v);
}

// Update 4 consecutive elements at flat index i (16-byte aligned).
template <bool EXT, bool CLIP, bool WD>
__device__ __forceinline__ float4 upd4(const OptArgs& a, size_t i, const Hyper& h) {
  float4 w = *reinterpret_cast<float4*>(a.w + i);
  const float4 g = *reinterpret_cast<float4*>(a.g + i);
  float4 m = {0.f, 0.f, 0.f, 0.f}, v = {0.f, 0.f, 0.f, 0.f};
  if (opt_has_m<EXT>(a.h.kind)) m = *reinterpret_cast<float4*>(a.m + i);
  if (opt_has_v<EXT>(a.h.kind)) v = *reinterpret_cast<float4*>(a.v + i);
  if constexpr (WD) w = float4{wd_start(w.x, h), wd_start(w.y, h), wd_start(w.z, h), wd_start(w.w, h)};
  w.x = upd1<EXT, CLIP>(a, w.x, g.x, m.x, v.x, h);
  w.y = upd1<EXT, CLIP>(a, w.y, g.y, m.y, v.y, h);
  w.z = upd1<EXT, CLIP>(a, w.z, g.z, m.z, v.z, h);
  w.w = upd1<EXT, CLIP>(a, w.w, g.w, m.w, v.w, h);
  *reinterpret_cast<float4*>(a.w + i) = w;
  if (a.zero_grad) *reinterpret_cast<float4*>(a.g + i) = float4{0.f, 0.f, 0.f, 0.f};
  if (opt_has_m<EXT>(a.h.kind)) *reinterpret_cast<float4*>(a.m + i) = m;
  if (opt_has_v<EXT>(a.h.kind)) *reinterpret_cast<float4*>(a.v + i) = v;
  return w;
}

template <bool EXT, bool CLIP, bool WD>
__device__ __forceinline__ float upds(const OptArgs& a, size_t i, const Hyper& h) {
  float w;
  if constexpr (WD)
    w = opt_step_at<EXT>(h.oh, h.lr_t, wd_start(a.w[i], h), a.w, a.m, a.v, i, grad_eff<CLIP>(a, a.g[i], h));
  else
    w = opt_step_at<EXT>(h.oh, h.lr_t, a.w, a.m, a.v, i, grad_eff<CLIP>(a, a.g[i], h));
  if (a.zero_grad) a.g[i] = 0.f;
  return w;
}

template <bool EXT, bool CLIP, bool WD = false>
__device__ __forceinline__ void optim_apply(const OptArgs a, const ClipArgs k, const WdArgs d = WdArgs{}) {
  __shared__ bf16 tile[kTileR][72];
  const int4 ent = a.table[blockIdx.x];
  const OptSeg s = a.segs[ent.x];
  Hyper h{a.h, 0.f, 1.f, __builtin_inff(), 0.f};
  if (a.lr_ptr) h.oh.lr = *a.lr_ptr;
  if constexpr (WD) h.wd = d.wd[ent.x];   // in the round trip of lr_ptr and iterations
  if constexpr (CLIP) {   // loaded in the round trip of lr_ptr and iterations
    if (k.mode == kClipValue) h.cv = k.c;
    else h.cs = k.scale[k.mode == kClipGlobalNorm ? 0 : ent.x];
  }
  h.lr_t = opt_lr_t(h.oh, opt_uses_t(a.h.kind) ? *a.iterations : 0);
  const int tid = threadIdx.x;


  if (ent.y == 0) {
    const long long n = (long long)s.rows * s.cols;
    const long long beg = (long long)ent.z * kChunk;
    const long long end = beg + kChunk < n ? beg + kChunk : n;
#pragma unroll
    for (int it = 0; it < kChunk / 1024; ++it) {
      const long long e = beg + it * 1024 + tid * 4;
      if (e + 4 <= end) {
        const float4 w = upd4<EXT, CLIP, WD>(a, (size_t)(s.off + e), h);
        if (s.sh_off >= 0) {
          bf16x4 hv = {f2bf(w.x), f2bf(w.y), f2bf(w.z), f2bf(w.w)};
          *reinterpret_cast<bf16x4*>(a.shadow + s.sh_off + e) = hv;
        }
      } else {
        for (long long q = e; q < end && q < e + 4; ++q) {
          const float w = upds<EXT, CLIP, WD>(a, (size_t)(s.off + q), h);
          if (s.sh_off >= 0) a.shadow[s.sh_off + q] = f2bf(w);
        }
      }
    }
  } else {
    // 16x64 tiles (one float4 per thread): ~4x more workgroups than 64x64 tiles, so
    // a 5408x64 Dense kernel spreads over 338 workgroups instead of 85 CUs.
    const int r0 = ent.z * kTileR, c0 = ent.w * 64;
    const bool vec = (s.cols % 4) == 0;
    {
      const int r = tid >> 4, c = (tid & 15) * 4;
      const int gr = r0 + r, gc = c0 + c;
      if (gr < s.rows) {
        const long long e = (long long)gr * s.cols + gc;
        if (vec && gc + 4 <= s.cols) {
          const float4 w = upd4<EXT, CLIP, WD>(a, (size_t)(s.off + e), h);
          bf16x4 hv = {f2bf(w.x), f2bf(w.y), f2bf(w.z), f2bf(w.w)};
          if (s.sh_off >= 0) *reinterpret_cast<bf16x4*>(a.shadow + s.sh_off + e) = hv;
          *reinterpret_cast<bf16x4*>(&tile[r][c]) = hv;
        } else {
          for (int q = 0; q < 4 && gc + q < s.cols; ++q) {
            const float w = upds<EXT, CLIP, WD>(a, (size_t)(s.off + e + q), h);
            const bf16 hv = f2bf(w);
            if (s.sh_off >= 0) a.shadow[s.sh_off + e + q] = hv;
            tile[r][c + q] = hv;
          }
        }
      }
    }
    lds_barrier();
#pragma unroll
    for (int it = 0; it < kTileR * 64 / 256; ++it) {
      const int i = it * 256 + tid;
      const int c = i / kTileR, r = i % kTileR, gr = r0 + r, gc = c0 + c;
      if (gr < s.rows && gc < s.cols) a.shadow[s.sht_off + (long long)gc * s.rows + gr] = tile[r][c];
    }
  }
}

// The CLIP kernels.  A norm within c (scale exactly 1): nothing is clipped in this workgroup's segment, and
// it runs the unclipped kernel's own program text, so its result is that kernel's bit for bit.  (Multiplying
// by 1 is exact, but the compiler contracts opt_step's multiplies and adds differently around it: with the
// multiply in place the RMSprop kinds came out one bit off on some elements.)  The choice needs the table
// entry and the scale ahead of the prologue's other loads; both are read again there from the cache.
template <bool EXT>
__device__ __forceinline__ void optim_apply_clip(const OptArgs a, const ClipArgs k) {
  if (k.mode != kClipValue && k.scale[k.mode == kClipGlobalNorm ? 0 : a.table[blockIdx.x].x] == 1.f)
    optim_apply<EXT, false>(a, ClipArgs{});
  else
    optim_apply<EXT, true>(a, k);
}

// The WD kernels, with a clip (k.mode) or without (kClipNone).  A workgroup whose segment's decay is zero (a
// variable excluded from it) runs the program text without the decay, clipped or not as above: bit for bit
// what tde_optim_apply / tde_optim_apply_clip give that variable.
template <bool EXT>
__device__ __forceinline__ void optim_apply_wd(const OptArgs a, const ClipArgs k, const WdArgs d) {
  const int seg = a.table[blockIdx.x].x;
  const bool clip = k.mode == kClipValue ||
                    (k.mode != kClipNone && k.scale[k.mode == kClipGlobalNorm ? 0 : seg] != 1.f);
  if (d.wd[seg] != 0.f) {
    if (clip) optim_apply<EXT, true, true>(a, k, d);
    else optim_apply<EXT, false, true>(a, ClipArgs{}, d);
  } else {
    if (clip) optim_apply<EXT, true>(a, k);
    else optim_apply<EXT, false>(a, ClipArgs{});
  }
}

__global__ __launch_bounds__(256) void optim_apply_kernel(OptArgs a) {
  optim_apply<false, false>(a, ClipArgs{});
}

__global__ __launch_bounds__(256) void optim_apply_ext_kernel(OptArgs a) {
  optim_apply<true, false>(a, ClipArgs{});
}

__global__ __launch_bounds__(256) void optim_apply_clip_kernel(OptArgs a, ClipArgs k) {
  optim_apply_clip<false>(a, k);
}

__global__ __launch_bounds__(256) void optim_apply_ext_clip_kernel(OptArgs a, ClipArgs k) {
  optim_apply_clip<true>(a, k);
}

__global__ __launch_bounds__(256) void optim_apply_wd_kernel(OptArgs a, ClipArgs k, WdArgs d) {
  optim_apply_wd<false>(a, k, d);
}

__global__ __launch_bounds__(256) void optim_apply_ext_wd_kernel(OptArgs a, ClipArgs k, WdArgs d) {
  optim_apply_wd<true>(a, k, d);
}

// Writes bf16 shadows from the current weights without updating (init/restore).
__global__ __launch_bounds__(256) void shadow_refresh_kernel(const float* w, bf16* shadow,
                                                             const OptSeg* segs,
                                                             const int4* table) {
  __shared__ bf16 tile[kTileR][66];
  const int4 ent = table[blockIdx.x];
  const OptSeg s = segs[ent.x];
  const int tid = threadIdx.x;
  if (ent.y == 0) {
    const long long n = (long long)s.rows * s.cols;
    const long long beg = (long long)ent.z * kChunk;
    const long long end = beg + kChunk < n ? beg + kChunk : n;
    if (s.sh_off >= 0)
      for (long long e = beg + tid; e < end; e += 256) shadow[s.sh_off + e] = f2bf(w[s.off + e]);
  } else {
    const int r0 = ent.z * kTileR, c0 = ent.w * 64;
    for (int i = tid; i < kTileR * 64; i += 256) {
      const int r = i >> 6, c = i & 63, gr = r0 + r, gc = c0 + c;
      if (gr < s.rows && gc < s.cols) {
        const long long e = (long long)gr * s.cols + gc;
        const bf16 h = f2bf(w[s.off + e]);
        if (s.sh_off >= 0) shadow[s.sh_off + e] = h;
        tile[r][c] = h;
      }
    }
    __syncthreads();
    for (int i = tid; i < kTileR * 64; i += 256) {
      const int c = i / kTileR, r = i % kTileR, gr = r0 + r, gc = c0 + c;
      if (gr < s.rows && gc < s.cols) shadow[s.sht_off + (long long)gc * s.rows + gr] = tile[r][c];
    }
  }
}

// Deferred-update flush (one workgroup): applies the ranges if *pend with t = *iterations, then clears
// *pend.  Without pend (an unconditional update) the ranges are spread over the whole grid.
__global__ __launch_bounds__(256) void flat_apply_kernel(FlatApply f) {
  __shared__ int go;
  if (threadIdx.x == 0) go = f.pend ? *f.pend : 1;
  __syncthreads();
  if (!go) return;
  flat_apply(f, opt_uses_t(f.h.kind) ? *f.iterations : 0, blockIdx.x * 256 + threadIdx.x, 256 * gridDim.x);
  __syncthreads();
  if (threadIdx.x == 0 && f.pend) *f.pend = 0;
  if (threadIdx.x == 0 && blockIdx.x == 0 && f.count) atomicAdd(f.count, 1ull);
}

}  // namespace tde

using namespace tde;

// ranges: int[2*nr] = {lo0, n0, lo1, n1, ...}
TDE_API int tde_flat_apply(float* w, float* g, float* m, float* v, const long long* iterations, int* pend,
                           int kind, float lr, float mom, float b1, float b2, float eps, const int* ranges,
                           int nr, int grep, long long grep_stride, unsigned long long* count,
                           hipStream_t stream) {
  if (!opt_kind_fused(kind)) return -1;   // flat_apply is opt_step<false>: kinds 0..3
  if (nr < 0 || nr > kFlatRanges || !opt_slots_ok(kind, m, v) || (opt_uses_t(kind) && !iterations))
    return -1;
  FlatApply f{w, g, m, v, iterations, pend, OptHyper{kind, lr, mom, b1, b2, eps}, nr, {0}, {0}, grep, grep_stride, count};
  for (int i = 0; i < nr; ++i) {
    f.lo[i] = ranges[2 * i];
    f.n[i] = ranges[2 * i + 1];
  }
  int maxn = 0;
  for (int i = 0; i < nr; ++i) maxn = f.n[i] > maxn ? f.n[i] : maxn;
  // pend: one workgroup (it reads and clears the flag); otherwise about one element per thread
  const int nb = pend ? 1 : (maxn + 255) / 256 < 1 ? 1 : ((maxn + 255) / 256 > 64 ? 64 : (maxn + 255) / 256);
  flat_apply_kernel<<<nb, 256, 0, stream>>>(f);
  TDE_LAUNCH_CHECK();
  return 0;
}

// Host helper: number of table entries for a segment list (for sizing).
TDE_API int tde_optim_table_size(const void* segs_host, int nseg) {
  const OptSeg* s = (const OptSeg*)segs_host;
  int n = 0;
  for (int i = 0; i < nseg; ++i) {
    if (s[i].sht_off >= 0)
      n += ((s[i].rows + kTileR - 1) / kTileR) * ((s[i].cols + 63) / 64);
    else
      n += (int)(((long long)s[i].rows * s[i].cols + kChunk - 1) / kChunk);
  }
  return n;
}

// Fills `table_host` (int4 per block) for a segment list.
TDE_API int tde_optim_build_table(const void* segs_host, int nseg, void* table_host) {
  const OptSeg* s = (const OptSeg*)segs_host;
  int4* t = (int4*)table_host;
  int n = 0;
  for (int i = 0; i < nseg; ++i) {
    if (s[i].sht_off >= 0) {
      for (int r = 0; r < (s[i].rows + kTileR - 1) / kTileR; ++r)
        for (int c = 0; c < (s[i].cols + 63) / 64; ++c) t[n++] = int4{i, 1, r, c};
    } else {
      int nb = (int)(((long long)s[i].rows * s[i].cols + kChunk - 1) / kChunk);
      for (int b = 0; b < nb; ++b) t[n++] = int4{i, 0, b, 0};
    }
  }
  return n;
}

TDE_API int tde_optim_apply(float* w, float* g, float* m, float* v, void* shadow,
                            const void* segs_dev, const void* table_dev, int nblocks,
                            const long long* iterations, int kind, float lr, float mom, float b1,
                            float b2, float eps, float grad_scale, int zero_grad,
                            const float* lr_ptr, hipStream_t stream) {
  if (!opt_kind_known(kind) || !opt_slots_ok(kind, m, v)) return -2;
  if (nblocks <= 0) return 0;
  if (((uintptr_t)w | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) return -1;
  OptArgs a{w, g, m, v, (bf16*)shadow, (const OptSeg*)segs_dev, (const int4*)table_dev,
            iterations, OptHyper{kind, lr, mom, b1, b2, eps}, grad_scale, zero_grad, lr_ptr};
  if (opt_kind_fused(kind)) optim_apply_kernel<<<nblocks, 256, 0, stream>>>(a);
  else optim_apply_ext_kernel<<<nblocks, 256, 0, stream>>>(a);
  TDE_LAUNCH_CHECK();
  return 0;
}

// tde_optim_apply with the gradient clipped first: g_eff = (g * grad_scale) * scale, scale = clip_scale[0]
// (kClipGlobalNorm) or clip_scale[seg] (kClipNorm), or g * grad_scale clamped to [-clip_c, clip_c]
// (kClipValue).  An unknown mode, clip_c not positive and finite or a null clip_scale in a norm mode: -3;
// otherwise tde_optim_apply's codes.  A refusal launches nothing and writes nothing.
TDE_API int tde_optim_apply_clip(float* w, float* g, float* m, float* v, void* shadow,
                                 const void* segs_dev, const void* table_dev, int nblocks,
                                 const long long* iterations, int kind, float lr, float mom, float b1,
                                 float b2, float eps, float grad_scale, int zero_grad,
                                 const float* lr_ptr, int clip_mode, float clip_c, const float* clip_scale,
                                 hipStream_t stream) {
  if (!opt_kind_known(kind) || !opt_slots_ok(kind, m, v)) return -2;
  if (!clip_mode_known(clip_mode)) return -3;
  if (clip_mode == kClipValue ? !clip_c_ok(clip_c) : !clip_scale) return -3;
  if (nblocks <= 0) return 0;
  if (((uintptr_t)w | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) return -1;
  if ((uintptr_t)clip_scale & 3) return -1;
  OptArgs a{w, g, m, v, (bf16*)shadow, (const OptSeg*)segs_dev, (const int4*)table_dev,
            iterations, OptHyper{kind, lr, mom, b1, b2, eps}, grad_scale, zero_grad, lr_ptr};
  const ClipArgs k{clip_scale, clip_c, clip_mode};
  if (opt_kind_fused(kind)) optim_apply_clip_kernel<<<nblocks, 256, 0, stream>>>(a, k);
  else optim_apply_ext_clip_kernel<<<nblocks, 256, 0, stream>>>(a, k);
  TDE_LAUNCH_CHECK();
  return 0;
}

// tde_optim_apply / tde_optim_apply_clip with decoupled weight decay in front of the step: the step of segment
// s starts from w - (w * wd[s]) * lr, lr = *lr_ptr when given.  clip_mode kClipNone (0): no clip; otherwise
// tde_optim_apply_clip's rules and codes.  A null wd: -3; wd off the 4-byte grid: -1.  The values of wd live
// on the device: the caller checks them (finite, >= 0).  A refusal launches nothing and writes nothing.
TDE_API int tde_optim_apply_wd(float* w, float* g, float* m, float* v, void* shadow,
                               const void* segs_dev, const void* table_dev, int nblocks,
                               const long long* iterations, int kind, float lr, float mom, float b1,
                               float b2, float eps, float grad_scale, int zero_grad,
                               const float* lr_ptr, int clip_mode, float clip_c, const float* clip_scale,
                               const float* wd, hipStream_t stream) {
  if (!opt_kind_known(kind) || !opt_slots_ok(kind, m, v)) return -2;
  if (clip_mode != kClipNone) {
    if (!clip_mode_known(clip_mode)) return -3;
    if (clip_mode == kClipValue ? !clip_c_ok(clip_c) : !clip_scale) return -3;
  }
  if (!wd) return -3;
  if (nblocks <= 0) return 0;
  if (((uintptr_t)w | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) return -1;
  if (((uintptr_t)clip_scale | (uintptr_t)wd) & 3) return -1;
  OptArgs a{w, g, m, v, (bf16*)shadow, (const OptSeg*)segs_dev, (const int4*)table_dev,
            iterations, OptHyper{kind, lr, mom, b1, b2, eps}, grad_scale, zero_grad, lr_ptr};
  const ClipArgs k{clip_scale, clip_c, clip_mode};
  const WdArgs d{wd};
  if (opt_kind_fused(kind)) optim_apply_wd_kernel<<<nblocks, 256, 0, stream>>>(a, k, d);
  else optim_apply_ext_wd_kernel<<<nblocks, 256, 0, stream>>>(a, k, d);
  TDE_LAUNCH_CHECK();
  return 0;
}

TDE_API int tde_shadow_refresh(const float* w, void* shadow, const void* segs_dev,
                               const void* table_dev, int nblocks, hipStream_t stream) {
  if (nblocks <= 0) return 0;
  shadow_refresh_kernel<<<nblocks, 256, 0, stream>>>(w, (bf16*)shadow, (const OptSeg*)segs_dev,
                                                     (const int4*)table_dev);
  TDE_LAUNCH_CHECK();
  return 0;
}
