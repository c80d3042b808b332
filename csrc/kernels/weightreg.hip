// Weight regularizers on the device (tde_reg.h): two launches on the step's stream, in front of a clip's norm
// launches (gradclip.hip) and the multi-tensor optimizer launch (optim.hip), and so inside the step's hipGraph.
//
// 1. reg_grad_kernel: one workgroup of 256 threads per {segment, 4096-element chunk} table entry; the table
//    holds regularized segments only.  Thread t loads the float4 of w and of g at chunk + 1024 it + 4 t for
//    it = 0..3 (all eight loads before the first use).  Per element, with c2 = l2 + l2 (exact):
//        g   <- g + fmaf(c2, w, l1 * sgn(w))        sgn(+-0) = 0, so l1 * sgn(w) is -l1, 0 or l1 exactly
//        acc <- fmaf(l1, |w|, fmaf(l2 * w, w, acc))
//    over its 16 elements in that order; elements past the segment's end are neither read nor written and
//    enter the sum as zeros (both fmaf return acc).  wave_sum, then thread 0 adds the four wave partials in
//    index order and stores partials[block].  No atomics: bitwise reproducible.  A null g: partials only.
// 2. reg_finish_kernel: one workgroup.  Thread t sums partials t, t + 256, ... in float64, a fixed xor tree
//    over the 64 lanes, the four wave sums added in index order; penalty[0] = (float)sum, and with a metrics
//    pointer thread 0 stores metrics[0] = fmaf((float)rows, penalty, metrics[0]): the head kernels that add the
//    step's losses there ran earlier on the stream.
//
// Roundings.  g: two per element (the fmaf, the add).  A partial, longest path: 16 x (l2 * w, fmaf, fmaf) = 48,
// + 6 wave levels + 3 adds = 57 (float32); the float64 sums add nothing at float32 scale; the cast to float32:
// 58 in all.  Every term is >= 0, so the penalty is within 58 / 2 units of 2^-24 of the float64 value,
// relatively; the tests (tests/test_weight_reg_gpu.py) allow twice the count.
#include "tde_reg.h"

namespace tde {

__device__ __forceinline__ float4 reg_load4(const float* p, long long e, long long end) {
  if (e + 4 <= end) return *reinterpret_cast<const float4*>(p + e);
  float4 x = float4{0.f, 0.f, 0.f, 0.f};   // the ragged tail: element by element, nothing past `end` is read
  if (e < end) x.x = p[e];
  if (e + 1 < end) x.y = p[e + 1];
  if (e + 2 < end) x.z = p[e + 2];
  return x;
}

__device__ __forceinline__ float reg_g(float g, float w, float l1, float c2) {
  const float s = w > 0.f ? l1 : (w < 0.f ? -l1 : 0.f);
  return g + fmaf(c2, w, s);
}

__device__ __forceinline__ float reg_acc(float acc, float w, float l1, float l2) {
  return fmaf(l1, fabsf(w), fmaf(l2 * w, w, acc));
}

__global__ __launch_bounds__(256) void reg_grad_kernel(const float* __restrict__ w, float* __restrict__ g,
                                                       const OptSeg* __restrict__ segs,
                                                       const RegCoef* __restrict__ coef,
                                                       const int2* __restrict__ ents, float* __restrict__ partials) {
  __shared__ float wp[4];
  const int2 ent = ents[blockIdx.x];   // {seg, chunk}
  const OptSeg s = segs[ent.x];
  const RegCoef k = coef[ent.x];
  const int tid = threadIdx.x;
  const long long n = (long long)s.rows * s.cols;
  const long long beg = (long long)ent.y * kRegChunk;
  const long long end = beg + kRegChunk < n ? beg + kRegChunk : n;
  const float* pw = w + s.off;
  float* pg = g ? g + s.off : nullptr;
  float4 x[kRegChunk / 1024], y[kRegChunk / 1024];
#pragma unroll
  for (int it = 0; it < kRegChunk / 1024; ++it) x[it] = reg_load4(pw, beg + it * 1024 + tid * 4, end);
  if (pg) {
#pragma unroll
    for (int it = 0; it < kRegChunk / 1024; ++it) y[it] = reg_load4(pg, beg + it * 1024 + tid * 4, end);
  }
  const float c2 = k.l2 + k.l2;
  if (pg) {
#pragma unroll
    for (int it = 0; it < kRegChunk / 1024; ++it) {
      const long long e = beg + it * 1024 + tid * 4;
      const float4 r = {reg_g(y[it].x, x[it].x, k.l1, c2), reg_g(y[it].y, x[it].y, k.l1, c2),
                        reg_g(y[it].z, x[it].z, k.l1, c2), reg_g(y[it].w, x[it].w, k.l1, c2)};
      if (e + 4 <= end) {
        *reinterpret_cast<float4*>(pg + e) = r;
      } else {   // nothing past `end` is written
        if (e < end) pg[e] = r.x;
        if (e + 1 < end) pg[e + 1] = r.y;
        if (e + 2 < end) pg[e + 2] = r.z;
      }
    }
  }
  float acc = 0.f;
#pragma unroll
  for (int it = 0; it < kRegChunk / 1024; ++it) {
    acc = reg_acc(acc, x[it].x, k.l1, k.l2);
    acc = reg_acc(acc, x[it].y, k.l1, k.l2);
    acc = reg_acc(acc, x[it].z, k.l1, k.l2);
    acc = reg_acc(acc, x[it].w, k.l1, k.l2);
  }
  acc = wave_sum(acc);
  if ((tid & 63) == 0) wp[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) partials[blockIdx.x] = ((wp[0] + wp[1]) + wp[2]) + wp[3];
}

__global__ __launch_bounds__(256) void reg_finish_kernel(const float* __restrict__ partials, int nent,
                                                         float* __restrict__ penalty, float* __restrict__ metrics,
                                                         int rows) {
  __shared__ double wp[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double acc = 0.0;
  for (int i = tid; i < nent; i += 256) acc += (double)partials[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (lane == 0) wp[wave] = acc;
  __syncthreads();
  if (tid == 0) {
    const float p = (float)(((wp[0] + wp[1]) + wp[2]) + wp[3]);
    penalty[0] = p;
    if (metrics) metrics[0] = fmaf((float)rows, p, metrics[0]);
  }
}

}  // namespace tde

using namespace tde;

static int reg_chunks(const OptSeg& s) {
  return (int)(((long long)s.rows * s.cols + kRegChunk - 1) / kRegChunk);
}

// Host helper: number of reg_grad workgroups (table entries) for a segment list and its coefficients; a
// segment whose l1 and l2 are both zero has none.  A null pointer: -1; a coefficient that is negative or not
// finite: -3.
TDE_API int tde_reg_table_size(const void* segs_host, const void* coef_host, int nseg) {
  if (!segs_host || !coef_host || nseg < 0) return -1;
  const OptSeg* s = (const OptSeg*)segs_host;
  const RegCoef* k = (const RegCoef*)coef_host;
  int n = 0;
  for (int i = 0; i < nseg; ++i) {
    if (!reg_coef_ok(k[i].l1) || !reg_coef_ok(k[i].l2)) return -3;
    if (k[i].l1 != 0.f || k[i].l2 != 0.f) n += reg_chunks(s[i]);
  }
  return n;
}

// Fills `ents_host` (int2 {seg, chunk} per workgroup; a segment's entries are consecutive).  Returns the
// number of entries, or tde_reg_table_size's codes with nothing written.
TDE_API int tde_reg_build_table(const void* segs_host, const void* coef_host, int nseg, void* ents_host) {
  const int want = tde_reg_table_size(segs_host, coef_host, nseg);
  if (want < 0) return want;
  if (!ents_host) return -1;
  const OptSeg* s = (const OptSeg*)segs_host;
  const RegCoef* k = (const RegCoef*)coef_host;
  int2* e = (int2*)ents_host;
  int n = 0;
  for (int i = 0; i < nseg; ++i) {
    if (k[i].l1 == 0.f && k[i].l2 == 0.f) continue;
    const int nc = reg_chunks(s[i]);
    for (int c = 0; c < nc; ++c) e[n++] = int2{i, c};
  }
  return n;
}

// g += the regularizers' gradient over the table's chunks (g null: skipped), partials[b] = the penalty of
// entry b's chunk of w.  A null pointer or w / g off the 16-byte grid: -1, nothing launched.
TDE_API int tde_reg_grad(const float* w, float* g, const void* segs_dev, const void* coef_dev, const void* ents_dev,
                         int nent, float* partials, hipStream_t stream) {
  if (!w || !segs_dev || !coef_dev || !ents_dev || !partials || nent < 0) return -1;
  if (((uintptr_t)w | (uintptr_t)g) & 15) return -1;
  if ((uintptr_t)partials & 3) return -1;
  if (nent == 0) return 0;
  reg_grad_kernel<<<nent, 256, 0, stream>>>(w, g, (const OptSeg*)segs_dev, (const RegCoef*)coef_dev,
                                            (const int2*)ents_dev, partials);
  TDE_LAUNCH_CHECK();
  return 0;
}

// penalty[0] = the float64 sum of the `nent` partials; metrics (nullable): metrics[0] += rows * penalty[0].
// A null pointer, a misaligned word or rows < 0: -1, nothing launched, nothing written.
TDE_API int tde_reg_finish(const float* partials, int nent, float* penalty, float* metrics, int rows,
                           hipStream_t stream) {
  if (!partials || !penalty || nent < 0 || rows < 0) return -1;
  if (((uintptr_t)partials | (uintptr_t)penalty | (uintptr_t)metrics) & 3) return -1;
  reg_finish_kernel<<<1, 256, 0, stream>>>(partials, nent, penalty, metrics, rows);
  TDE_LAUNCH_CHECK();
  return 0;
}
