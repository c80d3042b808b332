// Gradient norms for clipnorm / global_clipnorm (tde_clip.h): two launches in front of the clipped
// multi-tensor optimizer launch (optim.hip), all three on the step's stream and so inside its hipGraph.
//
// 1. clip_sumsq_kernel: one workgroup of 256 threads per {segment, 4096-element chunk} table entry.  Thread t
//    loads the float4 at chunk + 1024 it + 4 t for it = 0..3 (all four loads before the first use) and
//    accumulates acc = fmaf(x, x, acc) over its 16 elements in that order; elements past the segment's end
//    are not read and enter as zeros (fmaf(0, 0, acc) == acc).  wave_sum, then thread 0 adds the four wave
//    partials in index order and stores partials[block].  No atomics: the result is bitwise reproducible.
// 2. clip_scale_kernel: one workgroup.  clipnorm: wave w takes segments w, w + 4, ...; lane l sums the
//    segment's partials l, l + 64, ... in float64, a fixed xor tree over the 64 lanes follows.
//    global_clipnorm: thread t sums partials t, t + 256, ... in float64, the same tree per wave, the four wave
//    sums added in index order.  Then norm = sqrtf((float)sum), scale = c / fmaxf(norm, c), both stored.
//
// Roundings on the longest path of a partial: 16 fmaf + 6 wave levels + 3 adds = 25 (float32); the float64
// sums add nothing at float32 scale; then the cast to float32, the root and the divide: 28 in all.  A norm is
// therefore within (25 + 1) / 2 + 1 < 28 / 2 units of 2^-24 of the float64 value, relatively; the tests
// (tests/test_grad_clip_gpu.py) allow twice the count, halved for the root.
#include "tde_clip.h"

namespace tde {

__global__ __launch_bounds__(256) void clip_sumsq_kernel(const float* __restrict__ g, const OptSeg* __restrict__ segs,
                                                         const int2* __restrict__ ents, float* __restrict__ partials) {
  __shared__ float wp[4];
  const int2 ent = ents[blockIdx.x];   // {seg, chunk}
  const OptSeg s = segs[ent.x];
  const int tid = threadIdx.x;
  const long long n = (long long)s.rows * s.cols;
  const long long beg = (long long)ent.y * kClipChunk;
  const long long end = beg + kClipChunk < n ? beg + kClipChunk : n;
  const float* p = g + s.off;
  float4 x[kClipChunk / 1024];
#pragma unroll
  for (int it = 0; it < kClipChunk / 1024; ++it) {
    const long long e = beg + it * 1024 + tid * 4;
    if (e + 4 <= end) {
      x[it] = *reinterpret_cast<const float4*>(p + e);
    } else {   // the ragged tail of the segment's last chunk: element by element, nothing past `end` is read
      x[it] = float4{0.f, 0.f, 0.f, 0.f};
      if (e < end) x[it].x = p[e];
      if (e + 1 < end) x[it].y = p[e + 1];
      if (e + 2 < end) x[it].z = p[e + 2];
    }
  }
  float acc = 0.f;
#pragma unroll
  for (int it = 0; it < kClipChunk / 1024; ++it) {
    acc = fmaf(x[it].x, x[it].x, acc);
    acc = fmaf(x[it].y, x[it].y, acc);
    acc = fmaf(x[it].z, x[it].z, acc);
    acc = fmaf(x[it].w, x[it].w, acc);
  }
  acc = wave_sum(acc);
  if ((tid & 63) == 0) wp[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) partials[blockIdx.x] = ((wp[0] + wp[1]) + wp[2]) + wp[3];
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ void clip_store(double sumsq, float c, float* norm, float* scale, int i) {
  const float nrm = sqrtf((float)sumsq);
  norm[i] = nrm;
  scale[i] = c / fmaxf(nrm, c);
}

__global__ __launch_bounds__(256) void clip_scale_kernel(const float* __restrict__ partials,
                                                         const int2* __restrict__ ranges, int nseg, int nent,
                                                         int mode, float c, float* __restrict__ norm,
                                                         float* __restrict__ scale) {
  __shared__ double wp[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (mode == kClipNorm) {
    for (int sg = wave; sg < nseg; sg += 4) {
      const int2 r = ranges[sg];   // {first, count} of the segment's partials
      double acc = 0.0;
      for (int i = lane; i < r.y; i += 64) acc += (double)partials[r.x + i];
      acc = wave_sum_f64(acc);
      if (lane == 0) clip_store(acc, c, norm, scale, sg);
    }
    return;
  }
  double acc = 0.0;
  for (int i = tid; i < nent; i += 256) acc += (double)partials[i];
  acc = wave_sum_f64(acc);
  if (lane == 0) wp[wave] = acc;
  __syncthreads();
  if (tid == 0) clip_store(((wp[0] + wp[1]) + wp[2]) + wp[3], c, norm, scale, 0);
}

}  // namespace tde

using namespace tde;

static int clip_chunks(const OptSeg& s) {
  return (int)(((long long)s.rows * s.cols + kClipChunk - 1) / kClipChunk);
}

// Host helper: number of sum-of-squares workgroups (table entries) for a segment list.
TDE_API int tde_clip_table_size(const void* segs_host, int nseg) {
  const OptSeg* s = (const OptSeg*)segs_host;
  int n = 0;
  for (int i = 0; i < nseg; ++i) n += clip_chunks(s[i]);
  return n;
}

// Fills `ents_host` (int2 {seg, chunk} per workgroup) and `ranges_host` (int2 {first, count} per segment: the
// segment's entries, consecutive).  Returns the number of entries.
TDE_API int tde_clip_build_table(const void* segs_host, int nseg, void* ents_host, void* ranges_host) {
  const OptSeg* s = (const OptSeg*)segs_host;
  int2* e = (int2*)ents_host;
  int2* r = (int2*)ranges_host;
  int n = 0;
  for (int i = 0; i < nseg; ++i) {
    const int nc = clip_chunks(s[i]);
    r[i] = int2{n, nc};
    for (int c = 0; c < nc; ++c) e[n++] = int2{i, c};
  }
  return n;
}

// partials[b] = the sum of squares of entry b's chunk of g.  A null pointer or g off the 16-byte grid: a
// negative code, nothing launched.
TDE_API int tde_clip_sumsq(const float* g, const void* segs_dev, const void* ents_dev, int nent, float* partials,
                           hipStream_t stream) {
  if (!g || !segs_dev || !ents_dev || !partials || nent < 0) return -1;
  if ((uintptr_t)g & 15) return -1;
  if (nent == 0) return 0;
  clip_sumsq_kernel<<<nent, 256, 0, stream>>>(g, (const OptSeg*)segs_dev, (const int2*)ents_dev, partials);
  TDE_LAUNCH_CHECK();
  return 0;
}

// mode kClipNorm: norm[s], scale[s] for every segment s from its range of partials; kClipGlobalNorm: norm[0],
// scale[0] from all `nent` partials.  Any other mode, c not positive and finite, or a null pointer: a
// negative code, nothing launched, nothing written.
TDE_API int tde_clip_scale(const float* partials, const void* ranges_dev, int nseg, int nent, int mode, float c,
                           float* norm, float* scale, hipStream_t stream) {
  if (mode != kClipNorm && mode != kClipGlobalNorm) return -3;
  if (!clip_c_ok(c)) return -3;
  if (!partials || !norm || !scale || nseg < 0 || nent < 0 || (mode == kClipNorm && !ranges_dev)) return -1;
  clip_scale_kernel<<<1, 256, 0, stream>>>(partials, (const int2*)ranges_dev, nseg, nent, mode, c, norm, scale);
  TDE_LAUNCH_CHECK();
  return 0;
}
