// GroupNormalization / LayerNormalization, float32 forms: forward (saves mean and rstd per group) and backward
// (dx, per-workgroup partials of dgamma / dbeta, and the ordered reduction of those partials).
//
// One geometry: R independent rows, S positions per row, C channels, G groups, D = C / G.  Group (r, g) holds
// S*D elements: for each s, D contiguous floats at ((r*S + s)*C + g*D).  GroupNormalization on an image is
// (N, H*W, C, groups), on [N, C] it is (N, 1, C, groups), LayerNormalization(axis=-1) is (N*H*W, 1, C, 1).
// y = (x - mean) * rstd * gamma + beta with the population variance of the group; C <= 2048, any D, any S.
//
// * Row form (S == 1).  One wave per row, four rows per workgroup at a time, a workgroup persistent over a
//   strip of `per` rows.  A lane holds the row's float4s lane + 64*j in registers (NV = 1, 2, 4 or 8 of them),
//   so x (and dy in the backward) is read once.  The mean and then the sum of squares of the centred values
//   are reduced with DPP (quad xor 1 / xor 2, row_half_mirror, row_mirror; the last two steps across DPP rows
//   are lane exchanges).  With G > 1 the reduction is segmented: a group of D/4 quads is an aligned run of
//   2^k lanes (only the first k steps run) or, from 64 quads on, a run of register slots j (summed in the lane
//   first).  The scalar form (C % 4 != 0, D % 4 != 0, D/4 no power of two under G > 1, or a base pointer off
//   16 bytes) keeps the row in LDS instead and folds a group with a wave (D > 16) or a lane (D <= 16).
// * Slab form (S > 1).  One workgroup per (row, block of GB whole groups); the host picks GB for 128-byte
//   channel runs, smaller while the grid would not fill the chip.  Lanes run over the block's channel quads
//   first and positions second (16-byte loads along C).  A lane keeps Welford's (n, mean, M2) per channel over
//   its positions; lanes with the same quad are combined through LDS with Chan's update in a fixed tree, and a
//   wave folds the D channels of a group the same way, so D = 1, 2, 3 ... are one code path and a float4 may
//   straddle two groups.  When the slab fits the LDS budget it is staged during that one sweep and y comes out
//   of LDS (one HBM read of x, one write of y); otherwise the normalising sweep reads x again.
// * The variance is never E[x^2] - mean^2: centred values (row form) or Welford / Chan (slab form).
// * Backward, with xh = (x - mean)*rstd and g = dy*gamma:  dx = rstd*(g - mean_grp(g) - xh*mean_grp(g*xh)),
//   dgamma_c = sum dy*xh, dbeta_c = sum dy.  The dx launch has the forward's geometry (x and dy in registers /
//   in LDS when both fit) and produces the per-channel sums on its way: the group means are gamma-weighted
//   folds of exactly those.  Each workgroup (row form) or row (slab form) stores one partial row [2][C]; a
//   second small launch sums the partial rows in order: no atomics, bitwise reproducible.  `accum` adds onto
//   dx; dx == nullptr skips it (the input is the model input).
#include "tde_common.h"

#include <initializer_list>

namespace tde {
namespace gn {

constexpr int kThreads = 256, kWaves = 4;
constexpr int kMaxC = 2048;
constexpr int kMaxRowWgs = 512;        // row form: at most this many persistent workgroups (partial rows)
constexpr int kMinStrip = 4;           // ... each over at least one row per wave
constexpr int kSlabLds = 32 * 1024;    // bytes of dynamic LDS a staged slab may take (plus 24 KiB of combine arrays)
constexpr int kRowLds = 64 * 1024;     // scalar row form: bytes of LDS per workgroup
constexpr int kMaxGB = 64;             // groups per slab workgroup

struct Args {
  const float* x;
  const float* dy;
  const float* gamma;   // null: 1
  const float* beta;    // null: 0
  float* y;             // forward: y; backward: dx (null: skipped)
  float* mean;          // [R*G] saved statistics: the forward writes them, the backward reads them
  float* rstd;
  float* part;          // backward: partial rows [P][2][C] (sum dy*xh, sum dy)
  int R, S, C, G, D, per, GB, nblk, accum;
  float eps;
};

template <int V> struct VecOf;
template <> struct VecOf<1> { typedef float T; };
template <> struct VecOf<4> { typedef f32x4 T; };
__device__ __forceinline__ float getc(float v, int) { return v; }
__device__ __forceinline__ float getc(const f32x4& v, int e) { return v[e]; }
__device__ __forceinline__ void setc(float& v, int, float x) { v = x; }
__device__ __forceinline__ void setc(f32x4& v, int e, float x) { v[e] = x; }
__device__ __forceinline__ float hsum(const f32x4& v) { return (v[0] + v[1]) + (v[2] + v[3]); }

// four consecutive floats of a parameter vector that need not be 16-byte aligned (store views); null: fill
__device__ __forceinline__ f32x4 ld4s(const float* p, int c, float fill) {
  f32x4 r = {fill, fill, fill, fill};
  if (p) { r[0] = p[c]; r[1] = p[c + 1]; r[2] = p[c + 2]; r[3] = p[c + 3]; }
  return r;
}

// ------------------------------------------------------------------------------ segmented wave reduction
// Sum over aligned runs of 2^lg lanes (lg 0..6); every lane of a run ends with the run's sum.  All 64 lanes
// must be active.
__device__ __forceinline__ float seg_sum(float v, int lg) {
  if (lg >= 1) v += dpp_f<0xB1>(v);    // quad_perm [1,0,3,2]
  if (lg >= 2) v += dpp_f<0x4E>(v);    // quad_perm [2,3,0,1]
  if (lg >= 3) v += dpp_f<0x141>(v);   // row_half_mirror
  if (lg >= 4) v += dpp_f<0x140>(v);   // row_mirror
  if (lg >= 5) v += __shfl_xor(v, 16, 64);
  if (lg >= 6) v += __shfl_xor(v, 32, 64);
  return v;
}

struct Seg { int all, lg, jg; };   // one group per row | lanes per group = 2^lg | register slots per group
__device__ __forceinline__ Seg seg_of(int G, int DQ) {
  Seg s;
  s.all = G == 1;
  s.jg = DQ >= 64 ? DQ >> 6 : 1;
  s.lg = DQ >= 64 ? 6 : 31 - __clz(DQ);
  return s;
}

// s[j] = the sum over the group that quad (lane + 64*j) belongs to (slots past the row hold zeros)
template <int NV>
__device__ __forceinline__ void seg_reduce(float (&s)[NV], const Seg sg) {
  if (sg.all) {
    float t = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j) t += s[j];
    t = seg_sum(t, 6);
#pragma unroll
    for (int j = 0; j < NV; ++j) s[j] = t;
    return;
  }
#pragma unroll
  for (int h = 1; h < NV; h <<= 1)
    if (sg.jg > h) {
#pragma unroll
      for (int j = 0; j < NV; ++j)
        if (!(j & h)) {
          const float a = s[j] + s[j | h];
          s[j] = a;
          s[j | h] = a;
        }
    }
#pragma unroll
  for (int j = 0; j < NV; ++j) s[j] = seg_sum(s[j], sg.lg);
}

// ------------------------------------------------------------------------------ row form, vector
template <int NV>
__global__ __launch_bounds__(kThreads) void gn_row_fwd_kernel(Args p) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int nq = p.C >> 2, DQ = p.D >> 2;
  const int r0 = blockIdx.x * p.per, r1 = min(p.R, r0 + p.per);
  const Seg sg = seg_of(p.G, DQ);
  const float invD = 1.f / (float)p.D;
  f32x4 ga[NV], be[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int q = lane + 64 * j;
    ga[j] = ld4s(q < nq ? p.gamma : nullptr, 4 * q, 1.f);
    be[j] = ld4s(q < nq ? p.beta : nullptr, 4 * q, 0.f);
  }
  for (int r = r0 + w; r < r1; r += kWaves) {
    const f32x4* xr = reinterpret_cast<const f32x4*>(p.x + (size_t)r * p.C);
    f32x4* yr = reinterpret_cast<f32x4*>(p.y + (size_t)r * p.C);
    f32x4 v[NV];
    float s[NV], mu[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int q = lane + 64 * j;
      v[j] = q < nq ? xr[q] : f32x4{0.f, 0.f, 0.f, 0.f};
      s[j] = hsum(v[j]);
    }
    seg_reduce<NV>(s, sg);
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int q = lane + 64 * j;
      mu[j] = s[j] * invD;
      v[j] = q < nq ? v[j] - mu[j] : f32x4{0.f, 0.f, 0.f, 0.f};
      s[j] = hsum(v[j] * v[j]);
    }
    seg_reduce<NV>(s, sg);
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int q = lane + 64 * j;
      const float rs = 1.f / sqrtf(s[j] * invD + p.eps);
      if (q < nq) {
        yr[q] = v[j] * rs * ga[j] + be[j];
        if (sg.all ? q == 0 : (q & (DQ - 1)) == 0) {
          const size_t gi = (size_t)r * p.G + (sg.all ? 0 : q / DQ);
          p.mean[gi] = mu[j];
          p.rstd[gi] = rs;
        }
      }
    }
  }
}

// dynamic LDS: kWaves x [2][C] channel sums (sum dy*xh, sum dy).  A lane owns its quads of its wave's rows, so
// the accumulators live there race-free and leave the registers to x and dy.
template <int NV>
__global__ __launch_bounds__(kThreads) void gn_row_bwd_kernel(Args p) {
  extern __shared__ float4 gn_smem4[];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int C = p.C, nq = C >> 2, DQ = p.D >> 2;
  float* smem = reinterpret_cast<float*>(gn_smem4);
  f32x4* acc = reinterpret_cast<f32x4*>(smem + (size_t)w * 2 * C);
  const int r0 = blockIdx.x * p.per, r1 = min(p.R, r0 + p.per);
  const Seg sg = seg_of(p.G, DQ);
  const float invD = 1.f / (float)p.D;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 ga[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int q = lane + 64 * j;
    ga[j] = ld4s(q < nq ? p.gamma : nullptr, 4 * q, 1.f);
    if (q < nq) {
      acc[q] = zero;
      acc[nq + q] = zero;
    }
  }
  for (int r = r0 + w; r < r1; r += kWaves) {
    const f32x4* xr = reinterpret_cast<const f32x4*>(p.x + (size_t)r * C);
    const f32x4* dyr = reinterpret_cast<const f32x4*>(p.dy + (size_t)r * C);
    f32x4 xh[NV], g[NV];
    float s1[NV], s2[NV], rs[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int q = lane + 64 * j;
      xh[j] = zero;
      g[j] = zero;
      rs[j] = 0.f;
      if (q < nq) {
        const size_t gi = (size_t)r * p.G + (sg.all ? 0 : q / DQ);
        rs[j] = p.rstd[gi];
        xh[j] = (xr[q] - p.mean[gi]) * rs[j];
        const f32x4 d = dyr[q];
        g[j] = d * ga[j];
        acc[q] += d * xh[j];
        acc[nq + q] += d;
      }
      s1[j] = hsum(g[j]);
      s2[j] = hsum(g[j] * xh[j]);
    }
    seg_reduce<NV>(s1, sg);
    seg_reduce<NV>(s2, sg);
    if (p.y) {
      f32x4* dxr = reinterpret_cast<f32x4*>(p.y + (size_t)r * C);
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        const int q = lane + 64 * j;
        if (q < nq) {
          f32x4 d = (g[j] - s1[j] * invD - xh[j] * (s2[j] * invD)) * rs[j];
          if (p.accum) d += dxr[q];
          dxr[q] = d;
        }
      }
    }
  }
  __syncthreads();
  float* pr = p.part + (size_t)blockIdx.x * 2 * C;   // the four waves' sums in wave order: one partial row
  for (int c = threadIdx.x; c < 2 * C; c += kThreads)
    pr[c] = ((smem[c] + smem[2 * C + c]) + smem[4 * C + c]) + smem[6 * C + c];
}

// ------------------------------------------------------------------------------ row form, scalar (row in LDS)
// blockDim.x = 64 * wpb; a wave's LDS: forward xs[C] st[2G], backward xs[C] ds[C] st[2G] acc[2C].
// Group sums of the row a wave holds in LDS: f(c) summed over the D channels of each group, result through
// out(g, sum).  D > 16: the wave folds one group at a time; otherwise a lane folds a group.
template <typename F, typename O>
__device__ __forceinline__ void row_groups(int G, int D, int lane, F f, O out) {
  if (D > 16) {
    for (int g = 0; g < G; ++g) {
      float s = 0.f;
      for (int d = lane; d < D; d += 64) s += f(g, g * D + d);
      s = seg_sum(s, 6);
      if (lane == 0) out(g, s);
    }
  } else {
    for (int g = lane; g < G; g += 64) {
      float s = 0.f;
      for (int d = 0; d < D; ++d) s += f(g, g * D + d);
      out(g, s);
    }
  }
}

__global__ __launch_bounds__(kThreads) void gn_row_fwd_scalar_kernel(Args p) {
  extern __shared__ float4 gn_smem4[];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wpb = blockDim.x >> 6;
  const int C = p.C, G = p.G, D = p.D;
  float* xs = reinterpret_cast<float*>(gn_smem4) + (size_t)w * (C + 2 * G);
  float* st = xs + C;
  const int r0 = blockIdx.x * p.per, r1 = min(p.R, r0 + p.per);
  const float invD = 1.f / (float)D;
  for (int rr = r0; rr < r1; rr += wpb) {   // uniform over the workgroup: the barriers below are reached by all
    const int r = rr + w;
    const bool on = r < r1;
    const size_t off = (size_t)r * C;
    if (on)
      for (int c = lane; c < C; c += 64) xs[c] = p.x[off + c];
    __syncthreads();
    if (on) row_groups(G, D, lane, [&](int, int c) { return xs[c]; }, [&](int g, float s) { st[g] = s * invD; });
    __syncthreads();
    if (on)
      row_groups(G, D, lane, [&](int g, int c) { const float d = xs[c] - st[g]; return d * d; },
                 [&](int g, float s) {
                   const float rs = 1.f / sqrtf(s * invD + p.eps);
                   st[G + g] = rs;
                   p.mean[(size_t)r * G + g] = st[g];
                   p.rstd[(size_t)r * G + g] = rs;
                 });
    __syncthreads();
    if (on)
      for (int c = lane; c < C; c += 64) {
        const int g = c / D;
        p.y[off + c] = (xs[c] - st[g]) * st[G + g] * (p.gamma ? p.gamma[c] : 1.f) + (p.beta ? p.beta[c] : 0.f);
      }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kThreads) void gn_row_bwd_scalar_kernel(Args p) {
  extern __shared__ float4 gn_smem4[];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wpb = blockDim.x >> 6;
  const int C = p.C, G = p.G, D = p.D, per_wave = 4 * C + 2 * G;
  float* smem = reinterpret_cast<float*>(gn_smem4);
  float* xs = smem + (size_t)w * per_wave;   // xh
  float* ds = xs + C;                        // dy
  float* st = ds + C;                        // group means of g and g*xh
  float* acc = st + 2 * G;                   // sum dy*xh [C], sum dy [C]: a lane owns its channels
  const int r0 = blockIdx.x * p.per, r1 = min(p.R, r0 + p.per);
  const float invD = 1.f / (float)D;
  for (int c = lane; c < 2 * C; c += 64) acc[c] = 0.f;
  for (int rr = r0; rr < r1; rr += wpb) {
    const int r = rr + w;
    const bool on = r < r1;
    const size_t off = (size_t)r * C, goff = (size_t)r * G;
    if (on)
      for (int c = lane; c < C; c += 64) {
        const int g = c / D;
        xs[c] = (p.x[off + c] - p.mean[goff + g]) * p.rstd[goff + g];
        ds[c] = p.dy[off + c];
      }
    __syncthreads();
    if (on) {
      row_groups(G, D, lane, [&](int, int c) { return ds[c] * (p.gamma ? p.gamma[c] : 1.f); },
                 [&](int g, float s) { st[g] = s * invD; });
      row_groups(G, D, lane, [&](int, int c) { return ds[c] * (p.gamma ? p.gamma[c] : 1.f) * xs[c]; },
                 [&](int g, float s) { st[G + g] = s * invD; });
    }
    __syncthreads();
    if (on)
      for (int c = lane; c < C; c += 64) {
        const int g = c / D;
        const float d = ds[c], xh = xs[c];
        acc[c] += d * xh;
        acc[C + c] += d;
        if (p.y) {
          float v = (d * (p.gamma ? p.gamma[c] : 1.f) - st[g] - xh * st[G + g]) * p.rstd[goff + g];
          if (p.accum) v += p.y[off + c];
          p.y[off + c] = v;
        }
      }
    __syncthreads();
  }
  __syncthreads();
  float* pr = p.part + (size_t)blockIdx.x * 2 * C;
  for (int c = threadIdx.x; c < 2 * C; c += blockDim.x) {
    float s = 0.f;
    for (int ww = 0; ww < wpb; ++ww) s += smem[(size_t)ww * per_wave + 2 * C + 2 * G + c];
    pr[c] = s;
  }
}

// ------------------------------------------------------------------------------ slab form
struct Wf { float n, m, s; };   // Welford: count, mean, sum of squared deviations
__device__ __forceinline__ Wf wf_add(const Wf a, const Wf b) {   // Chan's combination
  if (b.n == 0.f) return a;
  if (a.n == 0.f) return b;
  const float n = a.n + b.n, d = b.m - a.m, f = b.n / n;
  Wf r;
  r.n = n;
  r.m = a.m + d * f;
  r.s = a.s + b.s + d * d * a.n * f;
  return r;
}

struct Block {   // a workgroup's (row, group block) and the lane's place in it
  int r, g0, gb, c0, cb, nq, QS, PL, qi, pl;
  bool on;
  size_t base;
};
template <int V>
__device__ __forceinline__ Block block_of(const Args& p) {
  Block b;
  b.r = blockIdx.x / p.nblk;
  b.g0 = (blockIdx.x % p.nblk) * p.GB;
  b.gb = min(p.GB, p.G - b.g0);
  b.c0 = b.g0 * p.D;
  b.cb = b.gb * p.D;
  b.nq = b.cb / V;
  b.QS = min(b.nq, kThreads);
  b.PL = kThreads / b.QS;
  b.qi = threadIdx.x % b.QS;
  b.pl = threadIdx.x / b.QS;
  b.on = b.pl < b.PL;
  b.base = (size_t)b.r * p.S * p.C + b.c0;
  return b;
}
__device__ __forceinline__ int pow2_below(int n) {   // the largest power of two < n (n >= 2), 0 for n < 2
  return n < 2 ? 0 : 1 << (31 - __clz(n - 1));
}

template <int V, bool ST>
__global__ __launch_bounds__(kThreads) void gn_slab_fwd_kernel(Args p) {
  typedef typename VecOf<V>::T T;
  __shared__ float rn[kMaxC], rm[kMaxC], rv[kMaxC];   // (n, mean, M2) per (position lane, channel)
  __shared__ float gmu[kMaxGB], grs[kMaxGB];
  extern __shared__ float4 gn_smem4[];
  float* slab = reinterpret_cast<float*>(gn_smem4);
  const Block b = block_of<V>(p);
  const int S = p.S, C = p.C, D = p.D, cb = b.cb;
  const float* xg = p.x + b.base;
  if (b.on)
    for (int q = b.qi; q < b.nq; q += b.QS) {
      T m = T{}, s2 = T{};
      float n = 0.f;
      for (int s = b.pl; s < S; s += b.PL) {
        const T v = *reinterpret_cast<const T*>(xg + (size_t)s * C + q * V);
        if (ST) *reinterpret_cast<T*>(slab + (size_t)s * cb + q * V) = v;
        n += 1.f;
        const T d = v - m;
        m += d * (1.f / n);
        s2 += d * (v - m);
      }
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const int i = b.pl * cb + q * V + e;
        rn[i] = n;
        rm[i] = getc(m, e);
        rv[i] = getc(s2, e);
      }
    }
  __syncthreads();
  for (int h = pow2_below(b.PL); h >= 1; h >>= 1) {   // position lanes, a fixed tree
    if (b.on && b.pl < h && b.pl + h < b.PL)
      for (int q = b.qi; q < b.nq; q += b.QS)
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const int i = b.pl * cb + q * V + e, k = i + h * cb;
          const Wf a = wf_add(Wf{rn[i], rm[i], rv[i]}, Wf{rn[k], rm[k], rv[k]});
          rn[i] = a.n;
          rm[i] = a.m;
          rv[i] = a.s;
        }
    __syncthreads();
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int g = w; g < b.gb; g += kWaves) {   // the D channels of a group, folded by one wave
    Wf a = {0.f, 0.f, 0.f};
    for (int d = lane; d < D; d += 64) a = wf_add(a, Wf{rn[g * D + d], rm[g * D + d], rv[g * D + d]});
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      Wf o2;
      o2.n = __shfl_xor(a.n, o, 64);
      o2.m = __shfl_xor(a.m, o, 64);
      o2.s = __shfl_xor(a.s, o, 64);
      a = (lane & o) ? wf_add(o2, a) : wf_add(a, o2);
    }
    if (lane == 0) {
      const float rs = 1.f / sqrtf(a.s / a.n + p.eps);
      gmu[g] = a.m;
      grs[g] = rs;
      p.mean[(size_t)b.r * p.G + b.g0 + g] = a.m;
      p.rstd[(size_t)b.r * p.G + b.g0 + g] = rs;
    }
  }
  __syncthreads();
  if (!b.on) return;
  float* yg = p.y + b.base;
  for (int q = b.qi; q < b.nq; q += b.QS) {
    T mu, a, be;
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const int c = q * V + e, g = c / D;
      setc(mu, e, gmu[g]);
      setc(a, e, grs[g] * (p.gamma ? p.gamma[b.c0 + c] : 1.f));
      setc(be, e, p.beta ? p.beta[b.c0 + c] : 0.f);
    }
    for (int s = b.pl; s < S; s += b.PL) {
      const T v = ST ? *reinterpret_cast<const T*>(slab + (size_t)s * cb + q * V)
                     : *reinterpret_cast<const T*>(xg + (size_t)s * C + q * V);
      *reinterpret_cast<T*>(yg + (size_t)s * C + q * V) = (v - mu) * a + be;
    }
  }
}

template <int V, bool ST>
__global__ __launch_bounds__(kThreads) void gn_slab_bwd_kernel(Args p) {
  typedef typename VecOf<V>::T T;
  __shared__ float ra[kMaxC], rb[kMaxC];   // sum dy, sum dy*xh per (position lane, channel)
  __shared__ float gm1[kMaxGB], gm2[kMaxGB];
  extern __shared__ float4 gn_smem4[];
  const Block b = block_of<V>(p);
  const int S = p.S, C = p.C, D = p.D, cb = b.cb;
  float* xs = reinterpret_cast<float*>(gn_smem4);   // xh
  float* ds = xs + (size_t)S * cb;                   // dy
  const float* xg = p.x + b.base;
  const float* dyg = p.dy + b.base;
  const size_t goff = (size_t)b.r * p.G + b.g0;
  if (b.on)
    for (int q = b.qi; q < b.nq; q += b.QS) {
      T mu, rs, sa = T{}, sb = T{};
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const int g = (q * V + e) / D;
        setc(mu, e, p.mean[goff + g]);
        setc(rs, e, p.rstd[goff + g]);
      }
      for (int s = b.pl; s < S; s += b.PL) {
        const T xh = (*reinterpret_cast<const T*>(xg + (size_t)s * C + q * V) - mu) * rs;
        const T d = *reinterpret_cast<const T*>(dyg + (size_t)s * C + q * V);
        if (ST) {
          *reinterpret_cast<T*>(xs + (size_t)s * cb + q * V) = xh;
          *reinterpret_cast<T*>(ds + (size_t)s * cb + q * V) = d;
        }
        sa += d;
        sb += d * xh;
      }
#pragma unroll
      for (int e = 0; e < V; ++e) {
        ra[b.pl * cb + q * V + e] = getc(sa, e);
        rb[b.pl * cb + q * V + e] = getc(sb, e);
      }
    }
  __syncthreads();
  for (int h = pow2_below(b.PL); h >= 1; h >>= 1) {
    if (b.on && b.pl < h && b.pl + h < b.PL)
      for (int q = b.qi; q < b.nq; q += b.QS)
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const int i = b.pl * cb + q * V + e, k = i + h * cb;
          ra[i] += ra[k];
          rb[i] += rb[k];
        }
    __syncthreads();
  }
  float* pr = p.part + (size_t)b.r * 2 * C + b.c0;   // this row's partial: the block's channels
  for (int c = threadIdx.x; c < cb; c += kThreads) {
    pr[c] = rb[c];
    pr[C + c] = ra[c];
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const float inv = 1.f / ((float)S * (float)D);
  for (int g = w; g < b.gb; g += kWaves) {
    float s1 = 0.f, s2 = 0.f;
    for (int d = lane; d < D; d += 64) {
      const float ga = p.gamma ? p.gamma[b.c0 + g * D + d] : 1.f;
      s1 += ga * ra[g * D + d];
      s2 += ga * rb[g * D + d];
    }
    s1 = seg_sum(s1, 6);
    s2 = seg_sum(s2, 6);
    if (lane == 0) {
      gm1[g] = s1 * inv;
      gm2[g] = s2 * inv;
    }
  }
  __syncthreads();
  if (!b.on || !p.y) return;
  float* dxg = p.y + b.base;
  for (int q = b.qi; q < b.nq; q += b.QS) {
    T mu, rs, ga, m1, m2;
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const int c = q * V + e, g = c / D;
      setc(mu, e, p.mean[goff + g]);
      setc(rs, e, p.rstd[goff + g]);
      setc(ga, e, p.gamma ? p.gamma[b.c0 + c] : 1.f);
      setc(m1, e, gm1[g]);
      setc(m2, e, gm2[g]);
    }
    for (int s = b.pl; s < S; s += b.PL) {
      T xh, d;
      if (ST) {
        xh = *reinterpret_cast<const T*>(xs + (size_t)s * cb + q * V);
        d = *reinterpret_cast<const T*>(ds + (size_t)s * cb + q * V);
      } else {
        xh = (*reinterpret_cast<const T*>(xg + (size_t)s * C + q * V) - mu) * rs;
        d = *reinterpret_cast<const T*>(dyg + (size_t)s * C + q * V);
      }
      T v = (d * ga - m1 - xh * m2) * rs;
      T* o = reinterpret_cast<T*>(dxg + (size_t)s * C + q * V);
      if (p.accum) v += *o;
      *o = v;
    }
  }
}

// dgamma[c] = sum_p part[p][0][c], dbeta[c] = sum_p part[p][1][c], in the order of p
__global__ __launch_bounds__(kThreads) void gn_part_reduce_kernel(const float* __restrict__ part, int P, int C,
                                                                  float* dgamma, float* dbeta) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= 2 * C) return;
  float* out = i < C ? dgamma : dbeta;
  if (!out) return;
  float s = 0.f;
  for (int q = 0; q < P; ++q) s += part[(size_t)q * 2 * C + i];
  out[i < C ? i : i - C] = s;
}

// ------------------------------------------------------------------------------ host
struct Plan {
  int slab, P, per, GB, nblk, st_fwd, st_bwd;
};

static bool geo_ok(int R, int S, int C, int G) {
  return R >= 1 && S >= 1 && C >= 1 && C <= kMaxC && G >= 1 && C % G == 0;
}
static int gcd4(int d) { return d % 4 == 0 ? 4 : (d % 2 == 0 ? 2 : 1); }

// Work split of a geometry.  P, the number of partial rows of the backward, follows (R, S) alone, so the
// partial buffer does not depend on operand alignment; V = 4 keeps a slab block's first channel a quad's.
static Plan plan_of(int R, int S, int C, int G, int V) {
  Plan pl = {};
  const int D = C / G;
  if (S == 1) {
    pl.per = (R + kMaxRowWgs - 1) / kMaxRowWgs;
    if (pl.per < kMinStrip) pl.per = kMinStrip;
    pl.P = (R + pl.per - 1) / pl.per;
    return pl;
  }
  pl.slab = 1;
  pl.P = R;
  const int m = V == 4 ? 4 / gcd4(D) : 1;
  for (int target = 32;; target >>= 1) {
    int gb = (target + D - 1) / D;
    gb = (gb + m - 1) / m * m;
    if (gb > G) gb = G;
    pl.GB = gb;
    pl.nblk = (G + gb - 1) / gb;
    if ((long long)R * pl.nblk >= 512 || target <= 4) break;
  }
  const long long slab = (long long)S * pl.GB * D * sizeof(float);
  pl.st_fwd = slab <= kSlabLds;
  pl.st_bwd = 2 * slab <= kSlabLds;
  return pl;
}

static int vec_of(int C, std::initializer_list<const void*> ptrs) {
  if (C % 4) return 1;
  for (const void* q : ptrs)
    if (q && (reinterpret_cast<uintptr_t>(q) & 15)) return 1;
  return 4;
}
// the register row form: whole quads per group, and a group an aligned power-of-two run of quads
static bool row_vec_ok(int C, int G, int V) {
  const int D = C / G;
  if (V != 4 || D % 4) return false;
  const int DQ = D / 4;
  return G == 1 || (DQ & (DQ - 1)) == 0;
}
static int row_wpb(size_t floats_per_wave) {
  const size_t n = kRowLds / (floats_per_wave * sizeof(float));
  return n >= kWaves ? kWaves : (n < 1 ? 1 : (int)n);
}

#define GN_NV_CASES(KERNEL, nq, lds)                                                       \
  do {                                                                                 \
    if ((nq) <= 64) KERNEL<1><<<grid, kThreads, lds, stream>>>(a);                     \
    else if ((nq) <= 128) KERNEL<2><<<grid, kThreads, lds, stream>>>(a);               \
    else if ((nq) <= 256) KERNEL<4><<<grid, kThreads, lds, stream>>>(a);               \
    else KERNEL<8><<<grid, kThreads, lds, stream>>>(a);                                \
  } while (0)
#define GN_SLAB_CASES(KERNEL, st, lds)                                                 \
  do {                                                                                 \
    if (V == 4) {                                                                      \
      if (st) KERNEL<4, true><<<grid, kThreads, lds, stream>>>(a);                     \
      else KERNEL<4, false><<<grid, kThreads, 0, stream>>>(a);                         \
    } else {                                                                           \
      if (st) KERNEL<1, true><<<grid, kThreads, lds, stream>>>(a);                     \
      else KERNEL<1, false><<<grid, kThreads, 0, stream>>>(a);                         \
    }                                                                                  \
  } while (0)

}  // namespace gn
}  // namespace tde

using namespace tde::gn;

// out = {slab form, partial rows P, rows per strip, groups per slab block, blocks per row, forward slab staged
// in LDS, backward slabs staged in LDS} for 16-byte aligned operands; returns P.
TDE_API int tde_gn32_plan(int R, int S, int C, int G, int* out) {
  if (!geo_ok(R, S, C, G)) return -1;
  const Plan pl = plan_of(R, S, C, G, C % 4 == 0 ? 4 : 1);
  if (out) {
    out[0] = pl.slab; out[1] = pl.P; out[2] = pl.per; out[3] = pl.GB; out[4] = pl.nblk;
    out[5] = pl.st_fwd; out[6] = pl.st_bwd;
  }
  return pl.P;
}

// y = (x - mean)*rstd*gamma + beta per group; mean, rstd [R*G] are saved for the backward.
TDE_API int tde_gn32_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                         int R, int S, int C, int G, float eps, hipStream_t stream) {
  if (!x || !y || !mean || !rstd || !geo_ok(R, S, C, G)) return -1;
  const int V = vec_of(C, {x, y});
  const Plan pl = plan_of(R, S, C, G, V);
  Args a = {};
  a.x = x; a.gamma = gamma; a.beta = beta; a.y = y; a.mean = mean; a.rstd = rstd;
  a.R = R; a.S = S; a.C = C; a.G = G; a.D = C / G; a.per = pl.per; a.GB = pl.GB; a.nblk = pl.nblk; a.eps = eps;
  if (!pl.slab) {
    const dim3 grid((unsigned)pl.P);
    if (row_vec_ok(C, G, V)) {
      GN_NV_CASES(gn_row_fwd_kernel, C / 4, 0);
    } else {
      const size_t per_wave = (size_t)C + 2 * G;
      const int wpb = row_wpb(per_wave);
      gn_row_fwd_scalar_kernel<<<grid, 64 * wpb, wpb * per_wave * sizeof(float), stream>>>(a);
    }
  } else {
    if (pl.GB > kMaxGB) return -3;
    const dim3 grid((unsigned)((long long)R * pl.nblk));
    const size_t lds = (size_t)S * pl.GB * a.D * sizeof(float);
    GN_SLAB_CASES(gn_slab_fwd_kernel, pl.st_fwd, lds);
  }
  TDE_LAUNCH_CHECK();
  return 0;
}

// dx (+)= the input gradient (dx null: skipped); dgamma / dbeta (either may be null) = the ordered sum of the
// partial rows `part` [tde_gn32_plan rows][2][C].
TDE_API int tde_gn32_bwd(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd,
                         float* dx, int accum, float* dgamma, float* dbeta, float* part, int R, int S, int C, int G,
                         hipStream_t stream) {
  if (!dy || !x || !mean || !rstd || !part || !geo_ok(R, S, C, G)) return -1;
  const int V = vec_of(C, {x, dy, dx});
  const Plan pl = plan_of(R, S, C, G, V);
  Args a = {};
  a.x = x; a.dy = dy; a.gamma = gamma; a.y = dx; a.mean = const_cast<float*>(mean); a.rstd = const_cast<float*>(rstd);
  a.part = part; a.accum = accum;
  a.R = R; a.S = S; a.C = C; a.G = G; a.D = C / G; a.per = pl.per; a.GB = pl.GB; a.nblk = pl.nblk;
  if (!pl.slab) {
    const dim3 grid((unsigned)pl.P);
    if (row_vec_ok(C, G, V)) {
      GN_NV_CASES(gn_row_bwd_kernel, C / 4, kWaves * 2 * (size_t)C * sizeof(float));
    } else {
      const size_t per_wave = 4 * (size_t)C + 2 * G;
      const int wpb = row_wpb(per_wave);
      gn_row_bwd_scalar_kernel<<<grid, 64 * wpb, wpb * per_wave * sizeof(float), stream>>>(a);
    }
  } else {
    if (pl.GB > kMaxGB) return -3;
    const dim3 grid((unsigned)((long long)R * pl.nblk));
    const size_t lds = 2 * (size_t)S * pl.GB * a.D * sizeof(float);
    GN_SLAB_CASES(gn_slab_bwd_kernel, pl.st_bwd, lds);
  }
  TDE_LAUNCH_CHECK();
  if (dgamma || dbeta) {
    gn_part_reduce_kernel<<<(2 * C + kThreads - 1) / kThreads, kThreads, 0, stream>>>(part, pl.P, C, dgamma, dbeta);
    TDE_LAUNCH_CHECK();
  }
  return 0;
}
