// MultiHeadAttention core (self-attention, short sequences), float32 on v_mfma_f32_16x16x4_f32: forward
// (O and the per-row log-sum-exp) and backward (dQ, dK, dV).  No T x T tensor reaches HBM.
//
// Operands: Q, K [B, T, H*dk], V, O, dO [B, T, H*dv], head-major in the last axis (a head's row is d contiguous
// floats at stride H*d), lse [B, H, T].  1 <= T <= 256, dk and dv multiples of 4 up to 64.
//   S = Q K^T / sqrt(dk),  P = softmax(S) over the keys,  O = P V,  lse_i = log sum_j exp(S_ij)
//   delta_i = sum_c dO_ic O_ic,  P = exp(S - lse),  dV = P^T dO,  dP = dO V^T,  dS = P o (dP - delta),
//   dQ = dS K / sqrt(dk),  dK = dS^T Q / sqrt(dk)
//
// The MFMA: a lane (fr = lane % 16, fq = lane / 16) gives A[m = fr][k = fq] and B[k = fq][n = fr] and gets
// D[m = 4 fq + r][n = fr] in register r.  Every product here is laid out so that the accumulator of one product
// IS the B operand of the next (k = 4 fq + r, n = fr), which is why the forward and the dQ sweep compute S
// TRANSPOSED (keys on m, query rows on n) and the dK / dV sweep computes it straight (query rows on m, keys on
// n): P and dS never pass through LDS, and never leave the registers.  (The other route, a per-wave LDS strip
// that transposes P, costs 16 KiB of LDS traffic per wave and key block each way and two more waits; the
// transposed product costs nothing: K and Q merely swap operand slots.)  A contraction over a head dimension
// reads float4s (lane: row fr, floats 16 ch + 4 fq ..+3) and issues four MFMAs, one per component: k runs over
// the 16 floats of chunk ch in a permuted order, the same for both operands.
//
// * Forward, one workgroup per (sample, head, block of 64 query rows), 4 waves of 16 query rows.  The wave's Q
//   rows are a B operand, which a lane holds in registers (4 float4s, scaled by 1/sqrt(dk) as they are loaded;
//   they need no LDS at all).  K comes through LDS in tiles of 64 keys (16-byte loads along d, rows past T and
//   columns past d zero); S^T of the whole strip, 16 x T, stays in 4 * ceil(T / 64) accumulator tiles
//   (at most 64 VGPRs; the kernel is instantiated per number of key blocks, so the strip is indexed statically).
//   Keys past T are set to -inf; the query row of a lane is fr, so the row maximum and the row sum fold the
//   lane's own registers and then the four lanes fr, fr + 16, fr + 32, fr + 48: the exact two-pass softmax,
//   no rescaling.  V then comes through LDS in the same tiles and O^T = V^T P^T accumulates with the strip as
//   B operand; a lane ends with four consecutive floats of its row: a 16-byte store, times 1 / row sum.
// * Backward, dK / dV: one workgroup per (sample, head, block of 64 keys), a wave owns 16 keys.  Its K and V
//   rows are B operands of S = Q K^T and dP = dO V^T and live in registers for the whole sweep (the LDS a
//   resident K_j / V_j would take is left to the query side); Q (scaled) and dO of a block of 64 query rows
//   are staged in LDS, with lse and delta (computed from O and dO while dO is staged).  P and dS tiles are B
//   operands of dV^T += dO^T P and dK^T += Q^T dS; the accumulators stay in registers across the query blocks.
// * Backward, dQ: a sweep of its own with the forward's geometry (a workgroup per query block, looping over the
//   key blocks; Q, dO, lse, delta of the wave's rows in registers, K and V tiles in LDS): S^T and dP^T tiles,
//   dS^T as B operand of dQ^T += K^T dS^T.  No partial buffers and no atomics: every output element has one
//   writer and one summation order, so the backward is bitwise reproducible.  It recomputes S and dP (7 instead
//   of 5 products in all).  `accum` adds onto dQ.
// * No kernel holds more than 35 KiB of LDS (two 64 x 68 float tiles), so the backward tiles by construction.
#include "tde_common.h"

#include <cstdint>
#include <initializer_list>

namespace tde {
namespace mha {

constexpr int kThreads = 256;
constexpr int kBlock = 64;             // query rows / keys per workgroup and per LDS tile
constexpr int kMaxT = 256, kMaxD = 64;
constexpr int kLd = kMaxD + 4;         // the widest LDS row (floats); a tile of d floats uses rows of 16*ceil(d/16) + 4
constexpr int kTile = kBlock * kLd;

struct Args {
  const float* q; const float* k; const float* v; const float* o; const float* d_o;
  float* out;       // forward: O
  float* lse;       // forward writes, backward reads
  float* dq; float* dk; float* dv;
  int B, H, T, dk_, dv_, accum;
  float scale;      // 1 / sqrt(dk)
};

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
// one 16-float chunk of a contraction over a head dimension: both operands float4s of the same columns
__device__ __forceinline__ f32x4 mfma_chunk(const f32x4 a, const f32x4 b, f32x4 c) {
  c = mfma4(a[0], b[0], c);
  c = mfma4(a[1], b[1], c);
  c = mfma4(a[2], b[2], c);
  return mfma4(a[3], b[3], c);
}
__device__ __forceinline__ float dot4(const f32x4 a, const f32x4 b) {
  return (a[0] * b[0] + a[1] * b[1]) + (a[2] * b[2] + a[3] * b[3]);
}

struct Where {   // the (sample, head, block) of a workgroup and the lane's place in the MFMA layout
  int b, h, blk, w, fr, fq;
  size_t qk0, v0;   // float offsets of (b, row 0, head h) in the [B, T, H*dk] and [B, T, H*dv] tensors
  size_t rk, rv;    // row strides H*dk, H*dv
  int nch, njv;     // 16-float chunks of dk, dv
  int ld, ldv;      // LDS row strides
};
__device__ __forceinline__ Where where(const Args& p) {
  Where x;
  const int nb = (p.T + kBlock - 1) / kBlock;
  x.blk = blockIdx.x % nb;
  const int bh = blockIdx.x / nb;
  x.h = bh % p.H;
  x.b = bh / p.H;
  const int lane = threadIdx.x & 63;
  x.w = threadIdx.x >> 6; x.fr = lane & 15; x.fq = lane >> 4;
  x.rk = (size_t)p.H * p.dk_; x.rv = (size_t)p.H * p.dv_;
  x.qk0 = (size_t)x.b * p.T * x.rk + (size_t)x.h * p.dk_;
  x.v0 = (size_t)x.b * p.T * x.rv + (size_t)x.h * p.dv_;
  x.nch = (p.dk_ + 15) >> 4; x.njv = (p.dv_ + 15) >> 4;
  x.ld = 16 * x.nch + 4; x.ldv = 16 * x.njv + 4;
  return x;
}

// rows row0 .. row0+63 of one head into an LDS tile [64][ld]: 16-byte loads along d, zeros past T and past d
__device__ __forceinline__ void stage_rows(float* dst, int ld, const float* src, size_t rs, int row0, int T, int d,
                                           float scale) {
  const int nq = (ld - 4) >> 2;
  for (int i = threadIdx.x; i < kBlock * nq; i += kThreads) {
    const int r = i / nq, c = (i - r * nq) << 2;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (row0 + r < T && c < d) v = *reinterpret_cast<const f32x4*>(src + (size_t)(row0 + r) * rs + c) * scale;
    *reinterpret_cast<f32x4*>(dst + r * ld + c) = v;
  }
}

// the lane's four float4s of row `row` (columns 16 ch + 4 fq): an MFMA B operand held in registers
__device__ __forceinline__ void load_row(f32x4 (&reg)[4], const float* src, size_t rs, int row, int T, int d, int fq,
                                         float scale) {
#pragma unroll
  for (int ch = 0; ch < 4; ++ch) {
    const int c = 16 * ch + 4 * fq;
    reg[ch] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (row < T && c < d) reg[ch] = *reinterpret_cast<const f32x4*>(src + (size_t)row * rs + c) * scale;
  }
}

// acc (+)= A^T-tile . B: the 16 rows 16 t .. of an LDS tile as A operand against a register row operand
__device__ __forceinline__ f32x4 rows_times_reg(const float* tile, int ld, int t, int nch, const f32x4 (&reg)[4],
                                                int fr, int fq) {
  f32x4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ch = 0; ch < 4; ++ch)
    if (ch < nch) a = mfma_chunk(*reinterpret_cast<const f32x4*>(tile + (16 * t + fr) * ld + 16 * ch + 4 * fq), reg[ch], a);
  return a;
}

// acc[j] += tile^T . x: the tile's rows 16 t + 4 fq + r (k) by its columns 16 j + fr (m) against the four
// accumulator registers x[r] of a 16 x 16 tile (k = 4 fq + r, n = fr)
__device__ __forceinline__ void cols_times_acc(f32x4 (&acc)[4], const float* tile, int ld, int t, int nj, const f32x4 x,
                                               int fr, int fq) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float* row = tile + (16 * t + 4 * fq + r) * ld + fr;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < nj) acc[j] = mfma4(row[16 * j], x[r], acc[j]);
  }
}

// the lane's four consecutive floats of row `row`, columns 16 j + 4 fq, for every chunk: 16-byte stores
__device__ __forceinline__ void store_row(float* dst, size_t rs, int row, int d, const f32x4 (&acc)[4], int fq, float mul,
                                          int accum) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = 16 * j + 4 * fq;
    if (c < d) {
      f32x4* out = reinterpret_cast<f32x4*>(dst + (size_t)row * rs + c);
      f32x4 v = acc[j] * mul;
      if (accum) v += *out;
      *out = v;
    }
  }
}

// ---------------------------------------------------------------------------------------------- forward
template <int NKB>
__global__ __launch_bounds__(kThreads) void mha_fwd_kernel(const Args p) {
  __shared__ __attribute__((aligned(16))) float tile[kTile];
  const Where x = where(p);
  const int T = p.T, q = x.blk * kBlock + 16 * x.w + x.fr;
  f32x4 qreg[4];
  load_row(qreg, p.q + x.qk0, x.rk, q, T, p.dk_, x.fq, p.scale);

  f32x4 s[4 * NKB];   // S^T: s[t][r] = S[q][key 16 t + 4 fq + r]
#pragma unroll
  for (int kb = 0; kb < NKB; ++kb) {
    stage_rows(tile, x.ld, p.k + x.qk0, x.rk, kb * kBlock, T, p.dk_, 1.f);
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 4; ++t) s[4 * kb + t] = rows_times_reg(tile, x.ld, t, x.nch, qreg, x.fr, x.fq);
    __syncthreads();
  }

  float m = -INFINITY;
#pragma unroll
  for (int t = 0; t < 4 * NKB; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (16 * t + 4 * x.fq + r >= T) s[t][r] = -INFINITY;
      m = fmaxf(m, s[t][r]);
    }
  m = fmaxf(m, __shfl_xor(m, 16, 64));
  m = fmaxf(m, __shfl_xor(m, 32, 64));   // key 0 is never masked: m is finite
  float l = 0.f;
#pragma unroll
  for (int t = 0; t < 4 * NKB; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      s[t][r] = expf(s[t][r] - m);
      l += s[t][r];
    }
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);

  f32x4 o[4] = {};   // O^T: o[j][r] = O[q][16 j + 4 fq + r]
#pragma unroll
  for (int kb = 0; kb < NKB; ++kb) {
    stage_rows(tile, x.ldv, p.v + x.v0, x.rv, kb * kBlock, T, p.dv_, 1.f);
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 4; ++t) cols_times_acc(o, tile, x.ldv, t, x.njv, s[4 * kb + t], x.fr, x.fq);
    __syncthreads();
  }
  if (q < T) {
    store_row(p.out + x.v0, x.rv, q, p.dv_, o, x.fq, 1.f / l, 0);
    if (x.fq == 0) p.lse[((size_t)x.b * p.H + x.h) * T + q] = m + logf(l);
  }
}

// ---------------------------------------------------------------------------------------------- backward: dK, dV
__global__ __launch_bounds__(kThreads) void mha_bwd_kv_kernel(const Args p) {
  __shared__ __attribute__((aligned(16))) float qs[kTile];
  __shared__ __attribute__((aligned(16))) float ds[kTile];
  __shared__ __attribute__((aligned(16))) float lses[kBlock];
  __shared__ __attribute__((aligned(16))) float dls[kBlock];
  const Where x = where(p);
  const int T = p.T, key = x.blk * kBlock + 16 * x.w + x.fr;
  f32x4 kreg[4], vreg[4];
  load_row(kreg, p.k + x.qk0, x.rk, key, T, p.dk_, x.fq, 1.f);
  load_row(vreg, p.v + x.v0, x.rv, key, T, p.dv_, x.fq, 1.f);
  f32x4 dka[4] = {}, dva[4] = {};   // dK^T, dV^T: [j][r] = d(K|V)[key][16 j + 4 fq + r]
  const float* lse = p.lse + ((size_t)x.b * p.H + x.h) * T;
  const int nqv = (x.ldv - 4) >> 2;

  for (int q0 = 0; q0 < T; q0 += kBlock) {
    __syncthreads();   // the previous block's tiles have been read
    stage_rows(qs, x.ld, p.q + x.qk0, x.rk, q0, T, p.dk_, p.scale);
    {   // dO into LDS, delta on the way: four lanes per row, each over every fourth float4
      const int r = threadIdx.x >> 2, part = threadIdx.x & 3, row = q0 + r;
      float sum = 0.f;
      for (int qd = part; qd < nqv; qd += 4) {
        const int c = qd << 2;
        f32x4 g = {0.f, 0.f, 0.f, 0.f};
        if (row < T && c < p.dv_) {
          const size_t at = x.v0 + (size_t)row * x.rv + c;
          g = *reinterpret_cast<const f32x4*>(p.d_o + at);
          sum += dot4(g, *reinterpret_cast<const f32x4*>(p.o + at));
        }
        *reinterpret_cast<f32x4*>(ds + r * x.ldv + c) = g;
      }
      sum += __shfl_xor(sum, 1, 64);
      sum += __shfl_xor(sum, 2, 64);
      if (part == 0) {
        dls[r] = sum;
        lses[r] = row < T ? lse[row] : INFINITY;   // rows past T: P = exp(0 - inf) = 0
      }
    }
    __syncthreads();
#pragma unroll 1
    for (int t = 0; t < 4; ++t) {
      if (q0 + 16 * t >= T) break;   // whole tiles of rows past T add nothing (block-uniform)
      // pr[r] = P[q0 + 16 t + 4 fq + r][key], then dS in its place
      f32x4 pr = rows_times_reg(qs, x.ld, t, x.nch, kreg, x.fr, x.fq);
      f32x4 dp = rows_times_reg(ds, x.ldv, t, x.njv, vreg, x.fr, x.fq);
      const f32x4 ls = *reinterpret_cast<const f32x4*>(lses + 16 * t + 4 * x.fq);
      const f32x4 dl = *reinterpret_cast<const f32x4*>(dls + 16 * t + 4 * x.fq);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        pr[r] = expf(pr[r] - ls[r]);
        dp[r] = pr[r] * (dp[r] - dl[r]);
      }
      cols_times_acc(dva, ds, x.ldv, t, x.njv, pr, x.fr, x.fq);
      cols_times_acc(dka, qs, x.ld, t, x.nch, dp, x.fr, x.fq);
    }
  }
  if (key < T) {   // the Q tile was staged scaled: dK = dS^T (Q / sqrt(dk))
    store_row(p.dk + x.qk0, x.rk, key, p.dk_, dka, x.fq, 1.f, 0);
    store_row(p.dv + x.v0, x.rv, key, p.dv_, dva, x.fq, 1.f, 0);
  }
}

// ---------------------------------------------------------------------------------------------- backward: dQ
__global__ __launch_bounds__(kThreads) void mha_bwd_q_kernel(const Args p) {
  __shared__ __attribute__((aligned(16))) float ks[kTile];
  __shared__ __attribute__((aligned(16))) float vs[kTile];
  const Where x = where(p);
  const int T = p.T, q = x.blk * kBlock + 16 * x.w + x.fr;
  f32x4 qreg[4], greg[4], oreg[4];
  load_row(qreg, p.q + x.qk0, x.rk, q, T, p.dk_, x.fq, p.scale);
  load_row(greg, p.d_o + x.v0, x.rv, q, T, p.dv_, x.fq, 1.f);
  load_row(oreg, p.o + x.v0, x.rv, q, T, p.dv_, x.fq, 1.f);
  float delta = (dot4(greg[0], oreg[0]) + dot4(greg[1], oreg[1])) + (dot4(greg[2], oreg[2]) + dot4(greg[3], oreg[3]));
  delta += __shfl_xor(delta, 16, 64);
  delta += __shfl_xor(delta, 32, 64);
  const float ls = q < T ? p.lse[((size_t)x.b * p.H + x.h) * T + q] : INFINITY;
  f32x4 dqa[4] = {};   // dQ^T: [j][r] = dQ[q][16 j + 4 fq + r]

  for (int k0 = 0; k0 < T; k0 += kBlock) {
    __syncthreads();
    stage_rows(ks, x.ld, p.k + x.qk0, x.rk, k0, T, p.dk_, 1.f);
    stage_rows(vs, x.ldv, p.v + x.v0, x.rv, k0, T, p.dv_, 1.f);
    __syncthreads();
#pragma unroll 1
    for (int t = 0; t < 4; ++t) {
      if (k0 + 16 * t >= T) break;
      f32x4 pr = rows_times_reg(ks, x.ld, t, x.nch, qreg, x.fr, x.fq);    // S^T[key 16 t + 4 fq + r][q]
      f32x4 dp = rows_times_reg(vs, x.ldv, t, x.njv, greg, x.fr, x.fq);   // dP^T
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float pe = k0 + 16 * t + 4 * x.fq + r < T ? expf(pr[r] - ls) : 0.f;
        dp[r] = pe * (dp[r] - delta);
      }
      cols_times_acc(dqa, ks, x.ld, t, x.nch, dp, x.fr, x.fq);
    }
  }
  if (q < T) store_row(p.dq + x.qk0, x.rk, q, p.dk_, dqa, x.fq, p.scale, p.accum);
}

static bool geo_ok(int B, int H, int T, int dk, int dv) {
  if (B < 1 || H < 1 || T < 1 || T > kMaxT) return false;
  if (dk < 4 || dk > kMaxD || dk % 4 || dv < 4 || dv > kMaxD || dv % 4) return false;
  const long long wgs = (long long)B * H * ((T + kBlock - 1) / kBlock);
  return wgs < (1LL << 31) && (long long)B * T * H * kMaxD < (1LL << 40);
}
static bool aligned16(std::initializer_list<const void*> ptrs) {
  for (const void* q : ptrs)
    if (!q || (reinterpret_cast<uintptr_t>(q) & 15)) return false;
  return true;
}

}  // namespace mha
}  // namespace tde

using namespace tde::mha;

// O [B,T,H*dv] = softmax(Q K^T / sqrt(dk)) V per (sample, head); lse [B,H,T] is saved for the backward.
TDE_API int tde_mha32_fwd(const float* q, const float* k, const float* v, float* o, float* lse, int B, int H, int T,
                          int dk, int dv, hipStream_t stream) {
  if (!lse || !geo_ok(B, H, T, dk, dv)) return -1;
  if (!aligned16({q, k, v, o})) return -2;
  Args a = {};
  a.q = q; a.k = k; a.v = v; a.out = o; a.lse = lse;
  a.B = B; a.H = H; a.T = T; a.dk_ = dk; a.dv_ = dv; a.scale = 1.f / sqrtf((float)dk);
  const int nb = (T + kBlock - 1) / kBlock;
  const dim3 grid((unsigned)((long long)B * H * nb));
  switch (nb) {
    case 1: mha_fwd_kernel<1><<<grid, kThreads, 0, stream>>>(a); break;
    case 2: mha_fwd_kernel<2><<<grid, kThreads, 0, stream>>>(a); break;
    case 3: mha_fwd_kernel<3><<<grid, kThreads, 0, stream>>>(a); break;
    default: mha_fwd_kernel<4><<<grid, kThreads, 0, stream>>>(a); break;
  }
  TDE_LAUNCH_CHECK();
  return 0;
}

// dQ (+)= , dK = , dV = from dO, the forward's operands, its O and its lse.
TDE_API int tde_mha32_bwd(const float* q, const float* k, const float* v, const float* o, const float* lse,
                          const float* d_o, float* dq, int accum, float* dk_out, float* dv_out, int B, int H, int T,
                          int dk, int dv, hipStream_t stream) {
  if (!lse || !geo_ok(B, H, T, dk, dv)) return -1;
  if (!aligned16({q, k, v, o, d_o, dq, dk_out, dv_out})) return -2;
  Args a = {};
  a.q = q; a.k = k; a.v = v; a.o = o; a.d_o = d_o; a.lse = const_cast<float*>(lse);
  a.dq = dq; a.dk = dk_out; a.dv = dv_out; a.accum = accum;
  a.B = B; a.H = H; a.T = T; a.dk_ = dk; a.dv_ = dv; a.scale = 1.f / sqrtf((float)dk);
  const dim3 grid((unsigned)((long long)B * H * ((T + kBlock - 1) / kBlock)));
  mha_bwd_kv_kernel<<<grid, kThreads, 0, stream>>>(a);
  TDE_LAUNCH_CHECK();
  mha_bwd_q_kernel<<<grid, kThreads, 0, stream>>>(a);
  TDE_LAUNCH_CHECK();
  return 0;
}
