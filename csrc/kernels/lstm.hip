// LSTM recurrence, float32 on v_mfma_f32_16x16x4_f32: a forward and a backward sweep over all T time steps in ONE
// launch each.  A workgroup stays resident for the whole sequence, its slice of the recurrent matrix U in registers
// and the state on chip; the input projection Z = x W + b and the weight gradient dU = hprev^T dZ are ordinary GEMMs
// over the N*T tokens and run outside (layers_f32.hip).
//
// Operands: Z, gates, dZ [N, T, 4u] (Keras's gate order i, f, c, o along the last axis), U [u, 4u], hseq, hprev, cseq
// [N, T, u], hlast [N, u]; u a multiple of 16 from 16 to 128, any N and T.  With a_t = Z_t + h_{t-1} U:
//   i, f, o = sigmoid(a_i), sigmoid(a_f), sigmoid(a_o);  g = tanh(a_c);  c_t = f c_{t-1} + i g;  h_t = o tanh(c_t)
//   dh = dh_t + dZ_{t+1} U^T;  do = dh tanh(c_t) o (1 - o);  dc += dh o (1 - tanh(c_t)^2);  di = dc g i (1 - i);
//   dg = dc i (1 - g^2);  df = dc c_{t-1} f (1 - f);  dc <- dc f                       (dZ_t = [di, df, dg, do])
//
// The MFMA: a lane (fr = lane % 16, fq = lane / 16) gives A[m = fr][k = fq] and B[k = fq][n = fr] and gets
// D[m = 4 fq + r][n = fr] in register r.  One workgroup owns 16 batch rows (the MFMA's M; rows past N compute on
// row N - 1's operands and store nothing) and runs u / 16 waves; wave w owns hidden units 16 w .. 16 w + 15.
//
// * Forward: the wave's four accumulator tiles are the i, f, g, o columns of ITS units, so one lane holds all four
//   gates of the same (row 4 fq + r, unit 16 w + fr) in matching registers: the gate math, c (4 VGPRs, never
//   stored but to cseq) and h are lane-local.  The wave's [u x 64] slice of U is loaded once and held as B
//   operands, u VGPRs.  h_{t-1} is all that crosses waves: each wave writes its 16 x 16 tile of h_t into a
//   double-buffered 16 x u LDS image and every wave reads the image back as its A operand, ONE barrier per step
//   (step t reads buffer t % 2 and writes the other; a buffer is rewritten two steps later, a barrier after its
//   last reader).  The image is read with 16-byte loads: lane group fq takes k = 4 fq .. 4 fq + 3 of each 16-float
//   chunk and U's registers are ordered to match (a sum over k has no order).  Z_{t+1} does not depend on the
//   recurrence: it is loaded one step ahead, straight into the accumulators' initial value.
// * Backward, t = T-1 .. 0: dc and the recurrent dh are the lane's registers, tanh(c_t) is recomputed.  dZ_t is
//   stored to HBM (the GEMM stage's output gradient) and written into a double-buffered 16 x 4u LDS image, the A
//   operand of dh_{t-1} = dZ_t U^T (K = 4u, N = the wave's 16 units): the B operands are 16-byte pieces of the
//   wave's ROWS of U, again u VGPRs.  The image's K order is unit-major, gate-minor, so a lane writes the four gate
//   gradients of a (row, unit) with one 16-byte store.  It is not padded (2 x 32 KiB at u = 128) but swizzled: the
//   16-byte column index is XORed with the row, which spreads both the writes and the reads over all banks.
//   The gate activations, c_{t-1} and the upstream dh_t of step t - 1 are loaded while step t computes.
//   One writer per element, no atomics: bitwise reproducible.
// * sigmoid and tanh run on v_exp_f32 / v_rcp_f32 with log2(e) folded into the argument.
// * Bidirectional (the BI instantiations, grid (ceil(N / 16), 2)): blockIdx.y is the direction and picks its
//   operand set; a direction's workgroups are the ones above.  Time order belongs to the direction: in the forward
//   sweep direction 0 walks t = 0 .. T-1 and direction 1 walks t = T-1 .. 0, in the backward sweep each walks the
//   other way, and everything that says "first", "last" or "next" (the prefetches, the zero state, the LDS parity)
//   counts STEPS s (up from 0 in the forward sweep, down to 0 in the backward sweep), not t.  hprev of direction 1 at position t is therefore h of position t + 1, zeros
//   at T-1.  h goes straight into the direction's half of the layer's output ([N, T, 2u], row stride 2u, column
//   offset d u, original time order; or the final states into [N, 2u]) and the upstream dh is read from the same
//   halves: no reverse, concat or split exists.  The unidirectional instantiations are BI = false: one direction,
//   s = t, every stride a compile-time u.
#include "tde_common.h"

#include <cstdint>

namespace tde {
namespace lstm {

constexpr int kRows = 16;              // batch rows per workgroup
constexpr int kMinU = 16, kMaxU = 128;
constexpr float kLog2e = 1.4426950408889634f;

// One direction's operands.  BI: hseq, hlast and dh point at the direction's column d u of a row that is 2u wide
// (hseq: hld wide, u for a dense tensor of its own) and hseq may be null.
struct FwdDir {
  const float* z; const float* u;
  float* hseq; float* hprev; float* gates; float* cseq;
  float* hlast;     // [N, u] or null
};
template <bool BI>
struct FwdArgs {
  FwdDir d[BI ? 2 : 1];
  int N, T, hld;
};
struct BwdDir {
  const float* gates; const float* cseq; const float* u;
  const float* dh;  // [N, T, u], or [N, u] with last_only
  float* dz;
};
template <bool BI>
struct BwdArgs {
  BwdDir d[BI ? 2 : 1];
  int N, T, last_only;
};

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
// exp2 overflows to inf and 1 / inf = 0: both saturate to their limits without a branch
__device__ __forceinline__ float sigmoid_(float x) {
  return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-kLog2e * x));
}
__device__ __forceinline__ float tanh_(float x) {
  return 1.f - 2.f * __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f((2.f * kLog2e) * x));
}

// The lane's four rows 4 fq + r of the workgroup's 16: 32-bit byte offsets of (row, step 0, column col) from the
// workgroup's first row in a [N, T, width] tensor, so an access is a uniform base (which carries the step), one
// VGPR and an immediate (the gate).  Rows past N are clamped to row N - 1 for the loads (finite values that nothing
// stores) and masked for the stores.
struct Rows {
  unsigned off[4];
  bool ok[4];
};
__device__ __forceinline__ Rows rows_of(int fq, int N, int T, int width, int col) {
  Rows x;
  const int first = blockIdx.x * kRows;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = first + 4 * fq + r;
    x.ok[r] = row < N;
    x.off[r] = 4u * (unsigned)((min(row, N - 1) - first) * T * width + col);
  }
  return x;
}
// the workgroup's first row at step t
__device__ __forceinline__ const float* at(const float* p, int T, int width, int t) {
  return p + ((size_t)blockIdx.x * kRows * T + t) * width;
}
__device__ __forceinline__ float* at(float* p, int T, int width, int t) {
  return p + ((size_t)blockIdx.x * kRows * T + t) * width;
}
__device__ __forceinline__ float& elem(float* base, unsigned off) {
  return *reinterpret_cast<float*>(reinterpret_cast<char*>(base) + off);
}
__device__ __forceinline__ f32x4 load_rows(const float* base, const Rows& x) {
  f32x4 v;
#pragma unroll
  for (int r = 0; r < 4; ++r) v[r] = elem(const_cast<float*>(base), x.off[r]);
  return v;
}

// ---------------------------------------------------------------------------------------------- forward
template <int NCH, bool BI>   // NCH = u / 16: waves per workgroup and 16-float chunks of K
__global__ __launch_bounds__(64 * NCH) void lstm_fwd_kernel(const FwdArgs<BI> p) {
  constexpr int U = 16 * NCH, LD = U + 4, W4 = 4 * U, HL = BI ? 2 * U : U;
  __shared__ __attribute__((aligned(16))) float himg[2][kRows * LD];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, fr = lane & 15, fq = lane >> 4;
  const int col = 16 * w + fr, N = p.N, T = p.T;
  const bool rev = BI && blockIdx.y;   // direction 1 walks t = T-1 .. 0
  const FwdDir q = rev ? p.d[BI] : p.d[0];
  const int dt = rev ? -1 : 1, hld = BI ? p.hld : U;
  const Rows x4 = rows_of(fq, N, T, W4, col), x1 = rows_of(fq, N, T, U, col), xh = rows_of(fq, N, T, hld, col);

  float ub[NCH][4][4];   // [chunk][k = 16 ch + 4 fq + j][gate]: B[k][n = fr]
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int g = 0; g < 4; ++g) ub[ch][j][g] = q.u[(16 * ch + 4 * fq + j) * W4 + g * U + col];

  f32x4 zn[4];   // Z of the coming step, gate by gate
#pragma unroll
  for (int g = 0; g < 4; ++g) zn[g] = load_rows(at(q.z, T, W4, rev ? T - 1 : 0) + g * U, x4);
  f32x4 c = {0.f, 0.f, 0.f, 0.f}, h = c;

#pragma unroll 1
  for (int s = 0, t = rev ? T - 1 : 0; s < T; ++s, t += dt) {   // step s works on position t
    const bool more = s + 1 < T;
    f32x4 acc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g] = zn[g];
    if (more) {
      const float* zt = at(q.z, T, W4, t + dt);
#pragma unroll
      for (int g = 0; g < 4; ++g) zn[g] = load_rows(zt + g * U, x4);
    }
    {   // hprev of this step: h of the step before, zeros at s = 0
      float* hp = at(q.hprev, T, U, t);
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (x1.ok[r]) elem(hp, x1.off[r]) = h[r];
    }
    if (s > 0) {   // from a zero state
      const float* hb = himg[s & 1] + fr * LD + 4 * fq;
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(hb + 16 * ch);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int g = 0; g < 4; ++g) acc[g] = mfma4(a[j], ub[ch][j][g], acc[g]);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float ig = sigmoid_(acc[0][r]), fg = sigmoid_(acc[1][r]), gg = tanh_(acc[2][r]), og = sigmoid_(acc[3][r]);
      c[r] = fg * c[r] + ig * gg;
      h[r] = og * tanh_(c[r]);
      acc[0][r] = ig; acc[1][r] = fg; acc[2][r] = gg; acc[3][r] = og;
    }
    if (more) {
      float* hw = himg[(s + 1) & 1] + 4 * fq * LD + col;
#pragma unroll
      for (int r = 0; r < 4; ++r) hw[r * LD] = h[r];
    }
    float* gt = at(q.gates, T, W4, t);
    float* ct = at(q.cseq, T, U, t);
    float* ht = at(q.hseq, T, hld, t);
    const bool hs = !BI || q.hseq;
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (x1.ok[r]) {
#pragma unroll
        for (int g = 0; g < 4; ++g) elem(gt + g * U, x4.off[r]) = acc[g][r];
        elem(ct, x1.off[r]) = c[r];
        if (hs) elem(ht, xh.off[r]) = h[r];
      }
    if (more) lds_barrier();
  }
  if (q.hlast) {
    const int first = blockIdx.x * kRows + 4 * fq;
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (x1.ok[r]) q.hlast[(size_t)(first + r) * HL + col] = h[r];
  }
}

// ---------------------------------------------------------------------------------------------- backward
// float offset of (row, 16-byte column c4) in a swizzled [16][K] image
__device__ __forceinline__ int swz(int row, int c4, int K) { return row * K + ((c4 ^ row) << 2); }

template <int NCH, bool BI>
__global__ __launch_bounds__(64 * NCH) void lstm_bwd_kernel(const BwdArgs<BI> p) {
  constexpr int U = 16 * NCH, K = 4 * U, DH = BI ? 2 * U : U;   // DH: the row of the upstream dh
  extern __shared__ __attribute__((aligned(16))) float dimg[];   // [2][16][K]
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, fr = lane & 15, fq = lane >> 4;
  const int col = 16 * w + fr, N = p.N, T = p.T;
  const bool up_ = BI && blockIdx.y;   // direction 1's backward walks t = 0 .. T-1
  const BwdDir q = up_ ? p.d[BI] : p.d[0];
  const int dt = up_ ? 1 : -1, t0 = up_ ? 0 : T - 1;
  const Rows x4 = rows_of(fq, N, T, K, col), x1 = rows_of(fq, N, T, U, col), xd = rows_of(fq, N, T, DH, col);

  // the image's K order is unit-major, gate-minor (k = 4 unit + gate): a lane's di, df, dg, do of one (row, unit)
  // are one 16-byte write, and lane group fq reads unit 4 ch + fq of chunk ch, gate j for the j-th MFMA
  f32x4 ub[4 * NCH];   // [chunk][gate j]: B[k][n = fr] = U[16 w + fr][j u + 4 ch + fq]
#pragma unroll
  for (int ch = 0; ch < 4 * NCH; ++ch)
#pragma unroll
    for (int j = 0; j < 4; ++j) ub[ch][j] = q.u[col * K + j * U + 4 * ch + fq];

  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  const int seq = !p.last_only;
  // the operands of the coming step: the four activations, the c of the position the forward came from (t + dt)
  // and the upstream dh_t
  f32x4 gn[4], cpn = zero, upn;
#pragma unroll
  for (int g = 0; g < 4; ++g) gn[g] = load_rows(at(q.gates, T, K, t0) + g * U, x4);
  if (T > 1) cpn = load_rows(at(q.cseq, T, U, t0 + dt), x1);
  if (seq) {
    upn = load_rows(at(q.dh, T, DH, t0), xd);
  } else {   // [N, DH]: the rows_of of a one-step tensor
    upn = load_rows(at(q.dh, 1, DH, 0), rows_of(fq, N, 1, DH, col));
  }
  f32x4 cc = load_rows(at(q.cseq, T, U, t0), x1);   // c_t
  f32x4 dc = zero, dhr = zero;

#pragma unroll 1
  for (int s = T - 1; s >= 0; --s) {   // s steps remain after this one, which works on position t
    const int t = up_ ? T - 1 - s : s;
    const bool more = s > 0;
    f32x4 ga[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) ga[g] = gn[g];
    const f32x4 cp = cpn, up = upn;
    if (more) {
      const float* gt = at(q.gates, T, K, t + dt);
#pragma unroll
      for (int g = 0; g < 4; ++g) gn[g] = load_rows(gt + g * U, x4);
      cpn = s > 1 ? load_rows(at(q.cseq, T, U, t + 2 * dt), x1) : zero;
      upn = seq ? load_rows(at(q.dh, T, DH, t + dt), xd) : zero;
    }
    f32x4 dzv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float ig = ga[0][r], fg = ga[1][r], gg = ga[2][r], og = ga[3][r];
      const float dh = dhr[r] + up[r], tc = tanh_(cc[r]);
      dzv[3][r] = dh * tc * (og * (1.f - og));
      dc[r] += dh * og * (1.f - tc * tc);
      dzv[0][r] = dc[r] * gg * (ig * (1.f - ig));
      dzv[1][r] = dc[r] * cp[r] * (fg * (1.f - fg));
      dzv[2][r] = dc[r] * ig * (1.f - gg * gg);
      dc[r] *= fg;
    }
    cc = cp;
    float* img = dimg + (s & 1) * (kRows * K);
    if (more) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        *reinterpret_cast<f32x4*>(img + swz(4 * fq + r, col, K)) = f32x4{dzv[0][r], dzv[1][r], dzv[2][r], dzv[3][r]};
    }
    float* dzt = at(q.dz, T, K, t);
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (x1.ok[r]) {
#pragma unroll
        for (int g = 0; g < 4; ++g) elem(dzt + g * U, x4.off[r]) = dzv[g][r];
      }
    if (!more) break;
    lds_barrier();
    f32x4 acc[4] = {zero, zero, zero, zero};   // four independent chains, summed in a fixed order
#pragma unroll
    for (int ch = 0; ch < 4 * NCH; ++ch) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(img + swz(fr, 4 * ch + fq, K));
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = mfma4(a[j], ub[ch][j], acc[j]);
    }
    dhr = (acc[0] + acc[1]) + (acc[2] + acc[3]);
  }
}

// hrow: the widest row that holds h or dh (u, or 2u for the bidirectional output); the gates' row is 4u
static bool geo_ok(int N, int T, int units, int hrow) {
  if (N < 1 || T < 1 || units < kMinU || units > kMaxU || units % 16) return false;
  const int row = hrow > 4 * units ? hrow : 4 * units;
  return (long long)kRows * T * row * 4 < (1LL << 32);   // a workgroup's rows by 32-bit byte offsets
}

}  // namespace lstm
}  // namespace tde

using namespace tde::lstm;

#define TDE_LSTM_DISPATCH(LAUNCH) \
  switch (units / 16) {           \
    case 1: LAUNCH(1); break;     \
    case 2: LAUNCH(2); break;     \
    case 3: LAUNCH(3); break;     \
    case 4: LAUNCH(4); break;     \
    case 5: LAUNCH(5); break;     \
    case 6: LAUNCH(6); break;     \
    case 7: LAUNCH(7); break;     \
    default: LAUNCH(8); break;    \
  }

template <bool BI>
static void launch_fwd(const FwdArgs<BI>& a, int units, hipStream_t stream) {
  const dim3 grid((unsigned)((a.N + kRows - 1) / kRows), BI ? 2 : 1);
#define TDE_LSTM_FWD(n) lstm_fwd_kernel<n, BI><<<grid, 64 * n, 0, stream>>>(a)
  TDE_LSTM_DISPATCH(TDE_LSTM_FWD)
#undef TDE_LSTM_FWD
}

template <bool BI>
static void launch_bwd(const BwdArgs<BI>& a, int units, hipStream_t stream) {
  const dim3 grid((unsigned)((a.N + kRows - 1) / kRows), BI ? 2 : 1);
  const int lds = 2 * kRows * 4 * units * (int)sizeof(float);   // 64 KiB at the upper end
  static bool attr_set = false;   // one per instantiation of this function
  if (!attr_set) {
#define TDE_LSTM_ATTR(n) \
  (void)hipFuncSetAttribute((const void*)lstm_bwd_kernel<n, BI>, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * kRows * 64 * n * 4)
    TDE_LSTM_ATTR(1); TDE_LSTM_ATTR(2); TDE_LSTM_ATTR(3); TDE_LSTM_ATTR(4);
    TDE_LSTM_ATTR(5); TDE_LSTM_ATTR(6); TDE_LSTM_ATTR(7); TDE_LSTM_ATTR(8);
#undef TDE_LSTM_ATTR
    attr_set = true;
  }
#define TDE_LSTM_BWD(n) lstm_bwd_kernel<n, BI><<<grid, 64 * n, lds, stream>>>(a)
  TDE_LSTM_DISPATCH(TDE_LSTM_BWD)
#undef TDE_LSTM_BWD
}

// hseq, hprev, gates, cseq (and hlast [N, units] unless null) from Z = x W + b [N, T, 4 units] and U [units, 4 units]
TDE_API int tde_lstm32_fwd(const float* z, const float* u, float* hseq, float* hprev, float* gates, float* cseq,
                           float* hlast, int N, int T, int units, hipStream_t stream) {
  if (!geo_ok(N, T, units, units)) return -1;
  if (!z || !u || !hseq || !hprev || !gates || !cseq) return -2;
  const FwdArgs<false> a = {{{z, u, hseq, hprev, gates, cseq, hlast}}, N, T, units};
  launch_fwd(a, units, stream);
  TDE_LAUNCH_CHECK();
  return 0;
}

// dZ [N, T, 4 units] from the forward's activations and cell states and the upstream dh ([N, T, units], or
// [N, units] for the last step only with last_only)
TDE_API int tde_lstm32_bwd(const float* gates, const float* cseq, const float* u, const float* dh, float* dz, int N,
                           int T, int units, int last_only, hipStream_t stream) {
  if (!geo_ok(N, T, units, units)) return -1;
  if (!gates || !cseq || !u || !dh || !dz) return -2;
  const BwdArgs<false> a = {{{gates, cseq, u, dh, dz}}, N, T, last_only};
  launch_bwd(a, units, stream);
  TDE_LAUNCH_CHECK();
  return 0;
}

// Both directions of a bidirectional layer in one launch.  Direction d (0: forward in time, 1: backward in time)
// has its own Z_d, U_d and saved tensors hprev_d, gates_d, cseq_d.  seq: every h into out [N, T, 2 units], columns
// d units .. of position t in the original time order (hseq_d unused).  Otherwise: the directions' final states into
// out [N, 2 units], and every h into hseq_d [N, T, units] unless null.
TDE_API int tde_lstm32_bi_fwd(const float* z0, const float* z1, const float* u0, const float* u1, float* hseq0,
                              float* hseq1, float* hprev0, float* hprev1, float* gates0, float* gates1, float* cseq0,
                              float* cseq1, float* out, int N, int T, int units, int seq, hipStream_t stream) {
  if (!geo_ok(N, T, units, 2 * units)) return -1;
  if (!z0 || !z1 || !u0 || !u1 || !hprev0 || !hprev1 || !gates0 || !gates1 || !cseq0 || !cseq1 || !out) return -2;
  const FwdArgs<true> a = {{{z0, u0, seq ? out : hseq0, hprev0, gates0, cseq0, seq ? nullptr : out},
                            {z1, u1, seq ? out + units : hseq1, hprev1, gates1, cseq1, seq ? nullptr : out + units}},
                           N, T, seq ? 2 * units : units};
  launch_fwd(a, units, stream);
  TDE_LAUNCH_CHECK();
  return 0;
}

// dZ_d [N, T, 4 units] of both directions from the upstream dh [N, T, 2 units] (or [N, 2 units] with last_only: the
// gradient of the final states), direction d reading columns d units ..
TDE_API int tde_lstm32_bi_bwd(const float* gates0, const float* gates1, const float* cseq0, const float* cseq1,
                              const float* u0, const float* u1, const float* dh, float* dz0, float* dz1, int N, int T,
                              int units, int last_only, hipStream_t stream) {
  if (!geo_ok(N, T, units, 2 * units)) return -1;
  if (!gates0 || !gates1 || !cseq0 || !cseq1 || !u0 || !u1 || !dh || !dz0 || !dz1) return -2;
  const BwdArgs<true> a = {{{gates0, cseq0, u0, dh, dz0}, {gates1, cseq1, u1, dh + units, dz1}}, N, T, last_only};
  launch_bwd(a, units, stream);
  TDE_LAUNCH_CHECK();
  return 0;
}
