// GRU recurrence (Keras's reset_after form), float32 on v_mfma_f32_16x16x4_f32: a forward and a backward sweep over
// all T time steps in ONE launch each.  A workgroup stays resident for the whole sequence, its slice of the recurrent
// matrix U in registers and the state on chip; the input projection X = x W + b[0], the weight gradient
// dU = hprev^T dR and the recurrent bias gradient (the column sum of dR) are ordinary launches over the N*T tokens
// and run outside (layers_f32.hip).  The decomposition, the row addressing and the transcendental forms are those
// of lstm.hip; what differs is said below.
//
// Operands: X, dX, dR [N, T, 3u] (Keras's gate order z, r, h along the last axis), U [u, 3u], the recurrent bias
// rb [3u] (row 1 of gru_cell/bias; null = none), acts [N, T, 4u] in the order z, r, hh, R_h, hseq, hprev [N, T, u],
// hlast [N, u]; u a multiple of 16 from 16 to 128, any N and T.  With R_t = h_{t-1} U + rb:
//   z = sigmoid(X_z + R_z);  r = sigmoid(X_r + R_r);  hh = tanh(X_h + r R_h);  h_t = z h_{t-1} + (1 - z) hh
//   dh = dh_t + dhr;  da = dh (1 - z) (1 - hh^2);  dXz = dh (h_{t-1} - hh) z (1 - z);  dXr = da R_h r (1 - r)
//   dX_t = [dXz, dXr, da];  dR_t = [dXz, dXr, da r];  dhr <- dh z + dR_t U^T
//
// The MFMA: a lane (fr = lane % 16, fq = lane / 16) gives A[m = fr][k = fq] and B[k = fq][n = fr] and gets
// D[m = 4 fq + r][n = fr] in register r.  One workgroup owns 16 batch rows (rows past N compute on row N - 1's
// operands and store nothing) and runs u / 16 waves; wave w owns hidden units 16 w .. 16 w + 15 of all three gates.
//
// * Forward: three accumulator tiles, the z, r and h columns of the wave's units, over its [u x 48] slice of U held
//   as B operands (3u / 4 VGPRs).  The reset gate scales the RECURRENT half of the candidate only, so the three
//   tiles do not start alike: z and r start from the prefetched X_z, X_r plus the lane's bias constants, the
//   candidate tile from rb_h alone.  After the MFMAs it is R_h, which is saved as it is (the factor of the reset
//   gate's gradient), and only then meets the X_h that waited in registers of its own.  h_{t-1} is needed twice: by
//   every wave as the A operand, through the double-buffered 16 x u LDS image of lstm.hip (16-byte reads, ONE
//   barrier per step), and lane-locally for the blend, where the lane's own h never left its registers.
// * Backward, t = T-1 .. 0: the recurrent dh is the lane's registers; the four saved activations, h_{t-1} and the
//   upstream dh_t of step t - 1 are loaded while step t computes.  dX_t and dR_t go to HBM (they differ in the
//   candidate's column only) and dR_t into a double-buffered 16 x 3u LDS image, the A operand of dR_t U^T
//   (K = 3u, N = the wave's 16 units; the B operands are the wave's ROWS of U, again 3u / 4 VGPRs).
//   The image: a (row, unit) has three values, not a 16-byte group, so the K order is U's own (gate-major: a
//   lane's three values of a row are three 4-byte writes u floats apart, the 16 lanes of a group write 64
//   consecutive bytes, and a B operand is U[unit][k] with the same k), and a row is 3u + 4 floats long.  That
//   stride is an ODD number of 16-byte columns, so the sixteen rows of a 16-byte A read start in sixteen
//   different columns, and 4 rows are 16 (12 n + 1) floats, so the four row groups of a write land 16 banks
//   apart: both spread over all 64 banks without an XOR (3u / 4 columns are no power of two) and without a
//   fourth slot per unit.  Four independent accumulator chains over the 3u / 4 k-steps, added in one written
//   order; one writer per element, no atomics: bitwise reproducible.
// * Bidirectional (the BI instantiations, grid (ceil(N / 16), 2)): as in lstm.hip.  blockIdx.y is the direction and
//   picks its operand set; direction 1's forward sweep walks t = T-1 .. 0 and its backward sweep t = 0 .. T-1;
//   "first", "last", "next" and the LDS parity count steps, not t; hprev of direction 1 at position t is h of
//   position t + 1; h goes straight into columns d u .. of the [N, T, 2u] (or [N, 2u]) output and dh is read from
//   there.  The unidirectional instantiations are BI = false: one direction, step = t, every stride a constant u.
#include "tde_common.h"

#include <cstdint>

namespace tde {
namespace gru {

constexpr int kRows = 16;              // batch rows per workgroup
constexpr int kMinU = 16, kMaxU = 128;
constexpr float kLog2e = 1.4426950408889634f;

// One direction's operands.  BI: hseq, hlast and dh point at the direction's column d u of a row that is 2u wide
// (hseq: hld wide, u for a dense tensor of its own) and hseq may be null.
struct FwdDir {
  const float* x; const float* u;
  const float* rb;   // [3u] or null
  float* hseq; float* hprev; float* acts;
  float* hlast;      // [N, u] or null
};
template <bool BI>
struct FwdArgs {
  FwdDir d[BI ? 2 : 1];
  int N, T, hld;
};
struct BwdDir {
  const float* acts; const float* hprev; const float* u;
  const float* dh;   // [N, T, u], or [N, u] with last_only
  float* dx; float* dr;
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
// VGPR and an immediate (the gate).  Rows past N are clamped to row N - 1 for the loads and masked for the stores.
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
__global__ __launch_bounds__(64 * NCH) void gru_fwd_kernel(const FwdArgs<BI> p) {
  constexpr int U = 16 * NCH, LD = U + 4, W3 = 3 * U, W4 = 4 * U, HL = BI ? 2 * U : U;
  __shared__ __attribute__((aligned(16))) float himg[2][kRows * LD];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, fr = lane & 15, fq = lane >> 4;
  const int col = 16 * w + fr, N = p.N, T = p.T;
  const bool rev = BI && blockIdx.y;   // direction 1 walks t = T-1 .. 0
  const FwdDir q = rev ? p.d[BI] : p.d[0];
  const int dt = rev ? -1 : 1, hld = BI ? p.hld : U;
  const Rows x3 = rows_of(fq, N, T, W3, col), x4 = rows_of(fq, N, T, W4, col), x1 = rows_of(fq, N, T, U, col);
  const Rows xh = rows_of(fq, N, T, hld, col);

  float ub[NCH][4][3];   // [chunk][k = 16 ch + 4 fq + j][gate]: B[k][n = fr]
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int g = 0; g < 3; ++g) ub[ch][j][g] = q.u[(16 * ch + 4 * fq + j) * W3 + g * U + col];
  float rb[3];           // the recurrent bias of the lane's unit, gate by gate
#pragma unroll
  for (int g = 0; g < 3; ++g) rb[g] = q.rb ? q.rb[g * U + col] : 0.f;

  f32x4 xn[3];   // X of the coming step, gate by gate
#pragma unroll
  for (int g = 0; g < 3; ++g) xn[g] = load_rows(at(q.x, T, W3, rev ? T - 1 : 0) + g * U, x3);
  f32x4 h = {0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
  for (int s = 0, t = rev ? T - 1 : 0; s < T; ++s, t += dt) {   // step s works on position t
    const bool more = s + 1 < T;
    // z and r: X + rb + h U as one sum.  The candidate: rb_h + h U_h alone, X_h joins after the reset gate
    f32x4 acc[3] = {xn[0] + rb[0], xn[1] + rb[1], f32x4{rb[2], rb[2], rb[2], rb[2]}};
    f32x4 act = xn[2];   // X_h now, hh after the gate math
    if (more) {
      const float* xt = at(q.x, T, W3, t + dt);
#pragma unroll
      for (int g = 0; g < 3; ++g) xn[g] = load_rows(xt + g * U, x3);
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
          for (int g = 0; g < 3; ++g) acc[g] = mfma4(a[j], ub[ch][j][g], acc[g]);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float zg = sigmoid_(acc[0][r]), rg = sigmoid_(acc[1][r]);
      const float hh = tanh_(act[r] + rg * acc[2][r]);
      h[r] = zg * h[r] + (1.f - zg) * hh;
      acc[0][r] = zg; acc[1][r] = rg; act[r] = hh;   // acc[2] stays R_h
    }
    if (more) {
      float* hw = himg[(s + 1) & 1] + 4 * fq * LD + col;
#pragma unroll
      for (int r = 0; r < 4; ++r) hw[r * LD] = h[r];
    }
    float* at_ = at(q.acts, T, W4, t);
    float* ht = at(q.hseq, T, hld, t);
    const bool hs = !BI || q.hseq;
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (x1.ok[r]) {
        elem(at_, x4.off[r]) = acc[0][r];
        elem(at_ + U, x4.off[r]) = acc[1][r];
        elem(at_ + 2 * U, x4.off[r]) = act[r];
        elem(at_ + 3 * U, x4.off[r]) = acc[2][r];
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
template <int NCH, bool BI>
__global__ __launch_bounds__(64 * NCH) void gru_bwd_kernel(const BwdArgs<BI> p) {
  constexpr int U = 16 * NCH, K = 3 * U, LD = K + 4, W4 = 4 * U, NK = 3 * NCH;   // NK 16-float chunks of K
  constexpr int DH = BI ? 2 * U : U;                                             // the row of the upstream dh
  __shared__ __attribute__((aligned(16))) float dimg[2][kRows * LD];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, fr = lane & 15, fq = lane >> 4;
  const int col = 16 * w + fr, N = p.N, T = p.T;
  const bool up_ = BI && blockIdx.y;   // direction 1's backward walks t = 0 .. T-1
  const BwdDir q = up_ ? p.d[BI] : p.d[0];
  const int dt = up_ ? 1 : -1, t0 = up_ ? 0 : T - 1;
  const Rows x3 = rows_of(fq, N, T, K, col), x4 = rows_of(fq, N, T, W4, col), x1 = rows_of(fq, N, T, U, col);
  const Rows xd = rows_of(fq, N, T, DH, col);

  // the image's K order is U's column order (k = gate u + unit); lane group fq reads k = 16 ch + 4 fq + j for the
  // j-th MFMA of chunk ch
  f32x4 ub[NK];   // [chunk][j]: B[k][n = fr] = U[16 w + fr][16 ch + 4 fq + j]
#pragma unroll
  for (int ch = 0; ch < NK; ++ch)
#pragma unroll
    for (int j = 0; j < 4; ++j) ub[ch][j] = q.u[col * K + 16 * ch + 4 * fq + j];

  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  const int seq = !p.last_only;
  // the operands of the coming step: z, r, hh, R_h, then hprev and the upstream dh_t
  f32x4 an[4], hpn, upn;
#pragma unroll
  for (int g = 0; g < 4; ++g) an[g] = load_rows(at(q.acts, T, W4, t0) + g * U, x4);
  hpn = load_rows(at(q.hprev, T, U, t0), x1);
  if (seq) {
    upn = load_rows(at(q.dh, T, DH, t0), xd);
  } else {   // [N, DH]: the rows_of of a one-step tensor
    upn = load_rows(at(q.dh, 1, DH, 0), rows_of(fq, N, 1, DH, col));
  }
  f32x4 dhr = zero;

#pragma unroll 1
  for (int s = T - 1; s >= 0; --s) {   // s steps remain after this one, which works on position t
    const int t = up_ ? T - 1 - s : s;
    const bool more = s > 0;
    const f32x4 zg = an[0], rg = an[1], hh = an[2], rh = an[3], hp = hpn, up = upn;
    if (more) {
      const float* a1 = at(q.acts, T, W4, t + dt);
#pragma unroll
      for (int g = 0; g < 4; ++g) an[g] = load_rows(a1 + g * U, x4);
      hpn = load_rows(at(q.hprev, T, U, t + dt), x1);
      upn = seq ? load_rows(at(q.dh, T, DH, t + dt), xd) : zero;
    }
    f32x4 dxz, dxr, da, drh, keep;   // keep: dh z, the lane-local half of the next dhr
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float dh = dhr[r] + up[r];
      da[r] = dh * (1.f - zg[r]) * (1.f - hh[r] * hh[r]);
      dxz[r] = dh * (hp[r] - hh[r]) * (zg[r] * (1.f - zg[r]));
      dxr[r] = da[r] * rh[r] * (rg[r] * (1.f - rg[r]));
      drh[r] = da[r] * rg[r];
      keep[r] = dh * zg[r];
    }
    float* img = dimg[s & 1];
    if (more) {
      float* iw = img + 4 * fq * LD + col;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        iw[r * LD] = dxz[r];
        iw[r * LD + U] = dxr[r];
        iw[r * LD + 2 * U] = drh[r];
      }
    }
    float* dxt = at(q.dx, T, K, t);
    float* drt = at(q.dr, T, K, t);
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (x1.ok[r]) {
        elem(dxt, x3.off[r]) = dxz[r];
        elem(dxt + U, x3.off[r]) = dxr[r];
        elem(dxt + 2 * U, x3.off[r]) = da[r];
        elem(drt, x3.off[r]) = dxz[r];
        elem(drt + U, x3.off[r]) = dxr[r];
        elem(drt + 2 * U, x3.off[r]) = drh[r];
      }
    if (!more) break;
    lds_barrier();
    f32x4 acc[4] = {zero, zero, zero, zero};   // four independent chains, summed in a fixed order
    const float* ir = img + fr * LD + 4 * fq;
#pragma unroll
    for (int ch = 0; ch < NK; ++ch) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(ir + 16 * ch);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = mfma4(a[j], ub[ch][j], acc[j]);
    }
    dhr = keep + ((acc[0] + acc[1]) + (acc[2] + acc[3]));
  }
}

// hrow: the widest row that holds h or dh (u, or 2u for the bidirectional output); the activations' row is 4u
static bool geo_ok(int N, int T, int units, int hrow) {
  if (N < 1 || T < 1 || units < kMinU || units > kMaxU || units % 16) return false;
  const int row = hrow > 4 * units ? hrow : 4 * units;
  return (long long)kRows * T * row * 4 < (1LL << 32);   // a workgroup's rows by 32-bit byte offsets
}

}  // namespace gru
}  // namespace tde

using namespace tde::gru;

#define TDE_GRU_DISPATCH(LAUNCH) \
  switch (units / 16) {          \
    case 1: LAUNCH(1); break;    \
    case 2: LAUNCH(2); break;    \
    case 3: LAUNCH(3); break;    \
    case 4: LAUNCH(4); break;    \
    case 5: LAUNCH(5); break;    \
    case 6: LAUNCH(6); break;    \
    case 7: LAUNCH(7); break;    \
    default: LAUNCH(8); break;   \
  }

template <bool BI>
static void launch_fwd(const FwdArgs<BI>& a, int units, hipStream_t stream) {
  const dim3 grid((unsigned)((a.N + kRows - 1) / kRows), BI ? 2 : 1);
#define TDE_GRU_FWD(n) gru_fwd_kernel<n, BI><<<grid, 64 * n, 0, stream>>>(a)
  TDE_GRU_DISPATCH(TDE_GRU_FWD)
#undef TDE_GRU_FWD
}

// the image is static LDS: 384 units + 512 bytes
template <bool BI>
static void launch_bwd(const BwdArgs<BI>& a, int units, hipStream_t stream) {
  const dim3 grid((unsigned)((a.N + kRows - 1) / kRows), BI ? 2 : 1);
#define TDE_GRU_BWD(n) gru_bwd_kernel<n, BI><<<grid, 64 * n, 0, stream>>>(a)
  TDE_GRU_DISPATCH(TDE_GRU_BWD)
#undef TDE_GRU_BWD
}

// hseq, hprev, acts (and hlast [N, units] unless null) from X = x W + b[0] [N, T, 3 units], U [units, 3 units] and the
// recurrent bias rb [3 units] (null: none)
TDE_API int tde_gru32_fwd(const float* x, const float* u, const float* rb, float* hseq, float* hprev, float* acts,
                          float* hlast, int N, int T, int units, hipStream_t stream) {
  if (!geo_ok(N, T, units, units)) return -1;
  if (!x || !u || !hseq || !hprev || !acts) return -2;
  const FwdArgs<false> a = {{{x, u, rb, hseq, hprev, acts, hlast}}, N, T, units};
  launch_fwd(a, units, stream);
  TDE_LAUNCH_CHECK();
  return 0;
}

// dX and dR [N, T, 3 units] from the forward's activations and h_{t-1} and the upstream dh ([N, T, units], or
// [N, units] for the last step only with last_only)
TDE_API int tde_gru32_bwd(const float* acts, const float* hprev, const float* u, const float* dh, float* dx, float* dr,
                          int N, int T, int units, int last_only, hipStream_t stream) {
  if (!geo_ok(N, T, units, units)) return -1;
  if (!acts || !hprev || !u || !dh || !dx || !dr) return -2;
  const BwdArgs<false> a = {{{acts, hprev, u, dh, dx, dr}}, N, T, last_only};
  launch_bwd(a, units, stream);
  TDE_LAUNCH_CHECK();
  return 0;
}

// Both directions of a bidirectional layer in one launch.  Direction d (0: forward in time, 1: backward in time)
// has its own X_d, U_d, rb_d (null: none) and saved tensors hprev_d, acts_d.  seq: every h into out [N, T, 2 units],
// columns d units .. of position t in the original time order (hseq_d unused).  Otherwise: the directions' final
// states into out [N, 2 units], and every h into hseq_d [N, T, units] unless null.
TDE_API int tde_gru32_bi_fwd(const float* x0, const float* x1, const float* u0, const float* u1, const float* rb0,
                             const float* rb1, float* hseq0, float* hseq1, float* hprev0, float* hprev1, float* acts0,
                             float* acts1, float* out, int N, int T, int units, int seq, hipStream_t stream) {
  if (!geo_ok(N, T, units, 2 * units)) return -1;
  if (!x0 || !x1 || !u0 || !u1 || !hprev0 || !hprev1 || !acts0 || !acts1 || !out) return -2;
  const FwdArgs<true> a = {{{x0, u0, rb0, seq ? out : hseq0, hprev0, acts0, seq ? nullptr : out},
                            {x1, u1, rb1, seq ? out + units : hseq1, hprev1, acts1, seq ? nullptr : out + units}},
                           N, T, seq ? 2 * units : units};
  launch_fwd(a, units, stream);
  TDE_LAUNCH_CHECK();
  return 0;
}

// dX_d and dR_d [N, T, 3 units] of both directions from the upstream dh [N, T, 2 units] (or [N, 2 units] with
// last_only: the gradient of the final states), direction d reading columns d units ..
TDE_API int tde_gru32_bi_bwd(const float* acts0, const float* acts1, const float* hprev0, const float* hprev1,
                             const float* u0, const float* u1, const float* dh, float* dx0, float* dx1, float* dr0,
                             float* dr1, int N, int T, int units, int last_only, hipStream_t stream) {
  if (!geo_ok(N, T, units, 2 * units)) return -1;
  if (!acts0 || !acts1 || !hprev0 || !hprev1 || !u0 || !u1 || !dh || !dx0 || !dx1 || !dr0 || !dr1) return -2;
  const BwdArgs<true> a = {{{acts0, hprev0, u0, dh, dx0, dr0}, {acts1, hprev1, u1, dh + units, dx1, dr1}},
                           N, T, last_only};
  launch_bwd(a, units, stream);
  TDE_LAUNCH_CHECK();
  return 0;
}
