// Fused forward and backward of the DWK/TF2M small CNN trunk — bf16 MFMA form (Keras
// mixed_bfloat16 policy; the float32 form is convnet_f32.hip, shared pieces in tde_convnet.h)
//   Conv2D(32,3x3,VALID,bias,ReLU) · MaxPooling2D(2) · Flatten · Dense(64)  (matmul part)
// (distributed_with_keras.py:34-37, tf2_mnist_distributed.py:67-70;
//  SURVEY.md §2.5 A1-A4 forward, A10-A13 backward).
//
// Design (latency-bound regime; measured with in-kernel s_memrealtime stamps):
//  * 1024-thread workgroups (16 waves): enough waves per CU to hide load latency;
//  * every global operand is loaded ONCE per workgroup with coalesced 16-byte
//    loads issued in the prologue and staged in LDS (rows padded so the
//    16x16x32 MFMA fragment reads are bank-conflict free);
//  * LDS-only barriers (lds_barrier): the scattered global stores of a phase
//    drain in the background instead of stalling the barrier;
//  * the pool-argmax side output is stored lane-contiguous ([P][C/8][ldA] u64).
//
// Forward: a workgroup owns FPW pooled positions x 64 images.
//   phase 1 (VALU; wave = (position, 8-channel group), lane = image): 3x3 conv of
//           the 2x2 pool window from a 4x4 register patch, bias, ReLU, max ->
//           bf16 pooled tile in LDS, argmax bytes, P^T (for the weight grad);
//   phase 2 (MFMA; wave = 16x16 output tile): tile . W1^T rows of the positions
//           -> split-K partial of the Dense pre-activation, f32 atomics into hpre.
// Backward, per workgroup of 4 positions, looping 64-image chunks:
//   dP   = G . W1[p*32:(p+1)*32]^T      (MFMA; Dense input-gradient, in-kernel)
//   dW1[p*32:(p+1)*32] = P^T . G        (MFMA; Dense weight-gradient rows, stored)
//   route dP through the pool argmax and ReLU mask and reduce over (image, window
//   slot) with MFMA: dWc[tap][c] = sum_k X[tap][k] D[k][c], k=(pos,b,q) — the
//   bias gradient is the extra all-ones tap row.
//
// Fused single-replica step (no gradient all-reduce between backward and update):
// the optimizer runs where each gradient is finished, with no extra launch and no
// cross-workgroup hand-off inside a kernel (on gfx950 an in-kernel release/acquire
// costs about as much as a kernel boundary):
//   * Dense(64) kernel rows: each backward workgroup owns its rows' dW1 completely,
//     so it updates the fp32 rows and rewrites their bf16 shadow in place;
//   * Dense(64) bias, Dense(10) kernel + bias (finished by the head workgroup):
//     the last backward workgroup updates them;
//   * Conv2D kernel + bias (finished by the backward's atomics): deferred — the next
//     forward computes the updated values on the fly from (w, g, slots) while *pend,
//     and the next head workgroup (which does not read them) commits them and clears
//     *pend; a flush launch commits them at the end of each execution.
#include "tde_convnet.h"

namespace tde {
using namespace cnet;

constexpr int PPW = 4;   // pooled positions per backward workgroup
constexpr int PSTR = 40; // padded LDS row stride (bf16) of the pooled tile
constexpr int RSTR = 72; // padded LDS row stride (bf16) of 64-wide operand rows

constexpr int fwd_lds(int fpw) { return fpw * 64 * PSTR * 2 + kXrBytes + kConvW * 4; }

// FPW pooled positions x 64 images per workgroup, 4*FPW waves (wave = position x 8-channel
// group).  Phase 1 is VALU-bound: fewer positions per workgroup spread the conv over more CUs
// (FPW=4: 43 workgroups x 16 waves for MNIST; FPW=2: 85 x 8) at the price of more split-K
// atomics in phase 2.
template <int FPW>
__global__ __launch_bounds__(FPW * 256) void convnet_fwd_kernel(FwdArgs a) {
  constexpr int NT = FPW * 256;
  extern __shared__ __attribute__((aligned(16))) unsigned char fsm[];
  bf16* Ps = reinterpret_cast<bf16*>(fsm);
  float* xr = reinterpret_cast<float*>(fsm + FPW * 64 * PSTR * 2);  // [64][XR][W]
  float* wcs = reinterpret_cast<float*>(fsm + FPW * 64 * PSTR * 2 + kXrBytes);  // [10][CC]
  stamp(a.stamps, 0);
  // Keras optimizer.iterations: advanced here, read (stable) by this step's backward / optimizer
  if (a.inc_iter && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) atomicAdd(a.inc_iter, 1ull);
  if (a.fly_count && a.pend && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && *a.pend)
    atomicAdd(a.fly_count, 1ull);
  fwd_snap_head(a, NT);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int fr = lane & 15, fk = (lane >> 4) * 8;
  const int W = a.W, H = a.H;
  const int Wp = (W - 2) / 2, Hp = (H - 2) / 2, P = Hp * Wp;
  const int p0 = blockIdx.x * FPW;
  const int b0 = blockIdx.y * 64;
  const int b = b0 + lane;
  const bool bok = b < a.B;
  // wave-uniform: the conv weights of this wave's 8 channels are scalar loads (SGPRs), not 72 VGPRs
  const int pp = __builtin_amdgcn_readfirstlane(wave >> 2), cg = __builtin_amdgcn_readfirstlane(wave & 3),
            c0 = cg * 8;
  const int p = p0 + pp;
  const bool pok = p < P;
  const int py0 = p0 / Wp;
  const int nrows = min(XR, H - 2 * py0);
  const bf16* W1c = reinterpret_cast<const bf16*>(a.W1);
  bf16* Pt = reinterpret_cast<bf16*>(a.Pt);

  // ---- prologue: all global loads, independent, issued back to back
  fwd_stage_x(a, xr, b0, py0, nrows, NT);
  fwd_stage_conv(a, wcs, NT);
  // W1^T fragments of this wave's output tiles: tile t = wave + 4*FPW*j (j < 4/FPW),
  // mt = t>>2 (image rows), nt = t&3 = wave&3 (units) for every j
  const int nt = wave & 3;
  bf16x8 wfr[FPW];
#pragma unroll
  for (int ks = 0; ks < FPW; ++ks) {
    const int kp = p0 + ks;
    if (kp >= P) {
      wfr[ks] = bf16x8{};
    } else if (a.w1_rows) {
      // row-major shadow [K][HD]: 8 K-consecutive elements of column nt*16+fr (16 lanes read
      // 32 contiguous bytes per element row)
      const bf16* src = W1c + (size_t)(kp * CC + fk) * a.ldw1 + nt * 16 + fr;
#pragma unroll
      for (int j = 0; j < 8; ++j) wfr[ks][j] = src[(size_t)j * a.ldw1];
    } else {
      wfr[ks] = *reinterpret_cast<const bf16x8*>(W1c + (size_t)(nt * 16 + fr) * a.ldw1 + (size_t)kp * CC + fk);
    }
  }
  stamp(a.stamps, 1);
  lds_barrier();
  ConvW8 cw;
  cw.load(wcs, c0);

  // ---- phase 1: conv + bias + ReLU + 2x2 max-pool for 8 channels
  bf16x8 outv;
  if (bok && pok) {
    const int py = p / Wp, px = p - py * Wp;
    float out[8];
    uint64_t packed;
    conv_pool8(xr + lane * fwd_istride(W) + (2 * (py - py0)) * W + 2 * px, W, cw, out, packed);
#pragma unroll
    for (int cc = 0; cc < 8; ++cc) outv[cc] = f2bf(out[cc]);
    if (a.amax) a.amax[((size_t)p * (CC / 8) + cg) * a.lda + b] = packed;
    if (Pt) {
#pragma unroll
      for (int cc = 0; cc < 8; ++cc) Pt[(size_t)(p * CC + c0 + cc) * a.ldPt + b] = outv[cc];
    }
  } else {
#pragma unroll
    for (int cc = 0; cc < 8; ++cc) outv[cc] = f2bf(0.f);
    if (pok && Pt && b < a.ldPt) {
#pragma unroll
      for (int cc = 0; cc < 8; ++cc) Pt[(size_t)(p * CC + c0 + cc) * a.ldPt + b] = outv[cc];
    }
  }
  *reinterpret_cast<bf16x8*>(Ps + ((size_t)pp * 64 + lane) * PSTR + c0) = outv;
  stamp(a.stamps, 2);
  lds_barrier();
  stamp(a.stamps, 3);

  // ---- phase 2: hpre[64 x 64] += Ps(64 x FPW*32) . W1^T(FPW*32 x 64); 16x16 tiles over the waves.
  // The ~85 workgroups' partial sums land on the same 16 KB: spread over hrep replicas (summed by the
  // consumer) so each address sees ~85/hrep memory-side adds instead of 85
  float* const hrow = a.hpre + (size_t)(blockIdx.x % a.hrep) * a.hrep_stride;
#pragma unroll
  for (int j = 0; j < 4 / FPW; ++j) {
    const int mt = (wave >> 2) + FPW * j;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < FPW; ++ks) {
      if (p0 + ks < P) {
        const bf16x8 av = *reinterpret_cast<const bf16x8*>(Ps + ((size_t)ks * 64 + mt * 16 + fr) * PSTR + fk);
        acc = mfma16(av, wfr[ks], acc);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = b0 + mt * 16 + (lane >> 4) * 4 + r;
      if (row < a.B) atomicAdd(hrow + (size_t)row * HD + nt * 16 + fr, acc[r]);
    }
  }
  stamp(a.stamps, 4);
}

// LDS carve of the backward (bytes)
constexpr int kG = 0;                                   // bf16 [64][RSTR]
constexpr int kW1 = kG + 64 * RSTR * 2;                 // bf16 [128][RSTR]
constexpr int kPt = kW1 + 128 * RSTR * 2;               // bf16 [128][RSTR]
constexpr int kGt = kPt + 128 * RSTR * 2;               // bf16 [64][RSTR]
constexpr int kXs = kGt + 64 * RSTR * 2;                // f32  [PPW][64][16]
constexpr int kAm = kXs + PPW * 64 * 16 * 4;            // u8   [PPW][64][CC]
constexpr int kDp = kAm + PPW * 64 * CC;                // f32  [PPW][64][DPS] (head scratch; red [NW][16][CC])
// dP row stride: 40 floats puts the 4 lane groups of the routing reads (rows 2 apart) on disjoint
// bank quarters (stride 32 made them 4-way LDS bank conflicts)
constexpr int DPS = 40;
constexpr int kW2s = kDp + PPW * 64 * DPS * 4;          // f32  [HD][16] W2, classes padded to 16
constexpr int kB2s = kW2s + kW2Bytes;                   // f32  [16]
constexpr int kLab = kB2s + kB2Bytes;                   // i32  [64]
constexpr int kBwdLds = kLab + kLabBytes;
static_assert(kHeadScratch <= PPW * 64 * DPS * 4, "head scratch exceeds the dP area");

// MODE 0: store gradients; 1: fused step, SGD; 2: fused step, optimizer with slots (momentum / Adam).
// Grid: one workgroup per PPW pooled positions + the head workgroup (last).
template <int MODE>
__global__ __launch_bounds__(1024) void convnet_bwd_kernel(BwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  bf16* Gs = reinterpret_cast<bf16*>(smem + kG);
  bf16* W1s = reinterpret_cast<bf16*>(smem + kW1);
  bf16* Pts = reinterpret_cast<bf16*>(smem + kPt);
  bf16* Gts = reinterpret_cast<bf16*>(smem + kGt);
  float* xs = reinterpret_cast<float*>(smem + kXs);
  uint8_t* am = smem + kAm;
  float* dps = reinterpret_cast<float*>(smem + kDp);
  const HeadLds hl = HeadLds::carve(smem + kDp, smem + kW2s, smem + kB2s, smem + kLab);
  stamp(a.stamps, 0);
  const int W = a.W, H = a.H;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, tid = threadIdx.x;
  const int fr = lane & 15, fq = lane >> 4, fk = fq * 8;
  const bf16* W1r = reinterpret_cast<const bf16*>(a.W1);
  const bf16* Pt = reinterpret_cast<const bf16*>(a.Pt);

  // ---- every workgroup: W2 image and b2 in LDS; its slice of the other parity buffer of hpre zeroed
  head_load_w2(a, hl, tid);
  zero_other_parity(a, tid);
  if (blockIdx.x == gridDim.x - 1) {
    head_workgroup<MODE>(a, hl, reinterpret_cast<float*>(smem + kG));   // the G area is unused there
    return;
  }

  const int Wp = (W - 2) / 2, Hp = (H - 2) / 2, P = Hp * Wp;
  const int p0 = blockIdx.x * PPW;
  const int nrow = min(PPW, P - p0) * CC;  // valid W1/Pt rows of this workgroup
  const int hr = tid >> 4, hc4 = (tid & 15) * 4;   // hpre element group of this thread: row, 4 units
  const float4 b1v = a.b1 ? *reinterpret_cast<const float4*>(a.b1 + hc4) : float4{0.f, 0.f, 0.f, 0.f};

  f32x4 accw[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  f32x4 accr[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};

  // ---- fused step: this workgroup's fp32 master rows (and slots), loaded now, updated after the loop
  constexpr int NS = MODE == 2 ? 2 : 1;   // slot registers (dummies unless MODE 2)
  f32x4 wp[2], mp[NS], vp[NS];
  long long t_it = 0;
  if (MODE != 0) {
    t_it = *a.iterations;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int t = wave + 16 * i;
      const int nt = t & 3, rt = t >> 2;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = rt * 16 + fq * 4 + r;
        const size_t e = (size_t)(p0 * CC + row) * HD + nt * 16 + fr;
        wp[i][r] = row < nrow ? a.w1[e] : 0.f;
        if (MODE == 2) {
          // the slot rule (opt_has_m / opt_has_v, tde_optim.h) spelled out, here and at the stores below: through
          // the helpers this kernel's register allocation changed (123 -> 222 spilled VGPRs)
          mp[i % NS][r] = (row < nrow && a.h.kind != kOptSGD) ? a.m1[e] : 0.f;
          vp[i % NS][r] = (row < nrow && a.h.kind == kOptAdam) ? a.v1[e] : 0.f;
        }
      }
    }
  }

  // W1 rows of the 4 positions: loaded once (independent of the image chunk)
  {
    const int r = tid >> 3, c = (tid & 7) * 8;  // 128 rows x 8 chunks of 16 B
    bf16x8 v = r < nrow ? *reinterpret_cast<const bf16x8*>(W1r + (size_t)(p0 * CC + r) * a.ldw1 + c) : bf16x8{};
    *reinterpret_cast<bf16x8*>(W1s + r * RSTR + c) = v;
  }

  for (int b0 = 0; b0 < a.B; b0 += 64) {
    const int nb = min(64, a.B - b0);
    // ---- prologue: coalesced loads of this chunk's operands
    float4 hv = {0.f, 0.f, 0.f, 0.f};
    if (hr < nb) hv = load_hpre(a, b0 + hr, hc4);
    const int lab = (tid < nb) ? a.labels[b0 + tid] : 0;
    bf16x8 ptv;
    {
      const int r = tid >> 3, c = (tid & 7) * 8;
      ptv = r < nrow ? load_frag(Pt + (size_t)(p0 * CC + r) * a.ldPt + b0 + c, b0 + c, a.B, true) : bf16x8{};
    }
    float4 xv = {0.f, 0.f, 0.f, 0.f};
    {
      const int pp = tid >> 8, bl = (tid >> 2) & 63, r = tid & 3;
      const int p = p0 + pp, b = b0 + bl;
      if (p < P && b < a.B) {
        const int py = p / Wp, px = p - py * Wp;
        const float2* row = reinterpret_cast<const float2*>(a.x + (size_t)b * H * W + (2 * py + r) * W + 2 * px);
        const float2 u = row[0], t = row[1];
        xv = float4{u.x, u.y, t.x, t.y};
      }
    }
    uint64_t amv = ~0ull;
    {
      const int pp = tid >> 8, cg = (tid >> 6) & 3, bl = tid & 63;
      const int p = p0 + pp, b = b0 + bl;
      if (p < P && b < a.B) amv = a.amax[((size_t)p * (CC / 8) + cg) * a.lda + b];
    }
    stamp(a.stamps, 1);
    head_stage(a, hv, b1v, hr, hc4, nb, hl.hs);
    if (tid < 64) hl.labs[tid] = lab;
    {
      const int r = tid >> 3, c = (tid & 7) * 8;
      *reinterpret_cast<bf16x8*>(Pts + r * RSTR + c) = ptv;
    }
    {
      const int pp = tid >> 8, bl = (tid >> 2) & 63, r = tid & 3;
      *reinterpret_cast<float4*>(xs + ((size_t)pp * 64 + bl) * 16 + r * 4) = xv;
    }
    {
      const int pp = tid >> 8, cg = (tid >> 6) & 3, bl = tid & 63;
      *reinterpret_cast<uint64_t*>(am + ((size_t)pp * 64 + bl) * CC + cg * 8) = amv;
    }
    lds_barrier();
    // ---- the head recomputed: G = dH (bf16) into LDS, row-major and transposed
    {
      float la = 0.f, ca = 0.f, na = 0.f;   // the head workgroup keeps these
      head_logits_ce(a, nb, hl, lane, wave, la, ca, na);
      const f32x4 gh = head_dh(a, nb, hl, lane, wave);
      const int rt = wave >> 2, j = (wave & 3) * 16 + fr;
      bf16x4 gt;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        gt[i] = f2bf(gh[i]);
        Gs[(rt * 16 + fq * 4 + i) * RSTR + j] = gt[i];
      }
      *reinterpret_cast<bf16x4*>(Gts + j * RSTR + rt * 16 + fq * 4) = gt;
    }
    lds_barrier();
    stamp(a.stamps, 2);

    // ---- dP[pp][b][c] = G[b] . W1[pp*32 + c]  (wave = position x 16 images)
    {
      const int pp = wave >> 2, mt = wave & 3;
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const bf16x8 av = *reinterpret_cast<const bf16x8*>(Gs + (mt * 16 + fr) * RSTR + ks * 32 + fk);
          const bf16x8 bv = *reinterpret_cast<const bf16x8*>(W1s + (pp * CC + ct * 16 + fr) * RSTR + ks * 32 + fk);
          acc = mfma16(av, bv, acc);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) dps[((size_t)pp * 64 + mt * 16 + fq * 4 + r) * DPS + ct * 16 + fr] = acc[r];
      }
    }
    // ---- dW1 rows += P^T . G   (32 tiles of 16x16: t = wave, wave+16)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int t = wave + 16 * i;
      const int nt = t & 3, rt = t >> 2;  // rt: 16-row block (of 8) within the 128 rows
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const bf16x8 av = *reinterpret_cast<const bf16x8*>(Pts + (rt * 16 + fr) * RSTR + ks * 32 + fk);
        const bf16x8 bv = *reinterpret_cast<const bf16x8*>(Gts + (nt * 16 + fr) * RSTR + ks * 32 + fk);
        accw[i] = mfma16(av, bv, accw[i]);
      }
    }
    lds_barrier();
    stamp(a.stamps, 3);

    // ---- routing MFMA: k = ((pp*64 + b)*4 + q); 32 k-steps, wave takes ks = wave, wave+16
    {
      const int tap = fr, ky = tap / 3, kx = tap - ky * 3;
#pragma unroll
      for (int h2 = 0; h2 < 2; ++h2) {
        const int ks = wave + 16 * h2;
        const int kb = ks * 32 + fk;
        const int pp = kb >> 8, bl = (kb >> 2) & 63;
        bf16x8 av;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int bb = bl + (j >> 2), q = j & 3, qy = q >> 1, qx = q & 1;
          float v;
          if (tap < 9) v = xs[((size_t)pp * 64 + bb) * 16 + (qy + ky) * 4 + qx + kx];
          else v = (tap == 9) ? 1.f : 0.f;
          av[j] = f2bf(v);
        }
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
          const int c = ct * 16 + fr;
          bf16x8 bv;
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const size_t idx = ((size_t)pp * 64 + bl + h) * CC + c;
            const unsigned id = am[idx];
            const float dv = dps[((size_t)pp * 64 + bl + h) * DPS + c];
#pragma unroll
            for (int q = 0; q < 4; ++q) bv[h * 4 + q] = f2bf(id == (unsigned)q ? dv : 0.f);
          }
          accr[ct] = mfma16(av, bv, accr[ct]);
        }
      }
    }
    lds_barrier();
  }
  stamp(a.stamps, 4);

  if (MODE != 0) {
    // ---- update this workgroup's Dense(64) rows (complete dW1: rows belong to one workgroup) and
    // rewrite their bf16 shadows; its W1 rows were read into LDS before the chunk loop
    const float lr_t = opt_lr_t(a.h, t_it);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int t = wave + 16 * i;
      const int nt = t & 3, rt = t >> 2;
      const int col = nt * 16 + fr, row0 = rt * 16 + fq * 4;
      if (row0 >= nrow) continue;   // nrow is a multiple of 32: all 4 rows valid or none
      bf16x4 hv4;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const size_t e = (size_t)(p0 * CC + row0 + r) * HD + col;
        float m = MODE == 2 ? mp[i % NS][r] : 0.f, v = MODE == 2 ? vp[i % NS][r] : 0.f;
        const float w = opt_step(a.h, lr_t, wp[i][r], accw[i][r], m, v);
        a.w1[e] = w;
        if (MODE == 2 && a.h.kind != kOptSGD) a.m1[e] = m;
        if (MODE == 2 && a.h.kind == kOptAdam) a.v1[e] = v;
        hv4[r] = f2bf(w);
        a.w1r_out[e] = hv4[r];
      }
      if (a.w1c_out) *reinterpret_cast<bf16x4*>(a.w1c_out + (size_t)col * a.ldw1c + p0 * CC + row0) = hv4;
    }
  } else {
    // ---- store dW1 tiles (each row of dW1 belongs to exactly one workgroup)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int t = wave + 16 * i;
      const int nt = t & 3, rt = t >> 2;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = rt * 16 + fq * 4 + r;
        if (row < nrow) a.dW1[(size_t)(p0 * CC + row) * HD + nt * 16 + fr] = accw[i][r];
      }
    }
  }
  // ---- reduce routing accumulators over the 16 waves, then 10*CC atomics
  conv_grad_reduce(a, accr, dps, lane, wave);
  stamp(a.stamps, 5);
}

}  // namespace tde

using namespace tde;
using namespace tde::cnet;

// Specialised for Conv2D(32, 3x3, valid) on 1-channel input + MaxPool(2) + Dense(64).
// w1_rows: W1c is the row-major [K][HD] shadow (ldw1c == HD) instead of [HD][K].
// opt (nullable): deferred conv update {w, g, m, v, pend} with wc/bc at offsets off_wc/off_bc.
TDE_API int tde_convnet_fwd(const float* x, const float* wc, const float* bc, const void* W1c, int ldw1c,
                            float* hpre, void* Pt, int ldPt, void* amax, int lda, int B, int H, int W,
                            long long* stamps, int w1_rows, const TdeStepOpt* opt, long long off_wc,
                            long long off_bc, long long* inc_iter, int hrep, long long hrep_stride,
                            hipStream_t stream) {
  if ((W & 3) || W > XW || ((W - 2) / 2) < 4 || (ldw1c & 7) || (Pt && (ldPt & 7)) || (amax && lda < B)) return -1;
  if (((uintptr_t)wc | (uintptr_t)bc) & 15) return -2;
  if (w1_rows && ldw1c != HD) return -3;
  if (opt && (!opt_ok(opt) || !opt->pend)) return -4;
  const int P = ((H - 2) / 2) * ((W - 2) / 2);
  int by = (B + 63) / 64;
  if (Pt) {
    const int byp = (ldPt + 63) / 64;
    if (byp > by) by = byp;
  }
  FwdArgs a{x, wc, bc, W1c, ldw1c, hpre, Pt, ldPt, (uint64_t*)amax, lda, B, H, W, stamps};
  a.w1_rows = w1_rows;
  fill_fwd_opt(a, opt, off_wc, off_bc, inc_iter, hrep, hrep_stride);
  // positions per workgroup (TDE_CONVNET_FPW = 1|2|4, default 2)
  static const int fpw = [] {
    const char* e = getenv("TDE_CONVNET_FPW");
    const int v = e ? atoi(e) : 2;
    return (v == 1 || v == 4) ? v : 2;
  }();
  static bool attr_set = false;
  if (!attr_set) {
    hipFuncSetAttribute((const void*)convnet_fwd_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, fwd_lds(1));
    hipFuncSetAttribute((const void*)convnet_fwd_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, fwd_lds(2));
    hipFuncSetAttribute((const void*)convnet_fwd_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize, fwd_lds(4));
    attr_set = true;
  }
  const dim3 grid((P + fpw - 1) / fpw, by);
  if (fpw == 1) convnet_fwd_kernel<1><<<grid, 256, fwd_lds(1), stream>>>(a);
  else if (fpw == 2) convnet_fwd_kernel<2><<<grid, 512, fwd_lds(2), stream>>>(a);
  else convnet_fwd_kernel<4><<<grid, 1024, fwd_lds(4), stream>>>(a);
  TDE_LAUNCH_CHECK();
  return 0;
}

// hpre: this step's Dense(64) pre-activation [B][64] f32; hzero: the other parity buffer (zeroed).
// MODE 0 (opt == null): dW1 stored, conv grads atomically added, head grads (dW2 [64][C], db2, db1)
// added by one workgroup.  opt: fused step (see BwdArgs).
TDE_API int tde_convnet_bwd(const float* x, const void* amax, int lda, const float* hpre, float* hzero,
                            int hrep, long long hrep_stride, const float* b1, const float* W2, const float* b2, int C, int pre_relu,
                            const int* labels, float scale, float* metrics, const void* W1r, int ldw1r,
                            const void* Pt, int ldPt, float* dW1, float* dwc, float* dbc, float* dW2, float* db2,
                            float* db1, int B, int H, int W, long long* stamps, const TdeBwdOpt* opt,
                            float* cpart, hipStream_t stream) {
  BwdArgs a;
  const int rc = fill_bwd(a, x, amax, lda, hpre, hzero, hrep, hrep_stride, b1, W2, b2, C, pre_relu, labels, scale,
                          metrics, W1r, ldw1r, Pt, ldPt, dW1, dwc, dbc, dW2, db2, db1, B, H, W, stamps, opt);
  if (rc) return rc;
  a.cpart = cpart;
  const int P = ((H - 2) / 2) * ((W - 2) / 2);
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)convnet_bwd_kernel<0>, hipFuncAttributeMaxDynamicSharedMemorySize, kBwdLds);
    (void)hipFuncSetAttribute((const void*)convnet_bwd_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, kBwdLds);
    (void)hipFuncSetAttribute((const void*)convnet_bwd_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, kBwdLds);
    attr_set = true;
  }
  const dim3 grid((P + PPW - 1) / PPW + 1);   // + the head workgroup
  if (!opt) convnet_bwd_kernel<0><<<grid, 1024, kBwdLds, stream>>>(a);
  else if (opt->h.kind == kOptSGD) convnet_bwd_kernel<1><<<grid, 1024, kBwdLds, stream>>>(a);
  else convnet_bwd_kernel<2><<<grid, 1024, kBwdLds, stream>>>(a);
  TDE_LAUNCH_CHECK();
  return 0;
}

// Deterministic mode (TDE_DETERMINISTIC): dwc / dbc += the backward's per-workgroup conv-gradient
// partials cpart [nwg][10 * 32], summed in workgroup order.
__global__ void __launch_bounds__(10 * CC) cgrad_reduce_kernel(const float* cpart, int nwg, float* dwc, float* dbc) {
  const int i = threadIdx.x;
  float s = 0.f;
  for (int w = 0; w < nwg; ++w) s += cpart[(size_t)w * 10 * CC + i];
  if (i < 9 * CC) dwc[i] += s;
  else if (dbc) dbc[i - 9 * CC] += s;
}
TDE_API int tde_convnet_cgrad_reduce(const float* cpart, int nwg, float* dwc, float* dbc, hipStream_t stream) {
  if (!cpart || !dwc || nwg < 1) return -1;
  cgrad_reduce_kernel<<<1, 10 * CC, 0, stream>>>(cpart, nwg, dwc, dbc);
  TDE_LAUNCH_CHECK();
  return 0;
}

// Empty kernel: measures the launch/boundary floor of the device (microbenchmarks).
__global__ void noop_kernel() {}
TDE_API int tde_noop(int blocks, int threads, hipStream_t stream) {
  noop_kernel<<<blocks, threads, 0, stream>>>();
  TDE_LAUNCH_CHECK();
  return 0;
}
