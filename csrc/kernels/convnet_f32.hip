// Fused forward and backward of the DWK/TF2M small CNN trunk in float32 — the reference's
// precision (distributed_with_keras.py:21 casts the images to float32; every Keras layer of
// distributed_with_keras.py:33-43 / tf2_mnist_distributed.py:66-72 runs in the float32 policy).
//
// Same dataflow as the bf16 form (convnet.hip; shared pieces in tde_convnet.h), with every
// GEMM on the exact-f32 MFMA v_mfma_f32_16x16x4_f32 (bit-for-bit a k-ordered fmaf chain, no
// reduced-precision operand anywhere) over f32 LDS tiles and the f32 master weights — no bf16
// shadow exists in this form, so the optimizer writes nothing but the master weights.
//
// The f32 MFMA issues at 1/16 of the bf16 rate (MI355X_MICROARCH.md § Matrix cores), so the work
// per workgroup is cut to keep each CU's matrix pipe time small and spread over more CUs:
//   forward   4 consecutive pooled positions x 16 images per workgroup (43 x 4 = 172 workgroups
//             for MNIST at batch 64), 8 waves (512 threads), two per SIMD: a wave alone on its SIMD
//             issues a vector instruction every 4 cycles where the SIMD takes one every 2
//             (MI355X_MICROARCH.md, "vector-instruction ISSUE cost"), and with one workgroup per CU
//             the second wave is the only other issuer there is.  Wave roles:
//               prologue  all 8 waves stage the image rows (2 float4 per thread); waves 0-4 the 320
//                         conv operands, one each; waves 0-3 load their W1 fragments;
//               conv      wave w computes channels 4w..4w+3 for (image, position slot) = lane: 4 rows
//                         of Pt, one float4 of the pooled tile and one 32-bit half of the argmax
//                         word wave >> 1 (waves 2cg and 2cg + 1 fill word cg);
//               Dense(64) waves 0-3 only (waves 4-7 end after the second barrier): wave w owns the
//                         output column tile w over K = 4 x 32 (one accumulator per position, 32
//                         MFMAs, summed in registers), then split-K atomics into hpre: 4
//                         wave-instructions per wave, a quarter of the float-atomic bytes of one
//                         position per workgroup (the adds run at ~1.3 TB/s chip-wide whatever their
//                         spread).  Spreading the MFMAs over all 8 waves (an LDS hand-off and a third
//                         barrier) and a raised priority for waves 4-7 were measured and were slower or
//                         no faster (profiles/fwd_waves/NOTES.md);
//   backward  ONE pooled position per workgroup (169 + the head workgroup); per 64-image chunk
//             waves 0-7 compute dP = G . W1^T (8 tiles x 16 MFMAs) while waves 8-15 compute
//             the position's dW1 rows = P^T . G (8 tiles x 16 MFMAs), then all 16 waves run the
//             routing MFMA dWc[tap][c] = sum_{b,q} X[tap][(b,q)] D[(b,q)][c] (lane group = pool
//             window slot q, 8 MFMAs per wave).
//
// Fragment map of the 16x16x4 f32 MFMA: lane l holds A[l&15][k] and B[k][l&15] with k set by
// (l>>4, step); a lane's k for step s of a 16-k group is fq*16 + 4*((s/4 + fq) & 3) + s%4
// (fq = l>>4), so each lane reads its operands as float4 rows and, with 72-float LDS rows
// (168 = 40 mod 64 for the forward's 128-wide tile, 8-k groups per position: a position's column
// offset shifts every lane's bank alike), the ds_read_b128 lane groups hit disjoint banks (searched
// exhaustively over strides and per-group rotations).
//
// Placement: every operand handed from one launch to the other (the W1 rows the backward rewrites and the next
// forward reads; the Pt rows and argmax words the forward stores and the backward reads) is written by plain
// stores, which stay in the writing XCD's L2.  Both launches have a 1-D grid whose workgroup ids are mapped
// (tde_convnet.h: fwd_slot, bwd_slot) so that writer and reader of those lines have ids of one class mod 8, that
// is, run on one XCD (profiles/xcd_handoff/NOTES.md: measured placement, eager and in a graph).  Only speed
// depends on it.  tde_convnet_f32_identity_slots(1) forces the identity maps.
//
// Each launch has a production form and a general one, picked by the entry points:
//   forward   convnet32_fwd_plain_kernel: no stamp buffer given (every training and inference step);
//             convnet32_fwd_kernel: the same body with its five phase stamps, for calls with a stamp buffer.
//   backward  convnet32g_bwd_kernel<MODE>: 28 x 28 images, B a positive multiple of 64 (whole chunks: no index
//             clamped, no row masked), 4 hpre replicas, no stamp buffer -- all compile-time constants
//             (Geo<28, 28>, ProdForm), and no diagnostics in the kernel text.  This is the step of the
//             reference model at its batch of 64 per worker;
//             convnet32_bwd_kernel<MODE>: every other call (other shapes, ragged batches, other replica counts,
//             the deterministic layout, a stamp buffer): everything read from the arguments, stamps included.
//             tde_convnet_f32_runtime_geom(1) forces it.
// A diagnostic run (bench/micro.py with a stamp buffer) therefore times the general forms: its stamps locate
// the phases, the production forms' times come from runs without a stamp buffer.
#include "tde_convnet.h"

namespace tde {
using namespace cnet;

constexpr int FG = 4;      // pooled positions per forward workgroup
constexpr int FB = 16;     // images per forward workgroup
constexpr int FNT = 512;   // threads of a forward workgroup: 8 waves, two per SIMD
constexpr int AS32 = 168;  // f32 LDS row stride of the forward's pooled tile [FB][FG*32]
constexpr int GS32 = 72;   // f32 LDS row stride of the backward's 64-wide operand rows
constexpr int DPS32 = 40;  // f32 LDS row stride of dP [64][32]
static_assert(FG == 4 && FB == 16, "the forward's lane maps are written for 4 positions x 16 images");

// per-image stride of the forward's staged rows: 4 (mod 64) floats, so the float2 patch reads of a
// ds_read_b64 lane group (16 images x 2 consecutive positions, 2 floats apart) cover the 64 banks once
__host__ __device__ constexpr int fwd32_istride(int W) { return XR * W + ((4 - (XR * W) % 64) + 64) % 64; }
constexpr int kXr32Bytes = FB * (XR * XW + 64) * 4;
constexpr int kFwd32Lds = FB * AS32 * 4 + kXr32Bytes + kConvW * 4;

// column of the float4 a lane reads for group i of a 32-wide (8 k per lane group) row
__device__ __forceinline__ int k8_col(int fq, int i) { return fq * 8 + 4 * ((i + fq) & 1); }
// ... and of a 64-wide (16 k per lane group) row
__device__ __forceinline__ int k16_col(int fq, int i) { return fq * 16 + 4 * ((i + fq) & 3); }

// Image geometry of a backward form: GH x GW known at compile time (the 28 x 28 of MNIST, which is all the
// benchmark and the reference model run: the division by Wp, the workgroup count and every image stride are
// then constants), or <0, 0>: read from the arguments.  Geo<28, 28> is used by the production form alone
// (with ProdForm: whole chunks, 4 replicas, no diagnostics); a 28 x 28 call that misses one of
// its conditions takes Geo<0, 0> like every other shape.  The forward keeps the runtime geometry in both of
// its forms: specialised, it was not faster (profiles/bwd_head/NOTES.md).
template <int GH, int GW>
struct Geo {
  static constexpr bool kFixed = GH > 0;
  template <class A> __device__ __forceinline__ static int H(const A& a) { return kFixed ? GH : a.H; }
  template <class A> __device__ __forceinline__ static int W(const A& a) { return kFixed ? GW : a.W; }
};
constexpr int kGH = 28, kGW = 28;   // the specialised form

// The <= XR input rows of the workgroup's FB images -> xr, in two halves: issue() the coalesced float4
// loads (16 images x 6 rows x 32 floats = 768 float4 at most: kU per thread, one pass of FNT threads),
// store() after the prologue's common wait (the 16-byte-aligned image stride takes whole float4 stores).
struct Fwd32X {
  static constexpr int kU = 2;
  static_assert(FB * XR * XW / 4 <= kU * FNT, "one pass of the workgroup stages the rows");
  float4 v[kU];
  __device__ __forceinline__ void issue(const FwdArgs& a, int b0, int py0, int nrows) {
    const int W = a.W, H = a.H;
    const int n4 = nrows * W / 4;  // float4 per image
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int i = threadIdx.x + u * FNT, bl = i / n4, q = i - bl * n4;
      v[u] = float4{0.f, 0.f, 0.f, 0.f};
      if (i < FB * n4 && b0 + bl < a.B)
        v[u] = *reinterpret_cast<const float4*>(a.x + (size_t)(b0 + bl) * H * W + (size_t)(2 * py0) * W + q * 4);
    }
  }
  __device__ __forceinline__ void store(const FwdArgs& a, float* xr, int nrows) const {
    const int W = a.W;
    const int istride = fwd32_istride(W);
    const int n4 = nrows * W / 4;
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int i = threadIdx.x + u * FNT, bl = i / n4, q = i - bl * n4;
      if (i < FB * n4) *reinterpret_cast<float4*>(xr + bl * istride + q * 4) = v[u];
    }
  }
};

// The forward's body.  DIAG: the five phase stamps exist (off: stamp() is not called at all and
// FwdArgs::stamps is ignored).
template <bool DIAG>
__device__ __forceinline__ void convnet32_fwd_body(const FwdArgs& a, unsigned char* fsm) {
  float* As = reinterpret_cast<float*>(fsm);                                  // [FB][AS32] pooled tile
  float* xr = reinterpret_cast<float*>(fsm + FB * AS32 * 4);                  // [FB][XR][W]
  float* wcs = reinterpret_cast<float*>(fsm + FB * AS32 * 4 + kXr32Bytes);    // [10][CC]
  // the two scalars of the deferred update, read ahead of the kernel's first store (scalar loads: nothing
  // waits for them before the prologue's common wait)
  int pendv;
  long long iterv;
  conv_flags_issue(a, pendv, iterv);
  if constexpr (DIAG) {
    stamp(a.stamps, 0);
    stamp_xcc(a.stamps, kXccSlot);
  }
  if (a.inc_iter && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) atomicAdd(a.inc_iter, 1ull);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const int W = a.W, H = a.H;
  const int Wp = (W - 2) / 2, Hp = (H - 2) / 2, P = Hp * Wp;
  // 1-D grid: this workgroup's position group and image tile (tde_convnet.h: fwd_slot)
  const FwdSlot sl = fwd_slot_runs((int)blockIdx.x, a.groups, a.tiles, a.slot_full);
  const int p0 = sl.g * FG;
  const int b0 = sl.y * FB;
  const int py0 = p0 / Wp;   // FG <= Wp (host check): the group's positions lie in pooled rows py0, py0 + 1
  const int nrows = min(XR, H - 2 * py0);
  const float* W1 = reinterpret_cast<const float*>(a.W1);
  float* Pt = reinterpret_cast<float*>(a.Pt);

  // ---- prologue: every global load is issued before the first wait and the first LDS store (one round
  // trip).  In the order of use: the image rows and the conv operands (phase 1; the kConvW = 320 elements
  // on waves 0-4, one each), the head snapshot's sources (workgroup (0,0)), then, on waves 0-3, which issue
  // the MFMAs, the B fragments (phase 2): W1[kp*32 + k][nt*16 + fr] for this lane's 8 k of each position
  // (f32 master, [K][HD]).
  static_assert(kConvW % 64 == 0 && kConvW <= FNT, "whole waves hold the conv operands, one element per thread");
  Fwd32X xst;
  xst.issue(a, b0, py0, nrows);
  const bool cv_wave = wave < kConvW / 64;
  ConvOperand cv;
  if (cv_wave) cv.issue(a, threadIdx.x);
  SnapHead<FNT> snap;
  const bool snap_wg = SnapHead<FNT>::mine(a);
  if (snap_wg) snap.issue(a);
  const bool mfma_wave = wave < 4;
  const int nt = wave;   // waves 0-3: the output column tile
  float wfr[FG][8];
  if (mfma_wave) {
#pragma unroll
    for (int ks = 0; ks < FG; ++ks) {
      const int kp = min(p0 + ks, P - 1);   // positions past P read the last one and count as 0 below
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) wfr[ks][4 * i + j] = W1[(size_t)(kp * CC + k8_col(fq, i) + j) * a.ldw1 + nt * 16 + fr];
    }
  }
  xst.store(a, xr, nrows);
  if (cv_wave) wcs[threadIdx.x] = cv.finish(a, pendv, iterv);
  if (snap_wg) snap.store(a);
  if (a.fly_count && pendv && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) atomicAdd(a.fly_count, 1ull);
  if constexpr (DIAG) stamp(a.stamps, 1);
  lds_barrier();

  // ---- phase 1: conv + bias + ReLU + 2x2 max-pool; lane = (image fr, position slot fq), wave = 4 channels.
  // Two waves share each SIMD (waves w and w + 4), so neither this VALU stream nor the prologue is issued by a
  // lone wave at half of the SIMD's rate.
  const int c0 = wave * 4;
  ConvW4 cw;
  cw.load(wcs, c0);
  const int p = p0 + fq, b = b0 + fr;
  const bool pok = p < P, bok = b < a.B;
  float out[4];
  if (bok && pok) {
    const int py = p / Wp, px = p - py * Wp;
    uint32_t packed;
    conv_pool4(xr + fr * fwd32_istride(W) + (2 * (py - py0)) * W + 2 * px, W, cw, out, packed);
    // word cg = wave >> 1 of the position holds channels 8cg..8cg+7: this wave stores the half of its 4
    if (a.amax)
      reinterpret_cast<uint32_t*>(a.amax + ((size_t)p * (CC / 8) + (wave >> 1)) * a.lda + b)[wave & 1] = packed;
  } else {
#pragma unroll
    for (int cc = 0; cc < 4; ++cc) out[cc] = 0.f;
  }
  if (pok && Pt && (bok || b < a.ldPt)) {
#pragma unroll
    for (int cc = 0; cc < 4; ++cc) Pt[(size_t)(p * CC + c0 + cc) * a.ldPt + b] = out[cc];
  }
  *reinterpret_cast<float4*>(As + fr * AS32 + fq * CC + c0) = float4{out[0], out[1], out[2], out[3]};
  if constexpr (DIAG) stamp(a.stamps, 2);
  lds_barrier();
  if constexpr (DIAG) stamp(a.stamps, 3);
  if (!mfma_wave) return;   // waves 4-7 end here: every float sum below is the four-wave form's, in its order

  // the fragments of positions past P were loaded from the last position: they count as 0
#pragma unroll
  for (int ks = 0; ks < FG; ++ks)
#pragma unroll
    for (int i = 0; i < 8; ++i) wfr[ks][i] = p0 + ks < P ? wfr[ks][i] : 0.f;
  // ---- phase 2 (waves 0-3): hpre[16 x 64] += As(16 x FG*32) . W1(FG*32 x 64) on the f32 MFMA; wave = column tile nt,
  // one accumulator per position (independent chains keep the pipe issuing), summed before the adds:
  // the FG positions' split-K partial sums meet in registers, not in memory
  // the replica is the group's, wherever its workgroups run: every replica's addends are the same under any map
  float* const hrow = a.hpre + (size_t)(sl.g % a.hrep) * a.hrep_stride;
  f32x4 acc[FG];
#pragma unroll
  for (int ks = 0; ks < FG; ++ks) acc[ks] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    float4 av[FG];
#pragma unroll
    for (int ks = 0; ks < FG; ++ks)
      av[ks] = *reinterpret_cast<const float4*>(As + fr * AS32 + ks * CC + k8_col(fq, i));
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int ks = 0; ks < FG; ++ks) acc[ks] = mfma_f32x4(f4get(av[ks], e), wfr[ks][4 * i + e], acc[ks]);
  }
  // positions past P hold zeros on both sides (out = 0, wfr = 0): they add nothing
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = b0 + fq * 4 + r;
    // summed in position order, the order in which the consumers sum the replicas of the deterministic layout
    const float s = ((acc[0][r] + acc[1][r]) + acc[2][r]) + acc[3][r];
    if (row < a.B) atomicAdd(hrow + (size_t)row * HD + nt * 16 + fr, s);
  }
  if constexpr (DIAG) stamp(a.stamps, 4);
}

// The forward with its stamps (diagnostic runs: a stamp buffer is given) and the production form without them.
// Register budget: allocated as for 4 waves per SIMD, that is at most 128 VGPRs (512-thread bounds alone allow
// 256), so the workgroup's two waves per SIMD fit with room.
#define FWD32_KERNEL __global__ __launch_bounds__(FNT) __attribute__((amdgpu_waves_per_eu(4, 4)))
FWD32_KERNEL void convnet32_fwd_kernel(FwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char fsm[];
  convnet32_fwd_body<true>(a, fsm);
}
FWD32_KERNEL void convnet32_fwd_plain_kernel(FwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char fsm[];
  convnet32_fwd_body<false>(a, fsm);
}

// LDS carve of the backward (bytes)
constexpr int kG32 = 0;                              // f32 [64 b][GS32]   G = dH (A of dP)
constexpr int kGt32 = kG32 + 64 * GS32 * 4;          // f32 [64 u][GS32]   G^T (B of dW1)
constexpr int kW1s32 = kGt32 + 64 * GS32 * 4;        // f32 [32 c][GS32]   W1 rows (B of dP; the update's w)
constexpr int kPts32 = kW1s32 + 32 * GS32 * 4;       // f32 [32 c][GS32]   P^T rows (A of dW1)
constexpr int kXs32 = kPts32 + 32 * GS32 * 4;        // f32 [64 b][16]     4x4 input patches
constexpr int kAm32 = kXs32 + 64 * 16 * 4;           // u8  [64 b][CC]     pool argmax
constexpr int kR32 = kAm32 + 64 * CC;                // head scratch | dP [64][DPS32] | red [NW][16][CC]
constexpr int kRBytes = kHeadScratch > NW * 16 * CC * 4 ? kHeadScratch : NW * 16 * CC * 4;
static_assert(64 * DPS32 * 4 <= kRBytes, "dP exceeds the shared scratch");
constexpr int kW2s32 = kR32 + kRBytes;
constexpr int kB2s32 = kW2s32 + kW2Bytes;
constexpr int kLab32 = kB2s32 + kB2Bytes;
constexpr int kBwd32Lds = kLab32 + kLabBytes;
static_assert(kBwd32Lds <= 160 * 1024, "backward LDS exceeds a CU");

// The thread's indices from an opaque copy of threadIdx.x (opaque_tid(): nothing computed from them is
// kept in registers across the chunk loop).
__device__ __forceinline__ void bwd32_ids(int& tid, int& lane, int& wave, int& fr, int& fq) {
  const int t = opaque_tid();
  tid = t;
  lane = t & 63;
  wave = t >> 6;
  fr = lane & 15;
  fq = lane >> 4;
}

// One image chunk's global operands of a trunk workgroup, in registers.
struct Bwd32Chunk {
  float4 hv;      // hpre row hr, units hc4.. (replicas summed)
  int lab;
  float2 ptv;     // P^T row tid>>5, images 2*(tid&31)..
  float4 xv;      // threads < 256: row tid&3 of the 4x4 patch of image tid>>2
  uint64_t amv;   // threads < 256: argmax bytes of channel group tid>>6, image tid&63
};

// Issues every global load of the chunk before anything waits: straight-line, with indices clamped
// into the chunk (rows past nb read row nb-1, replicas past hrep read replica hrep-1 — never an address
// outside the buffers) and the values of the clamped lanes replaced afterwards.  NREP = replica slots
// (0: the runtime loop of the deterministic mode, after the other loads are in flight).
// Fine stamp 8: the chunk's operands have landed (diagnostic runs only: the wait is inside the branch)
__device__ __forceinline__ void stamp_landed(long long* st, const Bwd32Chunk& c) {
  if (st) {
    asm volatile("" ::"v"(c.hv.x), "v"(c.lab), "v"(c.ptv.x), "v"(c.xv.x), "v"((int)c.amv));
    stamp_fine(st, 8);
  }
}

// Whole chunks (F::kWhole, nb == 64): every index lies in the chunk as it is (the label of thread tid is that of
// image tid & 63; threads < 64 store theirs), so there is no clamp and no select.  F::kRep > 0: exactly NREP replicas.
template <int NREP, class G, class F>
__device__ __forceinline__ void bwd32_chunk_issue(const BwdArgs& a, int tid, int p, int py, int px, int b0, int nb,
                                                  Bwd32Chunk& c) {
  constexpr bool kWhole = F::kWhole;
  const int last = nb - 1;
  const int hrow = b0 + (kWhole ? tid >> 4 : min(tid >> 4, last)), hc4 = (tid & 15) * 4;
  HpreRep<(NREP > 0 ? NREP : 1), (F::kRep > 0)> h;
  if (NREP > 0) h.issue(a, hrow, hc4);
  c.lab = a.labels[b0 + (kWhole ? tid & 63 : min(tid, last))];
  // the pair starts at an even column <= nb-1; ldPt is even and >= B, so its second float is in the row
  const int pc = (tid & 31) * 2;
  c.ptv = *reinterpret_cast<const float2*>(reinterpret_cast<const float*>(a.Pt) + (size_t)(p * CC + (tid >> 5)) * a.ldPt +
                                           b0 + (kWhole ? pc : min(pc, last & ~1)));
  c.xv = float4{0.f, 0.f, 0.f, 0.f};
  c.amv = ~0ull;
  if (tid < 256) {
    const int bl = tid >> 2, r = tid & 3;
    const float2* row = reinterpret_cast<const float2*>(a.x + (size_t)(b0 + (kWhole ? bl : min(bl, last))) * G::H(a) * G::W(a) +
                                                        (2 * py + r) * G::W(a) + 2 * px);
    const float2 u = row[0], t = row[1];
    c.xv = float4{u.x, u.y, t.x, t.y};
    const int cg = tid >> 6, bb = tid & 63;
    c.amv = a.amax[((size_t)p * (CC / 8) + cg) * a.lda + b0 + (kWhole ? bb : min(bb, last))];
  }
  c.hv = NREP > 0 ? h.sum(a) : load_hpre_loop(a, hrow, hc4);   // rows past nb: zeroed by head_stage
  if constexpr (!kWhole) {
    if ((tid >> 2) >= nb) c.xv = float4{0.f, 0.f, 0.f, 0.f};
    if ((tid & 63) >= nb) c.amv = ~0ull;
    if (tid >= nb) c.lab = 0;
    if (pc >= nb) c.ptv.x = 0.f;
    if (pc + 1 >= nb) c.ptv.y = 0.f;
  }
}

// G: the image geometry; F: what else the form knows (tde_convnet.h: BwdForm)
template <int MODE, class G, class F>
__device__ __forceinline__ void convnet32_bwd_body(const BwdArgs& a, unsigned char* smem) {
  float* Gs = reinterpret_cast<float*>(smem + kG32);
  float* Gts = reinterpret_cast<float*>(smem + kGt32);
  float* W1s = reinterpret_cast<float*>(smem + kW1s32);
  float* Pts = reinterpret_cast<float*>(smem + kPts32);
  float* xs = reinterpret_cast<float*>(smem + kXs32);
  uint8_t* am = smem + kAm32;
  float* dps = reinterpret_cast<float*>(smem + kR32);
  const HeadLds hl = HeadLds::carve(smem + kR32, smem + kW2s32, smem + kB2s32, smem + kLab32);
  // MODE 2: the step count, read before the kernel's first store (a scalar load, used only by the epilogue:
  // nothing waits for it here); MODE 1 (SGD) does not read it in the trunk workgroups
  long long t_it = 0;
  if (MODE == 2) t_it = *a.iterations;
  // workgroups of the launch: read once, ahead of the first branch (a scalar load); a constant in the fixed form
  const unsigned nwg = G::kFixed ? ((kGH - 2) / 2) * ((kGW - 2) / 2) + 1 : gridDim.x;
  if constexpr (F::kDiag) {
    stamp(a.stamps, 0);
    stamp_xcc(a.stamps, kXccSlot);
  }
  const int W = G::W(a);
  int tid, lane, wave, fr, fq;
  bwd32_ids(tid, lane, wave, fr, fq);
  const float* W1 = reinterpret_cast<const float*>(a.W1);

  // the head weights into registers now, stored to LDS with the chunk operands below: every global load
  // of the prologue is in flight before the first LDS store (one round trip, not three).  Straight-line:
  // classes past C read class C-1 and store 0.
  float w2v, b2v;
  {
    const int u2 = tid >> 4, c2 = tid & 15;   // 64 x 16
    w2v = a.W2[u2 * a.C + min(c2, a.C - 1)];
    b2v = a.b2[min(c2, a.C - 1)];
  }
  zero_other_parity_n(a, tid, (int)nwg);
  if (blockIdx.x == nwg - 1) {
    hl.w2s[(tid >> 4) * W2S + (tid & 15)] = (tid & 15) < a.C ? w2v : 0.f;
    if (tid < 16) hl.b2s[tid] = tid < a.C ? b2v : 0.f;
    head_workgroup<MODE, true, F>(a, hl, Gs);   // the G area is unused there
    return;
  }

  const int Wp = (W - 2) / 2;
  // one pooled position per workgroup (grid = P + 1), placed by tde_convnet.h: bwd_slot
  const int p = bwd_slot_runs((int)blockIdx.x, a.slot_full);
  const int py = p / Wp, px = p - py * Wp;
  // no Dense(64) bias: the load reads hpre's first row (same alignment) and counts as 0
  const float4 b1v = *reinterpret_cast<const float4*>((a.b1 ? a.b1 : a.hpre) + (tid & 15) * 4);
  // roles: waves 0-7 dP tile (mt = wave>>1 images, ct = wave&1 channels);
  //        waves 8-15 dW1 tile (rt = v>>2 channels, nt = v&3 units), v = wave-8
  f32x4 accw = {0.f, 0.f, 0.f, 0.f};
  f32x4 accr[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};

  // fused step with slots: the dW1-wave's slot values, loaded now (the weights come from W1s)
  f32x4 mp = {0.f, 0.f, 0.f, 0.f}, vp = {0.f, 0.f, 0.f, 0.f};
  if (MODE == 2 && wave >= 8) {
    const int rt = (wave & 7) >> 2, nt = wave & 3;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const size_t e = (size_t)(p * CC + rt * 16 + fq * 4 + r) * HD + nt * 16 + fr;
      if (opt_has_m(a.h.kind)) mp[r] = a.m1[e];
      if (opt_has_v(a.h.kind)) vp[r] = a.v1[e];
    }
  }

  // W1 rows of the position [32][64] f32: loaded once (independent of the image chunk), stored to LDS
  // after the first chunk's loads are issued
  const float2 w1v = *reinterpret_cast<const float2*>(W1 + (size_t)(p * CC + (tid >> 5)) * (G::kFixed ? HD : a.ldw1) + (tid & 31) * 2);

  for (int b0 = 0; b0 < a.B; b0 += 64) {
    const int nb = F::nb(a, b0);   // 64 with whole chunks
    bwd32_ids(tid, lane, wave, fr, fq);
    const bool dw_wave = wave >= 8;
    const int v8 = wave & 7;
    // ---- prologue: this chunk's operands, every load issued before the first wait; the replica count
    // picks the number of hpre registers (the form's own count, or a uniform switch; more than kMaxRep: the
    // deterministic mode)
    Bwd32Chunk ck;
    if constexpr (F::kRep > 0) bwd32_chunk_issue<F::kRep, G, F>(a, tid, p, py, px, b0, nb, ck);
    else if (a.hrep > kMaxRep) bwd32_chunk_issue<0, G, F>(a, tid, p, py, px, b0, nb, ck);
    else switch (a.hrep) {
      case 1: bwd32_chunk_issue<1, G, F>(a, tid, p, py, px, b0, nb, ck); break;
      case 2: bwd32_chunk_issue<2, G, F>(a, tid, p, py, px, b0, nb, ck); break;
      case 3: case 4: bwd32_chunk_issue<4, G, F>(a, tid, p, py, px, b0, nb, ck); break;
      default: bwd32_chunk_issue<8, G, F>(a, tid, p, py, px, b0, nb, ck); break;
    }
    if constexpr (F::kDiag) {
      stamp(a.stamps, 1);
      stamp_landed(a.stamps, ck);
    }
    // ragged chunks: the selects of the clamped chunk-0 loads use this iteration's thread indices: they stay
    // here, behind the chunk's loads, and are not moved up to the loads they would wait for (has_b1: always
    // a.b1 != null).  Whole chunks have no such selects to hold.
    const bool has_b1 = F::kWhole ? a.b1 != nullptr : a.b1 && tid >= 0;
    const float4 b1u = has_b1 ? b1v : float4{0.f, 0.f, 0.f, 0.f};
    if (b0 == 0) {
      hl.w2s[(tid >> 4) * W2S + (tid & 15)] = (tid & 15) < a.C ? w2v : 0.f;
      if (tid < 16) hl.b2s[tid] = tid < a.C ? b2v : 0.f;
      *reinterpret_cast<float2*>(W1s + (tid >> 5) * GS32 + (tid & 31) * 2) = w1v;
    }
    head_stage<F>(a, ck.hv, b1u, tid >> 4, (tid & 15) * 4, nb, hl.hs);
    if (tid < 64) hl.labs[tid] = ck.lab;
    *reinterpret_cast<float2*>(Pts + (tid >> 5) * GS32 + (tid & 31) * 2) = ck.ptv;
    if (tid < 256) {
      const int bl = tid >> 2, r = tid & 3;
      *reinterpret_cast<float4*>(xs + bl * 16 + r * 4) = ck.xv;
      const int cg = tid >> 6, bb = tid & 63;
      *reinterpret_cast<uint64_t*>(am + bb * CC + cg * 8) = ck.amv;
    }
    lds_barrier();
    if constexpr (F::kDiag) stamp_fine(a.stamps, 9);
    // ---- the head recomputed: G = dH (f32) into LDS, row-major and transposed
    {
      float la = 0.f, ca = 0.f, na = 0.f;   // the head workgroup keeps these: not computed here
      head_logits_ce16<false, F>(a, nb, hl, Gs, lane, wave, la, ca, na);   // partial 0 in Gs, free until dH
      if constexpr (F::kDiag) stamp_fine(a.stamps, 11);
      const f32x4 gh = head_dh<F>(a, nb, hl, lane, wave);
      const int rt = wave >> 2, j = (wave & 3) * 16 + fr;
#pragma unroll
      for (int i = 0; i < 4; ++i) Gs[(rt * 16 + fq * 4 + i) * GS32 + j] = gh[i];
      *reinterpret_cast<float4*>(Gts + j * GS32 + rt * 16 + fq * 4) = float4{gh[0], gh[1], gh[2], gh[3]};
      if constexpr (F::kDiag) stamp_fine(a.stamps, 12);
    }
    lds_barrier();
    if constexpr (F::kDiag) stamp(a.stamps, 2);

    // ---- waves 0-7: dP[b][c] = sum_u G[b][u] W1[c][u];  waves 8-15: dW1[c][u] += sum_b P[b][c] G[b][u]
    {
      const float* Ab = dw_wave ? Pts + ((v8 >> 2) * 16 + fr) * GS32 : Gs + ((v8 >> 1) * 16 + fr) * GS32;
      const float* Bb = dw_wave ? Gts + ((v8 & 3) * 16 + fr) * GS32 : W1s + ((v8 & 1) * 16 + fr) * GS32;
      f32x4 acc = dw_wave ? accw : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float4 av = *reinterpret_cast<const float4*>(Ab + k16_col(fq, i));
        const float4 bv = *reinterpret_cast<const float4*>(Bb + k16_col(fq, i));
        acc = mfma_f32x4(av.x, bv.x, acc);
        acc = mfma_f32x4(av.y, bv.y, acc);
        acc = mfma_f32x4(av.z, bv.z, acc);
        acc = mfma_f32x4(av.w, bv.w, acc);
      }
      if (dw_wave) {
        accw = acc;
      } else {
        const int mt = v8 >> 1, ct = v8 & 1;
#pragma unroll
        for (int r = 0; r < 4; ++r) dps[(mt * 16 + fq * 4 + r) * DPS32 + ct * 16 + fr] = acc[r];
      }
    }
    lds_barrier();
    if constexpr (F::kDiag) stamp(a.stamps, 3);

    // ---- routing MFMA: k = (b, q), lane group fq = window slot q; wave takes images 4w..4w+3
    {
      const int tap = fr, ky = tap / 3, kx = tap - ky * 3, qy = fq >> 1, qx = fq & 1;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int bl = wave * 4 + s;
        const float xa = tap < 9 ? xs[bl * 16 + (qy + ky) * 4 + qx + kx] : (tap == 9 ? 1.f : 0.f);
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
          const int c = ct * 16 + fr;
          const float d = am[bl * CC + c] == (unsigned)fq ? dps[bl * DPS32 + c] : 0.f;
          accr[ct] = mfma_f32x4(xa, d, accr[ct]);
        }
      }
    }
    lds_barrier();
  }
  if constexpr (F::kDiag) stamp(a.stamps, 4);

  bwd32_ids(tid, lane, wave, fr, fq);
  const bool dw_wave = wave >= 8;
  const int v8 = wave & 7;
  if (dw_wave) {
    const int rt = v8 >> 2, nt = v8 & 3;
    const int col = nt * 16 + fr;
    if (MODE != 0) {
      // ---- update this position's Dense(64) rows (complete dW1: the rows belong to this workgroup);
      // the weights were staged into W1s before the chunk loop
      const float lr_t = opt_lr_t(a.h, t_it);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = rt * 16 + fq * 4 + r;
        const size_t e = (size_t)(p * CC + row) * HD + col;
        float m = mp[r], v = vp[r];
        a.w1[e] = opt_step(a.h, lr_t, W1s[row * GS32 + col], accw[r], m, v);
        if (MODE == 2 && opt_has_m(a.h.kind)) a.m1[e] = m;
        if (MODE == 2 && opt_has_v(a.h.kind)) a.v1[e] = v;
      }
    } else if (a.push.nranks > 0) {
      // fused DP exchange: this position's complete dW1 rows [32][64] are staged in W1s (free after the
      // chunk loop) and pushed below as one contiguous 8 KB run of float4 stores
#pragma unroll
      for (int r = 0; r < 4; ++r) W1s[(rt * 16 + fq * 4 + r) * GS32 + col] = accw[r];
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) a.dW1[(size_t)(p * CC + rt * 16 + fq * 4 + r) * HD + col] = accw[r];
    }
  }
  conv_grad_reduce(a, accr, dps, lane, wave, p);   // its barrier also publishes the W1s staging
  if (MODE == 0 && a.push.nranks > 0 && tid < CC * HD / 4) {
    // the rows go straight into the owners' contribution areas of the all-reduce call that follows this
    // launch (its parity from the completed-calls count); the bucket offset is a multiple of 4 (host check)
    const int parity = (int)((*a.push.epoch + 1u) & 1u);
    const int row = tid >> 4, c4 = (tid & 15) * 4;
    xg_push_store4(a.push, parity, a.push.off + (long long)(p * CC + row) * HD + c4,
                   *reinterpret_cast<const float4*>(W1s + row * GS32 + c4));
    xg_push_drain();   // acknowledged before the wave ends
  }
  if constexpr (F::kDiag) stamp(a.stamps, 5);
}

// The general form (runtime geometry and counts, stamps: every call the production form does not take) and
// the production form
// The production form of the backward: no diagnostics, whole chunks, the 4 hpre replicas train/program.py uses by
// default
using ProdForm = BwdForm<false, true, 4>;
template <int MODE>
__global__ __launch_bounds__(1024) void convnet32_bwd_kernel(BwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  convnet32_bwd_body<MODE, Geo<0, 0>, BwdFormAny>(a, smem);
}
template <int MODE>
__global__ __launch_bounds__(1024) void convnet32g_bwd_kernel(BwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  convnet32_bwd_body<MODE, Geo<kGH, kGW>, ProdForm>(a, smem);
}

}  // namespace tde

using namespace tde;
using namespace tde::cnet;

// The form the backward's entry point launches: the production kernels for calls that meet every condition of
// prod_form(), the general ones for every other call.  tde_convnet_f32_runtime_geom(1) forces the general form
// for every call (the tests compare the two forms on the same inputs); it returns the previous setting.
static int g_runtime_geom = 0;
static bool geom_fixed(int H, int W) { return !g_runtime_geom && H == kGH && W == kGW; }
static bool prod_form(const BwdArgs& a) {
  return geom_fixed(a.H, a.W) && !a.stamps && a.B > 0 && a.B % 64 == 0 && a.hrep == ProdForm::kRep;
}
TDE_API int tde_convnet_f32_runtime_geom(int on) {
  const int prev = g_runtime_geom;
  g_runtime_geom = on ? 1 : 0;
  return prev;
}

// The placement maps of both launches (tde_convnet.h: fwd_slot, bwd_slot).  tde_convnet_f32_identity_slots(1)
// forces the identity maps (forward: group fastest, backward: position = id) for every call, for tests and A/B
// timing; it returns the previous setting.
static int g_identity_slots = 0;
static int fwd_full_runs(int groups) { return g_identity_slots ? 0 : groups / 8; }
static int bwd_full_runs(int P) { return g_identity_slots ? 0 : P / 32; }
TDE_API int tde_convnet_f32_identity_slots(int on) {
  const int prev = g_identity_slots;
  g_identity_slots = on ? 1 : 0;
  return prev;
}
// The whole map in effect, for checks without a GPU.  kind 0: the forward's, a = groups, b = tiles,
// out[2 id] = group, out[2 id + 1] = tile of workgroup id < a * b; kind 1: the backward's, a = P,
// out[id] = position of workgroup id < P (the head workgroup, id P, is not mapped).  Returns the workgroup count.
TDE_API int tde_convnet_slot_map(int kind, int a, int b, int* out) {
  if (!out || a < 1 || (kind == 0 && b < 1) || (kind != 0 && kind != 1)) return -1;
  if (kind == 0) {
    for (int id = 0; id < a * b; ++id) {
      const FwdSlot s = fwd_slot_runs(id, a, b, fwd_full_runs(a));
      out[2 * id] = s.g;
      out[2 * id + 1] = s.y;
    }
    return a * b;
  }
  for (int id = 0; id < a; ++id) out[id] = bwd_slot_runs(id, bwd_full_runs(a));
  return a;
}

// Float32 forward: W1 is the f32 master Dense(64) kernel [K][64] (ldw1 = 64), Pt f32 [K][ldPt].
// opt / off_wc / off_bc / inc_iter / hrep as tde_convnet_fwd.
TDE_API int tde_convnet_fwd_f32(const float* x, const float* wc, const float* bc, const float* W1, int ldw1,
                                float* hpre, float* Pt, int ldPt, void* amax, int lda, int B, int H, int W,
                                long long* stamps, const TdeStepOpt* opt, long long off_wc, long long off_bc,
                                long long* inc_iter, int hrep, long long hrep_stride, hipStream_t stream) {
  if ((W & 3) || W > XW || ((W - 2) / 2) < 4 || ldw1 != HD || (Pt && (ldPt & 7)) || (amax && lda < B)) return -1;
  if (((uintptr_t)wc | (uintptr_t)bc | (uintptr_t)W1) & 15) return -2;
  if (opt && (!opt_ok(opt) || !opt->pend)) return -4;
  const int P = ((H - 2) / 2) * ((W - 2) / 2);
  // image tiles: the padding columns B <= b < ldPt of Pt are written too (as zeros)
  const int by = ((Pt && ldPt > B ? ldPt : B) + FB - 1) / FB;
  FwdArgs a{x, wc, bc, W1, ldw1, hpre, Pt, ldPt, (uint64_t*)amax, lda, B, H, W, stamps};
  fill_fwd_opt(a, opt, off_wc, off_bc, inc_iter, hrep, hrep_stride);
  a.groups = (P + FG - 1) / FG;
  a.tiles = by;
  a.slot_full = fwd_full_runs(a.groups);
  const dim3 grid(a.groups * a.tiles);
  if (stamps) convnet32_fwd_kernel<<<grid, FNT, kFwd32Lds, stream>>>(a);
  else convnet32_fwd_plain_kernel<<<grid, FNT, kFwd32Lds, stream>>>(a);
  TDE_LAUNCH_CHECK();
  return 0;
}

// Float32 backward: W1 = the f32 master [K][64] (ldw1 = 64; in the fused step the same memory as
// opt->w + opt->off_w1), Pt f32.  Other arguments as tde_convnet_bwd (opt->W1c is ignored).
TDE_API int tde_convnet_bwd_f32(const float* x, const void* amax, int lda, const float* hpre, float* hzero,
                                int hrep, long long hrep_stride, const float* b1, const float* W2, const float* b2,
                                int C, int pre_relu, const int* labels, float scale, float* metrics, const float* W1,
                                int ldw1, const float* Pt, int ldPt, float* dW1, float* dwc, float* dbc, float* dW2,
                                float* db2, float* db1, int B, int H, int W, long long* stamps, const TdeBwdOpt* opt,
                                float* cpart, const XgPush* push, int crep, long long crep_stride,
                                hipStream_t stream) {
  if (ldw1 != HD || ((uintptr_t)W1 & 15) || ((uintptr_t)Pt & 7)) return -1;
  if (push && push->nranks > 0 &&
      (opt || push->nranks > kXgMaxRanks || push->L <= 0 || (push->L & 3) || (push->off & 3) || !push->epoch))
    return -7;
  if (opt && opt->w + opt->off_w1 != W1) return -3;   // the update is applied to the rows it reads
  BwdArgs a;
  const int rc = fill_bwd(a, x, amax, lda, hpre, hzero, hrep, hrep_stride, b1, W2, b2, C, pre_relu, labels, scale,
                          metrics, W1, ldw1, Pt, ldPt, dW1, dwc, dbc, dW2, db2, db1, B, H, W, stamps, opt);
  if (rc) return rc;
  a.cpart = cpart;
  a.w1r_out = nullptr;
  a.w1c_out = nullptr;
  if (push) a.push = *push;
  if (!opt && crep > 1) {   // data-parallel step: conv-gradient replicas summed by the all-reduce
    a.crep = crep;
    a.crep_stride = crep_stride;
  }
  const int P = ((H - 2) / 2) * ((W - 2) / 2);
  a.slot_full = bwd_full_runs(P);
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)convnet32_bwd_kernel<0>, hipFuncAttributeMaxDynamicSharedMemorySize, kBwd32Lds);
    (void)hipFuncSetAttribute((const void*)convnet32_bwd_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, kBwd32Lds);
    (void)hipFuncSetAttribute((const void*)convnet32_bwd_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, kBwd32Lds);
    (void)hipFuncSetAttribute((const void*)convnet32g_bwd_kernel<0>, hipFuncAttributeMaxDynamicSharedMemorySize, kBwd32Lds);
    (void)hipFuncSetAttribute((const void*)convnet32g_bwd_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, kBwd32Lds);
    (void)hipFuncSetAttribute((const void*)convnet32g_bwd_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, kBwd32Lds);
    attr_set = true;
  }
  const dim3 grid(P + 1);   // one workgroup per pooled position + the head workgroup
  const int mode = !opt ? 0 : (opt->h.kind == kOptSGD ? 1 : 2);
  if (prod_form(a)) {
    if (mode == 0) convnet32g_bwd_kernel<0><<<grid, 1024, kBwd32Lds, stream>>>(a);
    else if (mode == 1) convnet32g_bwd_kernel<1><<<grid, 1024, kBwd32Lds, stream>>>(a);
    else convnet32g_bwd_kernel<2><<<grid, 1024, kBwd32Lds, stream>>>(a);
  } else {
    if (mode == 0) convnet32_bwd_kernel<0><<<grid, 1024, kBwd32Lds, stream>>>(a);
    else if (mode == 1) convnet32_bwd_kernel<1><<<grid, 1024, kBwd32Lds, stream>>>(a);
    else convnet32_bwd_kernel<2><<<grid, 1024, kBwd32Lds, stream>>>(a);
  }
  TDE_LAUNCH_CHECK();
  return 0;
}

// Sizes of the ctypes-mirrored fused-step structs (tests/test_abi.py checks the Python mirrors in
// ops/kernels.py against them): out = {TdeStepOpt, TdeBwdOpt, FlatApply, OptHyper}.
TDE_API int tde_cnet_abi_sizes(long long* out, int n) {
  const long long s[] = {(long long)sizeof(TdeStepOpt), (long long)sizeof(TdeBwdOpt), (long long)sizeof(FlatApply),
                         (long long)sizeof(OptHyper)};
  for (int i = 0; i < n && i < 4; ++i) out[i] = s[i];
  return 4;
}
