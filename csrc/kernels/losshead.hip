// Softmax cross-entropy with label smoothing and per-class row weights for the layer-wise plan
// (csrc/include/tde_loss.h): the launch that takes the place of xent32_kernel (layers_f32.hip) / xent_kernel
// (layers.hip) when the loss has a non-trivial spec.  Same contract as those: one wave per row, four rows per
// 256-thread workgroup, any C by a lane-strided loop (bf16: over registers up to 1024 classes), lowest-index argmax, metrics[0..2] += (loss sum, correct,
// rows), `iterations` advanced by block 0, probabilities (or the logits) for predict.
//
// DT is the dlogits type and with it the plain kernel this one shadows: float keeps xent32_kernel's arithmetic
// (expf / logf, the block's partials summed pairwise), bf16 keeps xent_kernel's (__expf / __logf, summed left to
// right), so that smoothing 0 with all-ones weights gives either kernel's results bit for bit.  sum_c l_c rides
// the pass that computes sum exp; the weight is one class_w[y] load per row.
#include <type_traits>

#include "tde_common.h"
#include "tde_loss.h"

namespace tde {

struct XentSpecArgs {
  const float* logits;
  long long ldl;
  const int* labels;
  int B, C;
  float scale;
  void* dlogits;  // [B][ldd] DT, w (softmax - target) scale, or null
  long long ldd;
  float* metrics;  // [4] weighted loss sum, correct, rows, 0
  float* probs;    // [B][C] softmax (or logits copy when probs_are_logits)
  int probs_are_logits;
  long long* iterations;
  LossSpec ls;
};

// NV (bf16 only): xent_kernel's two forms -- NV > 0: C <= 64 * NV, the row is loaded into registers once and the
// passes run on registers; NV = 0 re-reads the row per pass (any C).  The float kernel is xent32_kernel's plain
// lane-strided loop (NV = 0).  Each branch writes its passes the way the kernel it shadows writes them.
template <typename DT, int NV>
__global__ __launch_bounds__(256) void xent_spec_kernel(XentSpecArgs a) {
  constexpr bool kF32 = std::is_same<DT, float>::value;
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  __shared__ float part[4][2];
  float loss = 0.f, corr = 0.f;
  const bool ok = row < a.B;
  if (ok) {
    const float* l = a.logits + (long long)row * a.ldl;
    const int C = a.C;
    DT* dl = a.dlogits ? reinterpret_cast<DT*>(a.dlogits) + (long long)row * a.ldd : nullptr;
    if constexpr (kF32) {
      float mx = -INFINITY;
      int am = 0x7fffffff;
      for (int c = lane; c < C; c += 64)
        if (l[c] > mx) {
          mx = l[c];
          am = c;
        }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float om = __shfl_xor(mx, o, 64);
        const int oi = __shfl_xor(am, o, 64);
        if (om > mx || (om == mx && oi < am)) {
          mx = om;
          am = oi;
        }
      }
      float se = 0.f, sl = 0.f;
      for (int c = lane; c < C; c += 64) {
        se += expf(l[c] - mx);
        sl += l[c];
      }
      se = wave_sum(se);
      sl = wave_sum(sl);
      const int y = a.labels[row];
      const float w = loss_row_weight(a.ls, y, C);
      const float lse = mx + logf(se);
      const float ly = (y >= 0 && y < C) ? l[y] : mx;
      loss = loss_row(a.ls, w, lse, lse - ly, sl, C);
      corr = (am == y) ? 1.f : 0.f;
      const float inv = 1.f / se;
      for (int c = lane; c < C; c += 64) {
        const float pr = expf(l[c] - mx) * inv;
        if (dl) dl[c] = loss_dlogit(w, pr, loss_target(a.ls, c == y, C), a.scale);
        if (a.probs) a.probs[(long long)row * C + c] = a.probs_are_logits ? l[c] : pr;
      }
    } else {
      float rv[NV > 0 ? NV : 1];
      if constexpr (NV > 0) {
#pragma unroll
        for (int j = 0; j < NV; ++j) rv[j] = lane + 64 * j < a.C ? l[lane + 64 * j] : -INFINITY;
      }
      auto lv = [&](int j, int c) -> float {
        if constexpr (NV > 0) return rv[j];
        else return l[c];
      };
      const int nit = NV > 0 ? NV : (a.C + 63) / 64;
      float mx = -INFINITY;
      int am = 0x7fffffff;
#pragma unroll
      for (int j = 0; j < nit; ++j) {
        const int c = lane + 64 * j;
        if (c >= a.C) continue;
        const float v = lv(j, c);
        if (v > mx) {
          mx = v;
          am = c;
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float om = __shfl_xor(mx, o, 64);
        const int oi = __shfl_xor(am, o, 64);
        if (om > mx || (om == mx && oi < am)) {
          mx = om;
          am = oi;
        }
      }
      float se = 0.f, sl = 0.f;
#pragma unroll
      for (int j = 0; j < nit; ++j) {
        const int c = lane + 64 * j;
        if (c < a.C) {
          se += __expf(lv(j, c) - mx);
          sl += lv(j, c);
        }
      }
      se = wave_sum(se);
      sl = wave_sum(sl);
      const int y = a.labels[row];
      const float w = loss_row_weight(a.ls, y, C);
      const float lse = mx + __logf(se);
      const float ly = (y >= 0 && y < a.C) ? l[y] : mx;
      loss = loss_row(a.ls, w, lse, lse - ly, sl, C);
      corr = (am == y) ? 1.f : 0.f;
      const float inv = 1.f / se;
#pragma unroll
      for (int j = 0; j < nit; ++j) {
        const int c = lane + 64 * j;
        if (c >= a.C) continue;
        const float x = lv(j, c);
        const float p = __expf(x - mx) * inv;
        if (dl) dl[c] = f2bf(loss_dlogit(w, p, loss_target(a.ls, c == y, C), a.scale));
        if (a.probs) a.probs[(long long)row * a.C + c] = a.probs_are_logits ? x : p;
      }
    }
  }
  if (lane == 0) {
    part[threadIdx.x >> 6][0] = ok ? loss : 0.f;
    part[threadIdx.x >> 6][1] = ok ? corr : 0.f;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (a.metrics) {
      const float ls = kF32 ? (part[0][0] + part[1][0]) + (part[2][0] + part[3][0])
                            : part[0][0] + part[1][0] + part[2][0] + part[3][0];
      const float cs = kF32 ? (part[0][1] + part[1][1]) + (part[2][1] + part[3][1])
                            : part[0][1] + part[1][1] + part[2][1] + part[3][1];
      atomicAdd(&a.metrics[0], ls);
      atomicAdd(&a.metrics[1], cs);
      atomicAdd(&a.metrics[2], (float)min(4, a.B - (int)blockIdx.x * 4));
    }
    if (a.iterations && blockIdx.x == 0) *a.iterations += 1;
  }
}

}  // namespace tde

using namespace tde;

// logits [B][ldl] f32, labels [B] int32.  dl_bf16: dlogits is bf16 [B][ldd] (else f32); the arithmetic follows
// (see above).  smooth in [0, 1); class_w: [C] device floats or null (every weight 1).  A bad spec or shape
// returns -1.
TDE_API int tde_xent_spec(const float* logits, long long ldl, const int* labels, int B, int C, float scale,
                          void* dlogits, long long ldd, int dl_bf16, float* metrics, float* probs,
                          int probs_are_logits, long long* iterations, float smooth, const float* class_w,
                          hipStream_t stream) {
  if (B <= 0) return 0;
  const LossSpec ls{smooth, class_w != nullptr, class_w};
  if (!logits || !labels || C < 1 || ldl < C || (dlogits && ldd < C) || !loss_spec_ok(ls)) return -1;
  XentSpecArgs a{logits, ldl, labels, B, C, scale, dlogits, ldd, metrics, probs, probs_are_logits, iterations, ls};
  if (!dl_bf16) xent_spec_kernel<float, 0><<<(B + 3) / 4, 256, 0, stream>>>(a);
  else if (C <= 64 * 16) xent_spec_kernel<bf16, 16><<<(B + 3) / 4, 256, 0, stream>>>(a);
  else xent_spec_kernel<bf16, 0><<<(B + 3) / 4, 256, 0, stream>>>(a);
  TDE_LAUNCH_CHECK();
  return 0;
}
