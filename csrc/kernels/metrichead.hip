// The metric launch of the layer-wise plan (csrc/include/tde_metric.h): top-k hits, crossentropy sums and the
// confusion block of a batch of logits, added to the plan's second accumulator.  It runs behind the softmax-CE
// launch (xent32_kernel / xent_kernel / xent_spec_kernel) on the same f32 logits buffer, float32 and bfloat16
// policy alike, and has xent32_kernel's shape: one wave per row, four rows per 256-thread workgroup, any C by
// lane-strided loops, its arithmetic (expf / logf, the four rows' partials summed pairwise).  The four rows'
// hits and sums meet in LDS, so a workgroup issues one atomic per word; the confusion block gets one atomic per
// valid row.  Neither `iterations` nor metrics[0..2] are touched: the rows are counted by the loss launch.
#include "tde_common.h"
#include "tde_metric.h"

namespace tde {

constexpr int kMetricWords = kMetricTopK + kMetricCe;

struct MetricRowsArgs {
  const float* logits;
  long long ldl;
  const int* labels;
  int B, C;
  float* ext;
  MetricSpec ms;
};

__global__ __launch_bounds__(256) void metric_rows_kernel(MetricRowsArgs a) {
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  const int row = blockIdx.x * 4 + wv;
  __shared__ float part[4][kMetricWords];
  float hit[kMetricTopK] = {0.f, 0.f, 0.f, 0.f};
  float ce[kMetricCe] = {0.f, 0.f};
  if (row < a.B) {
    const float* l = a.logits + (long long)row * a.ldl;
    const int C = a.C;
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
    const int y = a.labels[row];
    const bool valid = y >= 0 && y < C;
    const float ly = valid ? l[y] : mx;
    if (a.ms.n_topk > 0) {
      const float rank = metric_rank(l, C, ly, lane);
#pragma unroll
      for (int i = 0; i < kMetricTopK; ++i)
        if (i < a.ms.n_topk) hit[i] = metric_topk_hit(valid, ly, rank, a.ms.k[i]);
    }
    if (a.ms.n_ce > 0) {
      float se = 0.f, sl = 0.f;
      for (int c = lane; c < C; c += 64) {
        se += expf(l[c] - mx);
        sl += l[c];
      }
      se = wave_sum(se);
      sl = wave_sum(sl);
      const float lse = mx + logf(se);
#pragma unroll
      for (int i = 0; i < kMetricCe; ++i)
        if (i < a.ms.n_ce) ce[i] = metric_ce_row(a.ms.smooth[i], lse, ly, sl, C);
    }
    if (a.ms.cm && lane == 0) metric_cm_add(a.ext, a.ms, y, am, C);
  }
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < kMetricTopK; ++i) part[wv][i] = hit[i];
#pragma unroll
    for (int i = 0; i < kMetricCe; ++i) part[wv][kMetricTopK + i] = ce[i];
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t < kMetricWords) {
    const float s = (part[0][t] + part[1][t]) + (part[2][t] + part[3][t]);
    if (t < kMetricTopK) {
      if (t < a.ms.n_topk) atomicAdd(&a.ext[a.ms.off_topk + t], s);
    } else if (t - kMetricTopK < a.ms.n_ce) {
      atomicAdd(&a.ext[a.ms.off_ce + t - kMetricTopK], s);
    }
  }
}

}  // namespace tde

using namespace tde;

// logits [B][ldl] f32, labels [B] int32, spec: a MetricSpec whose layout is that of C classes, ext: spec->words
// floats.  A bad spec or shape returns -1.
TDE_API int tde_metric_rows(const float* logits, long long ldl, const int* labels, int B, int C, const void* spec,
                            float* ext, hipStream_t stream) {
  if (!spec || !logits || !labels || !ext || B < 0 || C < 1 || ldl < C) return -1;
  const MetricSpec ms = *(const MetricSpec*)spec;
  if (!metric_spec_ok(ms, C)) return -1;
  if (B == 0) return 0;
  MetricRowsArgs a{logits, ldl, labels, B, C, ext, ms};
  metric_rows_kernel<<<(B + 3) / 4, 256, 0, stream>>>(a);
  TDE_LAUNCH_CHECK();
  return 0;
}

// sizeof(MetricSpec) and the limits, for the host's ABI check: out[0..3] = size, top-k entries, crossentropy
// entries, classes of the confusion block.
TDE_API int tde_metric_abi(long long* out, int n) {
  const long long v[4] = {(long long)sizeof(MetricSpec), kMetricTopK, kMetricCe, kMetricCmClasses};
  for (int i = 0; i < n && i < 4; ++i) out[i] = v[i];
  return 4;
}
