// Classification metrics beyond the accuracy (Keras top-k accuracy, crossentropy as a metric, F-score), shared
// by the layer-wise plan's metric launch (metrichead.hip) and the small-net step's metric variant (smallnet.hip).
// A plan compiled with such metrics owns a second float32 accumulator, `ext`, beside metrics[4]; MetricSpec
// says what it holds.  For a row with integer label y over C classes and logits l:
//
//   top-k hit   = 0 <= y < C  and  l_y finite  and  #{c : l_c > l_y} < k        (tf.math.in_top_k: classes tied
//                 across the boundary all count)                                 -> ext[off_topk + i] += hit
//   crossentropy = (1 - e) (lse - l_y) + e (lse - mean_c l_c), unweighted         -> ext[off_ce + i]   += ce
//                 (a label outside [0, C): l_y := max, as the loss kernels treat it)
//   confusion    cm[y][argmax] += 1 for 0 <= y < C (lowest-index argmax)          -> ext[off_cm + y C + argmax]
//
// Hits and confusion entries are integers held in f32: exact in any atomic order below 2^24 rows between resets,
// the limit metrics[2] (the rows, the denominator of every mean here) already has.
#pragma once
#include "tde_common.h"

namespace tde {

constexpr int kMetricTopK = 4;          // top-k entries
constexpr int kMetricCe = 2;            // crossentropy entries
constexpr int kMetricCmClasses = 1024;  // the confusion block is C x C words: C up to here

// Passed by pointer from the host (ctypes: ops/metric_ops.py MetricSpec).  The parts lie in this order without
// gaps; the offsets are carried so that every reader indexes the same way.
struct MetricSpec {
  int n_topk;
  int k[kMetricTopK];
  int n_ce;
  float smooth[kMetricCe];  // label smoothing e in [0, 1) of each crossentropy entry
  int cm;                   // 1: the C x C confusion block is kept
  int off_topk, off_ce, off_cm;
  int words;                // floats of ext in all
};

// The host check: counts in range, every k >= 1, every e in [0, 1), the canonical layout for C classes.
inline bool metric_spec_ok(const MetricSpec& m, int C) {
  if (C < 1 || m.n_topk < 0 || m.n_topk > kMetricTopK || m.n_ce < 0 || m.n_ce > kMetricCe) return false;
  if (m.cm != 0 && m.cm != 1) return false;
  if (m.cm && C > kMetricCmClasses) return false;
  if (m.n_topk + m.n_ce + m.cm == 0) return false;
  for (int i = 0; i < m.n_topk; ++i)
    if (m.k[i] < 1) return false;
  for (int i = 0; i < m.n_ce; ++i)
    if (!(m.smooth[i] >= 0.f && m.smooth[i] < 1.f)) return false;
  return m.off_topk == 0 && m.off_ce == m.n_topk && m.off_cm == m.n_topk + m.n_ce &&
         m.words == m.off_cm + (m.cm ? C * C : 0);
}

// #{c : l_c > ly} over the row, any C: a lane-strided count and a wave sum (every lane gets it; a count below
// 2^24 is exact in f32).  A NaN on either side compares false.
__device__ __forceinline__ float metric_rank(const float* l, int C, float ly, int lane) {
  float n = 0.f;
  for (int c = lane; c < C; c += 64) n += l[c] > ly ? 1.f : 0.f;
  return wave_sum(n);
}

__device__ __forceinline__ float metric_topk_hit(bool valid, float ly, float rank, int k) {
  return (valid && isfinite(ly) && rank < (float)k) ? 1.f : 0.f;
}

// The row's smoothed negative log-likelihood from lse, l_y and sl = sum_c l_c (e = 0 never reads sl).
__device__ __forceinline__ float metric_ce_row(float smooth, float lse, float ly, float sl, int C) {
  const float nll = lse - ly;
  return smooth == 0.f ? nll : (1.f - smooth) * nll + smooth * (lse - sl / (float)C);
}

// cm[y][am] += 1: one atomic per valid row (am is out of range when no logit compares greater than -inf).
__device__ __forceinline__ void metric_cm_add(float* ext, const MetricSpec& m, int y, int am, int C) {
  if (y >= 0 && y < C && am >= 0 && am < C) atomicAdd(&ext[m.off_cm + y * C + am], 1.f);
}

}  // namespace tde
