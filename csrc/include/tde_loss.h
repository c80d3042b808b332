// The softmax cross-entropy head with label smoothing and per-class row weights (Keras
// CategoricalCrossentropy(label_smoothing=), fit(class_weight=)), shared by the layer-wise plan's loss launch
// (losshead.hip) and the small-net step's loss variant (smallnet.hip).  For a row with integer label y over C
// classes, smoothing e and weight w = class_w[y]:
//
//   t_c      = (1 - e) [c == y] + e / C
//   loss     = w ((1 - e) (lse - l_y) + e (lse - mean_c l_c)),   lse = max + log sum exp(l - max)
//   dlogit_c = w (p_c - t_c) scale
//
// A label outside [0, C) has weight 1, l_y := max and no one-hot term, as the plain kernels treat it.  The
// weight is not part of the metrics' row count: the reported loss is sum w_i l_i / rows.
//
// With e = 0 and every weight 1 each added term is an exact *1, +0 or -0/C, so the results are those of the plain
// kernels bit for bit (the callers keep the plain kernels' order of operations around these helpers).
#pragma once
#include "tde_common.h"

namespace tde {

struct LossSpec {
  float smooth;          // label smoothing e in [0, 1)
  int has_cw;            // class_w is read
  const float* class_w;  // [C] row weight by class (device memory; the plan rewrites it in place), or null
};

inline bool loss_spec_ok(const LossSpec& ls) {
  return ls.smooth >= 0.f && ls.smooth < 1.f && (!ls.has_cw || ls.class_w);
}

// The row's weight: one load.
__device__ __forceinline__ float loss_row_weight(const LossSpec& ls, int y, int C) {
  return (ls.has_cw && y >= 0 && y < C) ? ls.class_w[y] : 1.f;
}

// The row's loss from nll = lse - l_y and sl = sum_c l_c.
__device__ __forceinline__ float loss_row(const LossSpec& ls, float w, float lse, float nll, float sl, int C) {
  return w * ((1.f - ls.smooth) * nll + ls.smooth * (lse - sl / (float)C));
}

// The target t_c of class c (hit: c == y).
__device__ __forceinline__ float loss_target(const LossSpec& ls, bool hit, int C) {
  return (1.f - ls.smooth) * (hit ? 1.f : 0.f) + ls.smooth / (float)C;
}

// The gradient element from the probability p.
__device__ __forceinline__ float loss_dlogit(float w, float p, float t, float scale) {
  return w * (p - t) * scale;
}

}  // namespace tde
