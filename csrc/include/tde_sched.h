// Learning-rate schedules evaluated on the device (optimizers.schedules; tf.keras.optimizers.schedules of
// TF 2.x): a pure function of the device-resident step counter, so a step captured once into a hipGraph
// follows the schedule on every replay, and the rate may change between two steps of one replay.
//
// Step convention (Keras): the update that is the k-th ever applied (k = 0 for the first) uses sched_lr(s, k).
// The step kernels advance `iterations` before the optimizer runs (Adam reads t = iterations), so every
// device site passes `*iterations - 1`; ReferencePlan.apply passes the pre-increment value, which is k.
//
// Arithmetic is float32 on (float)step, as TensorFlow's own schedules compute, with the accurate powf /
// cosf / floorf / ceilf; the piecewise search compares 64-bit integers.  A negative step is treated as 0.
#pragma once
#include "tde_common.h"

namespace tde {

enum { kSchedNone = 0, kSchedExponential = 1, kSchedInverseTime = 2, kSchedPolynomial = 3, kSchedCosine = 4,
       kSchedPiecewise = 5 };
enum { kSchedStaircase = 1, kSchedCycle = 2 };   // LrSched::flags
constexpr int kSchedMaxBounds = 8;

// Passed by value (ctypes: ops/kernels.py LrSched).  p: exponential / inverse time {decay_rate}, polynomial
// {end_learning_rate, power}, cosine {alpha}.  Piecewise: val[i] while step <= bound[i], val[nb] beyond.
struct LrSched {
  int kind;    // 0: no schedule
  int flags;
  float lr0;
  float p[3];
  long long decay_steps;
  int nb;
  long long bound[kSchedMaxBounds];
  float val[kSchedMaxBounds + 1];
};

// Entry points: a descriptor the device function can evaluate.
inline bool sched_ok(const LrSched& s) {
  if (s.kind < kSchedExponential || s.kind > kSchedPiecewise) return false;
  if (s.kind == kSchedPiecewise) return s.nb >= 0 && s.nb <= kSchedMaxBounds;
  return s.decay_steps > 0;
}

__device__ __forceinline__ float sched_lr(const LrSched& s, long long step) {
  if (step < 0) step = 0;
  if (s.kind == kSchedPiecewise) {
    // at most 8 compares, no early exit: the last i with step > bound[i - 1] wins
    float v = s.val[0];
#pragma unroll
    for (int i = 0; i < kSchedMaxBounds; ++i)
      if (i < s.nb && step > s.bound[i]) v = s.val[i + 1];
    return v;
  }
  const float ds = (float)s.decay_steps;
  if (s.kind == kSchedExponential || s.kind == kSchedInverseTime) {
    float p = (float)step / ds;
    if (s.flags & kSchedStaircase) p = floorf(p);
    return s.kind == kSchedExponential ? s.lr0 * powf(s.p[0], p) : s.lr0 / (1.f + s.p[0] * p);
  }
  if (s.kind == kSchedPolynomial) {
    float st = (float)step, d = ds;
    if (s.flags & kSchedCycle) d = ds * fmaxf(1.f, ceilf(st / ds));
    else st = fminf(st, ds);
    return (s.lr0 - s.p[0]) * powf(1.f - st / d, s.p[1]) + s.p[0];
  }
  if (s.kind == kSchedCosine) {
    const float c = 0.5f * (1.f + cosf(3.14159265358979323846f * (fminf((float)step, ds) / ds)));
    return s.lr0 * ((1.f - s.p[0]) * c + s.p[0]);
  }
  return s.lr0;
}

}  // namespace tde
