// Weight regularizers (Keras kernel_regularizer / bias_regularizer / gamma_regularizer / beta_regularizer:
// l1, l2, l1_l2) and decoupled weight decay (Keras 2.11+ weight_decay, AdamW) on the device, shared by the
// regularizer launches (weightreg.hip) and the WD variants of the multi-tensor optimizer (optim.hip).
//
//   penalty of a variable   P = l1 * sum|w| + l2 * sum w^2             (added to the reported loss)
//   its gradient            g <- g + (2 l2 w + l1 sgn(w)), sgn(+-0) = 0  (the aggregated gradient, before a clip)
//   weight decay            w <- w - (w * wd) * lr                       (before the step; lr: this step's rate)
//
// Two launches on the step's stream in front of the norm launches of a clip (gradclip.hip): the gradient and
// the penalty partials (one workgroup per 4096-element chunk of a regularized segment), then the finish (one
// workgroup: partials -> penalty, metrics[0] += rows * penalty).  The decay needs no launch of its own: the WD
// variant of the apply reads wd[seg] as it reads a scheduled rate through lr_ptr.
#pragma once
#include "tde_clip.h"

namespace tde {

// Coefficients of one segment, parallel to the OptSeg array; {0, 0}: not regularized (no table entry).
struct RegCoef {
  float l1, l2;
};

constexpr int kRegChunk = kClipChunk;   // elements per workgroup: 256 threads x 4 float4

inline bool reg_coef_ok(float c) { return c >= 0.f && c <= 3.402823466e+38f; }   // not negative, finite, not NaN

}  // namespace tde
