// Gradient clipping on the device (Keras clipvalue / clipnorm / global_clipnorm), shared by the norm
// launches (gradclip.hip) and the clipped variants of the multi-tensor optimizer (optim.hip).
//
//   clipvalue = c         g <- min(max(g, -c), c)                  (no norm launch)
//   clipnorm = c          g <- g * (c / max(||g||_2, c))           one norm per variable
//   global_clipnorm = c   the same with one norm over all trainable variables
//
// Three launches on the step's stream: sum-of-squares partials (one workgroup per 4096-element chunk of a
// segment), the scale (one workgroup: partials -> norm, scale), the clipped apply, which reads the scale
// through a pointer as it reads a scheduled rate through lr_ptr.  A zero gradient gives scale 1 exactly.
#pragma once
#include "tde_common.h"

namespace tde {

// One trainable variable of the flat buffers (the multi-tensor optimizer's segment descriptor).
struct OptSeg {
  long long off;      // element offset in the flat buffers (a multiple of 64: 256-byte aligned)
  int rows, cols;     // logical 2-D shape (rows*cols elements)
  long long sh_off;   // bf16 row-major shadow offset or -1
  long long sht_off;  // bf16 transposed shadow offset or -1 (tiled blocks)
};

enum { kClipNone = 0, kClipValue = 1, kClipNorm = 2, kClipGlobalNorm = 3 };

constexpr int kClipChunk = 4096;   // elements per sum-of-squares workgroup: 256 threads x 4 float4

inline bool clip_mode_known(int mode) { return mode >= kClipValue && mode <= kClipGlobalNorm; }
inline bool clip_c_ok(float c) { return c > 0.f && c <= 3.402823466e+38f; }   // positive, finite, not NaN

}  // namespace tde
