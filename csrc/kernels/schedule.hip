// The learning-rate schedule as a launch of its own: one wave evaluates sched_lr (tde_sched.h) at the
// device-resident step counter and stores the rate into a device word, which the multi-tensor optimizer
// launch behind it reads through its `lr_ptr` (optim.hip).  Both launches sit inside the captured step, so a
// hipGraph captured once follows the schedule.  (The small-net plan's fused step evaluates the same function
// in the prologue of its weight-gradient launch instead: smallnet.hip.)
#include "tde_sched.h"

namespace tde {

__global__ __launch_bounds__(64) void lr_schedule_kernel(LrSched s, const long long* iterations, long long bias,
                                                         float* lr_out) {
  if (threadIdx.x == 0) *lr_out = sched_lr(s, *iterations + bias);
}

}  // namespace tde

using namespace tde;

// *lr_out = schedule(*iterations + bias).  bias: -1 behind a step kernel that has already advanced the
// counter (tde_sched.h).  An unknown kind, nb > 8, decay_steps < 1 or a null pointer: a negative code,
// nothing launched, nothing written.
TDE_API int tde_lr_schedule(const void* sched, const long long* iterations, long long bias, float* lr_out,
                            hipStream_t stream) {
  if (!sched || !iterations || !lr_out) return -1;
  const LrSched s = *(const LrSched*)sched;
  if (!sched_ok(s)) return -2;
  lr_schedule_kernel<<<1, 64, 0, stream>>>(s, iterations, bias, lr_out);
  TDE_LAUNCH_CHECK();
  return 0;
}

TDE_API int tde_sched_abi_sizes(long long* out, int n) {
  if (n > 0) out[0] = (long long)sizeof(LrSched);
  return 1;
}
