#!/usr/bin/env python
"""What a learning-rate schedule costs per step: constant-rate and scheduled twins timed in one session.

  lenet5 (batch 128), small-net plan, step mode "local": SGD and RMSprop, constant against scheduled (the
      scheduled step runs smallnet_wgrad_sched_kernel, which evaluates the schedule in its prologue)
  mnist_cnn (batch 64), fused CNN plan in step mode "plain" (what TDE_FUSED_STEP=0 selects): SGD constant
      against scheduled (the scheduled step has one more launch, lr_schedule_kernel, ahead of the multi-tensor
      optimizer launch)

Timed the way bench/smallnet_rmsprop.py times its plans: a captured hipGraph of ``--steps`` training steps,
``--warmup`` replays, then ``--reps`` timed replays; the row reports the best, the median and the spread
(max - min) of the replays in microseconds per step.  ``--constant-only`` times the constant-rate rows alone, so
that the same rows can be run against another build of the kernel library (TDE_HIP_LIB) for comparison.
Prints one JSON line per row and one per pair with scheduled - constant."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import tensorflow_distributed_example_amd as tde  # noqa: E402
from tensorflow_distributed_example_amd.train import program as PG  # noqa: E402

SCH = tde.optimizers.schedules
ROWS = {
    # name: (model, batch, plan kind, step mode, constant optimizer, scheduled optimizer)
    "lenet5_sgd": (tde.zoo.lenet5, 128, "fused_smallnet", "local", lambda: tde.optimizers.SGD(0.01),
                   lambda: tde.optimizers.SGD(SCH.ExponentialDecay(0.01, 1000, 0.96))),
    "lenet5_rmsprop": (tde.zoo.lenet5, 128, "fused_smallnet", "local", lambda: tde.optimizers.RMSprop(1e-3),
                       lambda: tde.optimizers.RMSprop(SCH.CosineDecay(1e-3, 100000))),
    "mnist_cnn_sgd_plain": (tde.zoo.mnist_cnn, 64, "fused_convnet", "plain", lambda: tde.optimizers.SGD(0.01),
                            lambda: tde.optimizers.SGD(SCH.ExponentialDecay(0.01, 1000, 0.96))),
}


def time_plan(row, scheduled, steps, reps, warmup):
    make, batch, kind, mode, const, sched = ROWS[row]
    model = make()
    model.compile(loss=tde.losses.SparseCategoricalCrossentropy(from_logits=True),
                  optimizer=(sched if scheduled else const)())
    model.build()
    plan = PG.make_plan(model, model._store, "cuda", batch, batch, model.optimizer, model.loss)
    if plan.kind != kind:
        raise SystemExit(f"{model.name} ran on the {plan.kind} plan")
    plan.set_step_mode(mode)
    x = torch.rand((batch,) + tuple(model.input_shape[1:]), device="cuda").to(plan.input_dtype)
    y = torch.randint(0, 10, (batch,), dtype=torch.int32, device="cuda")

    def run():
        for _ in range(steps):
            plan.train_step(x, y)
            if mode == "plain":
                plan.apply()
        plan.finish()

    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        run()
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            run()
        for _ in range(warmup):
            graph.replay()
        stream.synchronize()
        times = []
        for _ in range(reps):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            graph.replay()
            t1.record(stream)
            t1.synchronize()
            times.append(t0.elapsed_time(t1) * 1e3 / steps)
    return dict(row=row, rate="scheduled" if scheduled else "constant", plan=plan.kind, step_mode=plan.step_mode,
                batch=batch, steps=steps, reps=reps, us_per_step=round(min(times), 3),
                median_us=round(statistics.median(times), 3), spread_us=round(max(times) - min(times), 3),
                hip_lib=os.environ.get("TDE_HIP_LIB", "libtde_hip.so"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--constant-only", action="store_true")
    a = ap.parse_args()
    tde.backend.set_random_seed(0)
    for row in a.rows.split(","):
        c = time_plan(row, False, a.steps, a.reps, a.warmup)
        print(json.dumps(c), flush=True)
        if a.constant_only:
            continue
        s = time_plan(row, True, a.steps, a.reps, a.warmup)
        print(json.dumps(s), flush=True)
        print(json.dumps(dict(row=row, scheduled_minus_constant_us=round(s["us_per_step"] - c["us_per_step"], 3),
                              median_difference_us=round(s["median_us"] - c["median_us"], 3),
                              larger_spread_us=max(s["spread_us"], c["spread_us"]))), flush=True)


if __name__ == "__main__":
    main()
