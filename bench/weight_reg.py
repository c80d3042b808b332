#!/usr/bin/env python
"""What weight regularizers and decoupled weight decay cost per step: twins timed in one session.

  lenet5 (batch 128, small-net plan) and mnist_cnn (batch 64, fused CNN plan), SGD, step mode "plain":
      plain                  gradients to the bucket + the multi-tensor optimizer launch
      l2                     + reg_grad_kernel and reg_finish_kernel ahead of it (an L2 on every kernel)
      weight_decay           the WD variant of the multi-tensor launch, nothing else
      l2+weight_decay        both
      l2+global_clipnorm     the regularizer launches, the two norm launches, the CLIP variant
      global_clipnorm        (for the difference) the norm launches and the CLIP variant alone

The "plain" row is the yardstick: its kernels are the parent's, so run against another build of the kernel
library (TDE_HIP_LIB, ``--plain-only``, which also times global_clipnorm) it must reproduce.  Timed the way bench/lr_schedule.py times
its plans: a captured hipGraph of ``--steps`` training steps, ``--warmup`` replays, then ``--reps`` timed
replays; the row reports the best, the median and the spread (max - min) of the replays in microseconds per
step.  The rows of one model are timed in ``--rounds`` alternating passes and the best of each row is kept.
Prints one JSON line per row and one per row with the feature: row - plain."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import tensorflow_distributed_example_amd as tde  # noqa: E402
from tensorflow_distributed_example_amd.train import program as PG  # noqa: E402

MODELS = {"lenet5": (tde.zoo.lenet5, 128, "fused_smallnet"), "mnist_cnn": (tde.zoo.mnist_cnn, 64, "fused_convnet")}
# (row, l2 on every kernel or None, optimizer arguments); the costs depend on none of the values
VARIANTS = [("plain", None, {}), ("l2", 1e-4, {}), ("weight_decay", None, dict(weight_decay=1e-4)),
            ("l2+weight_decay", 1e-4, dict(weight_decay=1e-4)), ("l2+global_clipnorm", 1e-4, dict(global_clipnorm=1.0)),
            ("global_clipnorm", None, dict(global_clipnorm=1.0))]
PARENT_ROWS = ("plain", "global_clipnorm")     # what a library from before this feature can run


def time_plan(name, variant, l2, kw, steps, reps, warmup):
    make, batch, kind = MODELS[name]
    mode = "plain"
    model = make()
    if l2 is not None:
        for layer in model.layers:
            for s in layer.weight_specs:
                if s.name == "kernel":
                    s.l2 = float(l2)
    model.compile(loss=tde.losses.SparseCategoricalCrossentropy(from_logits=True),
                  optimizer=tde.optimizers.SGD(0.01, **kw))
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
    return dict(model=name, variant=variant, plan=plan.kind, step_mode=plan.step_mode, batch=batch, steps=steps,
                reps=reps, us_per_step=round(min(times), 3), median_us=round(statistics.median(times), 3),
                spread_us=round(max(times) - min(times), 3), hip_lib=os.environ.get("TDE_HIP_LIB", "libtde_hip.so"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--models", default=",".join(MODELS))
    ap.add_argument("--plain-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench/weight_reg.py measures on the GPU; none found")
    tde.backend.set_random_seed(0)
    variants = [v for v in VARIANTS if not a.plain_only or v[0] in PARENT_ROWS]
    for name in a.models.split(","):
        best = {}
        for _ in range(a.rounds):            # alternating passes: a drift of the machine hits every row alike
            for variant, l2, kw in variants:
                r = time_plan(name, variant, l2, kw, a.steps, a.reps, a.warmup)
                if variant not in best or r["us_per_step"] < best[variant]["us_per_step"]:
                    best[variant] = r
        for variant, _, _ in variants:
            print(json.dumps(best[variant]), flush=True)
        for variant, _, _ in variants:
            if variant != "plain":
                print(json.dumps(dict(model=name, variant=variant,
                                      row_minus_plain_us=round(best[variant]["us_per_step"] - best["plain"]["us_per_step"], 3),
                                      median_difference_us=round(best[variant]["median_us"] - best["plain"]["median_us"], 3),
                                      larger_spread_us=max(best[variant]["spread_us"], best["plain"]["spread_us"]))),
                      flush=True)


if __name__ == "__main__":
    main()
