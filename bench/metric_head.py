#!/usr/bin/env python
"""What the metrics beyond the accuracy cost per step: twins timed in one session.

  lenet5 (batch 128, small-net plan, step mode "local") and mnist_cnn (batch 64, the layer-wise plan, float32,
  "plain" -- the plan a model with such metrics runs; the accuracy-only row is put on it too), SGD:
      accuracy      metrics=["accuracy"]: the kernels of before
      top5          + SparseTopKCategoricalAccuracy(5)
      crossentropy  + SparseCategoricalCrossentropy
      f1            + F1Score("macro")
      all           + the three

The "accuracy" row is the yardstick: its kernels are the parent's, so run against another build of the kernel
library (TDE_HIP_LIB, ``--accuracy-only``) it must reproduce.  The other rows add the hidden atomics of
smallnet_step_metric_kernel (lenet5) or one launch, metric_rows_kernel, behind the softmax-CE launch (mnist_cnn).
Timed the way bench/loss_head.py times its plans: a captured hipGraph of ``--steps`` training steps, ``--warmup``
replays, then ``--reps`` timed replays; the row reports the best, the median and the spread (max - min) of the
replays in microseconds per step.  The rows of one model are timed in ``--rounds`` alternating passes and the best
of each row is kept.  Prints one JSON line per row."""
import argparse
import json
import os
import statistics
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import tensorflow_distributed_example_amd as tde  # noqa: E402
from tensorflow_distributed_example_amd.train import program as PG  # noqa: E402

# model -> (constructor, batch, plan, the plan asked of make_plan)
MODELS = {"lenet5": (tde.zoo.lenet5, 128, "fused_smallnet", None),
          "mnist_cnn": (tde.zoo.mnist_cnn, 64, "layerwise", "layerwise")}
# (row, top-5, crossentropy, F1)
VARIANTS = [("accuracy", False, False, False), ("top5", True, False, False), ("crossentropy", False, True, False),
            ("f1", False, False, True), ("all", True, True, True)]


def time_plan(name, variant, top5, ce, f1, steps, reps, warmup):
    make, batch, want, prefer = MODELS[name]
    model = make()
    fl = model.layers[-1].activation != "softmax"
    metrics = ["accuracy"]
    if top5:
        metrics.append(tde.keras.metrics.SparseTopKCategoricalAccuracy(5))
    if ce:
        metrics.append(tde.keras.metrics.SparseCategoricalCrossentropy(from_logits=fl))
    if f1:
        metrics.append(tde.keras.metrics.F1Score(average="macro"))
    model.compile(loss=tde.losses.SparseCategoricalCrossentropy(from_logits=fl), optimizer=tde.optimizers.SGD(0.01),
                  metrics=metrics)
    model.build()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")     # the fused CNN plan says that it declines the metrics
        plan = PG.make_plan(model, model._store, "cuda", batch, batch, model.optimizer, model.loss, prefer=prefer)
    if plan.kind != want or (getattr(plan, "metrics_ext", None) is not None) != (top5 or ce or f1):
        raise SystemExit(f"{model.name} ({variant}) ran on the {plan.kind} plan, not {want}")
    mode = "local" if plan.supports_step_mode("local") else "plain"
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
    ap.add_argument("--accuracy-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench/metric_head.py measures on the GPU; none found")
    tde.backend.set_random_seed(0)
    variants = [v for v in VARIANTS if not a.accuracy_only or v[0] == "accuracy"]
    for name in a.models.split(","):
        best = {}
        for _ in range(a.rounds):            # alternating passes: a drift of the machine hits every row alike
            for v in variants:
                tde.backend.clear_session()
                r = time_plan(name, *v, a.steps, a.reps, a.warmup)
                if v[0] not in best or r["us_per_step"] < best[v[0]]["us_per_step"]:
                    best[v[0]] = r
        for v in variants:
            print(json.dumps(best[v[0]]), flush=True)


if __name__ == "__main__":
    main()
