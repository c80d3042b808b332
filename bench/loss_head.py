#!/usr/bin/env python
"""What the loss head's spec costs per step: twins timed in one session.

  lenet5 (batch 128, small-net plan, step mode "local") and mnist_cnn (batch 64; fused CNN plan, step mode "local",
  for the trivial specs; the layer-wise plan, "plain", for the others), SGD:
      sparse                 SparseCategoricalCrossentropy: the kernels of before
      categorical            CategoricalCrossentropy(label_smoothing=0): the trivial spec, the same kernels
      smooth                 CategoricalCrossentropy(label_smoothing=0.1): smallnet_step_loss_kernel / xent_spec_kernel
      class_weight           the sparse loss in a program built for fit(class_weight=)

The "sparse" row is the yardstick: its kernels are the parent's, so run against another build of the kernel library
(TDE_HIP_LIB, ``--sparse-only``) it must reproduce.  Timed the way bench/weight_reg.py times its plans: a captured
hipGraph of ``--steps`` training steps, ``--warmup`` replays, then ``--reps`` timed replays; the row reports the
best, the median and the spread (max - min) of the replays in microseconds per step.  The rows of one model are
timed in ``--rounds`` alternating passes and the best of each row is kept.  Prints one JSON line per row."""
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

# model -> (constructor, batch, plan of the trivial specs, plan of the others)
MODELS = {"lenet5": (tde.zoo.lenet5, 128, "fused_smallnet", "fused_smallnet"),
          "mnist_cnn": (tde.zoo.mnist_cnn, 64, "fused_convnet", "layerwise")}
# (row, categorical, label smoothing, class weights)
VARIANTS = [("sparse", False, 0.0, False), ("categorical", True, 0.0, False), ("smooth", True, 0.1, False),
            ("class_weight", False, 0.0, True)]


def time_plan(name, variant, categorical, smooth, cw, steps, reps, warmup):
    make, batch, kind0, kind1 = MODELS[name]
    model = make()
    fl = model.layers[-1].activation != "softmax"
    loss = (tde.losses.CategoricalCrossentropy(from_logits=fl, label_smoothing=smooth) if categorical
            else tde.losses.SparseCategoricalCrossentropy(from_logits=fl))
    model.compile(loss=loss, optimizer=tde.optimizers.SGD(0.01))
    model.build()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")     # the fused CNN plan says that it declines the spec
        plan = PG.make_plan(model, model._store, "cuda", batch, batch, model.optimizer, model.loss, class_weight=cw)
    want = kind1 if (smooth or cw) else kind0
    if plan.kind != want:
        raise SystemExit(f"{model.name} ({variant}) ran on the {plan.kind} plan, not {want}")
    mode = "local" if plan.supports_step_mode("local") else "plain"
    plan.set_step_mode(mode)
    if cw:
        plan.set_class_weight(tde.losses.class_weight_table({0: 2.0, 1: 0.5}, model.output_shape[-1]))
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
    ap.add_argument("--sparse-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench/loss_head.py measures on the GPU; none found")
    tde.backend.set_random_seed(0)
    variants = [v for v in VARIANTS if not a.sparse_only or v[0] == "sparse"]
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
