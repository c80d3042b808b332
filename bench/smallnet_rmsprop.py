#!/usr/bin/env python
"""The small-net plan under every optimizer kind, with the update inside the step ("local": two launches)
and after it ("plain": the multi-tensor launch as a third): LeNet-5 and the dense MLP, batch 128, one
replica, under SGD, Adam, RMSprop and RMSprop with momentum.  Timed the way bench/smallnet_classic.py times
its models: a captured hipGraph of ``--steps`` training steps replayed ``--reps`` times, best replay.
Prints one JSON line per (model, optimizer, step mode) and one per (model, optimizer) with plain - local."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import tensorflow_distributed_example_amd as tde  # noqa: E402
from tensorflow_distributed_example_amd.train import program as PG  # noqa: E402

BATCH = 128
OPTIMIZERS = {
    "sgd": lambda: tde.optimizers.SGD(0.01),
    "adam": lambda: tde.optimizers.Adam(1e-3),
    "rmsprop": lambda: tde.optimizers.RMSprop(1e-3),
    "rmsprop_momentum": lambda: tde.optimizers.RMSprop(1e-3, momentum=0.9),
}


def time_plan(make, opt_name, mode, steps, reps, warmup):
    model = make()
    model.compile(loss=tde.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=OPTIMIZERS[opt_name]())
    model.build()
    plan = PG.make_plan(model, model._store, "cuda", BATCH, BATCH, model.optimizer, model.loss)
    if plan.kind != "fused_smallnet":
        raise SystemExit(f"{model.name} ran on the {plan.kind} plan")
    plan.set_step_mode(mode)
    local = mode == "local"
    x = torch.rand((BATCH,) + tuple(model.input_shape[1:]), device="cuda").to(plan.input_dtype)
    y = torch.randint(0, 10, (BATCH,), dtype=torch.int32, device="cuda")

    def run():
        for _ in range(steps):
            plan.train_step(x, y)
            if not local:
                plan.apply()

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
        best = float("inf")
        for _ in range(reps):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            graph.replay()
            t1.record(stream)
            t1.synchronize()
            best = min(best, t0.elapsed_time(t1))
    return dict(model=model.name, optimizer=opt_name, plan=plan.kind, step_mode=plan.step_mode, batch=BATCH,
                steps=steps, ms_per_step=round(best / steps, 5), us_per_step=round(best * 1e3 / steps, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--optimizers", default=",".join(OPTIMIZERS))
    a = ap.parse_args()
    tde.backend.set_random_seed(0)
    for name, make in (("lenet5", tde.zoo.lenet5), ("mnist_mlp", tde.zoo.mnist_mlp)):
        for opt_name in a.optimizers.split(","):
            r = {mode: time_plan(lambda: make(name=name), opt_name, mode, a.steps, a.reps, a.warmup)
                 for mode in ("local", "plain")}
            for mode in ("local", "plain"):
                print(json.dumps(r[mode]), flush=True)
            print(json.dumps(dict(model=name, optimizer=opt_name, plain_minus_local_us=round(
                r["plain"]["us_per_step"] - r["local"]["us_per_step"], 2))), flush=True)


if __name__ == "__main__":
    main()
