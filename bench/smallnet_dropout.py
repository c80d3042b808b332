#!/usr/bin/env python
"""Dropout models on the fused small-net plan against the layer-wise plan: LeNet-5 with Dropout(0.5)
after Dense(120) and after Dense(84), and the dense MLP with Dropout(0.2), batch 128, one replica.  Plans
are set up as in bench/smallnet_phases.py (``make_plan`` on random data); each is timed as a captured
hipGraph of ``--steps`` training steps (optimizer included) replayed ``--reps`` times.  The dropout-free
model on the fused plan is timed next to them.  Prints one JSON line per (model, plan)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import tensorflow_distributed_example_amd as tde  # noqa: E402
from tensorflow_distributed_example_amd.train import program as PG  # noqa: E402

K = tde.keras.layers
BATCH = 128


def lenet5(drop):
    d = [K.Dropout(0.5)] if drop else []
    d2 = [K.Dropout(0.5)] if drop else []
    return tde.Sequential([
        K.Conv2D(6, 5, padding="same", activation="relu", input_shape=(28, 28, 1)), K.MaxPooling2D(),
        K.Conv2D(16, 5, activation="relu"), K.MaxPooling2D(), K.Flatten(),
        K.Dense(120, activation="relu"), *d, K.Dense(84, activation="relu"), *d2,
        K.Dense(10)], name="lenet5_drop" if drop else "lenet5")


def mlp(drop):
    return tde.Sequential([K.Flatten(input_shape=(28, 28, 1)), K.Dense(128, activation="relu"),
                           *([K.Dropout(0.2)] if drop else []), K.Dense(10)], name="mnist_mlp_drop" if drop else "mnist_mlp")


def time_plan(model, prefer, steps, reps, warmup):
    model.compile(loss=tde.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=tde.optimizers.SGD(0.01))
    model.build()
    plan = PG.make_plan(model, model._store, "cuda", BATCH, BATCH, model.optimizer, model.loss, prefer=prefer)
    local = plan.supports_step_mode("local")
    if local:
        plan.set_step_mode("local")
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
    return dict(model=model.name, plan=plan.kind, step_mode=plan.step_mode, batch=BATCH, steps=steps,
                us_per_step=round(best * 1e3 / steps, 2), img_per_s=round(BATCH * steps / (best * 1e-3)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    tde.backend.set_random_seed(0)
    for make in (lenet5, mlp):
        for drop, prefer in ((False, None), (True, None), (True, "layerwise")):
            print(json.dumps(time_plan(make(drop), prefer, a.steps, a.reps, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
