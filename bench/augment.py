#!/usr/bin/env python
"""What an input stage costs per step of ``fit`` on the device feed: twins timed in one session.

  mnist_cnn (batch 64, fused CNN plan) and lenet5 (batch 128, small-net plan), SGD, in-memory float32 images
  (the HBM-resident cache, train/device_feed.py), ``steps_per_execution`` steps per hipGraph replay:
      none                   no input stage: tde_gather_rows_dev fills the x ring, the launches of before
      flip                   RandomFlip("horizontal")
      translate_nearest      RandomTranslation(0.1, 0.1, interpolation="nearest")
      translate_bilinear     RandomTranslation(0.1, 0.1) (bilinear, reflect)
  The three augmented rows launch tde_stage_rows_aug (csrc/kernels/augment.hip) in place of the x gather: the
  same number of launches per execution.

The "none" row is the yardstick: its launches are the parent's, so run against another build of the kernel library
(TDE_HIP_LIB, ``--none-only``) it must reproduce.  A row is the wall time of one ``fit`` epoch of ``--steps`` steps
(index stream, staging launches, graph replays, the final sync) divided by the steps: ``--warmup`` epochs, then
``--reps`` timed ones; the row reports the best, the median and the spread (max - min) in microseconds per step.
The rows of one model are timed in ``--rounds`` alternating passes and the best of each row is kept.  Prints one
JSON line per row."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import tensorflow_distributed_example_amd as tde  # noqa: E402

L = tde.keras.layers
# model -> (constructor, batch, plan)
MODELS = {"mnist_cnn": (tde.zoo.mnist_cnn, 64, "fused_convnet"), "lenet5": (tde.zoo.lenet5, 128, "fused_smallnet")}
VARIANTS = {"none": lambda: None,
            "flip": lambda: [L.RandomFlip("horizontal")],
            "translate_nearest": lambda: [L.RandomTranslation(0.1, 0.1, interpolation="nearest")],
            "translate_bilinear": lambda: [L.RandomTranslation(0.1, 0.1)]}


def time_fit(name, variant, steps, spe, reps, warmup):
    make, batch, kind = MODELS[name]
    stage = VARIANTS[variant]()
    model = make() if stage is None else tde.zoo.with_input_stage(make(), stage)
    model.compile(loss=tde.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=tde.optimizers.SGD(0.01),
                  steps_per_execution=spe)
    rng = np.random.default_rng(0)
    x = rng.random((batch * steps, 28, 28, 1), dtype=np.float32)
    y = rng.integers(0, 10, batch * steps).astype(np.int32)
    ds = tde.data.Dataset.from_tensor_slices((x, y)).batch(batch)
    for _ in range(warmup):
        model.fit(ds, epochs=1, verbose=0)
    prog = next(p for k, p in model._programs.items() if k[0] == "train")
    if prog.plan_kind != kind or not model._device_feed:
        raise SystemExit(f"{model.name} ({variant}) ran on the {prog.plan_kind} plan, device feed {model._device_feed}")
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model.fit(ds, epochs=1, verbose=0)      # ends with the program's sync
        times.append((time.perf_counter() - t0) * 1e6 / steps)
    return dict(model=name, variant=variant, plan=prog.plan_kind, batch=batch, steps=steps, steps_per_execution=spe,
                reps=reps, us_per_step=round(min(times), 3), median_us=round(statistics.median(times), 3),
                spread_us=round(max(times) - min(times), 3), hip_lib=os.environ.get("TDE_HIP_LIB", "libtde_hip.so"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--steps-per-execution", type=int, default=32)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--models", default=",".join(MODELS))
    ap.add_argument("--none-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench/augment.py measures on the GPU; none found")
    tde.backend.set_random_seed(0)
    variants = [v for v in VARIANTS if not a.none_only or v == "none"]
    for name in a.models.split(","):
        best = {}
        for _ in range(a.rounds):            # alternating passes: a drift of the machine hits every row alike
            for v in variants:
                tde.backend.clear_session()
                r = time_fit(name, v, a.steps, a.steps_per_execution, a.reps, a.warmup)
                if v not in best or r["us_per_step"] < best[v]["us_per_step"]:
                    best[v] = r
        for v in variants:
            print(json.dumps(best[v]), flush=True)


if __name__ == "__main__":
    main()
