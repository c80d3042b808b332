#!/usr/bin/env python
"""What a RandomRotation / RandomZoom input stage costs per step of ``fit`` on the device feed, beside the rows
that existed before: twins timed in one session.

  mnist_cnn (batch 64, fused CNN plan) and lenet5 (batch 128, small-net plan), SGD, in-memory float32 images
  (the HBM-resident cache, train/device_feed.py), ``steps_per_execution`` steps per hipGraph replay:
      none                   no input stage: tde_gather_rows_dev fills the x ring
      translate_bilinear     RandomTranslation(0.1, 0.1): the flips-and-shifts kernel of tde_stage_rows_aug
      rotate_nearest         RandomRotation(0.05, interpolation="nearest")
      rotate_bilinear        RandomRotation(0.05)
      zoom_bilinear          RandomZoom(0.1)
      flip_rotate_zoom       RandomFlip("horizontal") + nearest rotation + bilinear zoom
  The last four launch the general source-coordinate kernel of tde_stage_rows_aug (csrc/kernels/augment.hip) in
  place of the x gather: the same number of launches per execution.

The first two rows launch what they launched before the general kernel existed.  ``--parent-lib NAME`` times them
again in a child process that loads another build of the kernel library (``_lib/NAME``, through TDE_HIP_LIB),
before and after this process's rows: the old path is judged against those numbers within the run-to-run spread,
not against the library under test.  A row is the wall time of one ``fit`` epoch of ``--steps`` steps divided by
the steps: ``--warmup`` epochs, then ``--reps`` timed ones; the row reports the best, the median and the spread
(max - min) in microseconds per step.  The rows of one model are timed in ``--rounds`` alternating passes and the
best of each row is kept.  Prints one JSON line per row."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import tensorflow_distributed_example_amd as tde  # noqa: E402

L = tde.keras.layers
# model -> (constructor, batch, plan)
MODELS = {"mnist_cnn": (tde.zoo.mnist_cnn, 64, "fused_convnet"), "lenet5": (tde.zoo.lenet5, 128, "fused_smallnet")}
OLD = ("none", "translate_bilinear")


def variants():
    v = {"none": lambda: None, "translate_bilinear": lambda: [L.RandomTranslation(0.1, 0.1)]}
    if hasattr(L, "RandomRotation"):
        v.update({"rotate_nearest": lambda: [L.RandomRotation(0.05, interpolation="nearest")],
                  "rotate_bilinear": lambda: [L.RandomRotation(0.05)],
                  "zoom_bilinear": lambda: [L.RandomZoom(0.1)],
                  "flip_rotate_zoom": lambda: [L.RandomFlip("horizontal"),
                                               L.RandomRotation(0.05, interpolation="nearest"), L.RandomZoom(0.1)]})
    return v


def time_fit(name, variant, steps, spe, reps, warmup):
    make, batch, kind = MODELS[name]
    stage = variants()[variant]()
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


def parent_rows(a, when):
    """The old rows in a fresh child process on the other library."""
    cmd = [sys.executable, os.path.abspath(__file__), "--variants", ",".join(OLD), "--models", a.models,
           "--steps", str(a.steps), "--steps-per-execution", str(a.steps_per_execution), "--reps", str(a.reps),
           "--warmup", str(a.warmup), "--rounds", str(a.rounds)]
    r = subprocess.run(cmd, env=dict(os.environ, TDE_HIP_LIB=a.parent_lib), stdout=subprocess.PIPE, text=True,
                       timeout=a.child_timeout)
    if r.returncode != 0:
        raise SystemExit(f"the child on {a.parent_lib} failed ({r.returncode})")
    for ln in r.stdout.splitlines():
        if ln.startswith("{"):
            print(json.dumps(dict(json.loads(ln), when=when)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--steps-per-execution", type=int, default=32)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--models", default=",".join(MODELS))
    ap.add_argument("--variants", default="")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--child-timeout", type=float, default=240.0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench/augment_affine.py measures on the GPU; none found")
    tde.backend.set_random_seed(0)
    todo = [v for v in variants() if not a.variants or v in a.variants.split(",")]
    if a.parent_lib:
        parent_rows(a, "before")
    for name in a.models.split(","):
        best = {}
        for _ in range(a.rounds):            # alternating passes: a drift of the machine hits every row alike
            for v in todo:
                tde.backend.clear_session()
                r = time_fit(name, v, a.steps, a.steps_per_execution, a.reps, a.warmup)
                if v not in best or r["us_per_step"] < best[v]["us_per_step"]:
                    best[v] = r
        for v in todo:
            print(json.dumps(best[v]), flush=True)
    if a.parent_lib:
        parent_rows(a, "after")


if __name__ == "__main__":
    main()
