#!/usr/bin/env python
"""The classic LeNet-5 (``zoo.lenet5_classic``: tanh, 2x2 average pooling) next to the ReLU / max-pool
``zoo.lenet5`` on the fused small-net plan, batch 128, one replica, timed back to back the way
bench/smallnet_dropout.py times its models (a captured hipGraph of ``--steps`` training steps with the
optimizer, replayed ``--reps`` times, best replay).  Prints one JSON line per model and one with the ratio."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from smallnet_dropout import time_plan  # noqa: E402  (also puts the repository root on sys.path)

import tensorflow_distributed_example_amd as tde  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    tde.backend.set_random_seed(0)
    res = {}
    for name, make in (("lenet5_classic", tde.zoo.lenet5_classic), ("lenet5", tde.zoo.lenet5)):
        r = time_plan(make(name=name), None, a.steps, a.reps, a.warmup)
        if r["plan"] != "fused_smallnet":
            raise SystemExit(f"{name} ran on the {r['plan']} plan")
        res[name] = r
        print(json.dumps(r), flush=True)
    print(json.dumps(dict(classic_over_relu=round(res["lenet5_classic"]["us_per_step"] / res["lenet5"]["us_per_step"], 3))),
          flush=True)


if __name__ == "__main__":
    main()
