"""Child process of tests/test_loss_head_gpu.py: two MirroredStrategy replicas rehearsed on cuda:0 (as
tests/weight_reg_mirrored_child.py does), zoo.mnist_mlp under CategoricalCrossentropy(label_smoothing=0.1) with class
weights, three steps at global batch 64, then one replica at the same global batch from the same weights.  Prints
one JSON line: the plans, whether the replicas' weights and class-weight tables are bit-identical, the logged losses
of both runs and of the float64 oracle, and the distance of the weights to the one-replica run."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

G, STEPS = 64, 3
SMOOTH, CW = 0.1, {0: 2.0, 2: 0.0, 7: 0.5}


def _run(tde, torch, H, strategy, nrep, w0=None):
    with strategy.scope():
        model = tde.zoo.mnist_mlp()
        model.compile(loss=tde.losses.CategoricalCrossentropy(from_logits=True, label_smoothing=SMOOTH),
                      optimizer=tde.optimizers.SGD(0.05), metrics=["accuracy"], steps_per_execution=1)
    model.build()
    if w0 is not None:
        model.set_weights(w0)
    start = model.get_weights()
    prog = model._program("train", G, class_weight=True)
    prog.set_class_weight(tde.losses.class_weight_table(CW, 10))
    B = G // nrep
    batches = H.batches(model, G, STEPS, 4242)
    _, want_losses = H.trajectory(model, batches, model.optimizer, SMOOTH, CW)
    losses = []
    for x, y in batches:
        x, y = x[None], y[None]
        parts = [(x[:, r * B:(r + 1) * B].contiguous().to("cuda:0"), y[:, r * B:(r + 1) * B].contiguous().to("cuda:0"))
                 for r in range(nrep)]
        prog.reset_metrics()
        prog.stage(parts)
        prog.run()
        prog.sync()
        m = prog.global_metrics()
        losses.append(float(m[0] / m[2]))
    torch.cuda.synchronize()
    return model, prog, start, losses, want_losses


def main():
    import numpy as np
    import torch

    import tensorflow_distributed_example_amd as tde
    import loss_head_oracle as H

    tde.backend.set_random_seed(78)
    strategy = tde.distribute.MirroredStrategy(["cuda:0", "cuda:0"])
    model, prog, w0, losses, _ = _run(tde, torch, H, strategy, 2)
    a, b = (p.store for p in prog.plans)
    ta, tb = (p.class_w for p in prog.plans)
    two = [np.array(w) for w in model.get_weights()]
    out = dict(plan=prog.plan_kind, step_modes=[p.step_mode for p in prog.plans], loss_spec=[bool(p.loss_spec) for p in prog.plans],
               scale=[p.scale for p in prog.plans], graph=bool(prog.use_graph),
               iterations=[int(p.iterations.item()) for p in prog.plans],
               w_identical=bool(torch.equal(a.w.view(torch.int32), b.w.view(torch.int32))),
               tables_identical=bool(torch.equal(ta, tb)) and ta.cpu().tolist() == tde.losses.class_weight_table(CW, 10).tolist(),
               losses=losses, w_moved=float(max(np.abs(t - s).max() for t, s in zip(two, w0))))
    tde.backend.clear_session()
    one_model, one_prog, _, one_losses, want_losses = _run(tde, torch, H, tde.distribute.OneDeviceStrategy("cuda:0"), 1, w0)
    one = [np.array(w) for w in one_model.get_weights()]
    out["one_losses"], out["want_losses"] = one_losses, want_losses
    # the tolerance of tests/test_mirrored_gpu.py for two replicas against one: rtol 1e-4, atol 1e-5
    out["worst_excess"] = float(max((np.abs(t - o) - (1e-5 + 1e-4 * np.abs(o))).max() for t, o in zip(two, one)))
    print("RESULT " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
