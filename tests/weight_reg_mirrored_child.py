"""Child process of tests/test_weight_reg_gpu.py: two MirroredStrategy replicas rehearsed on cuda:0 (as
tests/grad_clip_mirrored_child.py does), zoo.mnist_mlp's layers with an l1_l2 kernel regularizer and an l2 bias
regularizer + SGD with weight_decay (the output bias excluded), three steps at global batch 64, then one replica at
the same global batch from the same weights.  Prints one JSON line: the runner's placement of the update, whether
the replicas' weights and penalty words are bit-identical, the logged losses of both runs and the distance of
the weights to the one-replica run."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

G, STEPS = 64, 3


def _opt(tde):
    opt = tde.optimizers.SGD(0.05, weight_decay=0.02)
    opt.exclude_from_weight_decay(var_names=["out/bias"])
    return opt


def _run(tde, torch, strategy, nrep, w0=None):
    L, R = tde.keras.layers, tde.regularizers
    with strategy.scope():
        model = tde.keras.Sequential([L.Flatten(input_shape=(28, 28, 1)),
                                      L.Dense(128, activation="relu", kernel_regularizer=R.l1_l2(1e-4, 1e-3),
                                              bias_regularizer=R.l2(0.01), name="hidden"),
                                      L.Dense(10, name="out")])
        model.compile(loss=tde.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=_opt(tde),
                      metrics=["accuracy"], steps_per_execution=1)
    model.build()
    if w0 is not None:
        model.set_weights(w0)
    start = model.get_weights()
    prog = model._program("train", G)
    B = G // nrep
    gen = torch.Generator().manual_seed(4242)
    losses, penalties = [], []
    for _ in range(STEPS):
        x = torch.rand((1, G) + tuple(prog.x_shape), generator=gen)
        y = torch.randint(0, 10, (1, G), generator=gen).to(torch.int32)
        parts = [(x[:, r * B:(r + 1) * B].contiguous().to("cuda:0"), y[:, r * B:(r + 1) * B].contiguous().to("cuda:0"))
                 for r in range(nrep)]
        penalties.append(float(sum(model.losses)))       # of the weights this step's forward uses
        prog.reset_metrics()
        prog.stage(parts)
        prog.run()
        prog.sync()
        m = prog.global_metrics()
        losses.append(float(m[0] / m[2]))
    torch.cuda.synchronize()
    return model, prog, start, losses, penalties


def main():
    import numpy as np
    import torch

    import tensorflow_distributed_example_amd as tde

    tde.backend.set_random_seed(77)
    strategy = tde.distribute.MirroredStrategy(["cuda:0", "cuda:0"])
    model, prog, w0, losses, penalties = _run(tde, torch, strategy, 2)
    a, b = (p.store for p in prog.plans)
    words = [(p.opt.reg.penalty, p.opt.reg.partials, p.opt.wd_dev) for p in prog.plans]
    two = [np.array(w) for w in model.get_weights()]
    out = dict(plan=prog.plan_kind, step_modes=[p.step_mode for p in prog.plans], comm_applies=bool(prog.comm_applies),
               comm=type(strategy.comm).__name__, graph=bool(prog.use_graph),
               iterations=[int(p.iterations.item()) for p in prog.plans],
               w_identical=bool(torch.equal(a.w.view(torch.int32), b.w.view(torch.int32))),
               words_identical=all(bool(torch.equal(x.view(torch.int32), y.view(torch.int32))) for x, y in zip(*words)),
               wd=[float(v) for v in prog.plans[0].opt.wd_dev.cpu()], losses=losses, penalties=penalties,
               last_penalty_word=float(prog.plans[0].opt.reg.penalty.item()),
               w_moved=float(max(np.abs(t - s).max() for t, s in zip(two, w0))))
    tde.backend.clear_session()
    one_model, one_prog, _, one_losses, _ = _run(tde, torch, tde.distribute.OneDeviceStrategy("cuda:0"), 1, w0)
    one = [np.array(w) for w in one_model.get_weights()]
    out["one_step_mode"] = one_prog.plans[0].step_mode
    out["one_losses"] = one_losses
    # the tolerance of tests/test_mirrored_gpu.py for two replicas against one: rtol 1e-4, atol 1e-5
    out["worst_excess"] = float(max((np.abs(t - o) - (1e-5 + 1e-4 * np.abs(o))).max() for t, o in zip(two, one)))
    print("RESULT " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
