"""Child process of tests/test_grad_clip_gpu.py: two MirroredStrategy replicas rehearsed on cuda:0 (as
tests/rmsprop_mirrored_child.py does), zoo.mnist_mlp + SGD with a clip, three steps at global batch 64, then
one replica at the same global batch from the same weights.  argv: mode, c.  Prints one JSON line: the
runner's placement of the update, whether the replicas' weights and clip words are bit-identical, and the
distance to the one-replica run."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

G, STEPS = 64, 3


def _run(tde, torch, strategy, opt, nrep, w0=None):
    with strategy.scope():
        model = tde.zoo.mnist_mlp()
        model.compile(loss=tde.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=opt,
                      metrics=["accuracy"], steps_per_execution=1)
    model.build()
    if w0 is not None:
        model.set_weights(w0)
    start = model.get_weights()
    prog = model._program("train", G)
    B = G // nrep
    gen = torch.Generator().manual_seed(4242)
    scale_max = 0.0
    for _ in range(STEPS):
        x = torch.rand((1, G) + tuple(prog.x_shape), generator=gen)
        y = torch.randint(0, 10, (1, G), generator=gen).to(torch.int32)
        parts = [(x[:, r * B:(r + 1) * B].contiguous().to("cuda:0"), y[:, r * B:(r + 1) * B].contiguous().to("cuda:0"))
                 for r in range(nrep)]
        prog.stage(parts)
        prog.run()
        prog.sync()
        sc = prog.plans[0].opt.clip_scale
        scale_max = max(scale_max, float(sc.max())) if sc is not None else scale_max
    torch.cuda.synchronize()
    return model, prog, start, scale_max


def main():
    import numpy as np
    import torch

    import tensorflow_distributed_example_amd as tde

    mode, c = sys.argv[1], float(sys.argv[2])
    tde.backend.set_random_seed(77)
    strategy = tde.distribute.MirroredStrategy(["cuda:0", "cuda:0"])
    model, prog, w0, scale_max = _run(tde, torch, strategy, tde.optimizers.SGD(0.05, **{mode: c}), 2)
    a, b = (p.store for p in prog.plans)
    words = [(p.opt.clip_norm, p.opt.clip_scale) for p in prog.plans]
    two = [np.array(w) for w in model.get_weights()]
    out = dict(plan=prog.plan_kind, step_modes=[p.step_mode for p in prog.plans], comm_applies=bool(prog.comm_applies),
               comm=type(strategy.comm).__name__, graph=bool(prog.use_graph),
               iterations=[int(p.iterations.item()) for p in prog.plans],
               w_identical=bool(torch.equal(a.w.view(torch.int32), b.w.view(torch.int32))),
               words_identical=all(x is None and y is None or bool(torch.equal(x.view(torch.int32), y.view(torch.int32)))
                                   for x, y in zip(*words)),
               scale_max=scale_max, w_moved=float(max(np.abs(t - s).max() for t, s in zip(two, w0))))
    tde.backend.clear_session()
    one_model, one_prog, _, _ = _run(tde, torch, tde.distribute.OneDeviceStrategy("cuda:0"),
                                     tde.optimizers.SGD(0.05, **{mode: c}), 1, w0)
    one = [np.array(w) for w in one_model.get_weights()]
    out["one_step_mode"] = one_prog.plans[0].step_mode
    # the tolerance of tests/test_mirrored_gpu.py for two replicas against one: rtol 1e-4, atol 1e-5
    out["worst_excess"] = float(max((np.abs(t - o) - (1e-5 + 1e-4 * np.abs(o))).max() for t, o in zip(two, one)))
    print("RESULT " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
