"""Child process of tests/test_optim_rmsprop_gpu.py: two MirroredStrategy replicas rehearsed on cuda:0
(as tests/test_mirrored_gpu.py does), zoo.mnist_mlp + RMSprop, three steps at global batch 64.  Prints one
JSON line: the runner's placement of the update and whether the replicas' weights and rms are bit-identical."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch

    import tensorflow_distributed_example_amd as tde

    momentum = float(sys.argv[1]) if len(sys.argv) > 1 else 0.0
    tde.backend.set_random_seed(77)
    strategy = tde.distribute.MirroredStrategy(["cuda:0", "cuda:0"])
    G, B = 64, 32
    with strategy.scope():
        model = tde.zoo.mnist_mlp()
        model.compile(loss=tde.losses.SparseCategoricalCrossentropy(from_logits=True),
                      optimizer=tde.optimizers.RMSprop(1e-3, momentum=momentum), metrics=["accuracy"],
                      steps_per_execution=1)
    prog = model._program("train", G)
    gen = torch.Generator().manual_seed(4242)
    w0 = prog.plans[0].store.w.clone()
    for _ in range(3):
        x = torch.rand((1, G) + tuple(prog.x_shape), generator=gen)
        y = torch.randint(0, 10, (1, G), generator=gen).to(torch.int32)
        parts = [(x[:, r * B:(r + 1) * B].contiguous().to("cuda:0"), y[:, r * B:(r + 1) * B].contiguous().to("cuda:0"))
                 for r in range(2)]
        prog.stage(parts)
        prog.run()
        prog.sync()
    torch.cuda.synchronize()
    a, b = (p.store for p in prog.plans)
    slots = sorted(a.slots)
    out = dict(plan=prog.plan_kind, step_modes=[p.step_mode for p in prog.plans], comm_applies=bool(prog.comm_applies),
               comm=type(strategy.comm).__name__, graph=bool(prog.use_graph), slots=slots,
               iterations=[int(p.iterations.item()) for p in prog.plans],
               w_identical=bool(torch.equal(a.w.view(torch.int32), b.w.view(torch.int32))),
               slots_identical=all(bool(torch.equal(a.slots[s].view(torch.int32), b.slots[s].view(torch.int32)))
                                   for s in slots),
               w_moved=float((a.w - w0).abs().max()), rms_max=float(a.slots["rms"].max()))
    print("RESULT " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
