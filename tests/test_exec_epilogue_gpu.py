"""What runs between two executions of the fused small-CNN step: the deferred-update flush (``tde_flat_apply``
in its ``pend`` form, the one-round-trip ``flat_flush`` of csrc/include/tde_optim.h) and the staging copy that
carries it (``tde_copy_pairs_apply``, csrc/kernels/gather.hip), and the Program's bookkeeping of a flush that
is due (train/runner.py, ``ReplicaPlan.flush_due``).

The flush is checked on the rig of tests/test_optim_gpu.py against the float64 oracle of tests/optim_oracle.py,
with that file's tolerances: sgd / momentum run on the exact grid and must equal the oracle bit for bit, Adam
within max(4 x the error of the same operations in torch fp32 on the host, 2^-22 max |value|) plus lr rho_t for
the weights.  The RMSprop kinds are refused, as before (``opt_step<false>`` does not know them).  Ranges: one
element, the small CNN's own two segments (288 + 32, more than one wave, one pass of 512 threads), and 1025
elements (the strided tail: two passes and one element of a third).

The copy: destinations byte-equal to the sources, the words in front of and behind every destination
untouched, at 16 B (one vector), 4 KB + 4 B (the 4-byte path, a partial last unit) and 1 MB (more than one
workgroup, every thread busy), with and without a flush in the launch.

The programs run under TDE_DETERMINISTIC=1, where the fused step is bitwise reproducible: replayed executions
with the flush carried by the next staging copy, or issued in front of the next replay, must leave the weights
of the eager run (TDE_GRAPH=0), which flushes at the end of every execution.  The generic plan sums with float
atomics in either mode, so no run of it reproduces another bit for bit; its replayed run is held to the
float64 trajectory of tests/test_convnet_gen_gpu.py instead, with that file's model, data and bounds (biases
5e-4, the conv kernel 5e-5, the Dense kernels 1e-5; a lost or doubled conv update shows as ~1e-3)."""
import ctypes

import pytest
import torch

import optim_oracle as O
import test_convnet_gen_gpu as G
from test_optim_gpu import ADAM_HYPER, FlatRig, _assert_state, rho_bound

pytestmark = pytest.mark.gpu

DEV = "cuda"
RANGES = {"one": [(0, 1)], "cnn": [(5, 288), (293, 32)], "tail": [(7, 1025)]}
RMS_KINDS = (4, 5)   # kOptRMSprop, kOptRMSpropMom (csrc/include/tde_optim.h)


def _rig(kind, seed):
    if kind == "adam":
        rig = FlatRig("adam", ADAM_HYPER, grid=False, seed=seed)
        rig.it.fill_(7)
        return rig, 7
    return FlatRig(kind, O.GRID_HYPER), 1


def _assert_applied(tag, rig, ranges, grep, t):
    """One applied update of ``ranges``: the oracle's state (exact kinds bit for bit, Adam within the bound of
    test_optim_gpu.test_flat_apply_adam), exactly the used replicas zeroed, flag cleared, count 1."""
    want, mask = rig.expect(ranges, grep, t)
    got = rig.device_state()
    assert rig.pend.item() == 0 and rig.count.item() == 1, (tag, rig.pend.item(), rig.count.item())
    if rig.kind != "adam":
        assert not torch.equal(want["w"][mask], rig.host["w"][mask])
        _assert_state(tag, got, want)
        return
    assert rig.it.item() == t
    d = O.first_diff(got["g"].double(), want["g"], bitwise=False)
    assert not d, f"{tag}: g: {d}"
    h = rig.host
    gs = h["g"][0].float()
    for r in range(1, max(grep, 1)):
        gs = gs + h["g"][r].float()
    host = O.fp32_step("adam", ADAM_HYPER, h["w"].float(), gs, h["m"].float(), h["v"].float(), t)
    _, rho = rho_bound(t)
    for key, hv in zip(("w", "m", "v"), host):
        d = O.first_diff(got[key][~mask].double(), want[key][~mask], bitwise=False)
        assert not d, f"{tag}: {key} outside the ranges: {d}"
        o = want[key][mask]
        e_dev = float((got[key][mask].double() - o).abs().max())
        e_host = float((hv[mask].double() - o).abs().max())
        bound = max(4.0 * e_host, 2.0 ** -22 * float(o.abs().max())) + (ADAM_HYPER["lr"] * rho if key == "w" else 0)
        print(f"[{tag}] {key}: dev {e_dev:.3g} host {e_host:.3g} bound {bound:.3g}")
        assert e_dev <= bound, (tag, key, e_dev, bound)


def _assert_unchanged(tag, rig, before, pend, count):
    after = rig.device_state()
    for k in before:
        d = O.first_diff(after[k], before[k])
        assert not d, f"{tag}: changed {k}: {d}"
    assert rig.pend.item() == pend and rig.count.item() == count, (tag, rig.pend.item(), rig.count.item())


@pytest.mark.parametrize("grep", [1, 3, 8])
@pytest.mark.parametrize("kind", ["sgd", "momentum", "adam"])
def test_flat_apply_one_round_trip(kind, grep):
    """pend = 0: nothing moves, the gradient replicas included.  pend = 1: the oracle's update."""
    from tensorflow_distributed_example_amd.ops import kernels as K
    for name, ranges in RANGES.items():
        rig, t = _rig(kind, 50 + grep)
        tag = f"{kind} grep={grep} {name}"
        before = rig.device_state()
        K.flat_apply(rig.spec(ranges, grep))
        _assert_unchanged(tag + " pend=0", rig, before, 0, 0)
        rig.pend.fill_(1)
        K.flat_apply(rig.spec(ranges, grep))
        _assert_applied(tag + " pend=1", rig, ranges, grep, t)


def test_flat_apply_refuses_rmsprop():
    from tensorflow_distributed_example_amd import _native as N
    rig = FlatRig("momentum", O.GRID_HYPER)
    rig.pend.fill_(1)
    before = rig.device_state()
    rng = (ctypes.c_int * 4)(5, 288, 293, 32)
    h = O.GRID_HYPER
    for kind in RMS_KINDS:
        rc = N.hip().tde_flat_apply(rig.w.data_ptr(), rig.g.data_ptr(), rig.m.data_ptr(), rig.v.data_ptr(),
                                    rig.it.data_ptr(), rig.pend.data_ptr(), kind, h["lr"], h["mom"], h["b1"], h["b2"],
                                    h["eps"], rng, 2, 8, rig.n, rig.count.data_ptr(), N.stream_ptr())
        assert rc == -1, kind
    _assert_unchanged("rmsprop", rig, before, 1, 0)


# ------------------------------------------------------------------------------------------ the staging copy
GUARD = 16              # int32 words in front of and behind every destination
SENTINEL = -0x5A5A5A5B
PAIR_BYTES = [16, 4096 + 4, 1 << 20]


class Pairs:
    def __init__(self, sizes=PAIR_BYTES, seed=3):
        gen = torch.Generator().manual_seed(seed)
        self.src, self.buf, self.dst = [], [], []
        for nb in sizes:
            n = nb // 4
            self.src.append(torch.randint(-2 ** 31, 2 ** 31 - 1, (max(n, 1),), generator=gen, dtype=torch.int64)
                            .to(torch.int32).to(DEV)[:n])
            buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
            self.buf.append(buf)
            self.dst.append(buf[GUARD: GUARD + n])     # 64 bytes in: the 16-byte alignment of the buffer kept

    def raw(self, n=None, nbytes=None, f=None):
        from tensorflow_distributed_example_amd import _native as N
        k = len(self.src)
        nb = nbytes if nbytes is not None else [s.numel() * 4 for s in self.src]
        return N.hip().tde_copy_pairs_apply(
            k if n is None else n, (ctypes.c_void_p * k)(*[s.data_ptr() for s in self.src]),
            (ctypes.c_void_p * k)(*[d.data_ptr() for d in self.dst]), (ctypes.c_longlong * k)(*nb),
            ctypes.byref(f) if f is not None else None, N.stream_ptr())

    def assert_copied(self, tag, copied=True):
        torch.cuda.synchronize()
        for i, (s, b) in enumerate(zip(self.src, self.buf)):
            n = s.numel()
            want = torch.full_like(b, SENTINEL)
            if copied:
                want[GUARD: GUARD + n] = s
            assert torch.equal(b, want), f"{tag}: pair {i} ({4 * n} bytes)"


@pytest.mark.parametrize("kind,grep", [(None, 0), ("momentum", 8), ("sgd", 3), ("adam", 1)])
def test_copy_pairs_apply(kind, grep):
    """The three pairs in one launch; with a flush in it, first while nothing is pending (the copy alone takes
    effect), then pending (the oracle's update, as ``tde_flat_apply``)."""
    from tensorflow_distributed_example_amd.ops import kernels as K
    if kind is None:
        p = Pairs()
        K.copy_pairs_apply(list(zip(p.src, p.dst)))
        p.assert_copied("no flush")
        return
    ranges = RANGES["cnn"]
    rig, t = _rig(kind, 70)
    before = rig.device_state()
    p = Pairs()
    K.copy_pairs_apply(list(zip(p.src, p.dst)), rig.spec(ranges, grep))
    p.assert_copied(f"{kind} pend=0")
    _assert_unchanged(f"{kind} pend=0", rig, before, 0, 0)
    rig.pend.fill_(1)
    p = Pairs(seed=4)
    K.copy_pairs_apply(list(zip(p.src, p.dst)), rig.spec(ranges, grep))
    p.assert_copied(f"{kind} pend=1")
    _assert_applied(f"copy + {kind} grep={grep}", rig, ranges, grep, t)


def test_copy_pairs_apply_flush_without_bytes():
    """Nothing to copy and a flush: the launch is the flush workgroup alone; the strided tail in it."""
    rig, t = _rig("momentum", 0)
    rig.pend.fill_(1)
    p = Pairs(sizes=[0])
    assert p.raw(f=rig.spec(RANGES["tail"], 8)) == 0
    p.assert_copied("0 bytes")
    _assert_applied("flush alone", rig, RANGES["tail"], 8, t)


def test_copy_pairs_apply_refusals_launch_nothing():
    rig = FlatRig("momentum", O.GRID_HYPER)
    rig.pend.fill_(1)
    before = rig.device_state()
    ok = rig.spec(RANGES["cnn"], 8)
    p = Pairs()
    assert p.raw(n=0, f=ok) == -1 and p.raw(n=5, f=ok) == -1             # the pair count
    assert p.raw(nbytes=[16, 4098, 1 << 20], f=ok) == -2                  # not whole words
    for rms in RMS_KINDS:                                                 # a kind the flush does not know
        f = rig.spec(RANGES["cnn"], 8)
        f.h.kind = rms
        assert p.raw(f=f) == -3
    assert p.raw(f=rig.spec(RANGES["cnn"], 8, slots=False)) == -3         # momentum without its slot
    f = rig.spec(RANGES["cnn"], 8)
    f.nr = 5
    assert p.raw(f=f) == -3                                               # too many ranges
    adam = FlatRig("adam", ADAM_HYPER, grid=False)
    f = adam.spec(RANGES["cnn"], 8)
    f.iterations = None
    assert p.raw(f=f) == -3                                               # Adam without the step counter
    p.assert_copied("refused", copied=False)
    _assert_unchanged("refused", rig, before, 1, 0)


# ------------------------------------------------------------------------------------------ the programs
def _execute(tde, monkeypatch, graph, restage):
    """Three executions of four steps from seeded weights: ``restage`` stages a device-resident group in front
    of each, else one group is staged and replayed three times.  (weights, plan, program)"""
    monkeypatch.setenv("TDE_GRAPH", "1" if graph else "0")
    tde.backend.clear_session()
    tde.backend.set_global_policy("float32")
    tde.backend.set_random_seed(5)
    m = tde.zoo.mnist_cnn()
    m.compile(loss=tde.losses.SparseCategoricalCrossentropy(from_logits=True),
              optimizer=tde.optimizers.SGD(0.05, momentum=0.9), metrics=["accuracy"], steps_per_execution=4)
    prog = m._program("train", 64)
    plan = prog.plans[0]
    assert plan.kind == "fused_convnet" and plan.step_mode == "local" and prog.use_graph == graph
    gen = torch.Generator().manual_seed(9)
    xs = torch.rand(3, 4, 64, 28, 28, 1, generator=gen).to(DEV)
    ys = torch.randint(0, 10, (3, 4, 64), generator=gen).to(torch.int32).to(DEV)
    for e in range(3):
        if restage or e == 0:
            prog.stage([(xs[e], ys[e])])
            assert not plan.flush_due            # the staging copy took it along
        prog.run()
        assert plan.flush_due == graph           # a replay leaves it due, an eager execution flushes itself
    prog.sync()
    assert not plan.flush_due
    return plan.store.w.clone(), plan, prog


@pytest.mark.parametrize("restage", [True, False], ids=["stage_run", "run_run"])
def test_replayed_executions_equal_eager(restage, monkeypatch):
    import tensorflow_distributed_example_amd as tde
    monkeypatch.setenv("TDE_DETERMINISTIC", "1")
    got = []
    for graph in (True, False):
        w, plan, _ = _execute(tde, monkeypatch, graph, restage)
        assert plan.det
        iv = plan.step_invariants()
        assert iv["commits"] == 12 and iv["applied_on_the_fly"] == 9, (graph, iv)
        assert iv["pending"] == [0, 0] and iv["gconv_abs_max"] == 0.0, (graph, iv)
        got.append(w)
    assert torch.equal(got[0], got[1]), float((got[0] - got[1]).abs().max())


@pytest.mark.usefixtures("fp32_policy")
def test_replayed_executions_generic_plan():
    """mnist_cnn_wide's widths (Conv2D(64) / Dense(128), SGD) on the generic plan: the three executions of
    test_convnet_gen_gpu.test_generic_plan_graph_trajectory_matches_float64 -- its model, data and float64
    trajectory, so its bounds hold here -- with no synchronisation between them: every flush but the last rides
    on the next staging copy."""
    import tensorflow_distributed_example_amd as tde
    lr = 0.05
    m = G._model(tde, 64, 128, tde.optimizers.SGD(lr), 4)
    st = m._store
    names = st.names(trainable=True)
    w64 = {n: st.view(n).detach().double().clone() for n in names}
    prog = m._program("train", 64)
    plan = prog.plans[0]
    assert prog.use_graph and plan.kind == "fused_convnet_generic" and plan.step_mode == "local" and plan.crep > 1
    groups = [[G._qdata(64, 300 + 4 * e + s) for s in range(4)] for e in range(3)]
    for data in groups:
        prog.stage([(torch.stack([d[0] for d in data]), torch.stack([d[1] for d in data]))])
        assert not plan.flush_due
        prog.run()
        assert plan.flush_due
    iv = plan.step_invariants()
    assert not plan.flush_due and iv["pending"] == [0, 0] and iv["gconv_abs_max"] == 0.0, iv
    assert int(plan.iterations) == 12 and float(st.g.abs().max()) == 0.0
    for data in groups:
        for x, y in data:
            g = G._grads64(m, w64, x, y, 64)
            for n in names:
                w64[n] = w64[n] - lr * g[n]
    for n in names:
        tol = 5e-4 if n.endswith("/bias") else (5e-5 if n == f"{m.layers[0].name}/kernel" else 1e-5)
        r = G._rel(st.view(n), w64[n])
        print(f"{n}: replayed vs float64 {r:.3e} (bound {tol:g})")
        assert r < tol, (n, r)
