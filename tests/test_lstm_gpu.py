"""The LSTM sweeps (csrc/kernels/lstm.hip) against the step loop in float64 torch with autograd, and LSTM through
the float32 layer-wise plan and ``fit``.  Bounds as in tests/test_layers_f32_gpu.py, in relative L2 norm: 1e-6 for
the forward outputs, 1e-5 for gradients and per variable of a step.  The same loop in plain float32 torch on the
CPU stays within a quarter of each bound at these cases (figures: profiles/lstm/NOTES.md)."""
import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("fp32_policy")]
DEV = "cuda"

SHAPES = [  # N, T, units
    (3, 2, 16),      # the first real recurrence, masked rows
    (16, 5, 32),     # a full row tile, two waves
    (17, 7, 48),     # one row into a second workgroup, odd wave count
    (5, 28, 64),     # the zoo shape
    (33, 12, 128),   # the upper units
    (2, 96, 16),     # a long chain
]
# one step, one wave: h_0 = 0, so dU is an exact zero; then every shape in both output forms
CASES = [(1, 1, 16, False)] + [s + (seq,) for s in SHAPES for seq in (False, True)]


def _r(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator(device="cpu").manual_seed(seed))


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def inputs(case):
    N, T, u, seq = case
    return _r(N, T, 4 * u, seed=1), _r(u, 4 * u, seed=2) / u ** 0.5, _r(*((N, T, u) if seq else (N, u)), seed=3)


def reference(case, dtype):
    """(hseq, the final c, dZ, dU) of the step loop written out in torch ops at ``dtype`` on the CPU."""
    N, T, u, seq = case
    z, U, dh = (t.to(dtype) for t in inputs(case))
    z.requires_grad_(True), U.requires_grad_(True)
    h = c = z.new_zeros(N, u)
    hs = []
    for t in range(T):
        i, f, g, o = (z[:, t] + h @ U).split(u, dim=-1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        hs.append(h)
    hseq = torch.stack(hs, 1)
    ((hseq if seq else h) * dh).sum().backward()
    return dict(hseq=hseq.detach(), c=c.detach(), dz=z.grad, du=U.grad)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_lstm_fwd_bwd(case):
    from tensorflow_distributed_example_amd.ops import layer_ops32 as O32
    N, T, u, seq = case
    ref = reference(case, torch.float64)
    z, U, dh = (t.to(DEV) for t in inputs(case))
    hseq, hprev, cseq = (torch.full((N, T, u), 7.0, device=DEV) for _ in range(3))
    gates, hlast = torch.zeros(N, T, 4 * u, device=DEV), None if seq else torch.zeros(N, u, device=DEV)
    O32.lstm_fwd(z, U, hseq, hprev, gates, cseq, N, T, u, hlast=hlast)
    runs = []
    for _ in range(2):
        dz, du = torch.full_like(z, 7.0), torch.full_like(U, 7.0)
        O32.lstm_bwd(gates, cseq, U, dh, dz, N, T, u, last_only=not seq)
        O32.dense_wgrad(hprev, dz, du, N * T)
        runs.append((dz, du))
    torch.cuda.synchronize()
    assert torch.equal(hprev[:, 1:], hseq[:, :-1]) and hprev[:, 0].abs().max() == 0
    assert seq or torch.equal(hlast, hseq[:, -1])
    errs = dict(hseq=_rel(hseq, ref["hseq"]), c=_rel(cseq[:, -1], ref["c"]), dz=_rel(runs[0][0], ref["dz"]))
    if T == 1:   # no ratio against an exact zero
        assert ref["du"].norm() == 0 and torch.count_nonzero(runs[0][1]) == 0
    else:
        errs["du"] = _rel(runs[0][1], ref["du"])
    print("lstm vs float64 rel err", case, errs)
    assert max(errs["hseq"], errs["c"]) < 1e-6 and max(errs.values()) < 1e-5, errs
    assert all(torch.equal(a, b) for a, b in zip(*runs))   # one writer, one summation order


def _model(tde, seed):
    tde.backend.set_random_seed(seed)
    m = tde.zoo.mnist_lstm()
    m.compile(loss=tde.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=tde.optimizers.SGD(0.05),
              metrics=["accuracy"], steps_per_execution=4)
    return m


def test_plan_step_matches_float64():
    import tensorflow_distributed_example_amd as tde
    from tensorflow_distributed_example_amd.train import layerwise as LW
    from tensorflow_distributed_example_amd.train import program as PG
    m = _model(tde, 0)
    m.build()
    st, B = m._store, 16
    plan = PG.make_plan(m, st, "cuda", B, B, m.optimizer, m.loss)   # no preference: the fused plans pass it on
    assert isinstance(plan, LW.LayerwisePlan) and plan.f32
    rec = [s for s in plan.stages if isinstance(s, LW._Lstm)]
    assert [(s.geom(B), s.seq) for s in rec] == [((16, 28, 64), True), ((16, 28, 64), False)]
    rng = np.random.default_rng(0)
    for n in st.names(trainable=True):   # biases off their initial 0 and 1
        if n.endswith("bias"):
            st.view(n).add_(torch.from_numpy(0.3 * rng.standard_normal(st.view(n).shape).astype(np.float32)).cuda())
    xt = torch.from_numpy(rng.random((B, 28, 28, 1), dtype=np.float32)).cuda()
    yt = torch.from_numpy(rng.integers(0, 10, B)).int().cuda()
    want, _ = LW.emulate_step(plan, xt, yt)
    plan.train_step(xt, yt)
    torch.cuda.synchronize()
    errs = {n: _rel(st.grad(n), v) for n, v in want.items()}
    print("LSTM step vs float64 oracle rel err", errs)
    assert len(errs) == len(st.names(trainable=True)) == 8 and max(errs.values()) < 1e-5, errs


def test_fit_with_a_ragged_last_batch():
    import tensorflow_distributed_example_amd as tde
    from tensorflow_distributed_example_amd.train import program as PG
    m = _model(tde, 4)
    rng = np.random.default_rng(5)
    x = rng.random((64 * 4 + 24, 28, 28, 1), dtype=np.float32)
    y = x.reshape(len(x), -1)[:, :10].argmax(1).astype(np.int64)   # learnable labels
    h = m.fit(x, y, batch_size=64, epochs=3, verbose=0).history["loss"]
    prog = m._program("train", 64)
    assert prog.plan_kind == "layerwise" and prog.plans[0].compute_dtype == "fp32"
    assert np.isfinite(h).all() and h[-1] < h[0], h
    got = m.predict(x[:88], batch_size=64, verbose=0)
    ref = PG.ReferencePlan(m, m._store.clone_to("cpu"), "cpu", 88, 88, None, m.loss)
    assert _rel(torch.as_tensor(got), ref.predict(torch.from_numpy(x[:88]), 88)) < 1e-5


def test_mixed_bfloat16_is_refused_by_name():
    import tensorflow_distributed_example_amd as tde
    L = tde.keras.layers
    tde.backend.set_global_policy("mixed_bfloat16")
    m = tde.keras.Sequential([L.LSTM(16, input_shape=(28, 28)), L.Dense(10)])
    m.compile(loss=tde.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=tde.optimizers.SGD(0.05))
    x = np.zeros((64, 28, 28), np.float32)
    with pytest.raises(NotImplementedError, match="lstm .LSTM.*float32 only"):
        m.fit(x, np.zeros(64, np.int64), batch_size=64, epochs=1, verbose=0)
