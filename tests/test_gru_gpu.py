"""The GRU sweeps (csrc/kernels/gru.hip) against the step loop in float64 torch with autograd, and GRU through the
float32 layer-wise plan and ``fit``.  Bounds as in tests/test_lstm_gpu.py, in relative L2 norm: 1e-6 for the
forward outputs, 1e-5 for gradients and per variable of a step.  The same loop in plain float32 torch on the CPU
stays within a quarter of each bound at these cases (figures: profiles/gru/NOTES.md)."""
import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("fp32_policy")]
DEV = "cuda"

SHAPES = [  # N, T, units
    (1, 1, 16),      # no recurrence: dU is an exact zero
    (3, 2, 16),      # the first real recurrence, masked rows
    (16, 5, 32),     # a full row tile, two waves
    (17, 7, 48),     # one row into a second workgroup, odd wave count
    (5, 28, 64),     # the zoo shape
    (33, 12, 128),   # the upper units
    (2, 96, 16),     # a long chain
]
CASES = [s + (seq,) for s in SHAPES for seq in (False, True)]
PAD = 5   # sentinel floats behind every output


def _r(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator(device="cpu").manual_seed(seed))


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def inputs(case):
    """X, U, the recurrent bias (off zero, so R_h differs from h U_h) and the upstream dh."""
    N, T, u, seq = case
    return (_r(N, T, 3 * u, seed=1), _r(u, 3 * u, seed=2) / u ** 0.5, 0.5 * _r(3 * u, seed=4),
            _r(*((N, T, u) if seq else (N, u)), seed=3))


def reference(case, dtype):
    """hseq, the saved R_h, dX, dU and db[1] of the step loop written out in torch ops at ``dtype`` on the CPU."""
    N, T, u, seq = case
    X, U, rb, dh = (t.to(dtype) for t in inputs(case))
    for t in (X, U, rb):
        t.requires_grad_(True)
    h = X.new_zeros(N, u)
    hs, rhs = [], []
    for t in range(T):
        xz, xr, xh = X[:, t].split(u, dim=-1)
        rz, rr, rh = (h @ U + rb).split(u, dim=-1)
        z, r = torch.sigmoid(xz + rz), torch.sigmoid(xr + rr)
        h = z * h + (1 - z) * torch.tanh(xh + r * rh)
        hs.append(h)
        rhs.append(rh)
    hseq = torch.stack(hs, 1)
    ((hseq if seq else h) * dh).sum().backward()
    return dict(hseq=hseq.detach(), rh=torch.stack(rhs, 1).detach(), dx=X.grad, du=U.grad, drb=rb.grad)


def _guarded(*shape):
    """A sentinel-filled flat buffer and its leading view of ``shape``: what lies behind the view must not change."""
    n = int(np.prod(shape))
    flat = torch.full((n + PAD,), 7.0, device=DEV)
    return flat, flat[:n].view(*shape)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_gru_fwd_bwd(case):
    from tensorflow_distributed_example_amd.ops import layer_ops32 as O32
    N, T, u, seq = case
    ref = reference(case, torch.float64)
    X, U, rb, dh = (t.to(DEV) for t in inputs(case))
    (fh, hseq), (fp, hprev), (fa, acts), (fl, hlast) = (_guarded(N, T, u), _guarded(N, T, u), _guarded(N, T, 4 * u),
                                                        _guarded(N, u))
    O32.gru_fwd(X, U, rb, hseq, hprev, acts, N, T, u, hlast=None if seq else hlast)
    runs = []
    for _ in range(2):
        (fx, dx), (fr, dr) = _guarded(N, T, 3 * u), _guarded(N, T, 3 * u)
        du, drb = torch.full_like(U, 7.0), torch.zeros_like(rb)   # the bias sum adds into its destination
        O32.gru_bwd(acts, hprev, U, dh, dx, dr, N, T, u, last_only=not seq)
        O32.dense_wgrad(hprev, dr, du, N * T)
        O32.act_bwd(dr, None, N * T, 3 * u, relu=False, dbias=drb)
        runs.append((dx, dr, du))
        assert all(f[-PAD:].eq(7.0).all() for f in (fx, fr))
    torch.cuda.synchronize()
    assert all(f[-PAD:].eq(7.0).all() for f in (fh, fp, fa, fl)) and (not seq or hlast.eq(7.0).all())
    assert torch.equal(hprev[:, 1:], hseq[:, :-1]) and hprev[:, 0].abs().max() == 0
    assert seq or torch.equal(hlast, hseq[:, -1])
    dx, dr, du = runs[0]
    assert torch.equal(dr[..., :2 * u], dx[..., :2 * u])             # dX and dR differ in the candidate's block
    assert torch.equal(dr[..., 2 * u:], dx[..., 2 * u:] * acts[..., u:2 * u])   # by the reset gate: da * r
    errs = dict(hseq=_rel(hseq, ref["hseq"]), rh=_rel(acts[..., 3 * u:], ref["rh"]), dx=_rel(dx, ref["dx"]),
                drb=_rel(drb, ref["drb"]))
    if T == 1:   # no ratio against an exact zero
        assert ref["du"].norm() == 0 and torch.count_nonzero(du) == 0
    else:
        errs["du"] = _rel(du, ref["du"])
    print("gru vs float64 rel err", case, errs)
    assert max(errs["hseq"], errs["rh"]) < 1e-6 and max(errs.values()) < 1e-5, errs
    assert all(torch.equal(a, b) for a, b in zip(*runs))   # one writer, one summation order


def _model(tde, seed):
    tde.backend.set_random_seed(seed)
    m = tde.zoo.mnist_gru()
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
    rec = [s for s in plan.stages if isinstance(s, LW._Gru)]
    assert [(s.geom(B), s.seq) for s in rec] == [((16, 28, 64), True), ((16, 28, 64), False)]
    rng = np.random.default_rng(0)
    for n in st.names(trainable=True):   # both bias rows off their initial zero
        if n.endswith("bias"):
            st.view(n).add_(torch.from_numpy(0.3 * rng.standard_normal(st.view(n).shape).astype(np.float32)).cuda())
    xt = torch.from_numpy(rng.random((B, 28, 28, 1), dtype=np.float32)).cuda()
    yt = torch.from_numpy(rng.integers(0, 10, B)).int().cuda()
    want, _ = LW.emulate_step(plan, xt, yt)
    plan.train_step(xt, yt)
    torch.cuda.synchronize()
    errs = {n: _rel(st.grad(n), v) for n, v in want.items()}
    for n, v in want.items():   # the two rows of a GRU bias are written by two stages: each on its own
        if n.endswith("gru_cell/bias"):
            errs.update({f"{n}[{i}]": _rel(st.grad(n).view(2, -1)[i], v[i]) for i in range(2)})
    print("GRU step vs float64 oracle rel err", errs)
    assert len(want) == len(st.names(trainable=True)) == 8 and len(errs) == 12 and max(errs.values()) < 1e-5, errs


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
    m = tde.keras.Sequential([L.GRU(16, input_shape=(28, 28)), L.Dense(10)])
    m.compile(loss=tde.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=tde.optimizers.SGD(0.05))
    x = np.zeros((64, 28, 28), np.float32)
    with pytest.raises(NotImplementedError, match="gru .GRU.*float32 only"):
        m.fit(x, np.zeros(64, np.int64), batch_size=64, epochs=1, verbose=0)
