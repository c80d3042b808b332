"""The bidirectional sweeps (csrc/kernels/lstm.hip, gru.hip) against the two step loops in float64 torch, direction 1 on
the flipped input and flipped back; then Bidirectional through the float32 layer-wise plan and ``fit``.  Bounds as in
tests/test_lstm_gpu.py (relative L2: 1e-6 forward, 1e-5 gradients); float32 CPU figures: profiles/birnn/NOTES.md."""
import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("fp32_policy")]

SHAPES = [  # N, T, units
    (1, 1, 16),      # no recurrence in either direction: dU is an exact zero, the first step is the last
    (3, 2, 16),      # the first real recurrence, masked rows; each direction's first position is the other's last
    (17, 3, 48),     # one row into a second workgroup, odd wave count, odd T (buffer parity in reversed order)
    (16, 4, 32),     # a full row tile, even T
    (33, 5, 128),    # the upper units, three workgroups per direction
    (2, 65, 64),     # a long chain, the zoo width
]
CASES = [(cell,) + s + (seq,) for cell in ("lstm", "gru") for s in SHAPES for seq in (False, True)]
DEV, PAD = "cuda", 5   # PAD sentinel floats behind every output


def _r(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator(device="cpu").manual_seed(seed))


def _rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def inputs(case):
    """Per direction X_d, U_d and (GRU) the recurrent bias off zero; then the upstream dh over the whole output."""
    (cell, N, T, u, seq), G = case, 3 if case[0] == "gru" else 4
    X = [_r(N, T, G * u, seed=10 + d) for d in range(2)]
    U = [_r(u, G * u, seed=20 + d) / u ** 0.5 for d in range(2)]
    rb = [0.5 * _r(G * u, seed=30 + d) for d in range(2)] if cell == "gru" else None
    return X, U, rb, _r(*((N, T, 2 * u) if seq else (N, 2 * u)), seed=3)


def _loop(cell, X, U, rb):
    u = U.shape[0]
    h = c = X.new_zeros(X.shape[0], u)
    hs, rhs = [], []
    for t in range(X.shape[1]):
        if cell == "gru":
            (xz, xr, xh), (rz, rr, rh) = X[:, t].split(u, dim=-1), (h @ U + rb).split(u, dim=-1)
            z, r = torch.sigmoid(xz + rz), torch.sigmoid(xr + rr)
            h = z * h + (1 - z) * torch.tanh(xh + r * rh)
            rhs.append(rh)
        else:
            i, f, g, o = (X[:, t] + h @ U).split(u, dim=-1)
            c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
            h = torch.sigmoid(o) * torch.tanh(c)
        hs.append(h)
    return torch.stack(hs, 1), torch.stack(rhs, 1) if rhs else None


def reference(case, dtype):
    """Per direction hseq, R_h, dX, dU, db[1] at ``dtype`` on the CPU: direction 1 loops over the flipped input."""
    cell, N, T, u, seq = case
    X, U, rb, dh = inputs(case)
    (X, U), dh = ([t.to(dtype).requires_grad_(True) for t in ts] for ts in (X, U)), dh.to(dtype)
    rb = [t.to(dtype).requires_grad_(True) for t in rb] if rb else [None, None]
    hs, rh = zip(*(_loop(cell, torch.flip(X[d], [1]) if d else X[d], U[d], rb[d]) for d in range(2)))
    hs = [hs[0], torch.flip(hs[1], [1])]
    out = torch.cat(hs, -1) if seq else torch.cat([hs[0][:, -1], hs[1][:, 0]], -1)
    (out * dh).sum().backward()
    return dict(hseq=[h.detach() for h in hs], rh=[rh[0], torch.flip(rh[1], [1])] if rh[0] is not None else None,
                dx=[t.grad for t in X], du=[t.grad for t in U], drb=[t.grad for t in rb] if rb[0] is not None else None)


def _pair(*shape):
    # two sentinel-filled flat buffers and their leading views of ``shape``: what lies behind a view must not change
    n = int(np.prod(shape))
    flats = [torch.full((n + PAD,), 7.0, device=DEV) for _ in range(2)]
    return flats, [f[:n].view(*shape) for f in flats]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_bi_fwd_bwd(case):
    from tensorflow_distributed_example_amd.ops import layer_ops32 as O32
    cell, N, T, u, seq = case
    gru, G, ref = cell == "gru", 3 if cell == "gru" else 4, reference(case, torch.float64)
    X, U, rb, dh = inputs(case)
    X, U, rb, dh = [t.to(DEV) for t in X], [t.to(DEV) for t in U], [t.to(DEV) for t in rb or []], dh.to(DEV)
    (fh, hseq), (fp, hprev), (fa, acts), (fc, cseq) = _pair(N, T, u), _pair(N, T, u), _pair(N, T, 4 * u), _pair(N, T, u)
    (fo, _), (out, _) = _pair(*((N, T, 2 * u) if seq else (N, 2 * u)))
    (O32.gru_bi_fwd(X, U, rb, hseq, hprev, acts, out, N, T, u, seq=seq) if gru else
     O32.lstm_bi_fwd(X, U, hseq, hprev, acts, cseq, out, N, T, u, seq=seq))
    runs = []
    for _ in range(2):
        (fx, dx), (fr, dr) = _pair(N, T, G * u), _pair(N, T, G * u)
        du = [torch.full_like(U[d], 7.0) for d in range(2)]
        drb = [torch.zeros_like(b) for b in rb] if gru else []   # the bias sum adds into its destination
        (O32.gru_bi_bwd(acts, hprev, U, dh, dx, dr, N, T, u, last_only=not seq) if gru else
         O32.lstm_bi_bwd(acts, cseq, U, dh, dx, N, T, u, last_only=not seq))
        for d in range(2):
            O32.dense_wgrad(hprev[d], dr[d] if gru else dx[d], du[d], N * T)
            if gru:
                O32.act_bwd(dr[d], None, N * T, 3 * u, relu=False, dbias=drb[d])
        runs.append(dx + (dr if gru else []) + du)   # the sweeps' outputs and dU; the bias column sum adds atomically
        assert all(f[-PAD:].eq(7.0).all() for f in fx + (fr if gru else []))
    assert all(f[-PAD:].eq(7.0).all() for f in fp + fa + [fo] + ([] if gru else fc) + ([] if seq else fh))
    assert not seq or all(f.eq(7.0).all() for f in fh)   # with sequences the output tensor is hseq
    hs = [out[..., d * u:(d + 1) * u] for d in range(2)] if seq else hseq
    assert torch.equal(hprev[0][:, 1:], hs[0][:, :-1]) and hprev[0][:, 0].abs().max() == 0
    assert torch.equal(hprev[1][:, :-1], hs[1][:, 1:]) and hprev[1][:, -1].abs().max() == 0
    assert seq or (torch.equal(out[:, :u], hseq[0][:, -1]) and torch.equal(out[:, u:], hseq[1][:, 0]))
    uni = [torch.empty(N, T, k * u, device=DEV) for k in (1, 1, 4, 1)]   # recorded, not asserted: the compiler's
    O32.gru_fwd(X[0], U[0], rb[0], *uni[:3], N, T, u) if gru else O32.lstm_fwd(X[0], U[0], *uni, N, T, u)  # contraction
    print("direction 0 bitwise equal to the unidirectional sweep:", case, torch.equal(uni[0], hs[0]))
    dx, du = runs[0][:2], runs[0][-2:]
    errs = {}
    for d in range(2):
        errs[f"hseq{d}"] = _rel(hs[d], ref["hseq"][d])
        errs[f"dx{d}"] = _rel(dx[d], ref["dx"][d])
        if gru:
            errs[f"rh{d}"] = _rel(acts[d][..., 3 * u:], ref["rh"][d])
            errs[f"drb{d}"] = _rel(drb[d], ref["drb"][d])
        if T > 1:
            errs[f"du{d}"] = _rel(du[d], ref["du"][d])
        assert T > 1 or (ref["du"][d].norm() == 0 and torch.count_nonzero(du[d]) == 0)   # an exact zero, no ratio
    print("bidirectional vs float64 rel err", case, errs)
    assert max(v for k, v in errs.items() if k[:2] in ("hs", "rh")) < 1e-6 and max(errs.values()) < 1e-5, errs
    assert all(torch.equal(a, b) for a, b in zip(*runs))   # one writer, one summation order


def _model(tde, make, seed):
    tde.backend.set_random_seed(seed)
    m = make()
    m.compile(loss=tde.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=tde.optimizers.SGD(0.5),
              metrics=["accuracy"], steps_per_execution=4)
    return m


def test_stacked_plan_step_matches_float64():
    import tensorflow_distributed_example_amd as tde
    from tensorflow_distributed_example_amd.train import layerwise as LW
    from tensorflow_distributed_example_amd.train import program as PG
    m = _model(tde, tde.zoo.text_bigru, 0)
    m.build()
    st, B = m._store, 16
    plan = PG.make_plan(m, st, "cuda", B, B, m.optimizer, m.loss)   # no preference: the fused plans pass it on
    rec = [s for s in plan.stages if isinstance(s, LW._BiRnn)]
    assert [(s.geom(B), s.seq, s.zs[0].shape) for s in rec] == [((16, 32, 64), True, (32, 192)),
                                                              ((16, 32, 64), False, (32, 192))]
    rng = np.random.default_rng(0)
    for n in st.names(trainable=True):   # both bias rows off their initial zero
        if n.endswith("bias"):
            st.view(n).add_(torch.from_numpy(0.3 * rng.standard_normal(st.view(n).shape).astype(np.float32)).cuda())
    xt = torch.from_numpy(rng.integers(0, 2000, (B, 32)).astype(np.float32)).cuda()
    yt = torch.from_numpy(rng.integers(0, 4, B)).int().cuda()
    want, _ = LW.emulate_step(plan, xt, yt)
    plan.train_step(xt, yt)
    errs = {n: _rel(st.grad(n), v) for n, v in want.items()}
    print("text_bigru step vs float64 oracle rel err", errs)
    # 15 variables: embeddings, 4 directions x (kernel, recurrent_kernel, bias), the head's kernel and bias
    assert len(want) == len(st.names(trainable=True)) == 15 and max(errs.values()) < 1e-5, errs


def test_fit_with_a_ragged_last_batch():
    import tensorflow_distributed_example_amd as tde
    from tensorflow_distributed_example_amd.train import program as PG
    m = _model(tde, tde.zoo.text_bilstm, 4)
    rng = np.random.default_rng(5)
    x = rng.integers(4, 2000, (64 * 4 + 24, 32)).astype(np.int64)
    y = rng.integers(0, 4, len(x)).astype(np.int64)
    x[np.arange(len(x))[:, None], rng.integers(0, 32, (len(x), 8))] = y[:, None]   # the class's marker id, ~8 times
    h = m.fit(x, y, batch_size=64, epochs=3, verbose=0).history["loss"]
    assert m._program("train", 64).plan_kind == "layerwise"
    assert np.isfinite(h).all() and h[-1] < h[0], h
    got = m.predict(x[:88], batch_size=64, verbose=0)
    ref = PG.ReferencePlan(m, m._store.clone_to("cpu"), "cpu", 88, 88, None, m.loss)
    assert _rel(got, ref.predict(torch.from_numpy(x[:88]).float(), 88)) < 1e-5


def test_mixed_bfloat16_is_refused_by_name():
    import tensorflow_distributed_example_amd as tde
    L = tde.keras.layers
    tde.backend.set_global_policy("mixed_bfloat16")
    m = _model(tde, lambda: tde.keras.Sequential([L.Bidirectional(L.LSTM(16), input_shape=(28, 28)), L.Dense(10)]), 0)
    with pytest.raises(NotImplementedError, match="bidirectional.* .Bidirectional.*float32 only"):
        m.fit(np.zeros((64, 28, 28), np.float32), np.zeros(64, np.int64), batch_size=64, epochs=1, verbose=0)
