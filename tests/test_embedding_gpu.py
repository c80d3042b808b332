"""The Embedding kernels (csrc/kernels/embedding.hip) against numpy: the gather bit for bit, the scatter-sum bit
for bit against ``np.add.at`` on a float32 zero array (the token-order contract) and within the bound of a
sequential float32 sum of the float64 result; then Embedding through the float32 layer-wise plan and ``fit``."""
import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("fp32_policy")]
DEV = "cuda"
PAD = 5   # sentinel floats behind every output


def _ids(kind, n, V):
    rng = np.random.default_rng(n + V)
    if kind == "random":
        return rng.integers(0, V, n).astype(np.float32)
    if kind == "distinct":
        return rng.permutation(V)[:n].astype(np.float32)
    if kind == "hot":                                   # every token on the last row of the table
        return np.full(n, V - 1, np.float32)
    ids = rng.integers(0, V, n).astype(np.float32)      # "mixed": invalid ids, a signed zero, a fraction
    ids[3::8], ids[4::8], ids[5::8], ids[6::8] = -1.0, -0.0, float(V), 2.7
    return ids


CASES = [  # n, V, D, ids, id dtype
    (1, 1, 4, "random", "f32"),        # one token, one row, one float4
    (5, 3, 4, "random", "f32"),        # V below one row block, duplicates within a wave
    (300, 70, 8, "random", "f32"),     # n not a multiple of 256, a second row block (RB = 64), partial last block
    (300, 300, 8, "distinct", "f32"),  # no duplicates (V raised to n: 300 distinct ids need 300 rows)
    (300, 300, 8, "distinct", "i32"),
    (700, 129, 64, "hot", "f32"),      # a hot row longer than the list's 512 entries; other blocks store zeros
    (513, 40, 512, "random", "f32"),   # largest D, smallest RB (16), two float4 columns per lane, empty blocks
    (64, 16, 12, "mixed", "f32"),      # invalid ids skipped, truncation, D not a power of two
]


def _guarded(*shape):
    n = int(np.prod(shape))
    flat = torch.full((n + PAD,), 7.0, device=DEV)
    return flat, flat[:n].view(*shape)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_embed_fwd_bwd(case):
    from tensorflow_distributed_example_amd.ops import layer_ops32 as O32
    n, V, D, kind, dt = case
    rng, ids = np.random.default_rng(7), _ids(kind, n, V)
    row = np.trunc(ids).astype(np.int64)
    ok = (row >= 0) & (row < V)
    table, dy = (rng.standard_normal(s).astype(np.float32) for s in ((V, D), (n, D)))
    want_out = np.where(ok[:, None], table[row.clip(0, V - 1)], np.float32(0))
    want_f32, want_f64, mag = np.zeros((V, D), np.float32), np.zeros((V, D)), np.zeros((V, D))
    np.add.at(want_f32, row[ok], dy[ok])                # unbuffered: in index order, in float32
    np.add.at(want_f64, row[ok], dy[ok].astype(np.float64))
    np.add.at(mag, row[ok], np.abs(dy[ok]).astype(np.float64))
    count = np.bincount(row[ok], minlength=V)
    idt = torch.from_numpy(row.astype(np.int32) if dt == "i32" else ids).to(DEV)
    tt, dyt = torch.from_numpy(table).to(DEV), torch.from_numpy(dy).to(DEV)
    fo, out = _guarded(n, D)
    O32.embed_fwd(idt, tt, out, n, V, D)
    runs = []
    for _ in range(2):
        fd, dtab = _guarded(V, D)                       # pre-filled with 7.0: the launch writes every element
        O32.embed_bwd(idt, dyt, dtab, n, V, D)
        runs.append(dtab.cpu().numpy())
        assert fd[-PAD:].eq(7.0).all()
    assert fo[-PAD:].eq(7.0).all()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want_out.astype(np.float32).view(np.uint32))
    got, bound = runs[0], np.maximum(count - 1, 0)[:, None] * 2.0 ** -24 * mag
    print("embed", case, "max |err| vs float64", np.abs(got - want_f64).max(), "largest bound", bound.max())
    assert np.array_equal(got.view(np.uint32), want_f32.view(np.uint32))
    assert (np.abs(got - want_f64) <= bound).all()
    assert np.array_equal(runs[0].view(np.uint32), runs[1].view(np.uint32))


def _rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _model(tde, make, seed):
    tde.backend.set_random_seed(seed)
    m = make()
    m.compile(loss=tde.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=tde.optimizers.SGD(0.5),
              metrics=["accuracy"], steps_per_execution=4)
    return m


def test_plan_step_matches_float64():
    import tensorflow_distributed_example_amd as tde
    from tensorflow_distributed_example_amd.train import layerwise as LW
    from tensorflow_distributed_example_amd.train import program as PG
    m = _model(tde, tde.zoo.text_gru, 0)
    m.build()
    st, B = m._store, 16
    plan = PG.make_plan(m, st, "cuda", B, B, m.optimizer, m.loss)   # no preference: the fused plans pass it on
    assert isinstance(plan, LW.LayerwisePlan) and plan.f32
    emb = [s for s in plan.stages if isinstance(s, LW._Embedding)]
    assert [s.geom(B) for s in emb] == [(16 * 32, 2000, 32)]
    rng = np.random.default_rng(0)
    ids = rng.integers(0, 2000, (B, 32))
    xt = torch.from_numpy(ids.astype(np.float32)).cuda()
    yt = torch.from_numpy(rng.integers(0, 4, B)).int().cuda()
    want, _ = LW.emulate_step(plan, xt, yt)
    plan.train_step(xt, yt)
    torch.cuda.synchronize()
    errs = {n: _rel(st.grad(n), v) for n, v in want.items()}
    print("text_gru step vs float64 oracle rel err", errs)
    assert len(want) == len(st.names(trainable=True)) == 6 and max(errs.values()) < 1e-5, errs
    g = st.grad(emb[0].wname).view(2000, 32).cpu()
    untouched = np.setdiff1d(np.arange(2000), ids)
    assert len(untouched) > 1000 and g[untouched].eq(0).all()


def test_fit_with_a_ragged_last_batch():
    import tensorflow_distributed_example_amd as tde
    from tensorflow_distributed_example_amd.train import program as PG
    m = _model(tde, tde.zoo.text_gap, 4)
    rng = np.random.default_rng(5)
    x = rng.integers(4, 2000, (64 * 4 + 24, 32)).astype(np.int64)
    y = rng.integers(0, 4, len(x)).astype(np.int64)
    x[np.arange(len(x))[:, None], rng.integers(0, 32, (len(x), 8))] = y[:, None]   # the class's marker id, ~8 times
    h = m.fit(x, y, batch_size=64, epochs=3, verbose=0).history["loss"]
    prog = m._program("train", 64)
    assert prog.plan_kind == "layerwise" and prog.plans[0].compute_dtype == "fp32"
    assert np.isfinite(h).all() and h[-1] < h[0], h
    got = m.predict(x[:88], batch_size=64, verbose=0)
    ref = PG.ReferencePlan(m, m._store.clone_to("cpu"), "cpu", 88, 88, None, m.loss)
    assert _rel(got, ref.predict(torch.from_numpy(x[:88]).float(), 88)) < 1e-5


def test_mixed_bfloat16_is_refused_by_name():
    import tensorflow_distributed_example_amd as tde
    tde.backend.set_global_policy("mixed_bfloat16")
    m = _model(tde, tde.zoo.text_gap, 0)
    x = np.zeros((64, 32), np.int64)
    with pytest.raises(NotImplementedError, match="embedding.* .Embedding.*float32 only"):
        m.fit(x, np.zeros(64, np.int64), batch_size=64, epochs=1, verbose=0)
