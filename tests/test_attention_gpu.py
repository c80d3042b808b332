"""The attention kernels (csrc/kernels/attention.hip) against float64 torch with autograd, and MultiHeadAttention
through the float32 layer-wise plan and ``fit``.  Bounds as in tests/test_layers_f32_gpu.py, in relative L2 norm:
1e-6 for O and lse, 1e-5 for gradients and per variable of a step.  The same formula in plain float32 torch on the
CPU stays within a quarter of each bound, but for O at T = 256 (2.8e-7; figures: profiles/attention/NOTES.md)."""
import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("fp32_policy")]
DEV = "cuda"

CASES = [  # B, heads, T, dk, dv, shift of Q and K, scale of Q and K
    (2, 1, 1, 4, 4, 0, 1),          # one token, one K step
    (1, 3, 16, 4, 8, 0, 1),         # exactly one MFMA tile, dv != dk
    (2, 2, 49, 8, 8, 3, 0.35),      # ragged tile, the zoo shape; a row maximum that matters
    (1, 2, 65, 20, 12, 0, 1),       # one row into the second query and key block; dims not multiples of 16
    (2, 1, 64, 64, 64, 0, 0.5),     # full blocks, the largest dims
    (1, 2, 256, 16, 64, 0, 0.5),    # the upper T, four key blocks of dQ contributions
    (3, 5, 130, 12, 4, 0, 0.5),     # odd counts everywhere
]
# The scales: float32 resolves a score s to about |s| * 2^-24, which is the relative error of exp(s), so plain
# float32 torch misses a quarter of the 1e-6 bound on O at unit scale in the last three cases and in the shifted
# one (scores near 25); at these scales it is within it everywhere except T = 256, where the 256-term float32
# sums of P V leave 2.8e-7 at any scale (profiles/attention/NOTES.md).


def _r(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator(device="cpu").manual_seed(seed))


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def inputs(case):
    B, h, T, dk, dv, shift, scale = case
    q, k, v, do = (_r(B, T, h * d, seed=i) for i, d in enumerate((dk, dk, dv, dv), 1))
    return (q + shift) * scale, (k + shift) * scale, v, do


def reference(case, dtype):
    """(O, lse, dQ, dK, dV) of the attention formula, written out in torch ops at ``dtype`` on the CPU."""
    B, h, T, dk, dv = case[:5]
    q, k, v, do = (t.to(dtype).requires_grad_(True) for t in inputs(case))
    qh, kh, vh = (t.view(B, T, h, -1).transpose(1, 2) for t in (q, k, v))
    s = qh @ kh.transpose(-1, -2) / dk ** 0.5
    o = (torch.softmax(s, -1) @ vh).transpose(1, 2).reshape(B, T, h * dv)
    o.backward(do.detach())
    return dict(o=o.detach(), lse=torch.logsumexp(s, -1).detach(), dq=q.grad, dk=k.grad, dv=v.grad)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_mha_fwd_bwd(case):
    from tensorflow_distributed_example_amd.ops import layer_ops32 as O32
    B, h, T, dk, dv = case[:5]
    ref = reference(case, torch.float64)
    q, k, v, do = (t.to(DEV) for t in inputs(case))
    o, lse = torch.zeros_like(v), torch.zeros(B, h, T, device=DEV)
    O32.mha_fwd(q, k, v, o, lse, B, h, T, dk, dv)
    runs = []
    for _ in range(2):
        dq, dk_, dv_ = torch.full_like(q, 0.5), torch.zeros_like(k), torch.zeros_like(v)
        O32.mha_bwd(q, k, v, o, lse, do, dq, dk_, dv_, B, h, T, dk, dv, accum=True)   # += onto 0.5
        runs.append((dq, dk_, dv_))
    torch.cuda.synchronize()
    errs = dict(o=_rel(o, ref["o"]), lse=_rel(lse, ref["lse"]), dq=_rel(runs[0][0], ref["dq"] + 0.5),
                dk=_rel(runs[0][1], ref["dk"]), dv=_rel(runs[0][2], ref["dv"]))
    if T == 1:   # one key: P = 1, and dS = dP - delta, so dK, is an exact zero; its error is taken relative to
        cancels = (do * v).view(B, 1, h, dv).sum(-1, keepdim=True).abs() * q.view(B, 1, h, dk).abs() / dk ** 0.5
        errs["dk"] = (runs[0][1].double().cpu().norm() / cancels.double().cpu().norm()).item()   # what cancels: |dP||Q|
        assert ref["dk"].norm() == 0
    print("attention vs float64 rel err", errs)
    assert max(errs["o"], errs["lse"]) < 1e-6 and max(errs.values()) < 1e-5, errs
    assert all(torch.equal(a, b) for a, b in zip(*runs))   # one writer, one summation order


def _model(tde, seed):
    tde.backend.set_random_seed(seed)
    m = tde.zoo.mnist_attn_cnn()
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
    att = [s for s in plan.stages if isinstance(s, LW._Attention)]
    assert [s.geom(B) for s in att] == [(16, 4, 49, 8, 8)]
    rng = np.random.default_rng(0)
    for n in st.names(trainable=True):   # biases, gamma, beta off their initial 0 and 1
        if n.endswith(("bias", "gamma", "beta")):
            st.view(n).add_(torch.from_numpy(0.3 * rng.standard_normal(st.view(n).shape).astype(np.float32)).cuda())
    xt = torch.from_numpy(rng.random((B, 28, 28, 1), dtype=np.float32)).cuda()
    yt = torch.from_numpy(rng.integers(0, 10, B)).int().cuda()
    want, _ = LW.emulate_step(plan, xt, yt)
    plan.train_step(xt, yt)
    torch.cuda.synchronize()
    errs = {n: _rel(st.grad(n), v) for n, v in want.items()}
    # the key bias: softmax does not see a shift of every score of a row, so sum_j dS_ij = 0 and the gradient
    # sum_rows dK is an exact zero; its error is taken relative to what the sum cancels from, sum_rows |dK|, at
    # the same 1e-5 (as for the bias in front of a BatchNormalization in tests/test_depthwise_gpu.py)
    nb, dK = "multi_head_attention/key/bias", att[0].qkv[1].root().grad.double().cpu().view(B * 49, 32)
    got, zero = st.grad(nb).double().cpu().view(-1), want[nb].double().cpu().view(-1)
    assert zero.norm() < 1e-12 * dK.abs().sum(0).norm()
    errs[nb] = ((got - zero).norm() / dK.abs().sum(0).norm()).item()
    print("attention CNN step vs float64 oracle rel err", errs)
    assert len(errs) == len(st.names(trainable=True)) == 20 and max(errs.values()) < 1e-5, errs


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
    inp = L.Input((28, 28, 1))   # no norm in front: the attention is the first layer without a bf16 form
    y = L.Conv2D(16, 4, strides=4)(inp)
    out = L.Dense(10)(L.GlobalAveragePooling2D()(L.MultiHeadAttention(2, 8)(y, y)))
    m = tde.keras.Model(inputs=inp, outputs=out)
    m.compile(loss=tde.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=tde.optimizers.SGD(0.05))
    x = np.zeros((64, 28, 28, 1), np.float32)
    with pytest.raises(NotImplementedError, match="multi_head_attention .MultiHeadAttention.*float32 only"):
        m.fit(x, np.zeros(64, np.int64), batch_size=64, epochs=1, verbose=0)
