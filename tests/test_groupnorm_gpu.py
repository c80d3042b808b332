"""The group-norm kernels (csrc/kernels/groupnorm.hip) against float64 ``F.group_norm`` with autograd, the
wrappers' host validation, and GroupNormalization / LayerNormalization through the float32 layer-wise plan and
``fit``.  Bounds as in tests/test_layers_f32_gpu.py: 1e-6 for y, 1e-5 for gradients and per variable of a step."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("fp32_policy")]
DEV = "cuda"
EPS = 1e-3

CASES = [  # R, S, C, G, shift[, x's storage offset in floats]
    (3, 1, 10, 1, 0),        # a row narrower than a wave, C % 4 != 0, fewer rows than a workgroup takes
    (5, 1, 64, 1, 4),        # nonzero mean
    (4, 1, 260, 1, 0),       # more than one float4 per lane, plus a tail
    (3, 1, 2048, 1, 0),      # the upper limit
    (6, 1, 24, 3, 0),        # segmented row reduction
    (7, 1, 12, 4, 0, 1),     # D = 3 and an unaligned base
    (2501, 1, 16, 2, 0),     # several partial strips with a ragged last one
    (5, 1, 1024, 2, 0),      # a group over two register slots of a lane
    (5, 1, 80, 2, 0),        # D / 4 = 10 quads, no power of two: the LDS row form with wave folds
    (2, 35, 8, 2, 0),        # one quad per group, ragged positions
    (3, 49, 6, 6, 0),        # instance norm, D = 1, scalar channels
    (2, 63, 12, 4, 4),       # a float4 straddling two groups
    (2, 25, 20, 1, 0),       # G = 1 over an image
    (1, 196, 64, 8, 0),      # several group blocks per sample
    (2, 3136, 16, 4, 0),     # a slab past the LDS budget, which takes the two-sweep form
    (2, 3, 1028, 1, 0),      # more channel quads than threads: one position lane, a wave fold over D > 64
]


def _r(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator(device="cpu").manual_seed(seed))


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_gn_fwd_bwd(case):
    from tensorflow_distributed_example_amd.ops import layer_ops32 as O32
    (R, S, C, G, shift), off = case[:5], (case[5:] or (0,))[0]
    plan = O32.gn_plan(R, S, C, G)
    if R == 2501:
        assert plan["parts"] > 1 and R % plan["strip"] != 0
    if S > 1:
        assert plan["slab"] and (S != 196 or plan["blocks"] > 1)
        assert plan["staged_fwd"] == plan["staged_bwd"] == (S != 3136)
    x = (_r(R * S * C + off, seed=1) + shift).to(DEV)[off:].view(R, S, C)
    assert x.data_ptr() % 16 == 4 * off
    gamma, beta, dy = (1 + 0.5 * _r(C, seed=2)).to(DEV), _r(C, seed=3).to(DEV), _r(R, S, C, seed=4).to(DEV)
    xr, gr, br = (t.detach().double().cpu().requires_grad_(True) for t in (x, gamma, beta))
    ref = F.group_norm(xr.permute(0, 2, 1), G, gr, br, EPS).permute(0, 2, 1)
    ref.backward(dy.double().cpu())
    y, mean, rstd = torch.zeros_like(x), torch.zeros(R * G, device=DEV), torch.zeros(R * G, device=DEV)
    O32.gn_fwd(x, y, mean, rstd, R, S, C, G, EPS, gamma=gamma, beta=beta)
    part = torch.empty(O32.gn_part_elems(R, S, C, G), device=DEV)
    dx = torch.full((R, S, C), 0.5, device=DEV)
    runs = []
    for i in range(2):
        dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
        O32.gn_bwd(dy, x, mean, rstd, R, S, C, G, part, gamma=gamma, dx=dx if i == 0 else None, accum=True,
                   dgamma=dg, dbeta=db)
        runs.append((dg, db))
    torch.cuda.synchronize()
    errs = dict(y=_rel(y, ref), dx=_rel(dx, xr.grad + 0.5), dgamma=_rel(runs[0][0], gr.grad),
                dbeta=_rel(runs[0][1], br.grad))
    print("group norm vs float64 rel err", errs, plan)
    assert errs["y"] < 1e-6 and max(errs.values()) < 1e-5, errs
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])   # fixed-order reduction


def test_wrappers_validate_before_launching():
    from tensorflow_distributed_example_amd.ops import layer_ops32 as O32
    x, st = torch.zeros(2, 9, 8), torch.zeros(4)   # host tensors: never launched
    with pytest.raises(ValueError, match="gn_fwd y"):
        O32.gn_fwd(x, x.view(-1)[:-1], st, st, 2, 9, 8, 2, EPS)
    with pytest.raises(ValueError, match="gn_fwd x"):
        O32.gn_fwd(torch.zeros(2, 8, 9).transpose(1, 2), x, st, st, 2, 9, 8, 2, EPS)
    with pytest.raises(ValueError, match="gn_fwd rstd"):
        O32.gn_fwd(x, x, st, st[:3], 2, 9, 8, 2, EPS)
    with pytest.raises(ValueError, match="3 groups do not divide 8"):
        O32.gn_fwd(x, x, st, st, 2, 9, 8, 3, EPS)
    with pytest.raises(ValueError, match="4096 channels"):
        O32.gn_part_elems(2, 1, 4096, 1)
    with pytest.raises(ValueError, match="gn_bwd dgamma"):
        O32.gn_bwd(x, x, st, st, 2, 9, 8, 2, torch.zeros(1 << 10), dgamma=torch.zeros(8, dtype=torch.float64))
    with pytest.raises(ValueError, match="gn_bwd partials"):
        O32.gn_bwd(x, x, st, st, 2, 9, 8, 2, torch.zeros(8))


def _model(tde, seed):
    tde.backend.set_random_seed(seed)
    m = tde.zoo.mnist_gn_cnn()
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
    gns = [s for s in plan.stages if isinstance(s, LW._GroupNorm)]
    assert [s.geom(B) for s in gns] == [(B, 676, 32, 8), (B, 144, 64, 8), (B, 1, 128, 1)]
    rng = np.random.default_rng(0)
    for n in st.names(trainable=True):   # gamma, beta off their initial 1 and 0
        if n.endswith(("gamma", "beta")):
            st.view(n).add_(torch.from_numpy(0.3 * rng.standard_normal(st.view(n).shape).astype(np.float32)).cuda())
    xt = torch.from_numpy(rng.random((B, 28, 28, 1), dtype=np.float32)).cuda()
    yt = torch.from_numpy(rng.integers(0, 10, B)).int().cuda()
    want, _ = LW.emulate_step(plan, xt, yt)
    plan.train_step(xt, yt)
    torch.cuda.synchronize()
    errs = {n: _rel(st.grad(n), v) for n, v in want.items()}
    print("group-norm CNN step vs float64 oracle rel err", errs)
    assert len(errs) == len(st.names(trainable=True)) == 14 and max(errs.values()) < 1e-5, errs


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
    tde.backend.set_global_policy("mixed_bfloat16")
    m = _model(tde, 0)
    x = np.zeros((64, 28, 28, 1), np.float32)
    with pytest.raises(NotImplementedError, match="group_normalization .GroupNormalization.*float32 only"):
        m.fit(x, np.zeros(64, np.int64), batch_size=64, epochs=1, verbose=0)
