"""The depthwise kernels (csrc/kernels/depthwise.hip) against float64 torch (``F.conv2d(groups=C)`` with
autograd), the wrappers' host validation, and DepthwiseConv2D / SeparableConv2D through the float32 layer-wise
plan and ``fit``.  Bounds as in tests/test_layers_f32_gpu.py: 1e-6 per kernel, 1e-5 per variable of a step."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("fp32_policy")]
DEV = "cuda"

CASES = [  # B, H, W, C, dm, kh, kw, sh, sw, padding[, x's storage offset in floats]
    (2, 5, 5, 1, 1, 3, 3, 1, 1, "same"),       # C = 1 scalar form, image smaller than a tile
    (2, 9, 7, 3, 2, 3, 3, 1, 1, "valid"),      # C % 4 != 0, dm = 2, odd extents
    (3, 16, 14, 8, 1, 3, 3, 2, 2, "same"),     # stride 2, asymmetric same pads (0, 1), phase taps in dgrad
    (2, 12, 12, 36, 1, 5, 5, 1, 1, "same"),    # channel-block tail, 5x5 accumulator dealing
    (2, 10, 10, 4, 4, 3, 3, 2, 2, "valid"),    # dm = 4 with stride
    (1, 11, 13, 8, 1, 3, 5, 2, 1, "same"),     # non-square kernel and strides
    (1, 14, 14, 16, 1, 7, 7, 1, 1, "same"),    # 7x7, halo larger than the tile interior
    (7, 20, 20, 16, 1, 3, 3, 1, 1, "same"),    # several wgrad splits with a ragged last one
    (2, 8, 8, 6, 8, 7, 7, 1, 1, "same"),       # scalar form, 48 outputs x 7 kernel rows > a workgroup's threads
    (2, 8, 8, 8, 8, 5, 5, 1, 1, "same", 1),    # x off 16-byte alignment: scalar form on the vector form's tiles
]


def _r(*shape, seed=0, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _c64(t):
    return t.detach().double().cpu()


def _geom(B, H, W, C, dm, kh, kw, sh, sw, pad):
    from tensorflow_distributed_example_amd.models.layers import tf_same_pads
    from tensorflow_distributed_example_amd.ops.layer_ops import ConvGeom
    if pad == "same":
        pads = tf_same_pads(H, kh, sh), tf_same_pads(W, kw, sw)
        Ho, Wo = -(-H // sh), -(-W // sw)
    else:
        pads = (0, 0), (0, 0)
        Ho, Wo = (H - kh) // sh + 1, (W - kw) // sw + 1
    return ConvGeom(B, H, W, C, Ho, Wo, C * dm, kh, kw, sh, sw, pads[0][0], pads[1][0]), pads


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_dw_fwd_dgrad_wgrad(case):
    from tensorflow_distributed_example_amd.ops import layer_ops32 as O32
    (B, H, W, C, dm, kh, kw, sh, sw, pad), off = case[:10], (case[10:] or (0,))[0]
    g, ((pt, pb), (pl, pr)) = _geom(B, H, W, C, dm, kh, kw, sh, sw, pad)
    x = _r(B * H * W * C + off, seed=1)[off:].view(B, H, W, C)
    assert x.data_ptr() % 16 == 4 * off
    w, bias = _r(kh, kw, C, dm, seed=2, scale=0.3), _r(g.Co, seed=3)
    dy = _r(B, g.Ho, g.Wo, g.Co, seed=4)
    xr, wr, br = (_c64(t).requires_grad_(True) for t in (x, w, bias))
    o = F.conv2d(F.pad(xr.permute(0, 3, 1, 2), (pl, pr, pt, pb)), wr.reshape(kh, kw, 1, g.Co).permute(3, 2, 0, 1),
                 stride=(sh, sw), groups=C).permute(0, 2, 3, 1)
    ref = F.relu(o + br)
    ref.backward(_c64(dy))
    y = torch.zeros(B, g.Ho, g.Wo, g.Co, device=DEV)
    O32.dw_fwd(x, w, y, g, bias=bias, relu=True)
    dx = torch.full((B, H, W, C), 0.5, device=DEV)
    O32.dw_dgrad(dy, w, dx, g, y=y, accum=True)   # ReLU mask from y, += onto 0.5
    S = O32.dw_splits(g)
    if B == 7:
        assert S > 1 and (B * g.Ho * g.Wo) % S != 0
    part = torch.empty(O32.dw_part_elems(g), device=DEV)
    runs = []
    for _ in range(2):
        dW, db = torch.zeros_like(w), torch.zeros_like(bias)
        O32.dw_wgrad(x, dy, dW, g, part, y=y, db=db)
        runs.append((dW, db))
    torch.cuda.synchronize()
    errs = dict(y=_rel(y, ref), dx=_rel(dx, xr.grad + 0.5), dW=_rel(runs[0][0], wr.grad), db=_rel(runs[0][1], br.grad))
    print("depthwise vs float64 rel err", errs, "splits", S)
    assert max(errs.values()) < 1e-6, errs
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])   # fixed-order reduction


def test_wrappers_validate_before_launching():
    from tensorflow_distributed_example_amd.ops import layer_ops32 as O32
    g, _ = _geom(2, 8, 8, 4, 1, 3, 3, 1, 1, "same")
    x, w, y = torch.zeros(2, 8, 8, 4), torch.zeros(3, 3, 4, 1), torch.zeros(2, 8, 8, 4)   # host tensors: never launched
    with pytest.raises(ValueError, match="dw_fwd y"):
        O32.dw_fwd(x, w, y.view(-1)[:-1], g)
    with pytest.raises(ValueError, match="dw_fwd x"):
        O32.dw_fwd(torch.zeros(2, 8, 4, 8).transpose(2, 3), w, y, g)
    g9, _ = _geom(2, 12, 12, 4, 1, 9, 9, 1, 1, "same")
    with pytest.raises(ValueError, match="9x9"):
        O32.dw_fwd(torch.zeros(2, 12, 12, 4), torch.zeros(9, 9, 4, 1), torch.zeros(2, 12, 12, 4), g9)
    g16, _ = _geom(2, 8, 8, 4, 16, 3, 3, 1, 1, "same")
    with pytest.raises(ValueError, match="depth multiplier 16"):
        O32.dw_wgrad(x, torch.zeros(2, 8, 8, 64), torch.zeros(3, 3, 4, 16), g16, torch.zeros(1 << 16))


def _model(tde, seed):
    tde.backend.set_random_seed(seed)
    m = tde.zoo.mnist_separable_cnn()
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
    plan = PG.make_plan(m, st, "cuda", B, B, m.optimizer, m.loss, prefer="layerwise")
    assert isinstance(plan, LW.LayerwisePlan) and plan.f32
    dws = [s for s in plan.stages if isinstance(s, LW._Depthwise)]
    assert [s.wname for s in dws] == ["separable_conv2d/depthwise_kernel", "depthwise_conv2d/depthwise_kernel"]
    assert any(isinstance(s, LW._Gemm) and s.wname == "separable_conv2d/pointwise_kernel" for s in plan.stages)
    rng = np.random.default_rng(0)
    xt = torch.from_numpy(rng.random((B, 28, 28, 1), dtype=np.float32)).cuda()
    yt = torch.from_numpy(rng.integers(0, 10, B)).int().cuda()
    want, _ = LW.emulate_step(plan, xt, yt)
    plan.train_step(xt, yt)
    torch.cuda.synchronize()
    errs = {n: _rel(st.grad(n) if st.segments[n].trainable else st.view(n), v) for n, v in want.items()}
    # the bias in front of BatchNormalization: its gradient sum_rows dy is an exact zero (the mean cancels the
    # bias), so its error is taken relative to what the sum cancels from, sum_rows |dy|, at the same 1e-5
    nb, dy = "depthwise_conv2d/bias", _c64(dws[1].out.root().grad).view(B * 49, 32)
    assert dws[1].bname == nb and _c64(want[nb]).norm() < 1e-12 * dy.abs().sum(0).norm()
    errs[nb] = ((_c64(st.grad(nb)) - _c64(want[nb])).norm() / dy.abs().sum(0).norm()).item()
    print("separable CNN step vs float64 oracle rel err", errs)
    assert len(errs) == len(st.names(trainable=True)) + 2 and max(errs.values()) < 1e-5, errs


def test_fit_evaluate_predict():
    import tensorflow_distributed_example_amd as tde
    from tensorflow_distributed_example_amd.train import program as PG
    m = _model(tde, 4)
    rng = np.random.default_rng(5)
    x = rng.random((64 * 8, 28, 28, 1), dtype=np.float32)
    y = x.reshape(len(x), -1)[:, :10].argmax(1).astype(np.int64)   # learnable labels
    h = m.fit(x, y, batch_size=64, epochs=3, verbose=0).history["loss"]
    prog = m._program("train", 64)
    assert prog.plan_kind == "layerwise" and prog.plans[0].compute_dtype == "fp32" and prog.use_graph
    assert np.isfinite(h).all() and h[-1] < h[0], h
    assert np.isfinite(m.evaluate(x[:128], y[:128], batch_size=64, verbose=0)).all()
    got = m.predict(x[:64], batch_size=64, verbose=0)
    ref = PG.ReferencePlan(m, m._store.clone_to("cpu"), "cpu", 64, 64, None, m.loss)
    assert _rel(torch.as_tensor(got), ref.predict(torch.from_numpy(x[:64]), 64)) < 1e-5


def test_mixed_bfloat16_is_refused_by_name():
    import tensorflow_distributed_example_amd as tde
    tde.backend.set_global_policy("mixed_bfloat16")
    m = _model(tde, 0)
    x = np.zeros((64, 28, 28, 1), np.float32)
    with pytest.raises(NotImplementedError, match="separable_conv2d .SeparableConv2D.*float32 only"):
        m.fit(x, np.zeros(64, np.int64), batch_size=64, epochs=1, verbose=0)
