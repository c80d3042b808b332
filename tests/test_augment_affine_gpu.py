"""RandomRotation / RandomZoom on the device: ``tde_stage_rows_aug``'s general source-coordinate kernel
(csrc/kernels/augment.hip) against its numpy twin (ops/augment.py) and the float64 oracle
(tests/augment_affine_oracle.py), and the paths that launch it.

Bounds.  ``params`` ([n][4 layers][4]: each layer's own draws) and the pixels of "nearest" layers equal the twin's
bit for bit: device and twin round every operation of a draw and of a source coordinate alike.  A "bilinear" pixel
lies within tests/test_augment_affine.py's bilinear bound of float64 evaluated at the device's own ``params`` (the
coordinates are the twin's; only the weighted sum may contract a multiply-add, inside the bound's 6 u M), plus
half a bf16 ulp of the value when the ring is bf16 (|v| 2^-8 bounds it).  Where a ring of a ``fit`` is compared
with the twin alone, twin and device each obey the bound against float64, so they lie within twice the bound of
each other.  The fit against the float64 small-net oracle reuses tests/smallnet_oracle.py's bound.
"""
import ctypes

import numpy as np
import pytest
import torch

import augment_affine_oracle as FO
import smallnet_oracle as SO
import tensorflow_distributed_example_amd as tde
from tensorflow_distributed_example_amd import _native as N
from tensorflow_distributed_example_amd.models import zoo
from tensorflow_distributed_example_amd.ops import augment as AU

pytestmark = pytest.mark.gpu

L = tde.keras.layers
SHAPES = [(1, 1, 1), (5, 7, 1), (4, 4, 3), (8, 8, 4), (28, 28, 1)]
FILLS = L.RandomRotation.FILL_MODES
INTERPS = L.RandomRotation.INTERPOLATIONS
FILL = 0.125
KEYS = {"RandomFlip": ("hflip", "vflip"), "RandomTranslation": ("dy", "dx"), "RandomRotation": ("f",),
        "RandomZoom": ("zh", "zw")}


def _launch(src, idx, n, B, shape, spec, step0, prefill=-7.0):
    """-> (dst [n, H, W, C] on the host, params [n, width], bad)."""
    dst = torch.full((n,) + shape, prefill, dtype=src.dtype, device="cuda")
    params = torch.full((n, AU.params_width(spec)), -1.0, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    it = None if idx is None else torch.from_numpy(idx).cuda()
    AU.stage_rows(src, src.shape[0], it, n, B, shape, dst, spec, step0, bad, params)
    torch.cuda.synchronize()
    return dst.cpu(), params.cpu().numpy(), int(bad.item())


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _raw(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _twin_params(spec, n, B, step0, H, W):
    return np.concatenate([AU.row_params(spec, step0 + s, min(B, n - s * B), H, W) for s in range((n + B - 1) // B)])


def _device_draws(stage, prow):
    """The oracle's draws of one row from the device's params row [16]: flip (hflip, vflip), translation (dy, dx),
    rotation (f, c, s), zoom (zh, zw)."""
    return [{k: (bool(prow[4 * j + q]) if k in ("hflip", "vflip") else float(prow[4 * j + q]))
             for q, k in enumerate(KEYS[type(l).__name__])} for j, l in enumerate(stage)]


def _check_bilinear(got, xg, stage, params, ext, rotation, dtype, where):
    M = max(float(np.abs(xg).max()), FILL)
    bound = FO.bilinear_bound(ext, M, rotation)
    ol = [FO.layer_of(l) for l in stage]
    g64 = got.double().numpy()
    for i in range(len(xg)):
        ref = FO.transform(xg[i], ol, _device_draws(stage, params[i]))
        tol = bound + (np.maximum(np.abs(g64[i]), np.abs(ref)) * 2.0 ** -8 if dtype == torch.bfloat16 else 0.0)
        err = np.abs(g64[i] - ref)
        assert (err <= tol).all(), (where, i, float(err.max()), bound)


def _cases():
    return [("turn", lambda **kw: L.RandomRotation((-0.3, 1.0), seed=4, **kw), True),
            ("zoom_same", lambda **kw: L.RandomZoom((-0.5, 0.7), seed=6, **kw), False),
            ("zoom_both", lambda **kw: L.RandomZoom((-0.9, 0.3), (-0.2, 1.0), seed=8, **kw), False)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_against_twin_and_oracle(shape, dtype):
    rng = np.random.default_rng(5)
    H, W, C = shape
    nrows, n, B = 11, 4, 3                # two steps: rows 0..2 at step0 (2^32 - 1), row 3 past 2^32
    step0 = 2 ** 32 - 1
    x = torch.from_numpy(rng.standard_normal((nrows,) + shape).astype(np.float32)).to(dtype)
    src = x.cuda()
    xf = x.float().numpy()
    for tag, make, rot in _cases():
        for fm in FILLS:
            for ip in INTERPS:
                stage = [make(fill_mode=fm, interpolation=ip, fill_value=FILL)]
                spec = AU.stage_spec(stage)
                for idx in (None, rng.permutation(nrows)[:n].astype(np.int32)):
                    where = (tag, fm, ip, idx is None)
                    got, params, bad = _launch(src, idx, n, B, shape, spec, step0)
                    assert bad == 0, where
                    assert np.array_equal(_bits(params), _bits(_twin_params(spec, n, B, step0, H, W))), where
                    xg = xf[:n] if idx is None else xf[idx]
                    if ip == "nearest":
                        want = torch.from_numpy(AU.apply(spec, xg, B, step0)).to(dtype)
                        assert torch.equal(_raw(got), _raw(want)), where
                    else:
                        _check_bilinear(got, xg, stage, params, max(H, W), rot, dtype, where)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_composed_layers(dtype):
    """Flip + nearest rotation + bilinear zoom + nearest translation as one launch; and four point maps."""
    rng = np.random.default_rng(6)
    shape, n, B = (8, 8, 4), 9, 4
    x = torch.from_numpy(rng.standard_normal((n,) + shape).astype(np.float32)).to(dtype)
    xf = x.float().numpy()
    stage = [L.RandomFlip(seed=2), L.RandomRotation(0.2, fill_mode="wrap", interpolation="nearest", seed=3),
             L.RandomZoom(0.3, fill_mode="constant", seed=5, fill_value=FILL),
             L.RandomTranslation(0.2, 0.2, fill_mode="reflect", interpolation="nearest", seed=7)]
    spec = AU.stage_spec(stage)
    got, params, _ = _launch(x.cuda(), None, n, B, shape, spec, 7)
    assert np.array_equal(_bits(params), _bits(_twin_params(spec, n, B, 7, 8, 8)))
    twin = AU.apply(spec, xf, B, 7)
    M = max(float(np.abs(xf).max()), FILL)
    # twin and device compute the same coordinates bit for bit; their weighted sums differ by a contraction at most
    tol = 2 * 6 * FO.U * M + (np.maximum(np.abs(twin), np.abs(got.float().numpy())) * 2.0 ** -8
                              if dtype == torch.bfloat16 else 0.0)
    assert (np.abs(got.float().numpy() - twin) <= tol).all()
    assert not np.array_equal(twin, xf)
    stage = [L.RandomRotation(1.0, fill_mode="reflect", interpolation="nearest", seed=4), L.RandomFlip(seed=2),
             L.RandomZoom((-0.5, 1.0), (-1.0, 0.5), fill_mode="constant", interpolation="nearest", seed=9,
                          fill_value=-2.0),
             L.RandomTranslation(0.25, 1.0, fill_mode="wrap", interpolation="nearest", seed=11)]
    spec = AU.stage_spec(stage)
    got, params, _ = _launch(x.cuda(), None, n, B, shape, spec, 7)
    assert np.array_equal(_bits(params), _bits(_twin_params(spec, n, B, 7, 8, 8)))
    assert torch.equal(_raw(got), _raw(torch.from_numpy(AU.apply(spec, xf, B, 7)).to(dtype)))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_identity_specs_reproduce_the_gather(shape, dtype):
    rng = np.random.default_rng(7)
    nrows, n = 40, 65
    x = torch.from_numpy(rng.standard_normal((nrows,) + shape).astype(np.float32)).to(dtype)
    x.view(-1)[::5] = -0.0
    src = x.cuda()
    idx = rng.integers(0, nrows, n).astype(np.int32)
    want = x[torch.from_numpy(idx).long()]
    for fm in FILLS:
        for ip in INTERPS:
            kw = dict(fill_mode=fm, interpolation=ip, fill_value=FILL)
            for stage in ([L.RandomRotation(0, **kw)], [L.RandomZoom(0, **kw)], [L.RandomZoom(0, 0, **kw)],
                          [L.RandomRotation((1.0, 1.0), **kw), L.RandomZoom(0, interpolation="nearest")]):
                spec = AU.stage_spec(stage)
                got, params, bad = _launch(src, idx, n, 3, shape, spec, 11)
                assert bad == 0
                assert np.array_equal(_bits(params), _bits(_twin_params(spec, n, 3, 11, shape[0], shape[1])))
                assert torch.equal(got.view(torch.uint8), want.view(torch.uint8)), [l.get_config() for l in stage]


def test_bad_index_and_refused_calls():
    rng = np.random.default_rng(8)
    shape, nrows, n = (5, 7, 1), 6, 8
    src = torch.from_numpy(rng.standard_normal((nrows,) + shape).astype(np.float32)).cuda()
    spec = AU.stage_spec([L.RandomRotation(0.25, seed=2), L.RandomZoom(0.25, interpolation="nearest", seed=4)])
    idx = np.array([0, 5, nrows, 2, -1, 3, 2 ** 31 - 1, 1], dtype=np.int32)
    good = np.array([0, 5, 0, 2, 0, 3, 0, 1], dtype=np.int32)
    got, params, bad = _launch(src, idx, n, 3, shape, spec, 2)
    ref, rparams, rbad = _launch(src, good, n, 3, shape, spec, 2)
    assert bad == 1 and rbad == 0 and params.shape == (n, 16)
    for i in range(n):
        if idx[i] == good[i]:
            assert torch.equal(got[i], ref[i]) and np.array_equal(params[i], rparams[i])
        else:   # the destination row and its params stay as they were
            assert (got[i] == -7.0).all() and (params[i] == -1.0).all()
    # refused: two interpolating layers of the new kinds, ranges and flags outside the definition; nothing written
    lib = N.hip()
    dst = torch.full((n,) + shape, -7.0, device="cuda")
    bad_t = torch.zeros(1, dtype=torch.int32, device="cuda")
    it = torch.from_numpy(good).cuda()

    def call(sp):
        return lib.tde_stage_rows_aug(src.data_ptr(), 0, nrows, it.data_ptr(), n, 3, 5, 7, 1, dst.data_ptr(),
                                      ctypes.byref(sp), 2, None, bad_t.data_ptr(), N.stream_ptr())

    def raw(*layers):
        sp = AU.AugSpec()
        sp.n = len(layers)
        for k, l in enumerate(layers):
            sp.layer[k] = l
        return sp

    rot = AU.rotate_layer((-0.1, 0.1), "reflect", "bilinear", 0.0, 0, 1)
    zoom = AU.zoom_layer((-0.1, 0.1), None, "reflect", "bilinear", 0.0, 1, 1)
    move = AU.translate_layer((-0.1, 0.1), (-0.1, 0.1), "reflect", "bilinear", 0.0, 1, 1)
    wide = AU.rotate_layer((-1.5, 0.1), "reflect", "nearest", 0.0, 0, 1)
    nan = AU.zoom_layer((float("nan"), 0.1), None, "reflect", "nearest", 0.0, 0, 1)
    flag = AU.zoom_layer((-0.1, 0.1), None, "reflect", "nearest", 0.0, 0, 1)
    flag.pad_ = 2
    mode = AU.rotate_layer((-0.1, 0.1), "reflect", "nearest", 0.0, 0, 1)
    mode.mode = 4
    for sp in (raw(rot, zoom), raw(rot, move), raw(zoom, zoom), raw(wide), raw(nan), raw(flag), raw(mode)):
        assert call(sp) != 0
    torch.cuda.synchronize()
    assert (dst == -7.0).all() and int(bad_t.item()) == 0
    assert call(spec) == 0
    torch.cuda.synchronize()
    assert torch.equal(dst.cpu(), ref)


# ------------------------------------------------------------------------------------ plans and paths
def _stage(interpolation="nearest"):
    return [L.RandomRotation(0.05, interpolation=interpolation, seed=31), L.RandomZoom(0.1, interpolation="nearest")]


def _compiled(base, stage, spe=1, lr=0.05):
    m = zoo.with_input_stage(base, stage) if stage is not None else base
    m.compile(tde.keras.optimizers.SGD(lr), tde.keras.losses.SparseCategoricalCrossentropy(from_logits=True),
              metrics=["accuracy"], steps_per_execution=spe)
    return m


class _Rings(tde.keras.callbacks.Callback):
    """The x ring of replica 0 after every execution."""

    def __init__(self):
        super().__init__()
        self.rings = []

    def on_train_batch_end(self, batch, logs=None):
        prog = next(p for k, p in self.model._programs.items() if k[0] == "train")
        prog.sync()
        self.rings.append(prog.x_ring[0].detach().float().cpu().clone())


def _data(n, seed=9):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, 28, 28, 1)).astype(np.float32), rng.integers(0, 10, n)


def _fit_rings(m, x, y, batch, **kw):
    cb = _Rings()
    m.fit(x, y, batch_size=batch, shuffle=False, verbose=0, callbacks=[cb], **kw)
    return cb.rings


@pytest.mark.parametrize("interpolation", ["nearest", "bilinear"])
def test_both_staging_paths_fill_the_ring_alike(interpolation, monkeypatch):
    x, y = _data(72)              # batch 16: 4 full steps as two executions of 2, then a ragged batch of 8
    rings = {}
    for path in ("feed", "host"):
        monkeypatch.setenv("TDE_DEVICE_DATA", "1" if path == "feed" else "0")
        tde.backend.clear_session()
        tde.backend.set_random_seed(0)
        m = _compiled(zoo.lenet5(), _stage(interpolation), spe=2)
        rings[path] = _fit_rings(m, x, y, 16)
        assert m._device_feed == (path == "feed")
        prog = next(p for k, p in m._programs.items() if k[0] == "train")
        ring_dtype = prog.x_ring[0].dtype
        spec = prog.aug
    assert len(rings["feed"]) == len(rings["host"]) == 3
    for a, b in zip(rings["feed"], rings["host"]):
        assert torch.equal(a, b)
    xs = torch.from_numpy(x).to(ring_dtype).float().numpy()      # what the cache holds
    M = float(np.abs(xs).max())

    def check(got, twin):
        if interpolation == "nearest":
            assert torch.equal(got, torch.from_numpy(twin).to(ring_dtype).float())
        else:   # the same coordinates; the weighted sums each within 6 u M of the exact sum
            tol = 2 * 6 * FO.U * M + (np.maximum(np.abs(twin), np.abs(got.numpy())) * 2.0 ** -8
                                      if ring_dtype == torch.bfloat16 else 0.0)
            assert (np.abs(got.numpy() - twin) <= tol).all()

    for e in range(2):
        check(rings["feed"][e].reshape(32, 28, 28, 1), AU.apply(spec, xs[e * 32:(e + 1) * 32], 16, 2 * e))
    check(rings["feed"][2].reshape(-1)[: 8 * 784].reshape(8, 28, 28, 1), AU.apply(spec, xs[64:72], 8, 4))
    assert not torch.equal(rings["feed"][0].reshape(32, 28, 28, 1), torch.from_numpy(xs[:32]))   # pixels did move


@pytest.mark.parametrize("name,kind", [("mnist_cnn", None), ("lenet5", "fused_smallnet"), ("mnist_bn_cnn", None)])
def test_plan_class_unchanged_by_a_rotation_and_zoom_stage(name, kind):
    from tensorflow_distributed_example_amd.train import program as PG
    plain = getattr(zoo, name)()
    aug = zoo.with_input_stage(getattr(zoo, name)(), _stage("bilinear"))
    plans = []
    for m in (plain, aug):
        logits = getattr(m.layers[-1], "activation", None) != "softmax"
        m.compile("sgd", tde.keras.losses.SparseCategoricalCrossentropy(from_logits=logits), metrics=["accuracy"])
        plans.append(PG.make_plan(m, m._store, "cuda", 8, 8, m.optimizer, m.loss))
    assert type(plans[0]) is type(plans[1]) and plans[0].kind == plans[1].kind
    assert plans[0].kind not in ("reference", "layerwise") and (kind is None or plans[0].kind == kind)
    if name == "mnist_cnn":
        assert isinstance(plans[1], PG.ConvNetPlan)


@pytest.mark.parametrize("graph", ["1", "0"], ids=["graph", "eager"])
def test_lenet5_fit_follows_the_float64_oracle_on_the_twins_inputs(graph, monkeypatch):
    monkeypatch.setenv("TDE_GRAPH", graph)
    tde.backend.set_global_policy("float32")
    steps, B, lr = 3, 8, 0.05
    x, y = _data(steps * B, seed=12)
    plain = zoo.lenet5()
    m = _compiled(plain, _stage("nearest"), spe=1, lr=lr)
    st = m._store
    names = st.names(trainable=True)
    w0 = {n: st.view(n).detach().cpu().double().clone() for n in names}
    m.fit(x, y, batch_size=B, shuffle=False, verbose=0)
    prog = next(p for k, p in m._programs.items() if k[0] == "train")
    prog.sync()
    assert prog.plan_kind == "fused_smallnet" and prog.use_graph == (graph == "1") and m.optimizer.iterations == steps
    got = {n: st.view(n).detach().cpu().double().clone() for n in names}
    spec = prog.aug
    assert AU.is_affine(spec)
    traj = {}
    for dt in (torch.float64, torch.float32):
        W = {n: w.clone().to(dt) for n, w in SO._weights(plain, st, dt, False).items()}
        W.update({n: w0[n].to(dt) for n in names})
        for k in range(steps):
            xk = torch.from_numpy(AU.apply(spec, x[k * B:(k + 1) * B], B, k))
            orc = SO.oracle(plain, st, xk, torch.from_numpy(y[k * B:(k + 1) * B]), B, B, None, dt, weights=W)
            W = {n: (w - lr * orc["grads"][n].to(dt)) if n in orc["grads"] else w for n, w in W.items()}
        traj[dt] = W
    for n in names:
        d64 = traj[torch.float64][n].double() - w0[n]
        e, r = SO.rel(got[n] - w0[n], d64), SO.rel(traj[torch.float32][n].double() - w0[n], d64)
        print(f"[{graph}] delta {n}: kernel {e:.3g} cpu-fp32 {r:.3g} bound {SO.bound(r):.3g}")
        assert e <= SO.bound(r), (n, e, r)
    # and the untransformed inputs give other weights: the stage did run
    W = {n: w.clone() for n, w in SO._weights(plain, st, torch.float64, False).items()}
    W.update(w0)
    for k in range(steps):
        orc = SO.oracle(plain, st, torch.from_numpy(x[k * B:(k + 1) * B]), torch.from_numpy(y[k * B:(k + 1) * B]), B, B,
                        None, torch.float64, weights=W)
        W = {n: (w - lr * orc["grads"][n]) if n in orc["grads"] else w for n, w in W.items()}
    assert max(SO.rel(got[n] - w0[n], W[n] - w0[n]) for n in names) > 1e-2


def test_same_seed_same_rings_and_restored_iterations():
    x, y = _data(96)

    def stage():
        return [L.RandomRotation(0.05), L.RandomZoom(0.1, interpolation="nearest")]      # unseeded layers

    runs = []
    for _ in range(2):
        tde.backend.clear_session()
        tde.backend.set_random_seed(0)
        runs.append(_fit_rings(_compiled(zoo.lenet5(), stage()), x, y, 16))
    assert len(runs[0]) == 6 and all(torch.equal(a, b) for a, b in zip(*runs))
    assert not torch.equal(runs[0][0], torch.from_numpy(x[:16]).reshape(runs[0][0].shape))
    m = _compiled(zoo.lenet5(), stage())
    k = 3
    m._set_iterations(k)
    after = _fit_rings(m, x[16 * k:], y[16 * k:], 16)
    assert torch.equal(after[0], runs[0][k]) and torch.equal(after[1], runs[0][k + 1])
    m2 = _compiled(zoo.lenet5(), stage())
    assert not torch.equal(_fit_rings(m2, x[16 * k:], y[16 * k:], 16)[0], runs[0][k])
