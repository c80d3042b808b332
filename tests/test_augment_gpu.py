"""The input stage on the device: ``tde_stage_rows_aug`` (csrc/kernels/augment.hip) against its numpy twin
(ops/augment.py) and the float64 oracle (tests/augment_oracle.py), and the paths that launch it.

Bounds.  ``params`` and the pixels of flips and "nearest" translations equal the twin's bit for bit.  A
"bilinear" pixel lies within 6 * 2^-24 * max|x| of float64 evaluated at the device's own ``params`` (four f32
weights, four products, three adds), plus half a bf16 ulp of the value when the ring is bf16 (|v| 2^-8 bounds
it).  Every row of every launch carries that bound: the oracle's array form (``transform_grid``, which
tests/test_augment.py holds equal to its per-pixel loops bit for bit) is cheap enough for that.  Where a ring of
a ``fit`` is compared with the twin alone, twin and device each obey the bound against float64, so they lie
within twice the bound of each other (triangle inequality).  The fit against the float64 small-net oracle reuses
tests/smallnet_oracle.py's bound.
"""
import ctypes
import json
import os
import signal
import subprocess
import sys

import numpy as np
import pytest
import torch

import augment_oracle as AO
import smallnet_oracle as SO
import tensorflow_distributed_example_amd as tde
from tensorflow_distributed_example_amd import _native as N
from tensorflow_distributed_example_amd.models import zoo
from tensorflow_distributed_example_amd.ops import augment as AU

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = tde.keras.layers
SHAPES = [(1, 1, 1), (5, 7, 1), (4, 4, 3), (8, 8, 4), (28, 28, 1)]
FACTORS = [0, 0.25, (-0.5, 0.1), 1.0]
FILL = 0.125


def _configs():
    """(tag, stage layers, kind): kind "exact" or "bilinear"."""
    out = [(f"flip_{m}", [L.RandomFlip(m, seed=2)], "exact") for m in L.RandomFlip.MODES]
    for f in FACTORS:
        for fm in L.RandomTranslation.FILL_MODES:
            for ip in L.RandomTranslation.INTERPOLATIONS:
                out.append((f"move_{f}_{fm}_{ip}", [L.RandomTranslation(f, f, fill_mode=fm, interpolation=ip, seed=4,
                                                                        fill_value=FILL)],
                            "exact" if ip == "nearest" or f == 0 else "bilinear"))
    return out


def _idx(kind, n, nrows, rng):
    if kind == "null":
        return None
    if kind == "reversed":
        return np.arange(nrows - 1, nrows - 1 - n, -1, dtype=np.int32)
    return (rng.integers(0, nrows, n) // 2 * 2 % nrows).astype(np.int32)   # with repeats


def _launch(src, idx, n, B, shape, spec, step0, prefill=-7.0):
    """-> (dst [n, H, W, C] on the host, params [n, 4], bad)."""
    dst = torch.full((n,) + shape, prefill, dtype=src.dtype, device="cuda")
    params = torch.full((n, 4), -1.0, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    it = None if idx is None else torch.from_numpy(idx).cuda()
    AU.stage_rows(src, src.shape[0], it, n, B, shape, dst, spec, step0, bad, params)
    torch.cuda.synchronize()
    return dst.cpu(), params.cpu().numpy(), int(bad.item())


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _twin_params(spec, n, B, step0, H, W):
    return np.concatenate([AU.row_params(spec, step0 + s, min(B, n - s * B), H, W) for s in range((n + B - 1) // B)])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_against_twin_and_oracle(shape, dtype):
    rng = np.random.default_rng(5)
    H, W, C = shape
    nrows = 70
    x = torch.from_numpy(rng.standard_normal((nrows,) + shape).astype(np.float32)).to(dtype)
    src = x.cuda()
    xf = x.float().numpy()
    bound = AO.BILINEAR_BOUND * float(np.abs(xf).max())
    worst = 0.0
    step0 = 2 ** 32 - 2 if dtype == torch.float32 else 3      # the step crosses 2^32 in the f32 runs
    for tag, stage, kind in _configs():
        spec = AU.stage_spec(stage)
        olayers = [AO.layer_of(l, j, l.resolved_seed(j)) for j, l in enumerate(stage)]
        for n in (1, 3, 65):
            for B in (1, 3, 64):
                for ik in ("null", "reversed", "repeats"):
                    idx = _idx(ik, n, nrows, rng)
                    got, params, bad = _launch(src, idx, n, B, shape, spec, step0)
                    where = (tag, n, B, ik)
                    assert bad == 0, where
                    assert np.array_equal(_bits(params), _bits(_twin_params(spec, n, B, step0, H, W))), where
                    xg = xf[:n] if idx is None else xf[idx]
                    twin = AU.apply(spec, xg, B, step0)
                    want = torch.from_numpy(twin).to(dtype)
                    if kind == "exact":
                        assert torch.equal(got.view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                                           want.view(torch.int16 if dtype == torch.bfloat16 else torch.int32)), where
                        continue
                    g64 = got.double().numpy()
                    for i in range(n):   # every row: float64 at the device's own parameters
                        dr = [dict(dy=float(params[i, 2]), dx=float(params[i, 3]))]
                        ref = AO.transform_grid(xg[i], olayers, dr)
                        err = np.abs(g64[i] - ref)
                        tol = bound + (np.maximum(np.abs(g64[i]), np.abs(ref)) * 2.0 ** -8
                                       if dtype == torch.bfloat16 else 0.0)
                        worst = max(worst, float((err - (tol - bound)).max()))
                        assert (err <= tol).all(), (where, i, float(err.max()), bound)
    print(f"{shape} {dtype}: worst bilinear error beyond the bf16 rounding {worst:.3g}, bound {bound:.3g}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_composed_layers(dtype):
    """Flips around one bilinear translation, and four layers of whole-pixel moves, as one launch."""
    rng = np.random.default_rng(6)
    shape, n, B = (8, 8, 4), 9, 4
    x = torch.from_numpy(rng.standard_normal((n,) + shape).astype(np.float32)).to(dtype)
    xf = x.float().numpy()
    stage = [L.RandomTranslation(1.0, 0.25, fill_mode="reflect", interpolation="nearest", seed=4), L.RandomFlip(seed=2),
             L.RandomTranslation(0.25, 1.0, fill_mode="constant", interpolation="nearest", seed=9, fill_value=-2.0),
             L.RandomFlip("vertical")]
    spec = AU.stage_spec(stage)
    got, params, _ = _launch(x.cuda(), None, n, B, shape, spec, 7)
    assert np.array_equal(_bits(params), _bits(_twin_params(spec, n, B, 7, 8, 8)))
    assert torch.equal(got.float(), torch.from_numpy(AU.apply(spec, xf, B, 7)).to(dtype).float())
    stage = [L.RandomFlip(seed=2), L.RandomTranslation(0.5, 0.5, fill_mode="constant", seed=4, fill_value=FILL),
             L.RandomFlip("vertical", seed=8)]
    spec = AU.stage_spec(stage)
    got, params, _ = _launch(x.cuda(), None, n, B, shape, spec, 7)
    assert np.array_equal(_bits(params), _bits(_twin_params(spec, n, B, 7, 8, 8)))
    bound = AO.BILINEAR_BOUND * float(np.abs(xf).max())
    olayers = [AO.layer_of(l, j, l.resolved_seed(j)) for j, l in enumerate(stage)]
    for i in range(n):
        dr = [AO.draws(l, i % B, 7 + i // B, 8, 8) for l in olayers]
        assert float(dr[1]["dy"]) == float(params[i, 2]) and float(dr[1]["dx"]) == float(params[i, 3])
        ref = AO.transform(xf[i], olayers, dr)
        g = got[i].double().numpy()
        tol = bound + (np.maximum(np.abs(g), np.abs(ref)) * 2.0 ** -8 if dtype == torch.bfloat16 else 0.0)
        assert (np.abs(g - ref) <= tol).all(), i


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_identity_specs_reproduce_the_gather(shape, dtype):
    rng = np.random.default_rng(7)
    nrows, n = 40, 65
    x = torch.from_numpy(rng.standard_normal((nrows,) + shape).astype(np.float32)).to(dtype)
    x.view(-1)[::5] = -0.0
    src = x.cuda()
    idx = rng.integers(0, nrows, n).astype(np.int32)
    it = torch.from_numpy(idx).cuda()
    want = src[it.long()]
    row_bytes = int(np.prod(shape)) * x.element_size()
    if row_bytes % 4 == 0:     # the gather moves whole 4-byte words
        g = torch.zeros_like(want)
        bad = torch.zeros(1, dtype=torch.int32, device="cuda")
        N.check(N.hip().tde_gather_rows_dev(src.data_ptr(), row_bytes, nrows, it.data_ptr(), n, g.data_ptr(),
                                            bad.data_ptr(), N.stream_ptr()), "tde_gather_rows_dev")
        torch.cuda.synchronize()
        assert torch.equal(g.view(torch.uint8), want.view(torch.uint8))
    stages = [[]] + [[L.RandomTranslation(0, 0, fill_mode=fm, interpolation=ip)]
                     for fm in L.RandomTranslation.FILL_MODES for ip in L.RandomTranslation.INTERPOLATIONS]
    for stage in stages:
        got, params, bad = _launch(src, idx, n, 3, shape, AU.stage_spec(stage), 11)
        assert bad == 0 and not params.any()
        assert torch.equal(got.view(torch.uint8), want.cpu().view(torch.uint8)), [l.get_config() for l in stage]


def test_bad_index_and_refused_calls():
    rng = np.random.default_rng(8)
    shape, nrows, n = (5, 7, 1), 6, 8
    src = torch.from_numpy(rng.standard_normal((nrows,) + shape).astype(np.float32)).cuda()
    spec = AU.stage_spec([L.RandomFlip(seed=2), L.RandomTranslation(0.25, 0.25, seed=4)])
    idx = np.array([0, 5, nrows, 2, -1, 3, 2 ** 31 - 1, 1], dtype=np.int32)
    good = np.array([0, 5, 0, 2, 0, 3, 0, 1], dtype=np.int32)
    got, params, bad = _launch(src, idx, n, 3, shape, spec, 2)
    ref, rparams, rbad = _launch(src, good, n, 3, shape, spec, 2)
    assert bad == 1 and rbad == 0
    for i in range(n):
        if idx[i] == good[i]:
            assert torch.equal(got[i], ref[i]) and np.array_equal(params[i], rparams[i])
        else:   # the destination row and its params stay as they were
            assert (got[i] == -7.0).all() and (params[i] == -1.0).all()
    # refused: more layers than the spec holds, a layer of no kind, two interpolating layers, a null dst
    lib = N.hip()
    dst = torch.full((n,) + shape, -7.0, device="cuda")
    bad_t = torch.zeros(1, dtype=torch.int32, device="cuda")
    it = torch.from_numpy(good).cuda()

    def call(sp, dst_ptr):
        return lib.tde_stage_rows_aug(src.data_ptr(), 0, nrows, it.data_ptr(), n, 3, 5, 7, 1, dst_ptr, ctypes.byref(sp),
                                      2, None, bad_t.data_ptr(), N.stream_ptr())

    five = AU.AugSpec()
    five.n = 5
    for k in range(4):
        five.layer[k] = AU.flip_layer("horizontal", k, 1)
    odd = AU.make_spec([AU.flip_layer("horizontal", 0, 1)])
    odd.layer[0].kind = 9
    two = AU.AugSpec()
    two.n = 2
    for k in range(2):
        two.layer[k] = AU.translate_layer((-0.1, 0.1), (-0.1, 0.1), "reflect", "bilinear", 0.0, k, 1)
    for sp in (five, odd, two):
        assert call(sp, dst.data_ptr()) != 0
    assert call(spec, None) != 0
    torch.cuda.synchronize()
    assert (dst == -7.0).all() and int(bad_t.item()) == 0
    assert call(spec, dst.data_ptr()) == 0
    torch.cuda.synchronize()
    assert torch.equal(dst.cpu(), ref)


# ------------------------------------------------------------------------------------ plans and paths
def _stage(interpolation="nearest"):
    return [L.RandomTranslation(0.1, 0.1, interpolation=interpolation, seed=31), L.RandomFlip("horizontal")]


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

    def check(got, twin):
        if interpolation == "nearest":
            assert torch.equal(got, torch.from_numpy(twin).to(ring_dtype).float())
        else:   # twin and device each within the bound of float64
            tol = 2 * AO.BILINEAR_BOUND * np.abs(xs).max() + (np.maximum(np.abs(twin), np.abs(got.numpy())) * 2.0 ** -8
                                                                if ring_dtype == torch.bfloat16 else 0.0)
            assert (np.abs(got.numpy() - twin) <= tol).all()

    for e in range(2):
        check(rings["feed"][e].reshape(32, 28, 28, 1), AU.apply(spec, xs[e * 32:(e + 1) * 32], 16, 2 * e))
    # the ragged step: B is its own row count
    check(rings["feed"][2].reshape(-1)[: 8 * 784].reshape(8, 28, 28, 1), AU.apply(spec, xs[64:72], 8, 4))
    assert not torch.equal(rings["feed"][0].reshape(32, 28, 28, 1), torch.from_numpy(xs[:32]))   # pixels did move


@pytest.mark.parametrize("name,kind", [("mnist_cnn", None), ("lenet5", "fused_smallnet"), ("mnist_bn_cnn", None)])
def test_plan_class_unchanged_by_an_input_stage(name, kind):
    from tensorflow_distributed_example_amd.train import program as PG
    plain = getattr(zoo, name)()
    aug = zoo.with_input_stage(getattr(zoo, name)(), _stage("bilinear"))
    plans = []
    for m in (plain, aug):
        logits = getattr(m.layers[-1], "activation", None) != "softmax"
        m.compile("sgd", tde.keras.losses.SparseCategoricalCrossentropy(from_logits=logits), metrics=["accuracy"])
        plans.append(PG.make_plan(m, m._store, "cuda", 8, 8, m.optimizer, m.loss))
    print(name, plans[0].kind)
    assert type(plans[0]) is type(plans[1]) and plans[0].kind == plans[1].kind
    assert plans[0].kind not in ("reference", "layerwise") and (kind is None or plans[0].kind == kind)
    if name == "mnist_cnn":
        assert isinstance(plans[1], PG.ConvNetPlan)


@pytest.mark.parametrize("graph", ["1", "0"], ids=["graph", "eager"])
def test_lenet5_fit_follows_the_float64_oracle_on_the_twins_inputs(graph, monkeypatch):
    monkeypatch.setenv("TDE_GRAPH", graph)
    tde.backend.set_global_policy("float32")
    steps, B, lr = 4, 8, 0.05
    x, y = _data(steps * B, seed=12)
    plain = zoo.lenet5()
    m = _compiled(plain, _stage("nearest"), spe=2, lr=lr)
    st = m._store
    names = st.names(trainable=True)
    w0 = {n: st.view(n).detach().cpu().double().clone() for n in names}
    m.fit(x, y, batch_size=B, shuffle=False, verbose=0)
    prog = next(p for k, p in m._programs.items() if k[0] == "train")
    prog.sync()
    assert prog.plan_kind == "fused_smallnet" and prog.use_graph == (graph == "1") and m.optimizer.iterations == steps
    got = {n: st.view(n).detach().cpu().double().clone() for n in names}
    spec = prog.aug
    traj = {}
    for dt in (torch.float64, torch.float32):
        W = {n: w.clone().to(dt) for n, w in SO._weights(plain, st, dt, False).items()}
        W.update({n: w0[n].to(dt) for n in names})
        for k in range(steps):
            xk = torch.from_numpy(AU.apply(spec, x[k * B:(k + 1) * B], B, k))
            orc = SO.oracle(plain, st, xk, torch.from_numpy(y[k * B:(k + 1) * B]), B, B, None, dt, weights=W)
            W = {n: (w - lr * orc["grads"][n].to(dt)) if n in orc["grads"] else w for n, w in W.items()}
        traj[dt] = W
    plainfit = {n: traj[torch.float64][n] for n in names}
    for n in names:
        d64 = plainfit[n].double() - w0[n]
        e, r = SO.rel(got[n] - w0[n], d64), SO.rel(traj[torch.float32][n].double() - w0[n], d64)
        print(f"[{graph}] delta {n}: kernel {e:.3g} cpu-fp32 {r:.3g} bound {SO.bound(r):.3g}")
    for n in names:
        d64 = plainfit[n].double() - w0[n]
        e, r = SO.rel(got[n] - w0[n], d64), SO.rel(traj[torch.float32][n].double() - w0[n], d64)
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
    runs = []
    for _ in range(2):
        tde.backend.clear_session()
        tde.backend.set_random_seed(0)
        m = _compiled(zoo.lenet5(), [L.RandomTranslation(0.1, 0.1), L.RandomFlip()])      # unseeded layers
        runs.append(_fit_rings(m, x, y, 16))
    assert len(runs[0]) == 6 and all(torch.equal(a, b) for a, b in zip(*runs))
    assert not torch.equal(runs[0][0], torch.from_numpy(x[:16]).reshape(runs[0][0].shape))
    # the same rows at another step: another transform
    m = _compiled(zoo.lenet5(), [L.RandomTranslation(0.1, 0.1), L.RandomFlip()])
    k = 3
    m._set_iterations(k)
    after = _fit_rings(m, x[16 * k:], y[16 * k:], 16)
    assert torch.equal(after[0], runs[0][k]) and torch.equal(after[1], runs[0][k + 1])
    m2 = _compiled(zoo.lenet5(), [L.RandomTranslation(0.1, 0.1), L.RandomFlip()])
    assert not torch.equal(_fit_rings(m2, x[16 * k:], y[16 * k:], 16)[0], runs[0][k])


def test_model_without_an_input_stage_never_resolves_the_launch(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("tde_stage_rows_aug launched for a model without an input stage")

    monkeypatch.setattr(AU, "stage_rows", refuse)
    x, y = _data(40)
    for path in ("1", "0"):
        monkeypatch.setenv("TDE_DEVICE_DATA", path)
        m = _compiled(zoo.lenet5(), None, spe=2)
        m.fit(x, y, batch_size=16, shuffle=False, verbose=0)
        m.evaluate(x, y, batch_size=16, verbose=0)
        assert all(p.aug is None for p in m._programs.values())
    # evaluate / predict / validation of a model WITH an input stage launch what they launched before
    m = _compiled(zoo.lenet5(), _stage(), spe=2)
    m.evaluate(x, y, batch_size=16, verbose=0)
    m.predict(x, batch_size=16)
    assert m._programs and all(p.aug is None for p in m._programs.values())


def test_mirrored_replicas_draw_equal_transforms_for_equal_local_rows():
    env = dict(os.environ, TDE_HEARTBEAT="0", OMP_NUM_THREADS="2", TDE_XGMI_TIMEOUT="20")
    p = subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "augment_mirrored_child.py")], env=env,
                         cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, start_new_session=True)
    try:
        out, _ = p.communicate(timeout=90)
    except subprocess.TimeoutExpired:
        os.killpg(p.pid, signal.SIGKILL)
        out, _ = p.communicate()
        raise AssertionError(f"timed out:\n{out[-3000:]}")
    assert p.returncode == 0, out[-4000:]
    res = json.loads([ln for ln in out.splitlines() if ln.startswith("RESULT ")][0][7:])
    print(res)
    assert res["replicas"] == 2 and res["equal_rings"] and res["equals_twin"] and res["moved"]
