"""tanh / sigmoid / AveragePooling2D on the fused small-net plan, the parts that need no GPU: the float64
oracle of tests/smallnet_oracle.py against the repository's fp32 ``ReferencePlan`` on the CPU for every model
and batch of tests/test_smallnet_act_gpu.py (the act suite of tests/smallnet_cases.py), the input conditions at
the committed seeds, what
``match_smallnet`` accepts and refuses, the plan table's kinds and activation codes, the
``AveragePooling2D`` layer itself and its ``AvgPool`` / ``Tanh`` export.

fp32 reference vs float64, norm-wise relative, as printed by this test (run with -s; the figures move in the
last digit with the CPU's conv / GEMM kernels): lenet5_classic conv2d/bias 1.2e-6 and conv2d/kernel 1.1e-6,
every other gradient of every case <= 5.3e-7, loss <= 1e-7, predict <= 3.8e-7 -- so every GPU bound is the
1e-5 floor.  Conditions at the committed seeds: relu_near 0.021 (act_layers B=67), pool_gap 2.0e-4
(tanh_maxpool B=67, seed 1), smallest margin 2.0e-3 (avg_linear B=67).  dgrad_tanh B=37/64: margin 0.011.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import smallnet_cases as C
import smallnet_oracle as O


def _logits(tde):
    return tde.losses.SparseCategoricalCrossentropy(from_logits=True)


@pytest.mark.parametrize("name,B,Bplan", C.CASES["act"])
def test_oracle_matches_fp32_reference(name, B, Bplan):
    import tensorflow_distributed_example_amd as tde
    m, x, y = C.make_case(tde, "act", name, B, Bplan)
    orc = O.oracle(m, m._store, x, y, B, Bplan)
    ref = O.reference_errors(tde, m, x, y, B, Bplan, orc)
    tag = f"{name} B={B}/{Bplan}"
    print(f"[{tag}] relu_near={orc['relu_near']:.3g} pool_gap={orc['pool_gap']:.3g} margin={orc['margin']:.3g} "
          f"loss={ref['loss']:.2g} predict={ref['predict']:.2g}")
    for n, e in ref["grads"].items():
        print(f"[{tag}] grad {n}: {e:.2g}")
    assert O.conditions_hold(orc), (orc["relu_near"], orc["pool_gap"], orc["margin"])
    assert all(torch.isfinite(g).all() and g.abs().max() > 0 for g in orc["grads"].values())
    assert set(orc["grads"]) == set(m._store.names(trainable=True))
    for n, e in ref["grads"].items():
        assert e < O.TOL, (n, e)
    assert ref["loss"] < O.TOL and ref["eval_loss"] < O.TOL and ref["predict"] < O.TOL
    assert ref["correct"] == ref["eval_correct"] == orc["correct"] and ref["count"] == B
    assert orc["out"].shape == (B, m.output_shape[-1])


def test_conditions_measure_what_they_name():
    """A ReLU at zero, a tied max-pool window behind a tanh conv and a tied head are each seen."""
    h = torch.tensor([[[[0.5], [0.5]], [[0.1], [0.2]]]], dtype=torch.float64)       # one 2x2 window, two maxima
    assert O._window_gap(h) == 0.0
    h[0, 0, 1, 0] = 0.25
    assert O._window_gap(h) == pytest.approx(0.25 / h.pow(2).mean().sqrt().item())
    odd = torch.zeros(1, 3, 3, 1, dtype=torch.float64)      # the odd row / column belongs to no window
    odd[0, :2, :2, 0] = torch.tensor([[1.0, 0.0], [0.0, 0.0]])
    odd[0, 2, :, 0] = 1.0
    assert O._window_gap(odd) > 0


@pytest.mark.parametrize("name", list(C.MODELS["act"]))
def test_matcher_and_plan_codes(name):
    """``match_smallnet`` accepts every model with the expected entry kinds and activation codes, no other
    fused plan's matcher takes it first, and the plan table carries the codes: ``act`` the entry's own,
    ``mask_in`` that of the activation whose output is the entry's input (a pool: the conv before it)."""
    import tensorflow_distributed_example_amd as tde
    from tensorflow_distributed_example_amd.train import program as PG
    from tensorflow_distributed_example_amd.train import smallnet as SN
    assert (SN.CONV, SN.POOL, SN.DENSE, SN.AVGPOOL) == (0, 1, 2, 3)
    assert (SN.LINEAR, SN.RELU, SN.TANH, SN.SIGMOID) == (0, 1, 2, 3)
    m, _ = C.build(tde, "act", name, 5)
    kinds, codes, mask_in = C.MODELS["act"][name].codes
    assert PG.match_convnet(m, m.loss) is None
    spec = SN.match_smallnet(m, m.loss)
    assert spec is not None
    assert [s["kind"] for s in spec] == kinds and [s["relu"] for s in spec] == codes
    plan = SN.SmallNetPlan(m, m._store, "cpu", 8, 8, m.optimizer, m.loss, spec)
    col = {f: i for i, f in enumerate(SN._FIELDS)}
    assert plan.layers[:, col["kind"]].tolist() == kinds
    assert plan.layers[:, col["act"]].tolist() == codes
    assert plan.layers[:, col["mask_in"]].tolist() == mask_in
    if name == "lenet5_classic":      # the compile-time geometries X(5,5,1,6,32,32) and X(5,5,6,16,14,14)
        geo = [tuple(int(plan.layers[i, col[f]]) for f in ("kh", "kw", "C", "Co", "H", "W", "pt", "pl"))
               for i in range(len(kinds)) if kinds[i] == SN.CONV]
        assert geo == [(5, 5, 1, 6, 32, 32, 0, 0), (5, 5, 6, 16, 14, 14, 0, 0)]
    if name == "dgrad_tanh":          # conv 2 is X(5,5,6,16,14,14) and needs an input gradient through a tanh
        i = [k for k in range(len(kinds)) if kinds[k] == SN.CONV][1]
        row = {f: int(plan.layers[i, col[f]]) for f in SN._FIELDS}
        assert tuple(row[f] for f in ("kh", "kw", "C", "Co", "H", "W", "pt", "pl")) == (5, 5, 6, 16, 14, 14, 0, 0)
        assert row["need_gin"] == 1 and row["mask_in"] == SN.TANH


def test_matcher_refusals():
    import tensorflow_distributed_example_amd as tde
    from tensorflow_distributed_example_amd.train.smallnet import match_smallnet
    K = tde.keras.layers
    lg = _logits(tde)
    cases = {
        "a tanh head": [K.Dense(8, activation="relu", input_shape=(6,)), K.Dense(3, activation="tanh")],
        "a sigmoid head": [K.Dense(8, activation="relu", input_shape=(6,)), K.Dense(3, activation="sigmoid")],
        "a tanh Activation behind the head": [K.Dense(8, input_shape=(6,)), K.Dense(3), K.Activation("tanh")],
        "AveragePooling2D(3)": [K.Conv2D(4, 3, activation="tanh", input_shape=(8, 8, 2)), K.AveragePooling2D(3),
                                K.Flatten(), K.Dense(3)],
        "an average pool with stride 1": [K.Conv2D(4, 3, input_shape=(8, 8, 2)), K.AveragePooling2D(2, strides=1),
                                          K.Flatten(), K.Dense(3)],
        "a same-padded average pool": [K.Conv2D(4, 3, input_shape=(7, 7, 2)), K.AveragePooling2D(padding="same"),
                                       K.Flatten(), K.Dense(3)],
        "an average pool with no conv before it": [K.AveragePooling2D(input_shape=(8, 8, 2)), K.Flatten(), K.Dense(3)],
        "an average pool behind a pool": [K.Conv2D(4, 3, input_shape=(10, 10, 2)), K.AveragePooling2D(),
                                          K.AveragePooling2D(), K.Flatten(), K.Dense(3)],
        "a Dropout on a tanh Dense": [K.Dense(8, activation="tanh", input_shape=(6,)), K.Dropout(0.5), K.Dense(3)],
        "a Dropout on a sigmoid conv": [K.Conv2D(4, 3, activation="sigmoid", input_shape=(6, 6, 2)), K.Dropout(0.3),
                                        K.Flatten(), K.Dense(3)],
        "a Dropout on a standalone tanh": [K.Dense(8, input_shape=(6,)), K.Activation("tanh"), K.Dropout(0.5),
                                           K.Dense(3)],
        "a Dropout between a conv and its average pool": [K.Conv2D(4, 3, input_shape=(6, 6, 2)), K.Dropout(0.5),
                                                          K.AveragePooling2D(), K.Flatten(), K.Dense(3)],
        "tanh twice": [K.Dense(8, activation="tanh", input_shape=(6,)), K.Activation("tanh"), K.Dense(3)],
    }
    for why, layers in cases.items():
        assert match_smallnet(tde.Sequential(layers), lg) is None, why
    # unchanged around the new ground: Dropout behind a pool that follows a tanh conv, and behind relu
    ok = [K.Conv2D(4, 3, activation="tanh", input_shape=(6, 6, 2)), K.AveragePooling2D(), K.Dropout(0.5),
          K.Flatten(), K.Dense(8, activation="relu"), K.Dropout(0.5), K.Dense(3)]
    spec = match_smallnet(tde.Sequential(ok), lg)
    assert spec is not None and [s["drop"] is not None for s in spec] == [False, True, True, False]


def test_dropout_on_tanh_has_no_hip_plan():
    """A Dropout directly on a tanh output: neither the small-net nor the layer-wise plan takes the model (the
    ``NotImplementedError`` ``make_plan`` ends in on the GPU: tests/test_smallnet_act_gpu.py)."""
    import tensorflow_distributed_example_amd as tde
    from tensorflow_distributed_example_amd.train import layerwise, smallnet
    K = tde.keras.layers
    m = tde.Sequential([K.Dense(8, activation="tanh", input_shape=(6,)), K.Dropout(0.5), K.Dense(3)])
    m.compile(loss=_logits(tde), optimizer=tde.optimizers.SGD(0.01))
    m.build()
    assert smallnet.try_make(m, m._store, "cpu", 4, 4, m.optimizer, m.loss) is None
    assert layerwise.try_make(m, m._store, "cpu", 4, 4, m.optimizer, m.loss) is None


@pytest.mark.parametrize("shape", [(2, 6, 6, 3), (3, 7, 5, 2)])
def test_average_pooling_layer(shape):
    import tensorflow_distributed_example_amd as tde
    from tensorflow_distributed_example_amd.models import layers as L
    K = tde.keras.layers
    assert K.AveragePooling2D is L.AveragePooling2D and L.LAYER_CLASSES["AveragePooling2D"] is L.AveragePooling2D
    assert not issubclass(L.AveragePooling2D, L.MaxPooling2D)
    x = torch.from_numpy(np.random.default_rng(0).standard_normal(shape)).float()
    xc = x.permute(0, 3, 1, 2)
    H, W, C = shape[1:]
    valid = K.AveragePooling2D()
    assert valid.name.startswith("average_pooling2d")
    assert (valid.pool_size, valid.strides, valid.padding) == ((2, 2), (2, 2), "valid")
    assert valid.compute_output_shape((H, W, C)) == (H // 2, W // 2, C)
    got = valid.ref_call(x, {}, False)
    assert tuple(got.shape[1:]) == (H // 2, W // 2, C)
    assert torch.allclose(got, F.avg_pool2d(xc, 2).permute(0, 2, 3, 1), rtol=1e-6, atol=1e-7)
    # 3/2 same: TF pads (0, 1) or (1, 1) per side; the divisor counts the in-image elements only
    same = K.AveragePooling2D(3, strides=2, padding="same")
    assert same.compute_output_shape((H, W, C)) == (-(-H // 2), -(-W // 2), C)
    (pt, pb), (pl, pr) = L.tf_same_pads(H, 3, 2), L.tf_same_pads(W, 3, 2)
    got = same.ref_call(x, {}, False)
    ones = F.pad(torch.ones(1, 1, H, W), (pl, pr, pt, pb))
    want = (F.avg_pool2d(F.pad(xc, (pl, pr, pt, pb)), 3, 2) / F.avg_pool2d(ones, 3, 2)).permute(0, 2, 3, 1)
    assert tuple(got.shape[1:]) == (-(-H // 2), -(-W // 2), C)
    assert torch.allclose(got, want, rtol=1e-5, atol=1e-6)
    if pt == pb and pl == pr:        # symmetric pads: torch's own count_include_pad=False is the same thing
        direct = F.avg_pool2d(xc, 3, 2, padding=(pt, pl), count_include_pad=False).permute(0, 2, 3, 1)
        assert torch.allclose(got, direct, rtol=1e-5, atol=1e-6)
    corner = x[:, -2:, -2:].mean(dim=(1, 2)) if pb and pr else None      # the last window holds 2x2 real elements
    if corner is not None:
        assert torch.allclose(got[:, -1, -1], corner, rtol=1e-5, atol=1e-6)
    # config round trip
    cfg = same.get_config()
    again = L.from_config("AveragePooling2D", cfg)
    assert isinstance(again, L.AveragePooling2D) and again.get_config() == cfg
    assert cfg == dict(name=same.name, pool_size=(3, 3), strides=(2, 2), padding="same")


def test_lenet5_classic_model():
    import tensorflow_distributed_example_amd as tde
    m = tde.zoo.lenet5_classic()
    m.build()
    assert m.count_params() == tde.zoo.lenet5().count_params() == 61706
    assert [type(l).__name__ for l in m.layers if type(l).__name__ != "InputLayer"] == [
        "Conv2D", "AveragePooling2D", "Conv2D", "AveragePooling2D", "Flatten", "Dense", "Dense", "Dense"]
    assert [getattr(l, "activation", None) for l in m.layers if hasattr(l, "units") or hasattr(l, "filters")] == [
        "tanh", "tanh", "tanh", "tanh", None]


def test_lenet5_classic_saved_model(tmp_path):
    """The exported graph holds Tanh and AvgPool nodes, parses, and the numpy interpreter reproduces predict."""
    import tensorflow_distributed_example_amd as tde
    from tensorflow_distributed_example_amd.io import export as EX
    from tensorflow_distributed_example_amd.io import saved_model_pb as SM
    from test_io import TB, _decode_attr, _saved_model_classes
    tde.backend.set_random_seed(0)
    m = tde.zoo.lenet5_classic()
    m.compile(loss=_logits(tde), optimizer=tde.optimizers.SGD(0.01))
    m.build()
    m._store.load_dict(O.make_weights(m, np.random.default_rng(5), None), strict=True)
    path = EX.export_saved_model(m, str(tmp_path / "exp"), lambda: EX.TensorServingInputReceiver(
        EX.placeholder("float32", [None, 28, 28, 1]), {}))
    path = path.decode() if isinstance(path, bytes) else path
    sm = _saved_model_classes()()
    sm.ParseFromString(open(f"{path}/saved_model.pb", "rb").read())
    mg = sm.meta_graphs[0]
    sig = mg.signature_def["serving_default"]
    (_, iv), = sig.inputs.items()
    (_, ov), = sig.outputs.items()
    nodes = [(n.name, n.op, list(n.input), {k: _decode_attr(v) for k, v in n.attr.items()}) for n in mg.graph_def.node]
    ops = [n[1] for n in nodes]
    assert ops.count("AvgPool") == 2 and ops.count("Tanh") == 4 and "MaxPool" not in ops and "Relu" not in ops
    pool = next(n for n in nodes if n[1] == "AvgPool")
    assert pool[3]["ksize"] == [1, 2, 2, 1] and pool[3]["strides"] == [1, 2, 2, 1] and pool[3]["padding"] == "VALID"
    bundle = TB.read_bundle(f"{path}/variables/variables")
    x = np.random.default_rng(2).standard_normal((5, 28, 28, 1)).astype(np.float32)
    got = SM.run_graph(nodes, {iv.name.split(":")[0]: x}, bundle, ov.name)
    want = m.predict(x, verbose=0)
    assert np.allclose(got, want, rtol=1e-4, atol=1e-5), np.abs(got - want).max()


def test_interpreter_ops():
    """AvgPool with SAME padding divides by the in-image count; Sigmoid and Tanh evaluate."""
    from tensorflow_distributed_example_amd.io import saved_model_pb as SM
    x = np.arange(2 * 5 * 5 * 1, dtype=np.float64).reshape(2, 5, 5, 1)
    got = SM._avgpool(x, (3, 3), (2, 2), "SAME")
    xc = torch.from_numpy(x).permute(0, 3, 1, 2)
    want = F.avg_pool2d(xc, 3, 2, padding=1, count_include_pad=False).permute(0, 2, 3, 1).numpy()
    assert got.shape == (2, 3, 3, 1) and np.allclose(got, want)
    assert np.allclose(SM._avgpool(x, (2, 2), (2, 2), "VALID"), F.avg_pool2d(xc, 2).permute(0, 2, 3, 1).numpy())
    nodes = [("x", "Placeholder", [], {}), ("t", "Tanh", ["x"], {}), ("s", "Sigmoid", ["t"], {})]
    v = np.array([-2.0, 0.0, 0.5])
    assert np.allclose(SM.run_graph(nodes, {"x": v}, {}, "s:0"), 1 / (1 + np.exp(-np.tanh(v))))
