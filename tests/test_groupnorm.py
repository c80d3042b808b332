"""GroupNormalization / LayerNormalization on the host: ``ref_call`` against a float64 numpy evaluation written
from the definition, Keras weight names / shapes / configs, the refusals, and the zoo model on the reference plan."""
import numpy as np
import pytest
import torch

import tensorflow_distributed_example_amd as tde
from tensorflow_distributed_example_amd.models import layers as L


def _definition(x, G, gamma, beta, eps):
    """y = (x - mean) / sqrt(var + eps) * gamma + beta over (positions x C/G channels) of each sample and group."""
    N, C = x.shape[0], x.shape[-1]
    xg = x.reshape(N, -1, G, C // G)
    mean, var = xg.mean((1, 3), keepdims=True), xg.var((1, 3), keepdims=True)
    return ((xg - mean) / np.sqrt(var + eps)).reshape(x.shape) * gamma + beta


@pytest.mark.parametrize("shape,groups", [((2, 5, 7, 12), 4), ((3, 4, 4, 6), -1), ((2, 3, 3, 8), 1), ((4, 24), 3)])
def test_ref_call_matches_the_definition(shape, groups):
    rng = np.random.default_rng(0)
    x, C = rng.standard_normal(shape) + 2.0, shape[-1]
    gamma, beta = rng.standard_normal(C), rng.standard_normal(C)
    W = {"gamma": torch.from_numpy(gamma), "beta": torch.from_numpy(beta)}
    gn = L.GroupNormalization(groups, epsilon=1e-3)
    assert gn._build_shapes(shape[1:]) == shape[1:]
    want = _definition(x, C if groups == -1 else groups, gamma, beta, 1e-3)
    assert np.abs(gn.ref_call(torch.from_numpy(x), W, True).numpy() - want).max() < 1e-12
    ln = L.LayerNormalization(epsilon=1e-3)
    ln._build_shapes(shape[1:])
    want = _definition(x.reshape(-1, C), 1, gamma, beta, 1e-3).reshape(shape)
    assert np.abs(ln.ref_call(torch.from_numpy(x), W, False).numpy() - want).max() < 1e-12


def test_weights_config_and_regularizers():
    inp = tde.keras.Input((6, 6, 8))
    g = L.GroupNormalization(4, gamma_regularizer=tde.regularizers.L2(0.1), name="gn")
    n = L.LayerNormalization(center=False, beta_regularizer=None, name="ln")
    i = L.GroupNormalization(-1, scale=False)
    out = L.Dense(3)(L.Flatten()(i(n(g(inp)))))
    m = tde.Model(inputs=inp, outputs=out)
    m.build()
    assert [(w.name, w.shape) for w in g.weight_specs] == [("gamma", (8,)), ("beta", (8,))]
    assert [(w.name, w.shape) for w in n.weight_specs] == [("gamma", (8,))]
    assert [(w.name, w.shape) for w in i.weight_specs] == [("beta", (8,))] and i.n_groups(8) == 8
    assert all(w.trainable for lay in (g, n, i) for w in lay.weight_specs) and len(m.losses) == 1
    for lay in (g, n, i):
        cfg = lay.get_config()
        twin = L.from_config(type(lay).__name__, cfg)
        assert twin.get_config() == cfg and type(twin) is type(lay)
    assert not isinstance(g, L.BatchNormalization)   # the fused-plan matchers go by layer type


def test_refusals():
    with pytest.raises(ValueError, match="groups=3 does not divide the 8 channels"):
        L.GroupNormalization(3)._build_shapes((4, 4, 8))
    with pytest.raises(ValueError, match="last axis"):
        L.GroupNormalization(2, axis=1)._build_shapes((4, 4, 8))
    with pytest.raises(ValueError, match="last axis"):
        L.LayerNormalization(axis=1)._build_shapes((4, 4, 8))
    with pytest.raises(ValueError, match=r"axis=\[1, 2, 3\].*GroupNormalization\(groups=1\)"):
        L.LayerNormalization(axis=[1, 2, 3])
    assert L.LayerNormalization(axis=[-1]).axis == -1 and L.GroupNormalization(2, axis=3)._build_shapes((4, 4, 8))
    m = tde.zoo.mnist_gn_cnn()
    m.build()
    from tensorflow_distributed_example_amd.io import saved_model_pb as SM
    with pytest.raises(NotImplementedError, match="no TensorFlow op mapping for GroupNormalization"):
        SM.build_graph(m)


def test_zoo_model_trains_on_the_reference_plan():
    tde.backend.set_random_seed(3)
    m = tde.zoo.mnist_gn_cnn()
    m.compile(loss=tde.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=tde.optimizers.SGD(0.05))
    assert m.count_params() == 320 + 64 + 18496 + 128 + 9216 * 128 + 128 + 256 + 1290
    rng = np.random.default_rng(1)
    x = rng.random((64, 28, 28, 1), dtype=np.float32)
    y = x.reshape(64, -1)[:, :10].argmax(1)
    h = m.fit(x, y, batch_size=16, epochs=4, verbose=0).history["loss"]
    assert h[-1] < h[0]
