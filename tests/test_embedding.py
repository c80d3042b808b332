"""Embedding and GlobalAveragePooling1D on the CPU: configs, the reference lookup against numpy indexing (a float
id truncates, an id outside the table reads zeros), every refusal by name and the limits of ``embed_check``."""
import numpy as np
import pytest
import torch

import tensorflow_distributed_example_amd as tde
from tensorflow_distributed_example_amd.models import layers as L

V, D, T = 11, 8, 5


def test_config_round_trip_and_variable():
    lay = L.Embedding(V, D, embeddings_regularizer=tde.regularizers.L2(0.01), input_length=T, name="emb")
    cfg = lay.get_config()
    twin = L.from_config("Embedding", cfg)
    assert twin.get_config() == cfg and (cfg["input_dim"], cfg["output_dim"], cfg["input_length"]) == (V, D, T)
    twin(L.Input((T,)))
    assert [(s.name, s.shape, s.l2) for s in twin.weight_specs] == [("embeddings", (V, D), 0.01)]
    assert twin.output_shape == (T, D) and twin.input_shape_arg == (T,)
    w = twin.weight_specs[0].initializer((V, D), torch.Generator().manual_seed(0))
    assert w.abs().max() <= 0.05 and w.std() > 0.02   # Keras's default uniform on [-0.05, 0.05]
    gap = L.GlobalAveragePooling1D(name="gap")
    assert L.from_config("GlobalAveragePooling1D", gap.get_config()).get_config() == gap.get_config()
    assert gap(L.Input((T, D))).shape[1:] == (D,)


def test_ref_call_is_numpy_indexing():
    lay = L.Embedding(V, D)
    lay(L.Input((T,)))
    table = np.random.default_rng(0).standard_normal((V, D))
    ids = np.array([[0, 3, 10, 3, 7], [2.7, -0.0, -1.0, float(V), 10.9]])
    want = table[np.trunc(ids).clip(0, V - 1).astype(int)]
    want[1, 2:4] = 0                                        # -1 and V lie outside the table
    got = lay.ref_call(torch.from_numpy(ids), {"embeddings": torch.from_numpy(table)}, True)
    assert np.array_equal(got.numpy(), want) and np.array_equal(got[1, 0].numpy(), table[2])
    pooled = L.GlobalAveragePooling1D().ref_call(got, {}, True)
    assert np.allclose(pooled.numpy(), want.mean(1), rtol=0, atol=1e-15)


@pytest.mark.parametrize("arg, make", [
    ("mask_zero", lambda: L.Embedding(V, D, mask_zero=True)),
    ("sparse", lambda: L.Embedding(V, D, sparse=True)),
    ("keepdims", lambda: L.GlobalAveragePooling1D(keepdims=True)),
])
def test_refusals_name_the_argument(arg, make):
    with pytest.raises(NotImplementedError, match=f"(Embedding|GlobalAveragePooling1D).*{arg}="):
        make()


def _plan(model, B=4):
    from tensorflow_distributed_example_amd.train.layerwise import LayerwisePlan
    model.compile(loss=tde.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=tde.optimizers.SGD(0.1))
    model.build()
    return LayerwisePlan(model, model._store, "cpu", B, B, model.optimizer, model.loss)


def test_plan_takes_the_first_layer_only(fp32_policy):
    from tensorflow_distributed_example_amd.train import layerwise as LW
    behind = tde.Sequential([L.Dense(T, input_shape=(3,)), L.Embedding(V, D, name="late"),
                             L.GlobalAveragePooling1D(), L.Dense(4)])
    with pytest.raises(LW.Unsupported, match="late .Embedding.*only the model input"):
        _plan(behind)
    emb, gap = _plan(tde.zoo.text_gap(vocab=V, seq_len=T, dim=D)).stages[:2]
    assert isinstance(emb, LW._Embedding) and emb.geom(4) == (4 * T, V, D) and emb.grad_inputs() == []
    assert emb.param_names() == [f"{emb.layer.name}/embeddings"]
    assert isinstance(gap, LW._GAP) and (gap.HW, gap.C) == (T, D)


@pytest.mark.parametrize("geom, limit", [((8, 5, 6), "output_dim=6"), ((8, 5, 516), "output_dim=516"),
                                         ((8, 2 ** 24 + 1, 4), "input_dim=16777217"), ((0, 5, 4), "empty"),
                                         ((2 ** 22, 5, 512), "n=4194304"), ((8, 2 ** 23, 256), "x output_dim=256")])
def test_embed_check_names_the_limit(geom, limit):
    from tensorflow_distributed_example_amd.ops import layer_ops32 as O32
    O32.embed_check(8, 2 ** 24, 4, "x")
    with pytest.raises(ValueError, match=f"embed_fwd.*{limit}"):
        O32.embed_check(*geom, "embed_fwd")
