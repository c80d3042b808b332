"""GRU on the CPU: weights, the reference forward against torch.nn.GRU in float64 (an implementation the layer's
author did not write) with both bias rows off zero, the config round trip, every refused argument, and a fit on
the reference plan."""
import numpy as np
import pytest
import torch

import tensorflow_distributed_example_amd as tde
from tensorflow_distributed_example_amd.models import layers as L

U, D, T = 6, 5, 7


def test_weight_names_shapes_and_count():
    lay = L.GRU(U, name="rnn")
    lay(L.Input((T, D)))
    assert [(s.name, s.shape) for s in lay.weight_specs] == [
        ("gru_cell/kernel", (D, 3 * U)), ("gru_cell/recurrent_kernel", (U, 3 * U)), ("gru_cell/bias", (2, 3 * U))]
    assert lay.count_params() == 3 * U * (D + U + 2) and lay.output_shape == (U,)
    assert lay.weight_specs[2].initializer((2, 3 * U), torch.Generator().manual_seed(0)).abs().sum() == 0
    nobias = L.GRU(U, use_bias=False, return_sequences=True)
    nobias(L.Input((T, D)))
    assert [s.name for s in nobias.weight_specs] == ["gru_cell/kernel", "gru_cell/recurrent_kernel"]
    assert nobias.output_shape == (T, U) and nobias.count_params() == 3 * U * (D + U)


@pytest.mark.parametrize("seq", [False, True], ids=["last", "sequence"])
def test_ref_call_matches_torch_nn_gru_in_float64(seq):
    lay = L.GRU(U, return_sequences=seq)
    lay(L.Input((T, D)))
    gen = torch.Generator().manual_seed(7)
    W = {s.name: torch.randn(s.shape, generator=gen, dtype=torch.float64) for s in lay.weight_specs}
    x = torch.randn(3, T, D, generator=gen, dtype=torch.float64)
    ref = torch.nn.GRU(D, U, batch_first=True).double()   # reset_after form; gate order r, z, n against z, r, h

    def to_torch(w):   # gate blocks along the last axis, then torch's [3u, in] layout
        z, r, h = w.split(U, dim=-1)
        return torch.cat([r, z, h], -1).t()

    with torch.no_grad():
        ref.weight_ih_l0.copy_(to_torch(W["gru_cell/kernel"]))
        ref.weight_hh_l0.copy_(to_torch(W["gru_cell/recurrent_kernel"]))
        ref.bias_ih_l0.copy_(to_torch(W["gru_cell/bias"][0]))
        ref.bias_hh_l0.copy_(to_torch(W["gru_cell/bias"][1]))
        hs, hn = ref(x)
    got, want = lay.ref_call(x, W, True), hs if seq else hn[0]
    assert got.shape == want.shape and (got - want).abs().max() < 1e-12


def test_config_round_trip():
    lay = L.GRU(U, use_bias=False, return_sequences=True, recurrent_regularizer=tde.regularizers.L2(0.01), name="rnn")
    cfg = lay.get_config()
    twin = L.from_config("GRU", cfg)
    assert twin.get_config() == cfg and cfg["return_sequences"] is True and cfg["units"] == U
    twin(L.Input((T, D)))
    assert [(s.l1, s.l2) for s in twin.weight_specs] == [(0.0, 0.0), (0.0, 0.01)]


@pytest.mark.parametrize("geom, limit", [((4, 3, 24), "units=24"), ((4, 3, 144), "units=144"), ((4, 0, 16), "empty"),
                                         ((4, 2 ** 17, 128), "2.24")])
def test_gru_check_names_the_limit(geom, limit):
    from tensorflow_distributed_example_amd.ops import layer_ops32 as O32
    assert O32.gru_check(3, 7, 48, "x") == 3 * 7 * 48
    with pytest.raises(ValueError, match=f"gru_fwd.*{limit}"):
        O32.gru_check(*geom, "gru_fwd")


@pytest.mark.parametrize("arg, make", [
    ("reset_after", lambda x: L.GRU(4, reset_after=False)),
    ("activation", lambda x: L.GRU(4, activation="relu")),
    ("recurrent_activation", lambda x: L.GRU(4, recurrent_activation="hard_sigmoid")),
    ("dropout", lambda x: L.GRU(4, dropout=0.1)),
    ("recurrent_dropout", lambda x: L.GRU(4, recurrent_dropout=0.1)),
    ("return_state", lambda x: L.GRU(4, return_state=True)),
    ("go_backwards", lambda x: L.GRU(4, go_backwards=True)),
    ("stateful", lambda x: L.GRU(4, stateful=True)),
    ("unroll", lambda x: L.GRU(4, unroll=True)),
    ("mask", lambda x: L.GRU(4)(x, mask=torch.ones(T))),
    ("initial_state", lambda x: L.GRU(4)(x, initial_state=[x])),
])
def test_refusals_name_the_argument(arg, make):
    with pytest.raises(NotImplementedError, match=f"GRU.*{arg}="):
        make(L.Input((T, D)))


def test_zoo_model_trains_on_the_reference_plan():
    tde.backend.set_random_seed(2)
    m = tde.zoo.mnist_gru()
    m.compile(loss=tde.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=tde.optimizers.SGD(0.1))
    assert m.count_params() == 3 * 64 * (28 + 64 + 2) + 3 * 64 * (64 + 64 + 2) + 650
    rng = np.random.default_rng(5)
    x = rng.random((40, 28, 28, 1), dtype=np.float32)
    y = x.reshape(len(x), -1)[:, :10].argmax(1).astype(np.int64)   # learnable labels
    h = m.fit(x, y, batch_size=16, epochs=3, verbose=0).history["loss"]   # a ragged last batch of 8
    assert np.isfinite(h).all() and h[-1] < h[0], h
