"""LSTM on the CPU: weights and their initial values, the reference forward against torch.nn.LSTM in float64 (an
implementation the layer's author did not write), the config round trip and every refused argument."""
import pytest
import torch

import tensorflow_distributed_example_amd as tde
from tensorflow_distributed_example_amd.models import initializers
from tensorflow_distributed_example_amd.models import layers as L

U, D, T = 6, 5, 7


def test_weight_names_shapes_count_and_forget_bias():
    lay = L.LSTM(U, name="rnn")
    lay(L.Input((T, D)))
    assert [(s.name, s.shape) for s in lay.weight_specs] == [
        ("lstm_cell/kernel", (D, 4 * U)), ("lstm_cell/recurrent_kernel", (U, 4 * U)), ("lstm_cell/bias", (4 * U,))]
    assert lay.count_params() == 4 * U * (D + U + 1) and lay.output_shape == (U,)
    bias = lay.weight_specs[2].initializer((4 * U,), torch.Generator().manual_seed(0))
    assert torch.equal(bias, torch.cat([torch.zeros(U), torch.ones(U), torch.zeros(2 * U)]))
    plain = L.LSTM(U, unit_forget_bias=False, return_sequences=True)
    plain(L.Input((T, D)))
    assert plain.output_shape == (T, U)
    assert plain.weight_specs[2].initializer((4 * U,), torch.Generator().manual_seed(0)).abs().sum() == 0
    nobias = L.LSTM(U, use_bias=False)
    nobias(L.Input((T, D)))
    assert [s.name for s in nobias.weight_specs] == ["lstm_cell/kernel", "lstm_cell/recurrent_kernel"]


@pytest.mark.parametrize("shape", [(16, 16), (64, 16), (16, 64)], ids=lambda s: "x".join(map(str, s)))
def test_orthogonal_initializer(shape):
    """U^T U = I where the columns are the fewer (square, tall); a wide matrix, the recurrent kernel's [u, 4u],
    has orthonormal rows instead, as in Keras."""
    q = initializers.get("orthogonal")(shape, torch.Generator().manual_seed(3)).double()
    gram = q.T @ q if shape[0] >= shape[1] else q @ q.T
    assert q.shape == shape and (gram - torch.eye(min(shape), dtype=torch.float64)).abs().max() < 1e-6


@pytest.mark.parametrize("seq", [False, True], ids=["last", "sequence"])
def test_ref_call_matches_torch_nn_lstm_in_float64(seq):
    lay = L.LSTM(U, return_sequences=seq)
    lay(L.Input((T, D)))
    gen = torch.Generator().manual_seed(7)
    W = {s.name: torch.randn(s.shape, generator=gen, dtype=torch.float64) for s in lay.weight_specs}
    x = torch.randn(3, T, D, generator=gen, dtype=torch.float64)
    ref = torch.nn.LSTM(D, U, batch_first=True).double()   # gate order i, f, g, o as well
    with torch.no_grad():
        ref.weight_ih_l0.copy_(W["lstm_cell/kernel"].T)
        ref.weight_hh_l0.copy_(W["lstm_cell/recurrent_kernel"].T)
        ref.bias_ih_l0.copy_(W["lstm_cell/bias"])
        ref.bias_hh_l0.zero_()
        hs, (hn, _) = ref(x)
    got, want = lay.ref_call(x, W, True), hs if seq else hn[0]
    assert got.shape == want.shape and (got - want).abs().max() < 1e-12


def test_config_round_trip():
    lay = L.LSTM(U, use_bias=False, unit_forget_bias=False, return_sequences=True,
                 recurrent_regularizer=tde.regularizers.L2(0.01), name="rnn")
    cfg = lay.get_config()
    twin = L.from_config("LSTM", cfg)
    assert twin.get_config() == cfg and cfg["return_sequences"] is True and cfg["units"] == U
    twin(L.Input((T, D)))
    assert [(s.l1, s.l2) for s in twin.weight_specs] == [(0.0, 0.0), (0.0, 0.01)]


@pytest.mark.parametrize("geom, limit", [((4, 3, 24), "units=24"), ((4, 3, 144), "units=144"), ((4, 0, 16), "empty"),
                                         ((4, 2 ** 17, 128), "2.24")])
def test_lstm_check_names_the_limit(geom, limit):
    from tensorflow_distributed_example_amd.ops import layer_ops32 as O32
    assert O32.lstm_check(3, 7, 48, "x") == 3 * 7 * 48
    with pytest.raises(ValueError, match=limit):
        O32.lstm_check(*geom, "lstm_fwd")


@pytest.mark.parametrize("arg, make", [
    ("activation", lambda x: L.LSTM(4, activation="relu")),
    ("recurrent_activation", lambda x: L.LSTM(4, recurrent_activation="hard_sigmoid")),
    ("dropout", lambda x: L.LSTM(4, dropout=0.1)),
    ("recurrent_dropout", lambda x: L.LSTM(4, recurrent_dropout=0.1)),
    ("return_state", lambda x: L.LSTM(4, return_state=True)),
    ("go_backwards", lambda x: L.LSTM(4, go_backwards=True)),
    ("stateful", lambda x: L.LSTM(4, stateful=True)),
    ("unroll", lambda x: L.LSTM(4, unroll=True)),
    ("mask", lambda x: L.LSTM(4)(x, mask=torch.ones(T))),
    ("initial_state", lambda x: L.LSTM(4)(x, initial_state=[x, x])),
])
def test_refusals_name_the_argument(arg, make):
    with pytest.raises(NotImplementedError, match=f"LSTM.*{arg}="):
        make(L.Input((T, D)))
