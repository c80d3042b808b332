"""MultiHeadAttention on the CPU: weights, the reference forward against the formula written out head by head,
the [N, H, W, D] form, the config round trip and every refused call or constructor argument."""
import math

import pytest
import torch

import tensorflow_distributed_example_amd as tde
from tensorflow_distributed_example_amd.models import layers as L

H, DK, DV, D = 3, 4, 8, 10


def _built(shape, **kw):
    lay = L.MultiHeadAttention(H, DK, value_dim=DV, **kw)
    lay(L.Input(shape))
    gen = torch.Generator().manual_seed(7)
    W = {s.name: torch.randn(s.shape, generator=gen, dtype=torch.float64) for s in lay.weight_specs}
    return lay, W


def test_weight_names_shapes_and_count():
    lay, _ = _built((5, D))
    assert [(s.name, s.shape) for s in lay.weight_specs] == [
        ("query/kernel", (D, H, DK)), ("query/bias", (H, DK)), ("key/kernel", (D, H, DK)), ("key/bias", (H, DK)),
        ("value/kernel", (D, H, DV)), ("value/bias", (H, DV)),
        ("attention_output/kernel", (H, DV, D)), ("attention_output/bias", (D,))]
    assert lay.count_params() == 2 * (D * H * DK + H * DK) + D * H * DV + H * DV + H * DV * D + D == 778
    assert lay.output_shape == (5, D)
    nobias, _ = _built((5, D), use_bias=False)
    assert [s.name for s in nobias.weight_specs] == [f"{n}/kernel" for n in ("query", "key", "value",
                                                                              "attention_output")]


@pytest.mark.parametrize("shape", [(2, 5, D), (2, 2, 3, D)], ids=["tokens", "image"])
def test_ref_call_matches_the_formula_head_by_head(shape):
    lay, W = _built(shape[1:])
    x = torch.randn(shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    xt = x.reshape(shape[0], -1, D)
    want = W["attention_output/bias"].expand(xt.shape).clone()
    for h in range(H):
        q, k, v = (xt @ W[f"{n}/kernel"][:, h] + W[f"{n}/bias"][h] for n in ("query", "key", "value"))
        p = torch.softmax(q @ k.transpose(1, 2) / math.sqrt(DK), dim=-1)
        want += p @ v @ W["attention_output/kernel"][h]
    got = lay.ref_call(x, W, True)
    assert got.shape == x.shape and torch.allclose(got, want.reshape(shape), rtol=1e-12, atol=1e-12)
    if len(shape) == 4:   # the image form is the token form after a reshape
        flat, _ = _built((shape[1] * shape[2], D))
        assert torch.equal(got.reshape(xt.shape), flat.ref_call(xt, W, True))


def test_config_round_trip():
    lay = L.MultiHeadAttention(H, DK, value_dim=DV, use_bias=False, kernel_regularizer=tde.regularizers.L2(0.01),
                               name="att")
    cfg = lay.get_config()
    twin = L.from_config("MultiHeadAttention", cfg)
    assert twin.get_config() == cfg and cfg["value_dim"] == DV and L.MultiHeadAttention(2, 6).value_dim == 6
    twin(L.Input((5, D)))
    assert {(s.l1, s.l2) for s in twin.weight_specs} == {(0.0, 0.01)}


@pytest.mark.parametrize("arg, make", [
    ("value", lambda l, x, y: l(x, y)),
    ("key", lambda l, x, y: l(x, x, key=y)),
    ("attention_mask", lambda l, x, y: l(x, x, attention_mask=torch.ones(5, 5))),
    ("use_causal_mask", lambda l, x, y: l(x, x, use_causal_mask=True)),
    ("return_attention_scores", lambda l, x, y: l(x, x, return_attention_scores=True)),
    ("dropout", lambda l, x, y: L.MultiHeadAttention(2, 4, dropout=0.1)),
    ("attention_axes", lambda l, x, y: L.MultiHeadAttention(2, 4, attention_axes=(1,))),
    ("output_shape", lambda l, x, y: L.MultiHeadAttention(2, 4, output_shape=16)),
])
def test_refusals_name_the_argument(arg, make):
    with pytest.raises(NotImplementedError, match=f"MultiHeadAttention.*{arg}="):
        make(L.MultiHeadAttention(2, 4), L.Input((5, D)), L.Input((5, D)))
