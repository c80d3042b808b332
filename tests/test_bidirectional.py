"""Bidirectional(LSTM | GRU) on the CPU: shapes, nested names, ref_call, refusals, lowering, a reference-plan fit."""
import numpy as np
import pytest
import torch

import tensorflow_distributed_example_amd as tde
from tensorflow_distributed_example_amd.models import layers as L

U, D, T = 8, 5, 7


@pytest.mark.parametrize("seq", [False, True], ids=["last", "sequence"])
def test_output_shape_names_and_count(seq):
    lay = L.Bidirectional(L.LSTM(U, return_sequences=seq, name="lstm"), name="bidirectional")
    lay(L.Input((T, D)))
    assert lay.output_shape == ((T, 2 * U) if seq else (2 * U,))
    assert [s.full_name for s in lay.weight_specs] == [
        f"bidirectional/{d}_lstm/lstm_cell/{w}" for d in ("forward", "backward")
        for w in ("kernel", "recurrent_kernel", "bias")]
    assert lay.count_params() == 2 * 4 * U * (D + U + 1)
    twin = L.from_config("Bidirectional", lay.get_config())   # the nested config goes back through the constructor
    assert twin.get_config() == lay.get_config() and type(twin.layer) is L.LSTM and not twin.built


@pytest.mark.parametrize("cell", [L.LSTM, L.GRU], ids=["lstm", "gru"])
@pytest.mark.parametrize("seq", [False, True], ids=["last", "sequence"])
def test_ref_call_is_the_flip_composition(cell, seq):
    lay = L.Bidirectional(cell(U, return_sequences=seq))
    lay(L.Input((T, D)))
    gen = torch.Generator().manual_seed(7)
    W = {s.name: torch.randn(s.shape, generator=gen, dtype=torch.float64) for s in lay.weight_specs}
    x = torch.randn(3, T, D, generator=gen, dtype=torch.float64)
    one = cell(U, return_sequences=True)   # a plain layer of its own, run once per direction
    one(L.Input((T, D)))
    halves = [one.ref_call(xx, {k.split("/", 1)[1]: v for k, v in W.items() if k.startswith(d)}, True)
              for d, xx in (("forward_", x), ("backward_", torch.from_numpy(x.numpy()[:, ::-1].copy())))]
    fw, bw = halves[0], torch.from_numpy(halves[1].numpy()[:, ::-1].copy())
    want = torch.cat([fw, bw], -1) if seq else torch.cat([fw[:, -1], bw[:, 0]], -1)
    got = lay.ref_call(x, W, True)
    assert got.shape == want.shape and torch.equal(got, want)


@pytest.mark.parametrize("arg, make", [
    ("layer", lambda x: L.Bidirectional(L.Dense(4))),
    ("merge_mode", lambda x: L.Bidirectional(L.LSTM(4), merge_mode="sum")),
    ("backward_layer", lambda x: L.Bidirectional(L.LSTM(4), backward_layer=L.LSTM(4))),
    ("weights", lambda x: L.Bidirectional(L.GRU(4), weights=[np.zeros(3)])),
    ("mask", lambda x: L.Bidirectional(L.GRU(4))(x, mask=torch.ones(T))),
    ("initial_state", lambda x: L.Bidirectional(L.LSTM(4))(x, initial_state=[x])),
])
def test_refusals_name_the_argument(arg, make):
    with pytest.raises(NotImplementedError, match=f"Bidirectional.*{arg}="):
        make(L.Input((T, D)))


def test_plan_lowers_to_two_projections_and_one_recurrent_stage(fp32_policy):
    from tensorflow_distributed_example_amd.train import layerwise as LW
    m = tde.zoo.text_bilstm()
    m.compile(loss=tde.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=tde.optimizers.SGD(0.1))
    m.build()
    emb, g0, g1, rec, head = LW.LayerwisePlan(m, m._store, "cpu", B := 4, B, m.optimizer, m.loss).stages
    bi, inner = m.layers[1].name, m.layers[1].layer.name
    assert [(type(g), g.wname, g.inp.root() is emb.out.root()) for g in (g0, g1)] == [
        (LW._Gemm, f"{bi}/forward_{inner}/lstm_cell/kernel", True),
        (LW._Gemm, f"{bi}/backward_{inner}/lstm_cell/kernel", True)]
    assert isinstance(rec, LW._BiRnn) and rec.geom(B) == (B, 32, 64) and not rec.seq and not rec.gru
    assert rec.grad_inputs() == [g0.out, g1.out] and rec.out.shape == (128,) and isinstance(emb, LW._Embedding)
    assert (g0.accum[emb.out.root().id], g1.accum[emb.out.root().id]) == (True, False)   # the first writer stores
    assert rec.param_names() == [f"{bi}/{d}_{inner}/lstm_cell/recurrent_kernel" for d in ("forward", "backward")]


def test_zoo_model_trains_on_the_reference_plan():
    tde.backend.set_random_seed(2)
    m = tde.zoo.text_bilstm()
    m.compile(loss=tde.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=tde.optimizers.SGD(0.5))
    rng = np.random.default_rng(5)
    x = rng.integers(4, 2000, (40, 32)).astype(np.int64)
    y = rng.integers(0, 4, len(x)).astype(np.int64)
    x[np.arange(len(x))[:, None], rng.integers(0, 32, (len(x), 8))] = y[:, None]   # the class's marker id, ~8 times
    h = m.fit(x, y, batch_size=16, epochs=3, verbose=0).history["loss"]   # a ragged last batch of 8
    assert np.isfinite(h).all() and h[-1] < h[0], h
