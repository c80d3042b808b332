"""The BN-CNN family's oracle and case table on the CPU (tests/bncnn_oracle.py, tests/bncnn_cases.py), before
tests/test_bncnn_family_gpu.py relies on them: every case is a member of the family (``match_bncnn`` takes it
silently), the oracle's geometry handling agrees with the model's own torch reference forward, the host planner
helper answers the stack-staging threshold, and no case or row count is too ill-conditioned to test anything:
the gradient bound ``max(1e-5 * |g64|, 4 * |g32 - g64|)`` stays below ``1e-4 * |g64|`` with the float32
reference alone (ReLU decisions of a float32 host forward standing in for the plan's)."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import bncnn_cases as BC
import bncnn_oracle as BO

pytestmark = pytest.mark.usefixtures("fp32_policy")

CAP = 1e-4


def _spec(m):
    from tensorflow_distributed_example_amd.train import bncnn
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        spec = bncnn.match_bncnn(m, m.loss)
    assert spec is not None and not rec, [str(w.message) for w in rec]
    return spec


def _conditioning(m, x, y, B):
    spec = _spec(m)
    st = m._store
    masks = BO.host_masks(st, spec, x, y, B)
    g64, _, _, _ = BO.oracle(st, spec, x, y, B, masks, 1.0 / B)
    g32, _, _, _ = BO.oracle(st, spec, x, y, B, masks, 1.0 / B, dtype=torch.float32)
    return {n: BO.bound(g64[n], g32[n]) / g64[n].norm().item() for n in g64}


@pytest.mark.parametrize("case", sorted(BC.CASES))
def test_case_is_a_family_member_and_well_conditioned(case):
    import tensorflow_distributed_example_amd as tde
    c = BC.CASES[case]
    m = BC.build(tde, case)
    x, y = BC.data(case, c["batch"], 11)
    worst = _conditioning(m, x, y, c["batch"])
    assert max(worst.values()) < CAP, worst


@pytest.mark.parametrize("B", [2, 5, 6, 17, 50, 130])
def test_case_a_row_counts_are_well_conditioned(B):
    import tensorflow_distributed_example_amd as tde
    m = BC.build(tde, "A")
    x, y = BC.data("A", 130, 11)
    worst = _conditioning(m, x, y, B)
    assert max(worst.values()) < CAP, worst


@pytest.mark.parametrize("B", [2, 3, 4, 5])
def test_model_b_short_batches_are_well_conditioned(B):
    import tensorflow_distributed_example_amd as tde
    m = BC.model_b(tde)
    x, y = BC.model_b_data(128, 11)
    worst = _conditioning(m, x, y, B)
    assert max(worst.values()) < CAP, worst


@pytest.mark.parametrize("case", sorted(BC.CASES))
def test_oracle_inference_matches_the_model_reference_forward(case):
    """``inference`` (moving statistics) against the layers' own torch forward: the oracle's padding, strides,
    BN flags and head agree with an implementation that shares no code with it."""
    import tensorflow_distributed_example_amd as tde
    c = BC.CASES[case]
    m = BC.build(tde, case)
    x, _ = BC.data(case, 7, 12)
    ref = m(x.reshape((7,) + c["input"]).numpy())
    ref = (ref if torch.is_tensor(ref) else torch.as_tensor(np.asarray(ref))).double()
    logits, probs = BO.inference(m._store, _spec(m), x, 7)
    assert BO.rel(probs if c["softmax"] else logits, ref) < 1e-5


def test_one_row_dense_gradient_is_zero_in_float64():
    """With one row the dense BN's output is its beta: no gradient reaches the dense kernel or the convs."""
    import tensorflow_distributed_example_amd as tde
    m = BC.build(tde, "A")
    x, y = BC.data("A", 4, 11)
    spec = _spec(m)
    g64, _, _, _ = BO.oracle(m._store, spec, x, y, 1, None, 1.0)
    dense, _, _ = spec["dense"]
    assert g64[f"{dense.name}/kernel"].abs().max().item() < 1e-12
    assert g64[f"{spec['head'].name}/bias"].norm().item() > 0.1


def test_stack_rows_helper_matches_the_forward_grid():
    """``tde_bncnn_conv_stack_rows``: ceil(staged floats / (msplit * 1024)) rows, 0 without a staged stack."""
    from tensorflow_distributed_example_amd import _native as N
    from tensorflow_distributed_example_amd.train import bncnn
    lib = N.hip()
    for geo in (bncnn.Geo(14, 14, 12, 7, 7, 24, 6, 6, 2, 2, 2, 2),    # Model B's third conv: 10752 / 2048
                bncnn.Geo(28, 28, 6, 14, 14, 12, 6, 6, 2, 2, 2, 2),   # its second: 3584 / 2048
                bncnn.Geo(7, 6, 5, 2, 1, 17, 5, 5, 2, 2, 0, 0),       # case A: 6144 / 1024
                bncnn.Geo(9, 9, 16, 5, 5, 24, 5, 5, 2, 2, 2, 2),      # case I: not staged
                bncnn.Geo(8, 8, 17, 4, 4, 4, 3, 3, 2, 2, 0, 0)):      # does not plan
        cfg, out = (C.c_int * 4)(), (C.c_int * 12)()
        ok = lib.tde_bncnn_conv_fwd_cfg(C.byref(geo), cfg) == 0 and lib.tde_bncnn_conv_bwd_plan(C.byref(geo), 1, out) == 0
        want = -(-out[5] // (cfg[2] * 1024)) if ok and out[5] > 0 else 0
        assert lib.tde_bncnn_conv_stack_rows(C.byref(geo)) == want
    assert lib.tde_bncnn_conv_stack_rows(C.byref(bncnn.Geo(14, 14, 12, 7, 7, 24, 6, 6, 2, 2, 2, 2))) == 6
