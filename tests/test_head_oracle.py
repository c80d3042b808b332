"""tests/head_oracle.py checked on the CPU: the formulas against float64 torch autograd, the first-maximum rule
against torch.argmax, the input conditions of every case (so that no element of any case needs to be excused), the
error of a plain float32 evaluation of the same formulas against a quarter of every bound that
tests/test_head_gpu.py holds the kernel to, and the one statement of the head's limits."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import head_oracle as HO
from layers_oracle import bf16_round

FORMS = [(True, True), (True, False), (False, True), (False, False)]   # (bias, relu)


def _t(a, dtype=torch.float64):
    return None if a is None else torch.tensor(np.asarray(a), dtype=dtype)


@pytest.mark.parametrize("bias,relu", FORMS)
@pytest.mark.parametrize("B,H,C", HO.CASES)
def test_oracle_matches_float64_autograd(B, H, C, bias, relu):
    inp = HO.head_inputs(B, H, C, bias, relu)
    o = HO.case_oracle(B, H, C, bias, relu)
    hin = _t(inp["hin"]).requires_grad_()
    pb = _t(inp["pre_bias"]).requires_grad_() if bias else None
    W = _t(inp["W2"]).requires_grad_()
    b2 = _t(inp["b2"]).requires_grad_() if bias else None
    lab = torch.tensor(inp["labels"], dtype=torch.int64)
    h = hin + pb if bias else hin
    h = F.relu(h) if relu else h
    z = h @ W + b2 if bias else h @ W
    ls = F.cross_entropy(z, lab, reduction="none")
    (ls.sum() * float(np.float32(HO.SCALE))).backward()
    ref = {"logits": z, "probs": torch.softmax(z, 1), "row_loss": ls, "loss_sum": ls.sum(), "dW2": W.grad,
           "dH": hin.grad}
    if bias:
        ref.update(db2=b2.grad, dpre_bias=pb.grad)
    for name, r in ref.items():
        assert HO.rel_l2(o[name], r) < 1e-12, name
    if not bias:     # the column sums the absent biases would have received
        assert HO.rel_l2(o["dpre_bias"], hin.grad.sum(0)) < 1e-12
    assert o["correct"] == int((z.argmax(1) == lab).sum()) and o["count"] == B


def test_first_maximum_rule_equals_torch_argmax():
    rng = np.random.default_rng(5)
    z = rng.integers(-2, 3, size=(64, 16)).astype(np.float64)     # five values over 16 classes: ties in every row
    assert (np.sort(z, 1)[:, -1] == np.sort(z, 1)[:, -2]).any()
    assert (HO.first_max(z) == torch.tensor(z).argmax(1).numpy()).all()
    for case, (a, b) in HO.TIE_CASES.items():
        o = HO.case_oracle(*case)
        z = o["logits"]
        assert (z[:, a] == z[:, b]).all()
        assert (o["argmax"] == torch.tensor(z).argmax(1).numpy()).all()
        led = z[:, a] == z.max(1)
        assert led.sum() >= 4 and (o["argmax"][led] == a).all()


@pytest.mark.parametrize("bias,relu", [(True, True), (False, False)])
@pytest.mark.parametrize("B,H,C", HO.CASES)
def test_input_conditions(B, H, C, bias, relu):
    inp = HO.head_inputs(B, H, C, bias, relu)
    o = HO.case_oracle(B, H, C, bias, relu)
    grid = [inp["hin"]] + ([inp["pre_bias"]] if bias else [])
    for a in grid:
        assert (a * 64 == np.rint(a * 64)).all() and np.abs(a).max() <= 4.0
    # exact as stored: float32 everywhere, bfloat16 for hin; hin + pre_bias exact in float32
    for a in grid + [inp["W2"]] + ([inp["b2"]] if bias else []):
        assert (a.astype(np.float32).astype(np.float64) == a).all()
    assert (bf16_round(inp["hin"], force=True) == inp["hin"]).all()
    pre = o["pre"]
    assert (pre.astype(np.float32).astype(np.float64) == pre).all()
    assert (pre == 0).mean() >= HO.ZERO_SHARE
    assert (np.abs(pre[pre != 0]) >= 2.0 ** -6).all()
    if relu:    # the exact zeros are masked, in dH and (as zeros among the summed terms) in dpre_bias
        assert (o["dH"][pre == 0] == 0).all() and (o["bound"]["dH"][pre == 0] == 0).all()
    lab = inp["labels"]
    assert set(lab.tolist()) == set(range(C)) if B >= C else len(set(lab.tolist())) == B
    z = o["logits"]
    gap, led = HO._gaps(z, inp["tie"])
    assert (gap >= HO.MIN_GAP).all()
    if inp["tie"] is not None:
        a, b = inp["tie"]
        assert (inp["W2"][:, a] == inp["W2"][:, b]).all() and inp["b2"][a] == inp["b2"][b]
        assert (lab[led] == a).sum() >= 2 and (lab[led] == b).sum() >= 1
        last_max = C - 1 - HO.first_max(z[:, ::-1])
        assert int((last_max == lab).sum()) != o["correct"]       # the last-maximum rule would be seen
    else:
        assert not led.any()
    # h W2 is exact in fp32 in any order (head_oracle._draw): multiples of 2^-18 below 2^6, or of 2^-12 below 2^11
    hw = o["h"] @ inp["W2"]
    if bias and relu and (B, H, C) == HO.STABLE_CASE:
        assert z.max() >= 70 and z.min() <= -70
        assert (inp["W2"] * 64 == np.rint(inp["W2"] * 64)).all() and np.abs(inp["W2"]).max() <= 3.0
        assert (np.abs(o["h"]) @ np.abs(inp["W2"])).max() <= 2048
    else:
        assert (inp["W2"] * 4096 == np.rint(inp["W2"] * 4096)).all()
        assert (np.abs(o["h"]) @ np.abs(inp["W2"])).max() <= HO.EXACT_SUM
    assert ((_t(o["h"], torch.float32) @ _t(inp["W2"], torch.float32)).double().numpy() == hw).all()
    if bias and relu:
        assert (inp["tie"] is not None) == ((B, H, C) in HO.TIE_CASES)


def f32_reference(inp, st, relu, B):
    """The same formulas in plain float32 torch on the CPU."""
    f = torch.float32
    hin, pb, W, b2 = _t(inp["hin"], f), _t(inp["pre_bias"], f), _t(inp["W2"], f), _t(inp["b2"], f)
    lab = torch.tensor(inp["labels"], dtype=torch.int64)
    pre = hin if pb is None else hin + pb
    h = torch.relu(pre) if relu else pre
    z = h @ W if b2 is None else h @ W + b2
    m = z.max(1, keepdim=True).values
    e = torch.exp(z - m)
    se = e.sum(1, keepdim=True)
    p = e / se
    loss = torch.log(se[:, 0]) + m[:, 0] - z[torch.arange(B), lab]
    dl = (p - F.one_hot(lab, z.shape[1]).to(f)) * torch.tensor(HO.SCALE, dtype=f)
    dH = dl @ W.T
    if relu:
        dH = torch.where(pre > 0, dH, torch.zeros((), dtype=f))
    return {"logits": z, "probs": p, "row_loss": loss, "loss_sum": _t(st["metrics"][0], f) + loss.sum(),
            "dW2": _t(st["dW2"], f) + h.T @ dl, "db2": _t(st["db2"], f) + dl.sum(0), "dH": dH,
            "dpre_bias": _t(st["dpre_bias"], f) + dH.sum(0)}


@pytest.mark.parametrize("bias,relu", [(True, True), (False, False)])
@pytest.mark.parametrize("B,H,C", HO.CASES)
def test_float32_reference_within_a_quarter_of_every_bound(B, H, C, bias, relu):
    """What the tolerances rest on: float32 arithmetic itself meets every bound with a margin of four, in relative
    L2 (1e-6 forward, 1e-5 gradients) and element by element (share of the element's own bound, in brackets)."""
    inp, st, o = HO.head_inputs(B, H, C, bias, relu), HO.head_start(H, C), HO.case_oracle(B, H, C, bias, relu)
    fig = HO.figures(f32_reference(inp, st, relu, B), o, st)
    HO.show(f"float32 CPU {(B, H, C)} bias={bias} relu={relu}", fig)
    for name, (rel, cap, share) in fig.items():
        assert rel <= cap / 4, (name, rel)
        assert share <= 0.25, (name, share)


def test_stored_forms():
    v = np.array([[1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -7), 0.3]], dtype=np.float32)   # two ties
    G, Gt = HO.stored_forms(np.repeat(v, 3, 0), 3, 8)
    want = torch.tensor(v).to(torch.bfloat16).double().numpy()
    assert (G == want).all() and (G[0] == [1.0, 1.0 + 2.0 ** -6, -(1.0 + 2.0 ** -7), want[0, 3]]).all()
    assert Gt.shape == (4, 8) and (Gt[:, :3] == G.T).all() and (Gt[:, 3:] == 0).all()


# ---------------------------------------------------------------------------------------- one rule for the limits
LIMIT_H, LIMIT_C = (252, 256, 260, 6), (1, 16, 17)


def plan_rule(H, C):
    """train/layerwise.py's fused-head rule for a Dense(C) on H features (the stage's own constructor, on stubs)."""
    from tensorflow_distributed_example_amd.train.layerwise import _Head
    ns = types.SimpleNamespace
    plan = ns(store=ns(view=lambda n: None, grad=lambda n: None), f32=False, det=False, loss_spec=None,
              metric_spec=None)
    tin = ns(shape=(H,), root=lambda: ns(id=0))
    return _Head(plan, ns(name="dense", use_bias=True, units=C), tin, ns(producer=1), False).fused


def wrapper_rule(H, C, dev="cpu"):
    from tensorflow_distributed_example_amd.ops import kernels as K
    hin = torch.zeros(1, H, device=dev)
    try:
        K.head_check(hin, torch.zeros(H, C, device=dev), torch.zeros(1, dtype=torch.int32, device=dev), B=1)
    except ValueError as e:
        assert ("W2 has C" in str(e)) == (C > 16) and ("W2 has H" in str(e)) == (C <= 16), str(e)
        return False
    return True


def test_limits_have_one_statement(monkeypatch):
    from tensorflow_distributed_example_amd.ops import kernels as K
    monkeypatch.delenv("TDE_FUSED_HEAD", raising=False)
    lim = K.head_limits()
    assert lim == dict(max_c=16, max_h=256, h_mult=4, rows=HO.ROWS)
    for H in LIMIT_H:
        for C in LIMIT_C:
            want = H in (252, 256) and C in (1, 16)
            assert K.head_fits(H, C) == wrapper_rule(H, C) == plan_rule(H, C) == want, (H, C)
