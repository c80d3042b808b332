"""The fused classifier head kernel (csrc/kernels/head.hip, ops/kernels.py: head_xent) against the float64 oracle of
tests/head_oracle.py: every output, both input forms (float32 / bfloat16 hin), every case of the oracle's table, each
a single launch of at most 3 workgroups.

Every buffer carries guards: hin is a column slice of a wider sentinel buffer with spare rows; the stored outputs (G,
Gf, probs, row_loss) start as NaN with spare columns and a spare row; Gt starts at a non-zero fill with a spare row;
the accumulate outputs start at seeded non-zero values in front of a sentinel tail.  After a launch the written
region must be right and everything else bit-unchanged.

Tolerances (head_oracle.REL_FWD / REL_GRAD and its element bounds; tests/test_head_oracle.py shows that plain float32
arithmetic meets each with a margin of four): relative L2 1e-6 for logits, probs, row_loss and the loss sum, 1e-5 for
dW2, db2, dpre_bias and Gf, and every element within its own u k sum|terms|.  G is checked through its bit-equality
with bf16(Gf), Gt through its bit-equality with G.T; correct / count exactly.  Each test prints the kernel's figures
(pytest -s); profiles/head/NOTES.md keeps them."""
import numpy as np
import pytest
import torch

import head_oracle as HO
from layers_oracle import bf16_round

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 7.0        # sentinel around hin, behind the accumulate outputs and in metrics[3]
GT_FILL = 3.0
FORMS = ["f32", "bf16"]
PAD_L, PAD_R = 4, 4     # sentinel columns left and right of hin (ldh = H + 8)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32
                                              if t.element_size() == 4 else torch.int64)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


class Rig:
    """The buffers of one launch, with their guards."""

    def __init__(self, B, H, C, form, *, bias=True, relu=True, ldgt=None):
        self.B, self.H, self.C, self.form, self.bias, self.relu = B, H, C, form, bias, relu
        inp = HO.head_inputs(B, H, C, bias, relu)
        st = HO.head_start(H, C)
        self.inp, self.st = inp, st
        dt = torch.float32 if form == "f32" else torch.bfloat16
        self.hwide = torch.full((B + 2, H + PAD_L + PAD_R), SENT, dtype=dt, device=DEV)
        self.hin = self.hwide[:, PAD_L:PAD_L + H]
        self.hin[:B] = torch.tensor(inp["hin"], dtype=dt, device=DEV)
        self.hwide0 = self.hwide.clone()
        f = lambda a: None if a is None else torch.tensor(a, dtype=torch.float32, device=DEV)
        self.pre_bias, self.W2, self.b2 = f(inp["pre_bias"]), f(inp["W2"]), f(inp["b2"])
        self.labels = torch.tensor(inp["labels"], dtype=torch.int32, device=DEV)
        nan = float("nan")
        self.G = torch.full((B + 1, H + 8), nan, dtype=torch.bfloat16, device=DEV)
        self.Gf = torch.full((B + 1, H + 4), nan, dtype=torch.float32, device=DEV)
        self.ldgt = (B + 7) // 8 * 8 if ldgt is None else ldgt
        self.Gt = torch.full((H + 1, self.ldgt), GT_FILL, dtype=torch.bfloat16, device=DEV)
        self.probs = torch.full((B + 1, C), nan, dtype=torch.float32, device=DEV)
        self.row_loss = torch.full((B + 3,), nan, dtype=torch.float32, device=DEV)
        self.acc = {}
        for name, shape in (("dW2", (H, C)), ("db2", (C,)), ("dpre_bias", (H,))):
            n = int(np.prod(shape))
            whole = torch.full((n + 8,), SENT, dtype=torch.float32, device=DEV)
            whole[:n] = torch.tensor(st[name], dtype=torch.float32, device=DEV).reshape(-1)
            self.acc[name] = (whole, whole[:n].view(*shape))
        self.metrics = torch.tensor(list(st["metrics"][:3]) + [SENT], dtype=torch.float32, device=DEV)
        self.iterations = torch.tensor([41, 99], dtype=torch.int64, device=DEV)
        self.before = {k: v.clone() for k, v in self.buffers().items()}

    def buffers(self):
        d = {"G": self.G, "Gf": self.Gf, "Gt": self.Gt, "probs": self.probs, "row_loss": self.row_loss,
             "metrics": self.metrics, "iterations": self.iterations, "hwide": self.hwide}
        d.update({k: v[0] for k, v in self.acc.items()})
        return d

    def launch(self, *, grad=True, logits=False, zero_hin=False, iterations=True, stored=("G", "Gf", "Gt"),
               metrics=True):
        from tensorflow_distributed_example_amd.ops import kernels as K
        K.head_xent(self.hin, self.W2, self.b2, self.labels, B=self.B, scale=HO.SCALE, pre_bias=self.pre_bias,
                    pre_relu=self.relu, compute_grad=grad, dW2=self.acc["dW2"][1], db2=self.acc["db2"][1],
                    dpre_bias=self.acc["dpre_bias"][1], G=self.G if "G" in stored else None,
                    Gt=self.Gt if "Gt" in stored else None, Gf=self.Gf if "Gf" in stored else None,
                    metrics=self.metrics if metrics else None, probs=self.probs, probs_are_logits=logits,
                    row_loss=self.row_loss, zero_hin=zero_hin, iterations=self.iterations if iterations else None)
        torch.cuda.synchronize()

    def oracle(self):
        return HO.case_oracle(self.B, self.H, self.C, self.bias, self.relu)

    def unchanged(self, *names):
        for n in names:
            assert _same(self.buffers()[n], self.before[n]), f"{n} was touched"

    # ---- checks
    def check_hin(self, zeroed):
        B, H = self.B, self.H
        w, w0 = self.hwide, self.hwide0
        assert _same(w[:, :PAD_L], w0[:, :PAD_L]) and _same(w[:, PAD_L + H:], w0[:, PAD_L + H:]), "hin guard columns"
        assert _same(w[B:], w0[B:]), "hin rows past B"
        if zeroed:
            assert (_bits(self.hin[:B]) == 0).all(), "zero_hin must leave +0 in hin[:B, :H]"
        else:
            assert _same(self.hin[:B], w0[:B, PAD_L:PAD_L + H]), "hin was written"

    def check_forward(self, tag, *, logits=False, metrics=True, extra=None):
        """probs (or logits), row_loss and the metrics of the last launch; returns the figures."""
        B, C, o = self.B, self.C, self.oracle()
        assert torch.isnan(self.probs[B:]).all() and torch.isnan(self.row_loss[B:]).all(), "guard rows written"
        assert torch.isfinite(self.probs[:B]).all() and torch.isfinite(self.row_loss[:B]).all()
        got = {"logits" if logits else "probs": self.probs[:B], "row_loss": self.row_loss[:B]}
        if metrics:
            m = self.metrics.cpu().double().numpy()
            got["loss_sum"] = m[0]
            assert m[1] == self.st["metrics"][1] + o["correct"], ("correct", m[1], o["correct"])
            assert m[2] == self.st["metrics"][2] + B, ("count", m[2])
            assert m[3] == SENT
        got.update(extra or {})
        fig = HO.figures(got, o, self.st)
        HO.show(f"kernel {tag} {(B, self.H, C)} {self.form} bias={self.bias} relu={self.relu}", fig)
        for name, (rel, cap, share) in fig.items():
            assert rel <= cap, (name, "relative L2", rel, cap)
            assert share <= 1.0, (name, "worst element over its bound", share)
        return fig

    def check_stored(self, stored):
        """G / Gf / Gt regions and their bit relations."""
        B, H = self.B, self.H
        if "Gf" in stored:
            assert torch.isfinite(self.Gf[:B, :H]).all()
            assert torch.isnan(self.Gf[:B, H:]).all() and torch.isnan(self.Gf[B:]).all(), "Gf guards written"
        else:
            self.unchanged("Gf")
        if "G" in stored:
            assert torch.isfinite(self.G[:B, :H].float()).all()
            assert torch.isnan(self.G[:B, H:].float()).all() and torch.isnan(self.G[B:].float()).all(), "G guards"
            if "Gf" in stored:
                want = bf16_round(self.Gf[:B, :H].cpu().double().numpy(), force=True)
                assert (self.G[:B, :H].cpu().double().numpy() == want).all(), "G != bf16(Gf)"
        else:
            self.unchanged("G")
        if "Gt" in stored:
            assert _same(self.Gt[:H, :B], self.G[:B, :H].T), "Gt[:, :B] != G.T"
            assert (_bits(self.Gt[:H, B:]) == 0).all(), "Gt padding columns must be +0"
            assert _same(self.Gt[H:], self.before["Gt"][H:]), "Gt guard row written"
        else:
            self.unchanged("Gt")

    def check_tails(self):
        for name, (whole, view) in self.acc.items():
            assert (whole[view.numel():] == SENT).all(), f"{name} tail written"

    def grads(self):
        d = {k: v[1] for k, v in self.acc.items()}
        d["dH"] = self.Gf[:self.B, :self.H]
        return d


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("B,H,C", HO.CASES)
def test_head_train(B, H, C, form):
    """The full training launch: bias + ReLU epilogue, ldh / ldg / ldgf > H, G + Gf + Gt (ldgt = B rounded up to 8),
    NaN-filled store outputs, seeded accumulate outputs, the step counter, and (f32 form) zero_hin."""
    r = Rig(B, H, C, form)
    zero = form == "f32"
    r.launch(zero_hin=zero)
    r.check_hin(zeroed=zero)
    r.check_stored(("G", "Gf", "Gt"))
    r.check_forward("train", extra=r.grads())
    r.check_tails()
    assert r.iterations.tolist() == [42, 99]
    # the gradient of an exactly-zero pre-activation is masked: exact zeros, not small numbers
    zero_pre = torch.tensor(r.oracle()["pre"] == 0, device=DEV)
    assert zero_pre.any() and (r.Gf[:B, :H][zero_pre] == 0).all() and (r.G[:B, :H][zero_pre] == 0).all()


def test_head_zero_hin_changes_no_result():
    """zero_hin only zeroes hin: the same one-workgroup launch without it stores the same bits everywhere else."""
    B, H, C = 16, 64, 10
    a, b = Rig(B, H, C, "f32"), Rig(B, H, C, "f32")
    a.launch(zero_hin=True)
    b.launch(zero_hin=False)
    a.check_hin(zeroed=True)
    b.check_hin(zeroed=False)
    for name in ("G", "Gf", "Gt", "probs", "row_loss", "dW2", "db2", "dpre_bias", "metrics", "iterations"):
        assert _same(a.buffers()[name], b.buffers()[name]), name


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("B,H,C", HO.CASES)
def test_head_eval_and_predict(B, H, C, form):
    """compute_grad=False: metrics, probs (both meanings) and row_loss are right, every gradient buffer keeps its
    fill bit for bit, and the step counter that is not passed stays."""
    for logits in (False, True):
        r = Rig(B, H, C, form)
        r.launch(grad=False, logits=logits, iterations=False)
        r.check_forward("logits" if logits else "eval", logits=logits)
        r.check_hin(zeroed=False)
        r.unchanged("G", "Gf", "Gt", "dW2", "db2", "dpre_bias", "iterations")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("B,H,C", HO.CASES)
def test_head_optional_inputs_absent(B, H, C, form):
    """pre_bias=None, b2=None, pre_relu=False; no G, no Gt, no metrics, no step counter: Gf alone."""
    r = Rig(B, H, C, form, bias=False, relu=False)
    r.launch(stored=("Gf",), metrics=False, iterations=False)
    r.check_hin(zeroed=False)
    r.check_stored(("Gf",))
    r.check_forward("absent", metrics=False, extra=r.grads())
    r.check_tails()
    r.unchanged("metrics", "iterations")


@pytest.mark.parametrize("form", FORMS)
def test_head_gt_padding_workgroups(form):
    """(B, ldgt) = (16, 40): workgroups 1 and 2 exist for Gt's padding columns only.  They zero them, and add
    nothing anywhere: every accumulate output equals, bit for bit, that of the one-workgroup launch (ldgt = 16)."""
    B, H, C = 16, 64, 10
    wide, one = Rig(B, H, C, form, ldgt=40), Rig(B, H, C, form, ldgt=16)
    wide.launch()
    one.launch()
    for r in (wide, one):
        r.check_stored(("G", "Gf", "Gt"))
        r.check_forward(f"ldgt={r.ldgt}", extra=r.grads())
        r.check_tails()
        assert r.iterations.tolist() == [42, 99]       # one step per launch, whatever the grid
    assert (_bits(wide.Gt[:H, B:]) == 0).all() and wide.Gt[:H, B:].numel() == H * 24
    for name in ("metrics", "dW2", "db2", "dpre_bias", "G", "Gf", "probs", "row_loss"):
        assert _same(wide.buffers()[name], one.buffers()[name]), name


def _refusals():
    """name -> (rig arguments, how to spoil the launch)."""
    def shape(H, C):
        def spoil(r):
            r.W2 = torch.zeros(H, C, device=DEV)
            r.hwide = torch.full((r.B + 2, H + 8), SENT, dtype=r.hwide.dtype, device=DEV)
            r.hin = r.hwide[:, 4:4 + H]
            r.pre_bias = torch.zeros(H, device=DEV)
        return spoil

    def shift_hin(r):
        r.hin = r.hwide[:, 1:1 + r.H]                  # 4 bytes (f32) / 2 bytes (bf16) off; ldh still H + 8

    def shift_bias(r):
        r.pre_bias = torch.zeros(r.H + 4, device=DEV)[1:1 + r.H]

    return {"C=17": ("f32", shape(64, 17), "W2 has C"), "H=260": ("f32", shape(260, 10), "W2 has H"),
            "H=6": ("f32", shape(6, 10), "W2 has H"), "f32 hin alignment": ("f32", shift_hin, "16-byte"),
            "pre_bias alignment": ("f32", shift_bias, "pre_bias"), "bf16 hin alignment": ("bf16", shift_hin, "8-byte"),
            "bf16 zero_hin": ("bf16", None, "zero_hin")}


@pytest.mark.parametrize("what", list(_refusals()))
def test_head_refusals(what):
    """Each is refused by a ValueError that names the argument, before any launch: no output buffer is touched."""
    form, spoil, word = _refusals()[what]
    r = Rig(16, 64, 10, form)
    if spoil:
        spoil(r)
    hwide0 = r.hwide.clone()
    with pytest.raises(ValueError, match=word):
        r.launch(zero_hin=what == "bf16 zero_hin")
    torch.cuda.synchronize()
    r.unchanged("G", "Gf", "Gt", "probs", "row_loss", "metrics", "iterations", "dW2", "db2", "dpre_bias")
    assert _same(r.hwide, hwide0)


def test_head_limits_agree_with_the_kernel_entry():
    """tde_head_xent itself (B = 1, forward only) accepts exactly the (H, C) that the wrapper's rule and the plan's
    rule accept (tests/test_head_oracle.py compares those two on the CPU)."""
    from tensorflow_distributed_example_amd import _native as N
    from tensorflow_distributed_example_amd.ops import kernels as K
    from test_head_oracle import LIMIT_C, LIMIT_H, plan_rule, wrapper_rule
    for H in LIMIT_H:
        for C in LIMIT_C:
            hin = torch.zeros(1, H, device=DEV)
            W2 = torch.zeros(H, C, device=DEV)
            lab = torch.zeros(1, dtype=torch.int32, device=DEV)
            met = torch.zeros(4, device=DEV)
            rc = N.hip().tde_head_xent(hin.data_ptr(), H, None, 0, W2.data_ptr(), None, lab.data_ptr(), 1, H, C, 1.0,
                                       0, None, None, None, None, 0, None, 0, None, 0, met.data_ptr(), None, 0, None,
                                       0, None, None, 0, N.stream_ptr())
            torch.cuda.synchronize()
            assert rc in (0, -1)
            assert (rc == 0) == K.head_fits(H, C) == wrapper_rule(H, C, DEV) == plan_rule(H, C), (H, C, rc)
            if rc == 0:     # zero inputs: uniform probabilities, the first maximum is class 0, the label
                assert abs(met[0].item() - np.log(C)) <= 1e-6 and met[1:].tolist() == [1.0, 1.0, 0.0]
            else:           # refused: nothing was launched
                assert met.tolist() == [0.0] * 4
