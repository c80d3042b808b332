"""The float32 step has a production form and a general one (csrc/kernels/convnet_f32.hip).  The backward of
28 x 28 images with whole 64-image chunks, 4 hpre replicas and no stamp buffer takes kernels that know all of that
at compile time and hold no diagnostics (convnet32g_bwd_kernel); every other call, a stamped one included, takes
the runtime form (the class count is read from the arguments in both).  The forward without a stamp buffer takes the body with the stamps compiled out.
The entry points are called directly: the production form against the float64 oracle of tests/test_prologue_gpu.py
(at its 1e-5) and bit for bit against the runtime form wherever no float atomic lies between the two, every call
next to the production form's conditions against the oracle between guard pages, and the stamped forms for their
stamps and for the results of the unstamped ones."""
import numpy as np
import pytest
import torch

from test_bwd_head_gpu import DET, _check, _inputs, _oracle, _run
from test_prologue_gpu import ADAM, DEV, HP, SGD, TOL, Guarded, _data, _f64, _rel

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("fp32_policy")]


@pytest.fixture(autouse=True)
def _float32_hyperparameters(monkeypatch):
    """The oracle steps with the hyperparameters the kernels are given, the float32 values of Adam's rates, like
    every other operand of these tests.  1 - b2 differs by 1.3e-5 (relative) between 0.999 and its float32 value:
    more than the whole bound once the gradient term dominates a second-moment slot, as it does for b2's slot
    at two whole chunks (1.13e-5 at B = 128 with the rates left unquantized on the oracle's side)."""
    monkeypatch.setitem(HP, ADAM, {k: float(np.float32(v)) for k, v in HP[ADAM].items()})


# the backward's slots in time order (bench/micro.py: BWD_SLOTS); 8..12 are the second bank of 8 per workgroup
PHASES = [0, 1, 8, 9, 10, 11, 12, 2, 3, 4, 5]
NWG = 13 * 13 + 1   # workgroups of the 28 x 28 backward: one per pooled position + the head


def _same(a, b, kind, cgrad_exact, what):
    """Two runs of one case: everything that does not go through float atomics bit for bit, the conv gradients
    (atomic adds of the workgroups' sums unless the deterministic partials are used) at the tolerance."""
    exact = ["met"] + (["dW1", "dW2", "db2", "db1"] if kind is None else ["w"] + (["m", "v"] if kind == ADAM else []))
    for n in exact + (["dwc", "dbc"] if cgrad_exact else []):
        assert torch.equal(a[n], b[n]), f"{what}: {n} differs"
    for n in ("dwc", "dbc"):
        assert _rel(a[n], _f64(b[n])) < TOL, (what, n)


_CASES = {}


def _case(B, kind):
    """Inputs, oracle and the two forms' results of one production-form case (computed once, shared)."""
    if (B, kind) not in _CASES:
        d = _inputs(B, 28, 10, 4, True, 500 + B)
        _CASES[B, kind] = (d, _oracle(d, kind), _run(d, kind), _run(d, kind, fallback=True))
    return _CASES[B, kind]


@pytest.mark.parametrize("kind", [None, SGD, ADAM])
@pytest.mark.parametrize("B", [64, 128])
def test_production_form(B, kind):
    d, ref, prod, fall = _case(B, kind)
    _check(d, kind, prod, ref, ("production form", B, kind))
    _check(d, kind, fall, ref, ("runtime form", B, kind))
    _same(prod, fall, kind, False, "production against runtime form")


@pytest.mark.parametrize("B,kind", [(64, SGD), (128, None)])
def test_production_form_deterministic_partials(B, kind):
    """4 replicas with the conv gradients as per-workgroup partials: no atomics, so these are bit-identical too."""
    d = dict(_inputs(B, 28, 10, 4, True, 500 + B), det=True)
    ref = _oracle(d, kind)
    prod, fall = _run(d, kind), _run(d, kind, fallback=True)
    _check(d, kind, prod, ref, ("production form, partials", B, kind))
    _same(prod, fall, kind, True, "production against runtime form, partials")


@pytest.mark.parametrize("B,C,hrep,kind", [(63, 10, 4, SGD), (65, 10, 4, None), (130, 10, 4, ADAM), (64, 3, 4, SGD),
                                           (64, 16, 4, None), (64, 10, 1, SGD), (64, 10, 2, ADAM), (64, 10, DET, SGD)])
def test_dispatch(B, C, hrep, kind):
    """One condition of the production form missed at a time (a ragged batch, another replica count, the deterministic
    layout): the runtime form serves the call; few and many classes: the production form reads the count (guard pages
    and the zeroed parity buffer are checked in _run)."""
    d = _inputs(B, 28, C, hrep, True, 600 + B + C)
    _check(d, kind, _run(d, kind), _oracle(d, kind), ("dispatch", B, C, hrep, kind))


@pytest.mark.parametrize("kind", [None, SGD])
def test_stamps_still_work(kind, monkeypatch):
    from tensorflow_distributed_example_amd.ops import kernels as Kk
    d, ref, prod, _ = _case(64, kind)
    st = torch.zeros(4096 * 8, dtype=torch.int64, device=DEV)
    bwd = Kk.convnet_bwd
    monkeypatch.setattr(Kk, "convnet_bwd", lambda *a, **k: bwd(*a, **dict(k, stamps=st)))
    got = _run(d, kind)
    _check(d, kind, got, ref, ("stamped", kind))
    _same(got, prod, kind, False, "stamped against unstamped")
    rows = st.view(-1, 8).cpu().numpy()
    rows = np.concatenate([rows[:NWG], rows[NWG:2 * NWG]], axis=1)   # slot s of workgroup w: rows[w, s]
    for w in (0, 84, NWG - 2):   # trunk workgroups
        t = rows[w, PHASES]
        assert (t > 0).all() and (np.diff(t) >= 0).all(), (w, t)
    assert rows[NWG - 1, 7] > 0, "the head workgroup's end stamp"


@pytest.mark.parametrize("B", [16, 64])
def test_forward_with_and_without_stamps(B):
    """One hpre replica per workgroup column (every element is one add into zero: no atomics order)."""
    from tensorflow_distributed_example_amd.ops import kernels as Kk
    g, x0, wc, bc = _data(B, 28, 700 + B)
    Pn, R = 169, (169 + 3) // 4
    W1 = (torch.randn(Pn * 32, 64, generator=g) * 0.02).to(DEV)
    out = []
    for stamped in (False, True):
        x = Guarded((B, 28, 28, 1), fill=x0)
        hpre = Guarded((R, B, 64), fill=torch.zeros(R, B, 64))
        Pt = Guarded((Pn * 32, B), fill=torch.full((Pn * 32, B), 5.0))
        amax = Guarded((Pn, 4, B), torch.int64, fill=torch.zeros(Pn, 4, B, dtype=torch.int64))
        st = torch.zeros(4096 * 8, dtype=torch.int64, device=DEV) if stamped else None
        Kk.convnet_fwd(x.t, wc.to(DEV), bc.to(DEV), W1, hpre.t, Pt.t, amax.t, stamps=st, hrep=R)
        torch.cuda.synchronize()
        for name, gb in [("x", x), ("hpre", hpre), ("Pt", Pt), ("amax", amax)]:
            assert gb.intact(), f"guard page of {name} overwritten"
        out.append((hpre.t.clone(), Pt.t.clone(), amax.t.clone()))
        if stamped:
            rows = st.view(-1, 8)[:R * ((B + 15) // 16), :5].cpu().numpy()
            assert (rows > 0).all() and (np.diff(rows, axis=1) >= 0).all()
    for n, a, b in zip(("hpre", "Pt", "amax"), *out):
        assert torch.equal(a, b), f"{n} differs between the forward with and without stamps"
    assert bool(out[0][0].abs().sum() > 0)
