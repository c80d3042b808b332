"""The float64 optimizer oracle (tests/optim_oracle.py) against the repository's own fp32
``Optimizer.apply_reference`` on the CPU, and the exact-grid premise of tests/test_optim_gpu.py.

fp32 ``apply_reference`` against the oracle after 3 steps on 4096 randn weights (max |w| about 4), as
printed by this test (run with -s), in units of the fp32 ulp of max |w|:
  sgd 0.79, momentum 0.62 (slot 0.72), nesterov 0.71 (slot 0.72), adam 0.65 (m 2.2 ulp of max |m|,
  v 1.31e-5 relative: the float32 rounding of beta_1 and beta_2, see the test)
"""
import pytest
import torch

import optim_oracle as O

ULP = 2.0 ** -23


def _optimizer(tde, kind):
    return {"sgd": tde.optimizers.SGD(0.1), "momentum": tde.optimizers.SGD(0.1, momentum=0.9),
            "nesterov": tde.optimizers.SGD(0.1, momentum=0.9, nesterov=True),
            "adam": tde.optimizers.Adam(0.01)}[kind]


@pytest.mark.parametrize("kind", O.KINDS)
def test_oracle_matches_fp32_reference(kind):
    """Bound on w and the momentum slot: 4 fp32 ulps of the largest magnitude.  Each step rounds the update
    term and the sum once or twice, at most about one ulp of max |w| per step and three steps.

    Adam: ``apply_reference`` keeps beta_1 and beta_2 as Python doubles while the kernels, and so the oracle,
    get them as floats.  float32(0.999) = 0.99900001287, so 1 - b2 is 0.99998713e-3 for the kernels and
    1e-3 for the reference: v differs by 1.3e-5 relative, hence the bound of 2e-5 on v here.  1 - b1 is
    1 - float32(0.9) = 0.10000002384 for the kernels and float32(0.1) = 0.10000000149 in the reference's
    fp32 product: m differs by 2.2e-7 relative, 1.9 ulp, which with the roundings of m stays inside 4 ulps.
    w hardly sees either: lr_t's sqrt(1 - b2^t) / (1 - b1^t) divides the same factors out again (exactly
    at t = 1, to first order later), and what is left scales an update of size lr = 0.01, under a tenth
    of an ulp of max |w|."""
    import tensorflow_distributed_example_amd as tde
    opt = _optimizer(tde, kind)
    hyper = dict(lr=opt.learning_rate, **opt.hparams())
    gen = torch.Generator().manual_seed(11)
    n = 4096
    w32 = torch.randn(n, generator=gen)
    slots32 = {s: torch.zeros(n) for s in opt.slot_names()}
    w, m, v = w32.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for step in range(3):
        g32 = torch.randn(n, generator=gen)
        opt.apply_reference(w32, g32, slots32, step)
        w, m, v = O.oracle_step(kind, hyper, w, g32.double(), m, v, step + 1)
        ew = float((w32.double() - w).abs().max() / w.abs().max())
        print(f"[{kind} step {step + 1}] w {ew / ULP:.2g} ulp of max|w| = {float(w.abs().max()):.3g}")
        assert ew <= 4 * ULP, (kind, step, ew)
        if kind in ("momentum", "nesterov"):
            em = float((slots32["momentum"].double() - m).abs().max() / m.abs().max())
            print(f"[{kind} step {step + 1}] slot {em / ULP:.2g} ulp")
            assert em <= 4 * ULP, (kind, step, em)
        if kind == "adam":
            em = float((slots32["m"].double() - m).abs().max() / m.abs().max())
            ev = float(((slots32["v"].double() - v).abs() / v).max())
            print(f"[{kind} step {step + 1}] m {em / ULP:.2g} ulp, v {ev:.3g} relative")
            assert em <= 4 * ULP and ev <= 2e-5, (kind, step, em, ev)


def test_oracle_treats_t_below_1_as_1():
    h = dict(lr=0.01, mom=0.0, b1=0.9, b2=0.999, eps=1e-7)
    assert O.lr_t64(h, 0) == O.lr_t64(h, 1) == O.lr_t64(h, -3)
    assert O.lr_t64(h, 2) != O.lr_t64(h, 1)


@pytest.mark.parametrize("kind", ["sgd", "momentum", "nesterov"])
@pytest.mark.parametrize("grad_scale,reps", [(1.0, 1), (0.25, 1), (1.0, 8)])
def test_exact_grid_is_exact_in_fp32(kind, grad_scale, reps):
    """On the dyadic inputs of test_optim_gpu.py the fp32 computation equals the float64 oracle bit for bit
    after each of 3 steps (also with grad_scale = 0.25 and with a gradient summed from 8 replicas), and the
    values leave 3 spare bits: they are multiples of 2^-14 below 2^7, 21 of fp32's 24 bits, so a fused
    multiply-add, which skips one rounding, cannot give anything else either."""
    store = O.make_store(O.SHAPES, "cpu")
    idx = torch.arange(store.n_trainable)
    w, m = O.grid_w(idx), O.grid_slot(idx)
    assert w.unique().numel() == 509 and w.abs().max() < 4 and torch.equal(w * 64, (w * 64).round())
    w32, m32 = w.float(), m.float()
    for step in range(3):
        g = sum(O.grid_g(idx, step, r) for r in range(reps))
        assert g.abs().max() < 4 * reps and torch.equal(g * 64, (g * 64).round())
        w, m, _ = O.oracle_step(kind, O.GRID_HYPER, w, g, m, None, step + 1, grad_scale)
        w32, m32, _ = O.fp32_step(kind, O.GRID_HYPER, w32, g.float(), m32, None, step + 1, grad_scale)
        assert torch.equal(w32.double(), w) and torch.equal(m32.double(), m), (kind, step)
        for x in (w, m):
            assert torch.equal(x * 16384, (x * 16384).round()) and x.abs().max() < 128, (kind, step)


def test_make_store_layout():
    """Segments in the order given, 64-element aligned, with gaps for the helpers to guard."""
    store = O.make_store(O.SHAPES, "cpu")
    assert store.names(trainable=True) == [n for n, _ in O.SHAPES]
    assert all(store.segments[n].offset % 64 == 0 and store.segments[n].shape == tuple(s) for n, s in O.SHAPES)
    mask = O.seg_mask(store)
    assert int(mask.sum()) == store.num_trainable_elements() < store.n_trainable
    assert float(store.w.abs().max()) == 0.0
