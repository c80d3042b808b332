"""tanh / sigmoid activations and AveragePooling2D(2) in the fused small-net plan (csrc/kernels/smallnet.hip,
train/smallnet.py) against the float64 oracle of tests/smallnet_oracle.py on the act suite of
tests/smallnet_cases.py.

Per (model, batch), step mode "plain": every variable's gradient, the loss sum, the eval loss and predict
norm-wise relative to float64, bound = max(1e-5, 4 x the error of the fp32 torch CPU reference plan against
the same oracle, computed on the spot); correct count, image count and ``iterations`` exact.  The new
operations are smooth, so data is unquantized randn; the decisions that remain (ReLU signs, max-pool argmax
behind a tanh conv, the head's argmax) are required to be 1e-4 rms away from a tie on the oracle
(smallnet_oracle: relu_near, pool_gap, margin; seeds committed in smallnet_cases).

What each model reaches (codes: 0 linear, 1 relu, 2 tanh, 3 sigmoid; sn_act = forward helper, sn_act_bwd =
derivative from the stored output, applied where a gradient overwrites that output):

act_padded, input 7x6x2 (B = 5 in a plan of 8, B = 67 in 67)
  Conv2D(4, 3, same, tanh)    staged zero-padded first layer, sn_conv_fwd<4> with code 2; no dgrad
  Conv2D(6, 3, same, sigmoid) clipped interior conv, sn_conv_fwd<2> code 3; sn_conv_dgrad<2> writes the input
                              gradient over conv 1's tanh output: mask_in = 2
  AveragePooling2D            7x6 -> 3x3: sn_avgpool_fwd; sn_avgpool_bwd with mask_in = 3 (g/4 y(1-y) over
                              the sigmoid outputs) and the zeroing of the odd row that feeds no window
  Conv2D(5, (2, 4), same)     linear; sn_conv_dgrad<1> over the pool output, mask_in = 0
  Dense(9, tanh, no bias)     scalar dense epilogue, code 2; sn_dense_bwd mask_in = 0
  Dense(5)                    head; sn_dense_bwd mask_in = 2
avg_linear, input 6x6x16: Conv2D(32, 3) linear . AveragePooling2D . Dense(10): sn_avgpool_bwd with code 0
tanh_maxpool, input 8x8x3
  Conv2D(8, 3, tanh), MaxPooling2D: sn_pool_bwd routes to the fp32 argmax and multiplies by 1 - y^2 there
  Conv2D(6, 2, sigmoid)       sn_conv_dgrad<2> over the pool output, mask_in = 0
  Dense(10, softmax)          sn_dense_bwd with mask_in = 3 over the flattened sigmoid conv output;
                              probability form of the loss
act_layers, input 6x6x4: Conv2D(8, 3) . Activation(tanh) . Dense(12) . Activation(sigmoid) .
  Dense(7, relu) . Dense(5): standalone Activation layers folded into their producers; float4 dense forward
  (12) and scalar ones (7, 5); sn_dense_bwd with mask_in 2, 3 and 1 side by side
mlp_tanh, input (50,): Dense(36, tanh) . Dense(21, sigmoid) . Dense(10): float4 + scalar dense, no conv
lenet5_classic (zoo), B = 37 in a plan of 64: X(5, 5, 1, 6, 32, 32) and X(5, 5, 6, 16, 14, 14)
  mask 3 (default)            sn_conv_fwd_m epilogue code 2; sn_conv_dgrad_c<4> with mask_in = 0 (a pool feeds
                              conv 2); both sn_avgpool_bwd with mask_in = 2
  mask 0 (child)              sn_conv_fwd_c<2> / <4>, whose tanh runs in a loop of its own after the stores
  mask 7 (child)              sn_conv_dgrad_m (mask_in = 0 here: a pool feeds conv 2)
dgrad_tanh, input 18x18x1, B = 37 in a plan of 64: Conv2D(6, 5, tanh) . Conv2D(16, 5, tanh) .
  AveragePooling2D . Dense(10).  Conv 2 is X(5, 5, 6, 16, 14, 14) and its input is conv 1's tanh output with no
  pool in between: the compile-time input-gradient forms with a derivative code, mask_in = 2
  mask 3 (default), mask 0    sn_conv_dgrad_c<4> multiplies by 1 - y^2 as it overwrites conv 1's output
  mask 7 (child)              sn_conv_dgrad_m does
Masks 0 and 7 run in one fresh child process each (tests/_smallnet_child.py act): the library reads
TDE_SN_MFMA once per process.  The children's conv-gradient hashes must differ from the in-process ones
where the mask changes the summation order, otherwise a child tested the default forms.

Results on an MI355X: no failure; no variable where the kernel is over 1e-5 (the fp32 CPU reference is under
it everywhere, so every bound is 1e-5).  Largest error against float64 per model (worst gradient and the
fp32 CPU reference's error on the same variable; loss, eval loss and predict below 2.8e-7 throughout):
  act_padded     4.6e-7 conv2d/bias (cpu-fp32 4.0e-7) at B=5, 2.7e-7 dense/kernel (2.4e-7) at B=67
  avg_linear     1.8e-7 conv2d/bias (1.9e-7), 2.1e-7 dense/kernel (2.6e-7)
  tanh_maxpool   5.3e-7 conv2d/bias (5.6e-7), 1.5e-7 dense/bias (5.0e-8)
  act_layers     5.7e-7 conv2d/bias (3.3e-7), 1.9e-7 conv2d/kernel (2.3e-7)
  mlp_tanh       2.5e-7 dense/bias (2.0e-7), 2.3e-7 dense_2/bias (4.7e-8)
  lenet5_classic mask 3: 3.4e-7 conv2d/kernel (7.7e-7); mask 0: 3.9e-7 conv2d/bias (1.2e-6); mask 7: 7.0e-7
                 conv2d/bias (1.2e-6)
  dgrad_tanh     4.97e-7 conv2d_1/bias (6.8e-7) at masks 3 and 7, 3.2e-7 conv2d/kernel (5.0e-7) at mask 0;
                 conv2d/kernel, which lies behind the tanh input gradient: 3.1e-7 / 3.2e-7 / 4.0e-7 at masks 3 / 0 / 7
Local step mode: the accumulated updates of three "local" steps equal those of three "plain" steps + the
multi-tensor optimizer bit for bit (relative difference 0 on every variable, momentum and Adam).  fit():
loss 1.909 -> 0.618 -> 0.203 over three epochs, accuracy 0.56 -> 1.0 -> 1.0.
One deliberate break -- sn_avgpool_bwd writing g / 4 without the derivative factor -- fails
test_act_default_mask for act_padded at both batches (conv2d/kernel at 3.22 and 3.25) and for lenet5_classic
(conv2d/kernel at 0.385); the other cases pass (avg_linear pools a linear conv, code 0; the rest have no
average pool).  A second one -- sn_conv_dgrad_c and sn_conv_dgrad_m writing the input gradient without the
derivative factor -- fails dgrad_tanh in-process and in both children (conv2d/kernel at 0.358 each) and
nothing else.
"""
import os

import numpy as np
import pytest
import torch

import smallnet_cases as C
import smallnet_oracle as O
from smallnet_child import guard, run

pytestmark = pytest.mark.gpu

_DEFAULT = {}


def _default_fig(tde, name, B, Bplan):
    if (name, B) not in _DEFAULT:
        _DEFAULT[name, B] = O.measure(tde, "act", name, B, Bplan)
    return _DEFAULT[name, B]


@pytest.mark.parametrize("name,B,Bplan", C.CASES["act"])
def test_act_default_mask(name, B, Bplan):
    """Every model and batch in-process (TDE_SN_MFMA default 3)."""
    import tensorflow_distributed_example_amd as tde
    guard()
    O.check(_default_fig(tde, name, B, Bplan))


@pytest.mark.parametrize("mask", ["0", "7"])
def test_act_child_mask(mask):
    """lenet5_classic with all VALU (0) / all MFMA (7) conv forms, and the evidence that the mask took effect:
    mask 0 sums both conv weight gradients in another order than the in-process default, mask 7 changes only
    conv 2's input gradient, so conv 1's kernel gradient (downstream of it) differs in bits and conv 2's
    (same MFMA forms on the same operands) does not."""
    import tensorflow_distributed_example_amd as tde
    out = run("act", mask)
    assert [(f["suite"], f["name"], f["data"]) for f in out["figs"]] == [("act", n, "randn") for n in C.FAST["act"]]
    for fig in out["figs"]:
        O.check(fig)
    guard()
    assert os.environ.get("TDE_SN_MFMA", "3") == "3", "the in-process side of this test is the default mask"
    h3 = _default_fig(tde, "lenet5_classic", *C.FAST_BATCH)["conv_grad_hash"]
    h = out["figs"][0]["conv_grad_hash"]
    c1, c2 = sorted(h3)          # conv2d/kernel, conv2d_1/kernel
    assert sorted(h) == [c1, c2]
    assert h[c1] != h3[c1]
    assert (h[c2] != h3[c2]) if mask == "0" else (h[c2] == h3[c2])


def _rel(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()


def _data(m, n, seed):
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.standard_normal((n,) + tuple(m.input_shape[1:])).astype(np.float32)).cuda()
    y = torch.from_numpy(rng.integers(0, m.output_shape[-1], n).astype(np.int32)).cuda()
    return x, y


@pytest.mark.parametrize("opt", ["momentum", "adam"])
def test_act_local_step_matches_plain(opt):
    """lenet5_classic, step mode "local" (the optimizer applied where each gradient is finished) vs "plain"
    (gradients to the bucket + the multi-tensor optimizer kernel), three steps: the same accumulated updates
    at test_smallnet_local_step_matches_plain's bound."""
    import tensorflow_distributed_example_amd as tde
    from tensorflow_distributed_example_amd.train import program as PG
    guard()

    def mk():
        return {"momentum": tde.optimizers.SGD(0.05, momentum=0.9), "adam": tde.optimizers.Adam(1e-3)}[opt]
    tde.backend.set_random_seed(3)
    m = tde.zoo.lenet5_classic()
    m.compile(loss=tde.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=mk(), metrics=["accuracy"])
    m.build()
    st = m._store
    st2 = st.clone_to("cuda")
    w0 = st.w.clone()
    a = PG.make_plan(m, st, "cuda", 64, 64, m.optimizer, m.loss)
    b = PG.make_plan(m, st2, "cuda", 64, 64, mk(), m.loss)
    assert a.kind == b.kind == "fused_smallnet"
    a.set_step_mode("local")
    for s in range(3):
        x, y = _data(m, 64, 10 + s)
        a.train_step(x, y)
        b.train_step(x, y)
        b.apply()
    torch.cuda.synchronize()
    for n in st.names(trainable=True):
        sg = st.segments[n]
        w = w0[sg.offset: sg.offset + sg.numel].view(sg.shape)
        r = _rel(st.view(n) - w, st2.view(n) - w)    # the accumulated updates
        print(f"[local {opt}] {n}: {r:.3g}")
        assert r < 1e-5, (n, r)
    assert a.iterations.item() == b.iterations.item() == 3


def test_act_fit_lenet5_classic():
    """fit() on the classic LeNet-5 picks the fused small-net plan and learns the separable synthetic task of
    test_smallnet_fit_lenet5 (same data, optimizer and loss criterion)."""
    import tensorflow_distributed_example_amd as tde
    guard()
    tde.backend.set_random_seed(4)
    m = tde.zoo.lenet5_classic()
    m.compile(loss=tde.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=tde.optimizers.SGD(0.05),
              metrics=["accuracy"], steps_per_execution=4)
    rng = np.random.default_rng(0)
    y = rng.integers(0, 10, 2048)
    x = rng.random((2048, 28, 28, 1), dtype=np.float32) * 0.2
    for c in range(10):   # class c lights up row band c
        x[y == c, 2 * c + 4: 2 * c + 6, 4:24, 0] += 1.0
    h = m.fit(x, y, batch_size=128, epochs=3, verbose=0)
    prog = m._program("train", 128)
    print(f"[fit lenet5_classic] loss {h.history['loss']} accuracy {h.history['accuracy']}")
    assert prog.plan_kind == "fused_smallnet" and prog.use_graph
    assert prog.plans[0].step_mode == "local"
    assert h.history["loss"][-1] < 0.5 * h.history["loss"][0]


def test_refused_model_keeps_todays_error():
    """A Dropout directly on a tanh output is matched by no HIP plan: ``make_plan`` ends in the same
    ``NotImplementedError`` as before."""
    import tensorflow_distributed_example_amd as tde
    from tensorflow_distributed_example_amd.train import program as PG
    guard()
    K = tde.keras.layers
    m = tde.Sequential([K.Dense(8, activation="tanh", input_shape=(6,)), K.Dropout(0.5), K.Dense(3)])
    m.compile(loss=tde.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=tde.optimizers.SGD(0.01))
    m.build()
    with pytest.raises(NotImplementedError, match="without a HIP kernel path"):
        PG.make_plan(m, m._store, "cuda", 4, 4, m.optimizer, m.loss)


def test_unknown_codes_are_refused():
    """tde_smallnet_step's host checks: an activation code or a kind outside 0..3 returns -8 before any launch."""
    import tensorflow_distributed_example_amd as tde
    from tensorflow_distributed_example_amd.train import program as PG
    from tensorflow_distributed_example_amd.train import smallnet as SN
    guard()
    m, x, y = C.make_case(tde, "act", "mlp_tanh", 5, 8)
    plan = PG.make_plan(m, m._store, "cuda", 8, 8, m.optimizer, m.loss)
    col = {f: i for i, f in enumerate(SN._FIELDS)}
    good = plan.layers.copy()
    for field, bad in (("act", 4), ("act", -1), ("mask_in", 4), ("kind", 4), ("kind", -1)):
        plan.layers = good.copy()
        plan.layers[1, col[field]] = bad
        with pytest.raises(RuntimeError, match="code -8"):
            plan.train_step(x.cuda(), y.cuda(), 5)
    plan.layers = good
    plan.train_step(x.cuda(), y.cuda(), 5)
    torch.cuda.synchronize()
    assert plan.iterations.item() == 1
