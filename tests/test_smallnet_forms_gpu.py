"""Every conv form and padded edge of the fused small-net plan (csrc/kernels/smallnet.hip,
train/smallnet.py) against the float64 oracle of tests/smallnet_oracle.py on the forms suite of
tests/smallnet_cases.py, step mode "plain".

Per (model, batch): every variable's gradient norm-wise relative to float64, bound = max(1e-5, 4 x the
error of the fp32 torch CPU reference plan against the same oracle, computed on the spot); loss sum at
1e-5; correct count, image count and ``iterations`` exact; eval metrics and predict the same way (the
forward convs have no entry point of their own: predict / eval are their check).  Inputs and conv
weights are quantized so every conv pre-activation is exact in fp32 under any summation order (a checked
condition, see smallnet_oracle.trunk_check), Dense ReLU units and the head's top-2 margin are required
to be 1e-4 rms away from a tie on the oracle: every ReLU / max-pool / argmax decision is then the same
in both precisions and the comparison measures the sums.

Which kernel function and branch each layer reaches (kSnScratch = 4096 floats, kSnItemsTarget = 1024
items, kSnThreads = 512; the runtime-geometry weight gradient takes S = max(1, min(Ho, 1024 / (Tb ng)))
output-row slices when n = Tb Co <= 4096 and S = 1 otherwise, with T = kh kw C taps, Tb = T + bias,
ng = Co / CG; CG = 4 / 2 / 1 by Co % 4 == 0 / Co even / Co odd):

padded, input 7x6x2 (B = 5 in a plan of 8: ragged image quads in the dense-wgrad MFMA and in the 8-slice
conv reduction; B = 67 in 67: three images past the 64-image block)
  Conv2D(4, 3, same, relu)    first layer: staged into a zero-padded 9x8x2 LDS image (the img_Hp != img_H
                              staging branch), then a valid conv: sn_conv_fwd<4>, pt = pl = 0;
                              sn_conv_wgrad<4> Tb = 19, ng = 1: S = 7 (LDS float atomics); no dgrad
  Conv2D(6, 3, same, relu)    interior, pt = pl = 1 (pb = pr = 1): sn_conv_fwd<2> clipping kh0/kh1/kw0/kw1;
                              sn_conv_wgrad<2> r0/r1/ow0/ow1, Tb = 37, ng = 3: S = 7; sn_conv_dgrad<2>
                              kh0 = max(0, ih + pt - Ho + 1) ..., Co = 6 < 8: co tail only, mask_in = 1
  MaxPooling2D                7x6 -> 3x3: the odd row feeds no window (sn_pool_bwd's zeroing loop), mask_in = 1
  Conv2D(5, (2, 4), same)     linear, non-square, asymmetric pads (0, 1) x (1, 2): the kernel knows pt = 0,
                              pl = 1 and Ho, Wo only; sn_conv_fwd<1>; sn_conv_wgrad<1> Tb = 49, ng = 5:
                              S = 3 = Ho; sn_conv_dgrad<1> Co = 5: main loop (4) + tail (1), mask_in = 0
  Dense(9, relu, no bias)     scalar dense forward (Co % 4 != 0), mask_in = 0 (a linear conv feeds it);
                              smallnet_wgrad_kernel strip 0 with bias == false
  Dense(5)                    head on logits, mask_in = 1
wide_taps, input 8x8x8
  Conv2D(16, 3, relu)         sn_conv_fwd<4>; sn_conv_wgrad<4> Tb = 73, ng = 4: Tb ng = 292, S = 3 over Ho = 6
  Conv2D(20, 3, relu, no bias) on 6x6x16: b_off < 0 in sn_conv_fwd<4>; sn_conv_wgrad<4> Tb = T = 144,
                              ng = 5: Tb ng = 720 > 512 so S = 1 (each thread writes `part` directly);
                              sn_conv_dgrad<4> Co = 20: main loop (16) + tail (4), mask_in = 1
  Dense(10, softmax)          probability form of the loss; predict returns probabilities
wide_out, input 6x6x16
  Conv2D(8, 1)                linear 1x1: sn_conv_fwd<4>; sn_conv_wgrad<4> Tb = 17, ng = 2: S = 6 = Ho
  Conv2D(32, 3, relu)         a conv after a linear conv (mask_in = 0): sn_conv_wgrad<4> Tb = 73, ng = 8:
                              Tb ng = 584 > 512 so S = 1 with n = 2336 <= 4096; sn_conv_dgrad<4> Co = 32:
                              main loop twice, no tail
  Dense(10)
wide_scratch, input 6x6x16
  Conv2D(32, 3)               linear: n = Tb Co = 145 x 32 = 4640 > kSnScratch, the scratch guard keeps S = 1.
                              The guard is never the only reason: with CG <= 4, Tb Co > 4096 implies
                              Tb ng > 1024, so the item count gives S = 1 as well (here Tb ng = 1160)
  MaxPooling2D                a pool after a linear conv: sn_pool_bwd with mask_in = 0
  Dense(10)
geo3: Conv2D(32, 3, relu, input 28x28x1) . Flatten . Dense(10), B = 37 in a plan of 64; 26842 floats of LDS
  mask 3 / 7                  X(3, 3, 1, 32, 28, 28): sn_conv_fwd_m K = 9 (KS = 3, ragged), MT = 43 (P = 676,
                              ragged), NT = 2; sn_conv_wgrad_m MT NT = 2, S = 4 slices of PS = 169 quads;
                              first layer, no dgrad
  mask 0                      sn_conv_fwd_c<4>; sn_conv_wgrad_c<4> S = 13 row slices of R = 2
lenet5 / lenet5_nobias (use_bias=False on both convs: b_off < 0 in fwd_c, fwd_m, wgrad_c, wgrad_m), B = 37 / 64
  Conv2D(6, 5, same, relu)    X(5, 5, 1, 6, 32, 32) on the zero-padded image.  mask 3 / 7: sn_conv_fwd_m
                              (MT = 49), sn_conv_wgrad_m MT = 2, S = 4.  mask 0: sn_conv_fwd_c<2>,
                              sn_conv_wgrad_c<2> S = 7, R = 4
  MaxPooling2D, Conv2D(16, 5, relu): X(5, 5, 6, 16, 14, 14).  mask 3: sn_conv_fwd_m (K = 150, ragged k
                              tail), sn_conv_wgrad_m MT = 10, S = 1, sn_conv_dgrad_c<4>.  mask 0:
                              sn_conv_fwd_c<4>, sn_conv_wgrad_c<4> S = 1, sn_conv_dgrad_c<4>.  mask 7:
                              sn_conv_dgrad_m, Q = 196: MT = 13 M tiles paired into MP = 7 items (the last
                              pair's second tile is all clamp), results written over the input
  MaxPooling2D, Dense(120, relu), Dense(84, relu), Dense(10): float4 dense forward / backward, scalar head

Masks 0 and 7 run in one fresh child process each (tests/_smallnet_child.py forms): the library reads
TDE_SN_MFMA once per process.  Each child also runs one lenet5 step on unquantized randn data; its conv
gradient hashes must differ from the in-process (mask 3) ones where the mask changes the summation order,
otherwise the child tested the default forms.

Results on an MI355X: no failure, no bug found in smallnet.hip or train/smallnet.py; no variable where the
kernel is over 1e-5 (the fp32 CPU reference is under it everywhere, so every bound is 1e-5).  Largest
error against float64 (worst gradient; loss, eval loss, predict below 3e-7 throughout):
  padded        1.6e-7 conv2d/kernel  (cpu-fp32 1.7e-7)    wide_taps     2.1e-7 conv2d/bias     (2.0e-7)
  wide_out      2.0e-7 dense/bias     (2.0e-7)              wide_scratch  1.5e-7 conv2d/kernel   (2.0e-7)
  lenet5        2.3e-7 conv2d/kernel  (3.8e-7), masks 0 / 7: 2.0e-7 / 2.2e-7
  lenet5_nobias 2.8e-7 conv2d_1/kernel (3.2e-7) at every mask
  geo3          2.2e-7 conv2d/bias    (9.2e-7), mask 0: 1.6e-7
  lenet5 randn  2.5e-7 at masks 0, 3 and 7
A kernel with one output row dropped from the padded weight gradient and one tap from the padded input
gradient (both in bounds) fails the two `padded` cases at 0.35 - 0.39 on conv2d/kernel while
tests/test_smallnet_gpu.py still passes.
"""
import os

import pytest

import smallnet_cases as C
import smallnet_oracle as O
from smallnet_child import guard, run

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,B,Bplan", C.CASES["forms"])
def test_forms_default_mask(name, B, Bplan):
    """Every model and batch in-process (TDE_SN_MFMA default 3: MFMA forward and weight gradient, VALU
    input gradient for the compile-time geometries; the runtime-geometry kernels for everything else)."""
    import tensorflow_distributed_example_amd as tde
    guard()
    O.check(O.measure(tde, "forms", name, B, Bplan))


@pytest.mark.parametrize("mask", ["0", "7"])
def test_forms_child_mask(mask):
    """lenet5, lenet5_nobias, geo3 (and the randn lenet5 step) with all VALU (0) / all MFMA (7) forms."""
    out = run("forms", mask)
    assert [(f["suite"], f["name"], f["data"]) for f in out["figs"]] == (
        [("forms", n, "grid") for n in C.FAST["forms"]] + [("forms", "lenet5", "randn")])
    for fig in out["figs"]:
        O.check(fig)


def test_mask_took_effect():
    """The same randn lenet5 step at masks 0, 3 (in-process) and 7.  Mask 0 sums both conv weight
    gradients in another order (VALU + LDS atomics against MFMA): bit-identical results would mean the
    child ran the default forms.  Mask 7 changes only conv2's input gradient: conv1's kernel gradient
    (downstream of it) differs in bits, conv2's (same MFMA forms on the same operands) does not."""
    import tensorflow_distributed_example_amd as tde
    guard()
    assert os.environ.get("TDE_SN_MFMA", "3") == "3", "the in-process side of this test is the default mask"
    B, Bplan = C.FAST_BATCH
    h0 = [f for f in run("forms", "0")["figs"] if f["data"] == "randn"][0]["conv_grad_hash"]
    h7 = [f for f in run("forms", "7")["figs"] if f["data"] == "randn"][0]["conv_grad_hash"]
    guard()
    fig = O.measure(tde, "forms", "lenet5", B, Bplan, "randn")
    O.check(fig)
    h3 = fig["conv_grad_hash"]
    c1, c2 = sorted(h3)          # conv2d/kernel, conv2d_1/kernel
    assert sorted(h0) == sorted(h7) == [c1, c2]
    assert h0[c1] != h3[c1] and h0[c2] != h3[c2]
    assert h7[c1] != h3[c1] and h7[c2] == h3[c2]
