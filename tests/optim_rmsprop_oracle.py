"""Float64 oracle of the RMSprop update (``opt_step_x`` in csrc/include/tde_optim.h, kinds 4 and 5) and the
fixtures of its tests (tests/test_optim_rmsprop_oracle.py on the CPU, tests/test_optim_rmsprop_gpu.py on the
GPU).  The grid, the store with every awkward segment, the gap sentinels and ``first_diff`` are those of
tests/optim_oracle.py.

    kind 4  "rmsprop"            r = rho r + (1 - rho) g g ;  w = w - lr g / (sqrt(r) + eps)
    kind 5  "rmsprop_momentum"   r = rho r + (1 - rho) g g ;  q = mom q + lr g / sqrt(r + eps) ;  w = w - q

(g already multiplied by grad_scale; epsilon outside the root without momentum and inside it with momentum,
as TF 2.x Keras has it).  ``oracle_step`` is these formulas in float64 on the float32-rounded
hyper-parameters, 1 - rho formed from the rounded rho as the kernel forms it.  ``fp32_step`` is the same
operation by operation in torch float32 on the host: one sample of what fp32 arithmetic loses.

The exact part: rho = 2^-1, the initial r = |grid_slot| (r is a mean square, so non-negative) and g on the
2^-6 grid below 4.  g g is a multiple of 2^-12 below 16, (1 - rho) g g of 2^-13 below 8, and each step halves
the grid of the old r: after three steps r is a multiple of 2^-15 below 16, 19 bits (with grad_scale = 2^-2:
multiples of 2^-19 below 4, 21 bits; tests/test_optim_rmsprop_oracle.py asserts both).  Every fp32 product
and sum on the way is exact, contracted or not, so the device r has to equal the oracle bit for bit: an
element written to a wrong place, skipped or updated twice shows there.  w and q go through a square root
and a division and are held to the rule the project uses for Adam: per tensor,
e_dev <= max(4 e_host, 2^-22 max |oracle|).
"""
from __future__ import annotations

import torch

import optim_oracle as O
from optim_oracle import (SEGMENTS, assert_shadow_gaps, assert_store_gaps, f32, fill_shadow_gaps,  # noqa: F401
                          fill_store_gaps, first_diff, grid_g, grid_slot, grid_w, hyper32, make_store, seg_mask,
                          view2d)

KINDS = ("rmsprop", "rmsprop_momentum")
KIND_ID = {"rmsprop": 4, "rmsprop_momentum": 5}
# lr and mom powers of two like optim_oracle.GRID_HYPER; b2 carries rho, b1 is unused
GRID_HYPER = dict(lr=0.125, mom=0.5, b1=0.0, b2=0.5, eps=1e-7)
V_SENTINEL = -7779.5      # fills the `v` buffer handed to kind 4, which must not touch it


def grid_r(idx):
    """Initial rms on the exact grid: |grid_slot|, multiples of 2^-6 in [0, 4)."""
    return grid_slot(idx).abs()


def grid_q(idx):
    """Initial momentum accumulator: the 2^-6 grid with a prime of its own."""
    return O.grid(idx, 491, 173, 5)


def oracle_step(kind, hyper, w, g, r, q, grad_scale=1.0):
    """One update on float64 tensors; returns the new (w, r, q) and modifies nothing.  ``q`` comes back
    unchanged (it may be None) for kind "rmsprop"."""
    assert kind in KINDS
    assert all(x is None or x.dtype == torch.float64 for x in (w, g, r, q))
    h = hyper32(hyper)
    g = g * f32(grad_scale)
    r = h["b2"] * r + (1.0 - h["b2"]) * g * g
    if kind == "rmsprop":
        return w - h["lr"] * g / (r.sqrt() + h["eps"]), r, q
    q = h["mom"] * q + h["lr"] * g / (r + h["eps"]).sqrt()
    return w - q, r, q


def fp32_step(kind, hyper, w, g, r, q, grad_scale=1.0):
    """``opt_step_x`` operation by operation in torch float32 (no contraction)."""
    assert kind in KINDS
    assert all(x is None or x.dtype == torch.float32 for x in (w, g, r, q))
    h = {k: torch.tensor(x, dtype=torch.float32) for k, x in hyper.items()}
    one = torch.tensor(1.0, dtype=torch.float32)
    g = g * torch.tensor(grad_scale, dtype=torch.float32)
    r = h["b2"] * r + (one - h["b2"]) * g * g
    if kind == "rmsprop":
        return w - h["lr"] * g / (r.sqrt() + h["eps"]), r, q
    q = h["mom"] * q + h["lr"] * g / (r + h["eps"]).sqrt()
    return w - q, r, q


def bound(e_host, oracle):
    """The per-tensor error bound of a value that went through sqrt and /."""
    return max(4.0 * e_host, 2.0 ** -22 * float(oracle.abs().max()))


def compare(tag, key, name, dev, host, orc, fails):
    """Device and host-fp32 error of one tensor against the oracle; prints the figures, collects a miss."""
    e_dev = float((dev.double() - orc).abs().max())
    e_host = float((host.double() - orc).abs().max())
    b = bound(e_host, orc)
    print(f"[{tag}] {key} {name}: e_dev {e_dev:.3g} e_host {e_host:.3g} bound {b:.3g} max|x| {float(orc.abs().max()):.3g}")
    if not e_dev <= b:
        fails.append((tag, key, name, e_dev, b))
    return e_dev, e_host, b


def optimizer(kind, hyper):
    import tensorflow_distributed_example_amd as tde
    return tde.optimizers.RMSprop(hyper["lr"], rho=hyper["b2"], momentum=hyper["mom"] if kind == "rmsprop_momentum"
                                  else 0.0, epsilon=hyper["eps"])


def row_band_task(n=2048, seed=0):
    """The separable task of tests/test_smallnet_gpu.py::test_smallnet_fit_lenet5: class c lights up row band c."""
    import numpy as np
    rng = np.random.default_rng(seed)
    y = rng.integers(0, 10, n)
    x = rng.random((n, 28, 28, 1), dtype=np.float32) * 0.2
    for c in range(10):
        x[y == c, 2 * c + 4: 2 * c + 6, 4:24, 0] += 1.0
    return x, y


# fit() criterion shared by the CPU and the GPU test: epochs chosen on the CPU reference plan (zoo.mnist_mlp,
# RMSprop(), batch 128) so that last-epoch loss / first-epoch loss is below 0.25 there; the tests assert < 0.5
FIT_EPOCHS = 3
FIT_BATCH = 128
