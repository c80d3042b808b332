"""The ctypes mirrors of the kernels' argument structs (ops/kernels.py) have the size of the C++ structs
they stand for (csrc/include/tde_convnet.h, tde_optim.h, csrc/comm/xgmi_allreduce.hip, csrc/kernels/bncnn.hip,
convnet_gen.hip).  A field added on one side only would shift every later field of a struct passed by pointer:
read without a GPU, from the built library's host-side size exports.

Every optimizer struct starts with ``OptHyper h`` (24 bytes, alignment 4) and its first pointer follows at
offset 24.  The sizes are also pinned as literals: they are those of the build in which the six
hyper-parameters were still written out field by field at the head of each struct, so moving them into ``h``
is shown to have moved nothing."""
import ctypes as C

import pytest

from tensorflow_distributed_example_amd import _native as N

PINNED = {"StepOpt": 136, "BwdOpt": 264, "FlatApply": 128, "OptHyper": 24, "XgApply": 160, "XgPush": 104,
          "CgenFly": 144, "CgenOpt": 56, "CgenHead": 96, "BnOpt": 64}
# the optimizer structs and their first pointer member
FIRST_POINTER = {"StepOpt": "w", "BwdOpt": "w", "XgApply": "w", "BnOpt": "g", "CgenOpt": "w", "CgenFly": "pend",
                 "CgenHead": "w"}


def _sizes(fn, n):
    out = (C.c_longlong * n)()
    got = fn(out, n)
    assert got == n
    return list(out)


def _check(names, sizes):
    from tensorflow_distributed_example_amd.ops import kernels as K
    for name, size in zip(names, sizes):
        assert C.sizeof(getattr(K, name)) == size == PINNED[name], name


@pytest.mark.skipif(not N.hip_available(), reason="libtde_hip.so not built")
def test_fused_step_structs_match_the_kernels():
    _check(["StepOpt", "BwdOpt", "FlatApply", "OptHyper"], _sizes(N.hip().tde_cnet_abi_sizes, 4))


@pytest.mark.skipif(not N.hip_available(), reason="libtde_hip.so not built")
def test_xgmi_structs_match_the_kernels():
    _check(["XgApply", "XgPush"], _sizes(N.hip().tde_xgmi_abi_sizes, 2))


@pytest.mark.skipif(not N.hip_available(), reason="libtde_hip.so not built")
def test_generic_step_and_bn_structs_match_the_kernels():
    _check(["CgenFly", "CgenOpt", "CgenHead"], _sizes(N.hip().tde_cgen_abi_sizes, 3))
    _check(["BnOpt"], _sizes(N.hip().tde_bncnn_abi_sizes, 1))


def test_every_optimizer_struct_starts_with_the_hyper_parameters():
    from tensorflow_distributed_example_amd.ops import kernels as K
    assert C.sizeof(K.OptHyper) == 24 and C.alignment(K.OptHyper) == 4
    assert [f[0] for f in K.OptHyper._fields_] == ["kind", "lr", "mom", "b1", "b2", "eps"]
    for name, first in FIRST_POINTER.items():
        S = getattr(K, name)
        assert S._fields_[0] == ("h", K.OptHyper) and S.h.offset == 0, name
        assert S._fields_[1][0] == first and getattr(S, first).offset == 24, name
        assert C.sizeof(S) == PINNED[name], name
