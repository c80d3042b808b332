"""The ``FlatApply`` that ``ops.kernels.copy_pairs_apply`` hands to ``tde_copy_pairs_apply`` by pointer is the
ctypes mirror of csrc/include/tde_optim.h's struct: the size the built library reports, read without a GPU."""
import ctypes as C

import pytest

from tensorflow_distributed_example_amd import _native as N


@pytest.mark.skipif(not N.hip_available(), reason="libtde_hip.so not built")
def test_copy_pairs_apply_takes_the_kernels_flat_apply():
    from tensorflow_distributed_example_amd.ops import kernels as K
    out = (C.c_longlong * 4)()
    assert N.hip().tde_cnet_abi_sizes(out, 4) == 4
    assert C.sizeof(K.FlatApply) == out[2]                     # {StepOpt, BwdOpt, FlatApply, OptHyper}
    fn = N.hip().tde_copy_pairs_apply
    assert fn.restype is C.c_int and len(fn.argtypes) == 6 and fn.argtypes[4] is C.c_void_p
