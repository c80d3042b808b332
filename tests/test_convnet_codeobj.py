"""The float32 step kernels of the fused MNIST-CNN plan keep their state in registers: a spill puts a scratch
store and a reload with a full wait into the prologue, ahead of the loads the kernel's time hangs on
(CPU: code-object metadata of the in-tree build; no instruction text is read)."""
import os

from test_codeobj import ROOT, _kernels


def test_convnet_f32_kernels_use_no_scratch(tmp_path):
    ks = _kernels(os.path.join(ROOT, "build", "obj", "convnet_f32.hip.o"), tmp_path)
    step = {k: v for k, v in ks.items() if "convnet32_fwd_kernel" in k or "convnet32_bwd_kernel" in k}
    # the forward and the backward's three instantiations (plain, fused SGD, fused with slots)
    assert len(step) == 4 and sum("convnet32_bwd_kernel" in k for k in step) == 3, ks.keys()
    for name, meta in step.items():
        assert meta["private_segment_fixed_size"] == "0", (name, meta)
        assert meta.get("uses_dynamic_stack", "false") == "false", (name, meta)
