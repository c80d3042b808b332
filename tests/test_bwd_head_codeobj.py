"""The float32 backward kernels specialised for 28 x 28 images (csrc/kernels/convnet_f32.hip: convnet32g_*) keep
their state in registers like the runtime-geometry forms that tests/test_convnet_codeobj.py checks, and the
backward stays within 128 VGPRs (CPU: code-object metadata of the in-tree build; no instruction text is read)."""
import os

from test_codeobj import ROOT, _kernels


def test_specialised_convnet_f32_kernels_use_no_scratch(tmp_path):
    ks = _kernels(os.path.join(ROOT, "build", "obj", "convnet_f32.hip.o"), tmp_path)
    spec = {k: v for k, v in ks.items() if "convnet32g_" in k}
    # the backward's three instantiations (plain, fused SGD, fused with slots)
    assert len(spec) == 3 and all("convnet32g_bwd_kernel" in k for k in spec), ks.keys()
    for name, meta in spec.items():
        assert meta["private_segment_fixed_size"] == "0", (name, meta)
        assert meta.get("uses_dynamic_stack", "false") == "false", (name, meta)
    for name, meta in ks.items():
        if "convnet32g_bwd_kernel" in name or "convnet32_bwd_kernel" in name:
            assert int(meta["vgpr_count"]) <= 128, (name, meta)
