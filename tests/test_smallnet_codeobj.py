"""The fused small-net kernels keep their state in registers: Dropout (Philox blocks drawn inside the
step kernel) must not push smallnet_step_kernel into scratch (CPU: code-object metadata of the in-tree build)."""
import os

from test_codeobj import ROOT, _kernels


def test_smallnet_kernels_use_no_scratch(tmp_path):
    ks = _kernels(os.path.join(ROOT, "build", "obj", "smallnet.hip.o"), tmp_path)
    sn = {k: v for k, v in ks.items() if "smallnet_step_kernel" in k or "smallnet_wgrad_kernel" in k}
    assert len(sn) == 2, ks.keys()
    for name, meta in sn.items():
        assert meta["private_segment_fixed_size"] == "0", (name, meta)
        assert meta.get("uses_dynamic_stack", "false") == "false", (name, meta)
