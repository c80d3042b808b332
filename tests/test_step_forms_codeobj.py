"""The float32 forward launched without a stamp buffer (csrc/kernels/convnet_f32.hip: convnet32_fwd_plain_kernel,
the forward's body with the phase stamps compiled out) keeps its state in registers and needs no more of them than
the form with stamps (CPU: code-object metadata of the in-tree build; no instruction text is read)."""
import os

from test_codeobj import ROOT, _kernels


def test_forward_without_stamps_is_no_larger(tmp_path):
    ks = _kernels(os.path.join(ROOT, "build", "obj", "convnet_f32.hip.o"), tmp_path)
    plain = {k: v for k, v in ks.items() if "convnet32_fwd_plain_kernel" in k}
    diag = {k: v for k, v in ks.items() if "convnet32_fwd_kernel" in k}
    assert len(plain) == 1 and len(diag) == 1, ks.keys()
    (name, meta), (_, dmeta) = next(iter(plain.items())), next(iter(diag.items()))
    assert meta["private_segment_fixed_size"] == "0", (name, meta)
    assert meta.get("uses_dynamic_stack", "false") == "false", (name, meta)
    assert int(meta["vgpr_count"]) <= int(dmeta["vgpr_count"]), (meta, dmeta)
