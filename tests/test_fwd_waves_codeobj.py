"""The float32 forward runs 512-thread workgroups, two waves per SIMD (csrc/kernels/convnet_f32.hip): both of its
kernels keep their state in registers, at most 128 of them, so that two waves per SIMD fit with room, and are built
for workgroups of 512 threads (CPU: code-object metadata of the in-tree build; no instruction text is read)."""
import os
import re
import shutil
import subprocess

import pytest

from test_codeobj import LLVM, ROOT

FIELDS = "name|private_segment_fixed_size|vgpr_count|vgpr_spill_count|uses_dynamic_stack|max_flat_workgroup_size"


def _metadata(obj, tmp_path):
    """{kernel name: {field: value}} of the gfx950 code object in ``obj``: one block per kernel, opened by its
    first key (``- .agpr_count``)."""
    if not os.path.exists(obj) or not shutil.which(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("in-tree build objects / LLVM tools not available")
    fat, co = tmp_path / "fat.bin", tmp_path / "k.co"
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", obj], check=True)
    subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={fat}",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True)
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", str(co)], check=True,
                           stdout=subprocess.PIPE, text=True).stdout
    out = {}
    for block in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
        meta = dict(re.findall(rf"\n\s+\.({FIELDS}):\s+(\S+)", block))
        if "name" in meta:
            out[meta.pop("name")] = meta
    return out


@pytest.mark.parametrize("kernel", ["convnet32_fwd_plain_kernel", "convnet32_fwd_kernel"])
def test_forward_fits_two_waves_per_simd(kernel, tmp_path):
    ks = _metadata(os.path.join(ROOT, "build", "obj", "convnet_f32.hip.o"), tmp_path)
    mine = {k: v for k, v in ks.items() if kernel + "E" in k}
    assert len(mine) == 1, ks.keys()
    name, meta = next(iter(mine.items()))
    assert meta["private_segment_fixed_size"] == "0", (name, meta)
    assert meta.get("uses_dynamic_stack", "false") == "false", (name, meta)
    assert meta["vgpr_spill_count"] == "0", (name, meta)
    assert int(meta["vgpr_count"]) <= 128, (name, meta)
    assert int(meta["max_flat_workgroup_size"]) == 512, (name, meta)
