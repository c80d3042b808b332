#!/usr/bin/env python
"""Outline of the memory instructions of the kernels in a gfx950 assembly file.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -I csrc/include -S --cuda-device-only \\
        csrc/kernels/convnet_f32.hip -o convnet_f32.s
    python bench/asm_outline.py convnet_f32.s [--kernel SUBSTR] [--barriers N] [--all]

For each kernel: the register / spill / scratch figures of its metadata, then, in program order up to
the N-th ``s_barrier`` (default 1), every global load, scratch access, ``s_waitcnt`` that names vmcnt,
branch target label and barrier.  Consecutive instructions of one kind are folded into one line with a
count.  A "full wait" is ``vmcnt(0)``: the number of full waits that precede the last global load of the
outline is the number of dependent round trips the prologue pays before its last load is even issued.
Program order is not execution order across branches: read the labels with the source next to it.
"""
from __future__ import annotations

import argparse
import re
import sys

KEEP = re.compile(r"^\s+(global_load\w*|global_store\w*|global_atomic\w*|scratch_\w+|s_waitcnt|s_barrier|s_load\w*|"
                  r"s_cbranch\w*|s_branch|s_endpgm|ds_write\w*|ds_store\w*)\b(.*)")
META = re.compile(r"^\s+\.(name|private_segment_fixed_size|sgpr_count|vgpr_count|vgpr_spill_count|sgpr_spill_count|"
                  r"uses_dynamic_stack):\s+(\S+)")


def kernels(lines):
    """{name: [body lines]} of the functions that end in s_endpgm."""
    out, name, body = {}, None, []
    for ln in lines:
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            name, body = m.group(1), []
            continue
        if name is not None:
            body.append(ln)
            if ln.startswith(".Lfunc_end"):
                out[name] = body
                name = None
    return out


def metadata(lines):
    out, cur = {}, {}
    for ln in lines:
        m = META.match(ln)
        if not m:
            continue
        if m.group(1) == "name":
            cur = out.setdefault(m.group(2), {})
        else:
            cur[m.group(1)] = m.group(2)
    return out


def outline(body, barriers, everything):
    rows, seen = [], 0
    for ln in body:
        lab = re.match(r"^(\.LBB\w+):", ln)
        if lab:
            rows.append(("label", lab.group(1)))
            continue
        m = KEEP.match(ln)
        if not m:
            continue
        op, rest = m.group(1), m.group(2).strip()
        if op == "s_waitcnt":
            if "vmcnt" not in rest:
                continue
            rows.append(("wait", "s_waitcnt " + rest))
        elif op == "s_barrier":
            seen += 1
            rows.append(("barrier", f"s_barrier #{seen}"))
            if not everything and seen >= barriers:
                break
        elif op.startswith("s_cbranch") or op == "s_branch":
            rows.append(("branch", f"{op} {rest}"))
        elif op.startswith("ds_") :
            rows.append(("lds", op))
        elif op == "s_endpgm":
            rows.append(("end", op))
        else:
            rows.append((op, op))
    return rows


def fold(rows):
    out = []
    for kind, text in rows:
        if out and out[-1][0] == kind and out[-1][1] == text and kind not in ("label", "wait", "barrier", "branch"):
            out[-1][2] += 1
        else:
            out.append([kind, text, 1])
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("asm")
    ap.add_argument("--kernel", default="", help="only kernels whose mangled name contains this")
    ap.add_argument("--barriers", type=int, default=1)
    ap.add_argument("--all", action="store_true", help="the whole kernel, not only up to the N-th barrier")
    ap.add_argument("--lds", action="store_true", help="also list the LDS stores")
    a = ap.parse_args(argv)
    lines = open(a.asm).read().splitlines()
    meta = metadata(lines)
    for name, body in kernels(lines).items():
        if a.kernel not in name or name not in meta:
            continue
        print(f"== {name}")
        print("   " + ", ".join(f"{k}={v}" for k, v in meta[name].items()))
        rows = outline(body, a.barriers, a.all)
        if not a.lds:
            rows = [r for r in rows if r[0] != "lds"]
        # labels and branches that no kept instruction separates add nothing
        loads_idx = [i for i, r in enumerate(rows) if r[0].startswith("global_load")]
        last = loads_idx[-1] if loads_idx else -1
        full = sum(1 for r in rows[:last] if r[0] == "wait" and re.search(r"vmcnt\(0\)", r[1]))
        for kind, text, n in fold(rows):
            print(f"   {text}" + (f"  x{n}" if n > 1 else ""))
        print(f"   -> global loads: {len(loads_idx)}, full waits (vmcnt(0)) before the last of them: {full}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
