#!/usr/bin/env python3
"""Loops of one kernel in a hipcc -S listing, by instruction kind.

    hipcc --offload-arch=gfx950 <flags of mujoco_sim_amd/build.py> --cuda-device-only -S csrc/window.hip -o window.s
    python tools/asm_loops.py window.s 'mjh_window_kernelILi24ELi6ELb1E' [min_instructions]

A loop is a backward branch to a label; its body is the text between the label and the branch (inner loops included).  Printed per
loop: the label, the static instruction count and the counts by kind — what the window kernel's sweep loops are made of (HISTORY.md,
"Lean window launch")."""
import collections
import re
import sys


def kind(op, rest):
    if op == "s_nop":
        return "s_nop " + rest.strip()
    if op in ("v_accvgpr_read_b32", "v_accvgpr_write_b32", "v_mov_b32_e32", "v_mov_b32", "v_accvgpr_mov_b32"):
        return op
    if op.startswith("ds_") or op.startswith("global_") or op.startswith("buffer_") or op.startswith("scratch_"):
        return "memory"
    if op.startswith("s_"):
        return "scalar"
    if op.startswith("v_cndmask"):
        return "v_cndmask"
    return "valu"


def main():
    path, pat = sys.argv[1], sys.argv[2]
    least = int(sys.argv[3]) if len(sys.argv) > 3 else 100
    lines = open(path).read().splitlines()
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\S*" + re.escape(pat) + r"\S*:", l))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    body = lines[start:end]
    labels, ins = {}, []
    for l in body:
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            labels[m.group(1)] = len(ins)
            continue
        m = re.match(r"^\t([a-z][a-z0-9_]+)\s*(.*?)(\s*;.*)?$", l)
        if m:
            ins.append((m.group(1), m.group(2)))
    print(f"{pat}: {len(ins)} instructions")
    for i, (op, rest) in enumerate(ins):
        if op.startswith("s_cbranch") or op == "s_branch":
            tgt = rest.strip()
            if tgt in labels and labels[tgt] <= i and i - labels[tgt] >= least:
                seg = ins[labels[tgt]:i + 1]
                c = collections.Counter(kind(o, r) for o, r in seg)
                dpp = sum(1 for o, r in seg if "dpp" in o or "row_" in r or "quad_perm" in r)
                print(f"{tgt}: {len(seg)} instructions (DPP {dpp}) " + ", ".join(f"{k} {v}" for k, v in sorted(c.items())))


if __name__ == "__main__":
    main()
