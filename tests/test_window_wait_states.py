"""CPU test: the wait states of the window kernel's cross-lane reads, checked on the compiler's listing.

csrc/window_kernel.h writes its sweeps as `asm volatile` statements of DPP and lane-swap instructions.  The compiler pads no hazard inside
such a statement, and the statements carry an `s_nop` only where a hazard exists: which instruction wrote the register a DPP read or a swap
takes, and how long ago, is decided by the order of the statements and by what the compiler put between them.  This test compiles
csrc/window.hip to a listing for gfx950 with build.py's flags (the command of tools/asm_loops.py) and walks every instruction of the three
window instances:

    a VALU write of a register  ->  a DPP instruction reading it through the DPP network (src0):  2 wait states
    a VALU write of a register  ->  v_permlane16_swap / v_permlane32_swap reading it (either operand):  2 wait states
    a swap's result -> a plain VALU read: none; -> a DPP read or another swap: the two rules above (the swap is a VALU write of both operands;
    what hipcc emits around `__builtin_amdgcn_permlane16_swap` / `32_swap`, profiles/window_slots_summary.md)

A wait state is one issued instruction; `s_nop N` counts as N + 1.  At a label the walk goes back through the fall-through predecessor and
through every branch to that label (the loops' back edges).  The counts at the end keep the nops from creeping back."""
import os
import re
import subprocess

import pytest

import hostbuild
from mujoco_sim_amd import build as mjbuild

# consumer kind -> (which operands are read across lanes, wait states a VALU write of them needs in front)
RULES = {
    "dpp": ("src0", 2),
    "v_permlane16_swap": ("both", 2),
    "v_permlane32_swap": ("both", 2),
}
# The filled row chain (window_kernel.h, WN_ROWF / WN64_RF): `v_max_f32 d` -> ONE independent VALU instruction -> `v_fmac_f32_dpp t, d, a row_newbcast`.
# Its wavefront is alone on its SIMD and issues one instruction per 8 clocks, so one instruction between the two is 16 clocks, more than the 12 that
# two wait states stand for (measured and bitwise against the chain with its nops: HISTORY.md, "The row chain with its wait states put to work").  Kept as it is.
# The exemption holds for the chain alone: the multiply-add accumulates into the register the v_max took its first source from (t -> d -> t).  Any
# other reader of a v_max result — the cross multiply-adds of a window pair read the closing v_max of the other window's chain — needs its two states.
ROW_CHAIN = ("v_max_f32", "v_fmac_f32_dpp", "row_newbcast", 1)
INSTANCES = {"lean": "_Z17mjh_window_kernelILi24ELi6ELb1E", "fat": "_Z17mjh_window_kernelILi24ELi6ELb0E", "32-slot": "_Z17mjh_window_kernelILi32E"}
# `s_nop 1` of the two critical sweep loops of the lean instance (static count of the loop body, both arms of its last-pair / last-odd-window
# branch; 16 of the straight loop's stand in the chain of the last odd window, one is the compiler's in front of the convergence reduce; 64 of the
# 64-row loop's stand in its first and last lane row):
# what the listing has with this change — 46 and 110 before it
MAX_NOP1_STRAIGHT6 = 17
MAX_NOP1_FORM64 = 84


def _regs(tok):
    """VGPR numbers of one operand: v12, v[12:13]; anything else (SGPRs, AGPRs, literals, vcc): none"""
    tok = tok.strip().lstrip("-|").rstrip("|")
    m = re.fullmatch(r"v(\d+)", tok)
    if m:
        return {int(m.group(1))}
    m = re.fullmatch(r"v\[(\d+):(\d+)\]", tok)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    return set()


class Ins:
    __slots__ = ("op", "ops", "writes", "kind", "xreads", "states", "target", "line")

    def __init__(self, op, rest, line):
        self.op, self.line = op, line
        mods = re.split(r"\s+(?=(?:row_|quad_perm|wave_|bank_mask|bound_ctrl|op_sel|neg_|clamp|mul:|div:|offset|gds|sc0|sc1|nt)\b)", rest, 1)
        self.ops = [t for t in (x.strip() for x in mods[0].split(",")) if t]
        self.writes, self.kind, self.xreads, self.target = set(), None, set(), None
        self.states = 1
        if op == "s_nop":
            self.states = int(self.ops[0], 0) + 1
        if op.startswith("s_cbranch") or op == "s_branch":
            self.target = self.ops[0]
        if op.startswith("v_") and self.ops:
            swap = next((k for k in RULES if k != "dpp" and op.startswith(k)), None)
            if swap:
                self.kind = swap
                self.writes = _regs(self.ops[0]) | _regs(self.ops[1])
                self.xreads = set(self.writes)
            else:
                self.writes = _regs(self.ops[0])
                if "_dpp" in op or re.search(r"\b(row_|quad_perm|wave_sh|wave_ro|row_newbcast|row_share|row_xmask)", rest):
                    self.kind = "dpp"
                    # src0: the first source — behind the destination (and behind a carry-out / compare destination that is no VGPR)
                    srcs = self.ops[1:]
                    while srcs and not _regs(srcs[0]) and re.fullmatch(r"vcc|s\[\d+:\d+\]|s\d+", srcs[0]):
                        srcs = srcs[1:]
                    self.xreads = _regs(srcs[0]) if srcs else set()


def _listing(tmp_path_factory):
    out = tmp_path_factory.mktemp("window_listing") / "window.s"
    src = os.path.join(mjbuild.CSRC, "window.hip")
    flags = [f for f in mjbuild.FLAGS if f != "-fPIC"] + mjbuild.SOURCE_FLAGS.get("window.hip", [])
    subprocess.check_call([hostbuild.hipcc()] + flags + ["--cuda-device-only", "-S", src, "-o", str(out)], stderr=subprocess.DEVNULL)
    return out.read_text().splitlines()


def _kernel(lines, prefix):
    start = next(i for i, l in enumerate(lines) if re.match(re.escape(prefix) + r"\S*:", l))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    ins, labels = [], {}
    for l in lines[start + 1:end]:
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            labels[m.group(1)] = len(ins)
            continue
        m = re.match(r"^\t([a-z][a-z0-9_]+)\s*(.*?)(\s*;.*)?$", l)
        if m:
            ins.append(Ins(m.group(1), m.group(2), l.strip()))
    return ins, labels


def _violations(ins, labels):
    at_label = {}
    for name, i in labels.items():
        at_label.setdefault(i, []).append(name)
    branches = {}
    for i, x in enumerate(ins):
        if x.target:
            branches.setdefault(x.target, []).append(i)
    bad = []

    def preds(i):
        p = []
        if i > 0 and ins[i - 1].op not in ("s_branch", "s_endpgm", "s_setpc_b64"):
            p.append(i - 1)
        for name in at_label.get(i, ()):
            p.extend(branches.get(name, ()))
        return p

    for i, x in enumerate(ins):
        if not x.kind:
            continue
        need = RULES[x.kind][1]
        stack, seen = [(p, need) for p in preds(i)], set()
        while stack:
            j, left = stack.pop()
            if (j, left) in seen:
                continue
            seen.add((j, left))
            w = ins[j]
            if w.op.startswith("v_") and (w.writes & x.xreads):
                chain = w.op.startswith(ROW_CHAIN[0]) and x.op == ROW_CHAIN[1] and ROW_CHAIN[2] in x.line and len(w.ops) > 1 and x.ops[0] == w.ops[1]
                if not (chain and need - left >= ROW_CHAIN[3]):
                    bad.append(f"{w.line}   ->   {x.line}   ({need - left} wait states between, {need} needed)")
                continue
            left -= w.states
            if left > 0:
                stack.extend((p, left) for p in preds(j))
    return bad


def _loops(ins, labels):
    """(first, last) of every loop: a backward branch to a label"""
    return [(labels[x.target], i) for i, x in enumerate(ins) if x.target in labels and labels[x.target] <= i]


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    return _listing(tmp_path_factory)


@pytest.mark.parametrize("name", list(INSTANCES))
def test_no_cross_lane_read_inside_the_wait_states_of_its_producer(listing, name):
    ins, labels = _kernel(listing, INSTANCES[name])
    n = sum(1 for x in ins if x.kind)
    assert n > 1000, "the instance's DPP and swap instructions"
    bad = _violations(ins, labels)
    print(f"{name}: {len(ins)} instructions, {n} DPP / swap instructions, {len(bad)} inside their producer's wait states")
    assert not bad, "\n".join(bad[:20])


def test_the_nops_do_not_creep_back(listing):
    ins, labels = _kernel(listing, INSTANCES["lean"])
    loops = _loops(ins, labels)

    def count(seg, pred):
        return sum(1 for x in seg if pred(x))
    is_nop1 = lambda x: x.op == "s_nop" and x.states == 2
    is_swap = lambda x: x.kind in ("v_permlane16_swap", "v_permlane32_swap")
    is_mem = lambda x: x.op.startswith(("ds_", "global_", "buffer_", "scratch_"))
    # the six-window straight loop: the loop whose only memory instructions are the twelve cross-tile reads of its three pairs
    straight6 = [ins[a:b + 1] for a, b in loops if b - a > 600 and count(ins[a:b + 1], is_mem) == 12 and count(ins[a:b + 1], lambda x: x.op == "ds_read_b128") == 12 and not count(ins[a:b + 1], is_swap)]
    assert len(straight6) == 1, [len(s) for s in straight6]
    # the 64-row form's loop over two register-resident windows: nine lane swaps per window, no memory
    form64 = [ins[a:b + 1] for a, b in loops if count(ins[a:b + 1], is_swap) == 18 and not count(ins[a:b + 1], is_mem)]
    assert len(form64) == 1, [len(s) for s in form64]
    n6, n64 = count(straight6[0], is_nop1), count(form64[0], is_nop1)
    print(f"six-window straight loop: {len(straight6[0])} instructions, {n6} s_nop 1; 64-row two-window loop: {len(form64[0])} instructions, {n64} s_nop 1")
    assert n6 <= MAX_NOP1_STRAIGHT6
    assert n64 <= MAX_NOP1_FORM64
