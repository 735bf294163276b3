"""CPU test: the register budget S24's step rests on, read from the code object's kernel metadata.

S24's cohort-step is the assemble-only launch `mjh_step_kernel<2, true, false, 1>` followed by the lean window instance
`mjh_window_kernel<24, 6, true, ...>` (csrc/window.hip: the one instance with the cross tiles in LDS, what launches without the LDS tier run).  The window wavefront stays on its SIMD for the whole launch; an assemble
wavefront of another cohort can only start on that SIMD if both allocations fit the SIMD's register file together:

    ceil8(vgpr + agpr of the window instance) + ceil8(vgpr + agpr of the assemble instance) <= 512

(8: allocation granule of the unified register file, 512: registers per lane and SIMD on CDNA4; the code object's .vgpr_count is already the unified sum).  Neither
may spill vector registers or use scratch memory.  A later edit that grows either kernel past the sum loses the overlap silently:
this test pins it."""
import os
import re
import shutil
import struct
import subprocess

import pytest

from mujoco_sim_amd import capi

GRANULE, REGISTER_FILE = 8, 512
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _readelf():
    for p in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-readelf"), shutil.which("llvm-readelf"), shutil.which("readelf")):
        if p and os.path.exists(p):
            return p
    return None


def _gfx950_code_objects(lib_path):
    """the gfx950 entries of every (uncompressed) offload bundle in the library: one per HIP translation unit"""
    data = open(lib_path, "rb").read()
    out = []
    for m in re.finditer(MAGIC, data):
        base = m.start()
        (n,) = struct.unpack_from("<Q", data, base + len(MAGIC))
        pos = base + len(MAGIC) + 8
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", data, pos)
            triple = data[pos + 24:pos + 24 + tl].decode()
            pos += 24 + tl
            if "gfx950" in triple and size > 0:
                out.append(data[base + off:base + off + size])
    return out


def _kernel_metadata(lib_path, tmp_path, tool):
    """{demangled kernel name: {field: int}} from the AMDGPU metadata note of every gfx950 code object"""
    kernels = {}
    for i, blob in enumerate(_gfx950_code_objects(lib_path)):
        p = tmp_path / f"co{i}.elf"
        p.write_bytes(blob)
        txt = subprocess.run([tool, "--notes", str(p)], capture_output=True, text=True, check=True).stdout
        # the metadata is printed as YAML: one "- .agpr_count: ..." item per kernel under amdhsa.kernels, keys in alphabetical order
        for item in re.split(r"\n\s*- \.agpr_count:", txt)[1:]:
            item = ".agpr_count:" + item
            name = re.search(r"\.name:\s+(\S+)", item)
            if not name:
                continue
            fields = {k: int(v) for k, v in re.findall(r"\.(agpr_count|vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s+(\d+)", item)}
            kernels[name.group(1)] = fields
    return kernels


def _ceil(x, g):
    return (x + g - 1) // g * g


def test_s24_window_and_assemble_wavefronts_fit_one_simd_together(lib, tmp_path):
    tool = _readelf()
    if tool is None:
        pytest.skip("no llvm-readelf / readelf on this machine: the code object's kernel metadata cannot be read")
    kernels = _kernel_metadata(capi.LIB_PATH, tmp_path, tool)
    assert len(kernels) > 10, "kernel metadata of the gfx950 code objects"
    # mangled names: mjh_window_kernel<24, 6, true, ...> and mjh_step_kernel<2, true, false, 1[, false]> (a trailing HF = false where the kernel has the parameter)
    win = [k for k in kernels if re.match(r"_Z17mjh_window_kernelILi24ELi6ELb1E", k)]
    pre = [k for k in kernels if re.match(r"_Z15mjh_step_kernelILi2ELb1ELb0ELi1E(Lb0E)?E", k)]
    assert len(win) == 1 and len(pre) == 1, (win, pre, sorted(k for k in kernels if "window" in k))
    w, a = kernels[win[0]], kernels[pre[0]]
    print(f"window instance {w}, assemble instance {a}")
    for name, k in (("window", w), ("assemble", a)):
        assert k["vgpr_spill_count"] == 0, f"{name}: vector registers spilled"
        assert k["private_segment_fixed_size"] == 0, f"{name}: scratch memory"
    # .vgpr_count of a gfx950 code object is the unified count: architectural registers (rounded up to their own granule where accumulation
    # registers follow) + .agpr_count
    w_regs, a_regs = w["vgpr_count"], a["vgpr_count"]
    assert w_regs >= w["agpr_count"] and a_regs >= a["agpr_count"]
    total = _ceil(w_regs, GRANULE) + _ceil(a_regs, GRANULE)
    print(f"window {w_regs} -> {_ceil(w_regs, GRANULE)}, assemble {a_regs} -> {_ceil(a_regs, GRANULE)}, together {total} of {REGISTER_FILE}")
    assert total <= REGISTER_FILE, f"window {w_regs} + assemble {a_regs} registers do not fit one SIMD together ({total} > {REGISTER_FILE})"
