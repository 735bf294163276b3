"""Host-side plumbing of the frame states, without a GPU: the two symbols exist in the built library and in capi.py, the header and
capi.py agree on them (the scheme of tests/test_contact_report_host.py), the frame record has the header's layout, and frame.hip is a
unit of the build with its headers."""
import ctypes as C
import os
import re

import pytest

from mujoco_sim_amd import build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mjh_frame_state_device", "mjh_frame_state"]


def _header():
    return open(os.path.join(ROOT, "include", "mjhip.h")).read()


def test_symbols_exist_in_the_library_and_in_capi(lib):
    table = {name for name, _, _ in capi.SYMBOLS}
    for name in NEW:
        assert name in table, name
        fn = getattr(lib, name)      # AttributeError: not exported by the built library
        assert fn.argtypes is not None, name      # capi.load() declared it


def _header_decl(name):
    text = re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S)
    m = re.search(r"\b(void|int)\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
    assert m, name
    args = [a.strip() for a in m.group(2).split(",")] if m.group(2).strip() not in ("", "void") else []
    return m.group(1), args


def _ctype_of(decl):
    if "*" in decl:
        if re.search(r"\bdouble\s*\*", decl): return capi.c_double_p
        if re.search(r"\bint\s*\*", decl): return capi.c_int_p
        return C.c_void_p
    assert re.match(r"(const\s+)?int\b", decl), decl
    return C.c_int


@pytest.mark.parametrize("name", NEW)
def test_header_and_capi_agree(name, lib):
    res, args = _header_decl(name)
    fn = getattr(lib, name)
    assert fn.restype == (None if res == "void" else C.c_int)
    want = [_ctype_of(a) for a in args]
    assert len(fn.argtypes) == len(want), (name, fn.argtypes, args)
    for got, w, a in zip(fn.argtypes, want, args):
        assert got == w, (name, a, got, w)


def test_frame_record_and_enums_match_the_header():
    text = re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S)
    m = re.search(r"typedef\s+struct\s+mjh_frame\s*\{\s*int\s+([^;]*);\s*\}\s*mjh_frame\s*;", text)
    assert m, "struct mjh_frame"
    assert [f.strip() for f in m.group(1).split(",")] == [n for n, _ in capi.Frame._fields_]
    assert all(t is C.c_int for _, t in capi.Frame._fields_) and C.sizeof(capi.Frame) == 5 * C.sizeof(C.c_int)
    assert re.search(r"MJH_FRAME_BODY\s*=\s*0\s*,\s*MJH_FRAME_SITE\s*=\s*1", text) and re.search(r"MJH_FRAME_LOCAL\s*=\s*1\b", text)


def test_frame_unit_is_part_of_the_build():
    assert "frame.hip" in build.SOURCES
    deps = build.SOURCES["frame.hip"]
    assert "dev_frame.h" in deps and build.API in deps
    assert "dev_frame.h" in build.SOURCES["engine.hip"]      # the host side packs the kernel's launch descriptor
    src = open(os.path.join(build.CSRC, "frame.hip")).read()
    for inc in re.findall(r'#include\s+"([^"]+)"', src):      # every project header the unit includes is tracked for staleness
        assert os.path.basename(inc) in [os.path.basename(d) for d in deps], inc
    assert os.path.exists(os.path.join(build.CSRC, "dev_frame.h"))
