"""Host-side plumbing of the frame accelerations, without a GPU (the scheme of tests/test_frame_host.py): the two symbols exist in the
built library and in capi.py, the header and capi.py agree on them, MJH_FRAME_PROPER = 2 stands in the header and in capi.py, and
frame_acc.hip is a unit of the build with its headers."""
import ctypes as C
import os
import re

import pytest

from mujoco_sim_amd import build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mjh_frame_accel_device", "mjh_frame_accel"]


def _header():
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "mjhip.h")).read(), flags=re.S)


def test_symbols_exist_in_the_library_and_in_capi(lib):
    table = {name for name, _, _ in capi.SYMBOLS}
    for name in NEW:
        assert name in table, name
        fn = getattr(lib, name)      # AttributeError: not exported by the built library
        assert fn.argtypes is not None, name      # capi.load() declared it


def _header_decl(name):
    m = re.search(r"\b(void|int)\s+" + name + r"\s*\(([^;]*)\)\s*;", _header())
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
    assert len(fn.argtypes) == len(want) == 7, (name, fn.argtypes, args)
    for got, w, a in zip(fn.argtypes, want, args):
        assert got == w, (name, a, got, w)


def test_proper_flag_in_the_header_and_in_capi():
    text = _header()
    assert re.search(r"MJH_FRAME_PROPER\s*=\s*2\b", text) and re.search(r"MJH_FRAME_LOCAL\s*=\s*1\b", text)
    assert capi.MJH_FRAME_PROPER == 2 and capi.MJH_FRAME_LOCAL == 1


def test_frame_acc_unit_is_part_of_the_build():
    assert "frame_acc.hip" in build.SOURCES
    deps = build.SOURCES["frame_acc.hip"]
    assert "dev_frame.h" in deps and "dev_math.h" in deps and build.API in deps
    src = open(os.path.join(build.CSRC, "frame_acc.hip")).read()
    for inc in re.findall(r'#include\s+"([^"]+)"', src):      # every project header the unit includes is tracked for staleness
        assert os.path.basename(inc) in [os.path.basename(d) for d in deps], inc
    assert "#pragma clang fp contract(off)" in src      # every product and sum rounded as written
    assert build.SOURCES["frame.hip"] == ["dev_frame.h", "dev_math.h", build.API]      # the merged unit's entry is as it was
