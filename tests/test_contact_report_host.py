"""Host-side plumbing of the contact report, without a GPU: the new symbols exist in the built library and in capi.py, the header and
capi.py agree on them, and the process-wide switch defaults to 0 and follows MJH_CONTACT_REPORT."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

from mujoco_sim_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mjh_set_contact_report", "mjh_contact_report", "mjh_contact_report_device", "mjh_get_contact_forces", "mjh_get_cfrc_ext",
       "mjh_body_contact_force_device", "mjh_body_contact_force"]


def test_symbols_exist_in_the_library_and_in_capi(lib):
    table = {name for name, _, _ in capi.SYMBOLS}
    for name in NEW:
        assert name in table, name
        fn = getattr(lib, name)      # AttributeError: not exported by the built library
        assert fn.argtypes is not None, name      # capi.load() declared it


def _header_decl(name):
    text = open(os.path.join(ROOT, "include", "mjhip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    m = re.search(r"\b(void|int)\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
    assert m, name
    args = [a.strip() for a in m.group(2).split(",")] if m.group(2).strip() not in ("", "void") else []
    return m.group(1), args


def _ctype_of(decl):
    if "*" in decl:
        if re.search(r"\bdouble\s*\*", decl): return capi.c_double_p
        if re.search(r"\bint\s*\*", decl): return capi.c_int_p
        if re.search(r"void\s*\*\s*\*", decl): return C.POINTER(C.c_void_p)
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


def _switch_in_child(env_value):
    env = dict(os.environ)
    env.pop("MJH_CONTACT_REPORT", None)
    if env_value is not None:
        env["MJH_CONTACT_REPORT"] = env_value
    code = ("import sys; sys.path.insert(0, %r); from mujoco_sim_amd import capi; L = capi.load(); a = L.mjh_contact_report(None); "
            "L.mjh_set_contact_report(1); b = L.mjh_contact_report(None); L.mjh_set_contact_report(0); print(a, b, L.mjh_contact_report(None))" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True).stdout.split()
    return [int(x) for x in out[-3:]]


def test_switch_defaults_to_off_and_follows_the_environment():
    # (the switch is read when the library is loaded: a fresh process per value)
    assert _switch_in_child(None) == [0, 1, 0]
    assert _switch_in_child("0") == [0, 1, 0]
    assert _switch_in_child("1") == [1, 1, 0]
