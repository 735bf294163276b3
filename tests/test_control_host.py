"""Host-side plumbing of the loop's device forms (commands, joint state, masked resets), without a GPU: the five symbols exist in the built
library and in capi.py, the header and capi.py agree on them, every entry point refuses a null engine, control.hip is a unit of the build,
and the validation of buffer arguments (engine.device_buffer) rejects what must not reach a kernel, naming the argument."""
import ctypes as C
import os
import re

import pytest

from mujoco_sim_amd import build, capi
from mujoco_sim_amd.engine import MjhError, device_buffer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mjh_set_cmd_device", "mjh_set_pd_target_device", "mjh_set_xfrc_applied_device", "mjh_get_joint_state_device", "mjh_reset_device"]
MJH_ERR_ARG = -1


def _header():
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "mjhip.h")).read(), flags=re.S)


def test_symbols_exist_in_the_library_and_in_capi(lib):
    table = {name for name, _, _ in capi.SYMBOLS}
    for name in NEW:
        assert name in table, name
        assert getattr(lib, name).argtypes is not None, name


@pytest.mark.parametrize("name", NEW)
def test_header_and_capi_agree(name, lib):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", _header())
    assert m, name
    args = [a.strip() for a in m.group(1).split(",")]
    fn = getattr(lib, name)
    assert fn.restype == C.c_int
    want = [C.c_void_p if "*" in a else C.c_int for a in args]      # engine and buffers: addresses; env0, n: int
    assert list(fn.argtypes) == want, (name, fn.argtypes, args)


def test_err_arg_value_is_the_headers():
    assert re.search(r"MJH_ERR_ARG\s*=\s*-1\b", _header())


@pytest.mark.parametrize("name", NEW)
def test_null_engine_is_an_argument_error(name, lib):
    fn = getattr(lib, name)
    rc = fn(None, 0, 1, *([None] * (len(fn.argtypes) - 3)))
    assert rc == MJH_ERR_ARG
    assert b"null engine" in lib.mjh_last_error()


def test_control_unit_is_part_of_the_build():
    assert "control.hip" in build.SOURCES
    deps = build.SOURCES["control.hip"]
    assert "dev_control.h" in deps and "dev_types.h" in deps and build.API in deps
    assert "dev_control.h" in build.SOURCES["engine.hip"]
    src = open(os.path.join(build.CSRC, "control.hip")).read()
    for inc in re.findall(r'#include\s+"([^"]+)"', src):
        assert os.path.basename(inc) in [os.path.basename(d) for d in deps], inc
    # the new kernels stay out of the step kernel's translation unit
    eng = open(os.path.join(build.CSRC, "engine.hip")).read()
    assert "__global__" in src and "mjh_reset_rows_kernel" not in eng and "mjh_control_rows_kernel" not in eng


# ------------------------------------------------------------------ buffer arguments
def test_integer_address_and_none_pass_through():
    assert device_buffer(0x7F0000001000, "ddq", 12) == 0x7F0000001000
    assert device_buffer(None, "dq", 12) is None


def test_object_without_data_ptr_is_refused():
    with pytest.raises(MjhError, match="ddq"):
        device_buffer([1.0, 2.0], "ddq", 2)


def test_cpu_tensor_is_refused():
    import torch
    t = torch.zeros(3, 4, dtype=torch.float32)
    with pytest.raises(MjhError, match=r"ddq.*device cpu"):
        device_buffer(t, "ddq", 12)
    with pytest.raises(MjhError, match=r"mask.*device cpu"):
        device_buffer(torch.zeros(6, dtype=torch.bool), "mask", 6, dtypes=("uint8", "bool"))


def test_wrong_dtype_is_refused():
    import torch
    with pytest.raises(MjhError, match=r"qvel.*dtype float64"):
        device_buffer(torch.zeros(3, 4, dtype=torch.float64), "qvel", 12)
    with pytest.raises(MjhError, match=r"mask.*dtype float32"):
        device_buffer(torch.zeros(6, dtype=torch.float32), "mask", 6, dtypes=("uint8", "bool"))
    with pytest.raises(MjhError, match=r"qpos.*dtype uint8"):
        device_buffer(torch.zeros(12, dtype=torch.uint8), "qpos", 12)


def test_non_contiguous_view_is_refused():
    import torch
    t = torch.zeros(4, 6, dtype=torch.float32)[:, ::2]      # 12 elements, strided
    with pytest.raises(MjhError, match=r"target.*not contiguous"):
        device_buffer(t, "target", 12)


def test_wrong_element_count_is_refused():
    import torch
    with pytest.raises(MjhError, match=r"xfrc.*12 elements, expected 18"):
        device_buffer(torch.zeros(3, 4, dtype=torch.float32), "xfrc", 18)
