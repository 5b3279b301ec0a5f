"""mz_rollout at the C-ABI boundary, without a GPU: declared in include/mazestep.h, listed in _capi.SYMBOLS, exported by the built
library, and refusing a NULL handle like mz_step."""
import ctypes as C
import os
import re

from mujoco_maze_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MZ_ERR_ARG = -1


def test_rollout_is_declared_listed_and_exported():
    header = open(os.path.join(ROOT, "include", "mazestep.h")).read()
    m = re.search(r"int32_t\s+mz_rollout\s*\(([^;]*)\);", header)
    assert m, "include/mazestep.h does not declare mz_rollout"
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert len(args) == 11 and args[0].startswith("mz_handle*") and "int64_t action_step_stride" in args[3] and args[-1] == "void* stream"
    assert "mz_rollout" in _capi.SYMBOLS
    lib = _capi.load()
    assert hasattr(lib, "mz_rollout")
    # the defining property is part of the interface
    assert re.search(r"exactly as n_steps successive mz_step calls on the same\s+(\*\s+)?stream would", header)
    assert re.search(r"#define MZ_ABI_VERSION 8\b", header)


def test_rollout_refuses_a_null_handle():
    lib = _capi.load()
    buf = (C.c_float * 4)()
    p = C.cast(buf, C.c_void_p)
    assert lib.mz_rollout(None, 4, p, 0, p, p, p, None, None, None, None) == MZ_ERR_ARG
