"""The row solver's contact slots 0 .. 3 each sit behind a wave-uniform guard of their own (csrc/ant_newton_rows.h each_contact),
seen on the compiled code of `ant_step_kernel<0, 16, false, 0>` (no GPU needed; skipped without hipcc).

The Hessian fold of one contact slot is 48 `v_fmac_f32_dpp`.  Split at labels and branches, the kernel's text used to hold three
branch-free runs with more than 100 of them: slots 0 - 3 in one run of 192, and the groups of four of slots 8 - 11 and 12 - 15.
With a guard per slot only the two groups remain, and the folds of slots 0 .. 3 are runs of 48.  Compiled the way
tests/test_ant_isa_slots.py compiles it, with the flags of csrc/Makefile."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mujoco_maze_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not present")


def _make_var(name):
    for line in open(os.path.join(CSRC, "Makefile")):
        m = re.match(rf"^{name}\s*=\s*(.*)$", line)
        if m:
            return m.group(1).split()
    raise AssertionError(f"{name} not set in csrc/Makefile")


def test_slots_0_to_3_fold_in_runs_of_their_own(tmp_path):
    out = str(tmp_path / "k_0_16.s")
    base = [f.replace("$(ARCH)", "gfx950") for f in _make_var("BASE")]
    cmd = [HIPCC] + base + _make_var("FAST") + ["-DMZ_ISA_ONLY", "-DMZ_ISA_NB=0", "-DMZ_ISA_G=16", "-DMZ_ISA_PROF=false", "-DMZ_ISA_WPS=0",
                                                "--cuda-device-only", "-S", "-o", out, "ant_kernels.hip"]
    res = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    runs, n, total = [], 0, 0
    for line in open(out):
        t = line.split(";")[0].strip()
        if re.match(r"^[.\w$]+:", t) or re.match(r"^s_c?branch", t) or t.startswith("s_setpc") or t.startswith("s_endpgm"):
            runs.append(n)
            n = 0
        elif t.startswith("v_fmac_f32_dpp"):
            n += 1
            total += 1
    runs.append(n)
    long_runs = sorted((r for r in runs if r >= 40), reverse=True)
    print(f"v_fmac_f32_dpp: {total}; branch-free runs of 40 and more: {long_runs}")
    assert total > 1000, total  # the folds of 16 slots alone are 768
    assert sum(1 for r in runs if r > 100) <= 2, long_runs  # slots 8 - 11 and 12 - 15; before: a third, slots 0 - 3
    assert runs.count(48) >= 4, long_runs                  # the folds of slots 0, 1, 2 and 3
