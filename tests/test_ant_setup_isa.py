"""The set-up of the plain ant's row solver, checked on the compiled code (no GPU needed; skipped without hipcc).

Between the forward pass's contact staging and the Newton loop, `ant_solve_rows_core` (csrc/ant_newton_rows.h) builds the contacts'
rows: 20 times per step, with one wave per SIMD and nothing to hide a wait or an exec-mask region behind.  Two things went and must
not come back (profiles/solve_setup/ab.md):
  * the contact counts read back from LDS right after the forward pass stored them, the wait the very next instruction (they arrive
    in registers now; only the wave-uniform fall-back reads them back, inside its own branch), and with them the overflow test
    that no count can meet, with the status word's read-modify-write;
  * `sees` of `wr_col` as an exec-mask region per contact slot (one bit of a per-lane table now).
The kernel is `ant_step_kernel<0, 16, false, 0>`, compiled with the command of tests/test_ant_isa_slots.py.

Figures, parent -> this change, each bound at what the change reaches plus 0.3 % of room for the compiler's scheduling (rounded up):
    instructions        17 613 -> 17 298   (bound 17 350)
    s_waitcnt              160 ->    163   (bound 164: the count read-back's wait and the status word's went, the compiler splits
                                            the wait for the staged contact's reads and the scalar loads behind it differently)
    s_and_saveexec_b64     765 ->    751   (bound 754)
"""
import math
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mujoco_maze_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not present")

MARK = "fall-back counts read back"  # comment of the asm statement at the end of the forward pass's fall-back (ant_forward_rows.h)


def _make_var(name):
    """value of a simple `NAME = ...` assignment of csrc/Makefile"""
    for line in open(os.path.join(CSRC, "Makefile")):
        m = re.match(rf"^{name}\s*=\s*(.*)$", line)
        if m:
            return m.group(1).split()
    raise AssertionError(f"{name} not set in csrc/Makefile")


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    """([(mnemonic, operand text)], index of the first instruction behind the fall-back's end mark or None)"""
    out = str(tmp_path_factory.mktemp("isa") / "k_0_16.s")
    base = [f.replace("$(ARCH)", "gfx950") for f in _make_var("BASE")]
    cmd = [HIPCC] + base + _make_var("FAST") + ["-DMZ_ISA_ONLY", "-DMZ_ISA_NB=0", "-DMZ_ISA_G=16", "-DMZ_ISA_PROF=false", "-DMZ_ISA_WPS=0",
                                                "--cuda-device-only", "-S", "-o", out, "ant_kernels.hip"]
    res = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    insts, mark = [], None
    for line in open(out):
        if MARK in line and mark is None:
            mark = len(insts)
        t = line.split(";")[0].strip()
        m = re.match(r"^((?:v|s|ds|global|buffer|flat|scratch)_\w+)\s*(.*)$", t)
        if m:
            insts.append((re.sub(r"_e(32|64)$", "", m.group(1)), m.group(2)))
    assert len(insts) > 10000, len(insts)
    return insts, mark


def _bound(reached):
    return math.ceil(reached * 1.003)


def test_three_figures(isa):
    insts = isa[0]
    n = len(insts)
    nwait = sum(1 for mn, _ in insts if mn == "s_waitcnt")
    nexec = sum(1 for mn, _ in insts if mn == "s_and_saveexec_b64")
    print(f"instructions {n}, s_waitcnt {nwait}, s_and_saveexec_b64 {nexec}")
    assert n <= _bound(17298), n        # parent: 17 613
    assert nwait <= _bound(163), nwait  # parent: 160 (module docstring)
    assert nexec <= _bound(751), nexec  # parent: 765


def test_no_read_back_in_front_of_the_setup(isa):
    """From the end of the forward pass's contact staging to the first `v_fmac_f32_dpp` of the set-up no `ds_read` stands directly in
    front of the `s_waitcnt` that waits for it.  The staging ends, in the kernel's text, with the fall-back (its records are the last
    16-byte staging stores), and the fall-back with the asm statement that holds the counts it read back — the one place where
    they are read as before.  The stretch starts behind that statement's mark, and the mark must stand behind the last staging store,
    close to it, and in front of the set-up.  `s_waitcnt lgkmcnt(0)` is the wait that covers the read in front of it; one with a
    count of N > 0 behind a batch of reads leaves the N latest in flight, the one in front of it among them."""
    insts, mark = isa
    assert mark is not None, "the fall-back's end mark is not in the kernel's text"
    end = next(i for i in range(mark, len(insts)) if insts[i][0] == "v_fmac_f32_dpp")
    last_store = max(i for i in range(end) if insts[i][0] == "ds_write_b128")
    assert last_store < mark and mark - last_store < 200, (last_store, mark)  # the fall-back's tail, nothing else, lies between
    assert 20 < end - mark < 4000, (mark, end)  # the limit row (with impedance_pair's text) lies in between
    bad = [(i - mark, insts[i], insts[i + 1]) for i in range(mark, end)
           if insts[i][0].startswith("ds_read") and insts[i + 1][0] == "s_waitcnt" and "lgkmcnt(0)" in insts[i + 1][1]]
    print(f"stretch: {end - mark} instructions, {mark - last_store} behind the last staging store; read-backs: {bad}")
    assert not bad, bad
