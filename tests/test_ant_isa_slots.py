"""Issue slots of the plain ant's step kernel, counted on the compiled code (no GPU needed; skipped without hipcc).

With one wave per SIMD nothing hides an instruction of `ant_step_kernel<0, 16, false, 0>` — the instantiation bench.py measures
— so what it costs is, first of all, how many instructions it issues.  Three things used to spend slots on
nothing and must not come back:
  * packed f32 arithmetic around the row butterflies: a `v_pk_add_f32` takes no DPP operand, so two butterflies side by side
    became two unfused `v_mov_b32_dpp`, the packed add and a wait state (now: rows::rsum3 / rsum3_scaled / rsum2, hand-scheduled
    `v_add_f32_dpp` chains);
  * the pivot of the row elimination as broadcast + fmaxf: a zero `old`, the `v_mov_b32_dpp`, a canonicalising `v_max x, x, x`
    and the `v_max` itself (now: one `v_max_f32_dpp`, rows::pivot_clamped);
  * hand-written DPP blocks are outside the compiler's hazard recogniser: tools/check_dpp_hazards.py must stay at 0.
The kernel is compiled the way tools/isa_one.sh compiles it (one instantiation, ~10 s), with the flags of csrc/Makefile.

The library is built WITHOUT `-fno-slp-vectorize` (it would take the remaining packed arithmetic out of this kernel as well, but
the lane-group solver of the mazes with several blocks loses 1.3 .. 2.8 % under it: profiles/issue_slots/ab.md), so the two
whole-kernel bounds that flag would have set — packed instructions and total length — are what the helpers alone reach, with
0.3 % of room for the compiler's scheduling: 613 packed f32 instructions (before: 991) and 17 675 instructions (before: 18 073,
counted as below: every line of the kernel's text that starts with a v_ / s_ / ds_ / global_ / buffer_ / flat_ / scratch_
mnemonic)."""
import importlib.util
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
    """value of a simple `NAME = ...` assignment of csrc/Makefile"""
    for line in open(os.path.join(CSRC, "Makefile")):
        m = re.match(rf"^{name}\s*=\s*(.*)$", line)
        if m:
            return m.group(1).split()
    raise AssertionError(f"{name} not set in csrc/Makefile")


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    """(path of the .s, [(mnemonic, operand text)]) of ant_step_kernel<0, 16, false, 0>, built with the library's own flags"""
    out = str(tmp_path_factory.mktemp("isa") / "k_0_16.s")
    base = [f.replace("$(ARCH)", "gfx950") for f in _make_var("BASE")]
    cmd = [HIPCC] + base + _make_var("FAST") + ["-DMZ_ISA_ONLY", "-DMZ_ISA_NB=0", "-DMZ_ISA_G=16", "-DMZ_ISA_PROF=false", "-DMZ_ISA_WPS=0",
                                                "--cuda-device-only", "-S", "-o", out, "ant_kernels.hip"]
    res = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    insts = []
    for line in open(out):
        t = line.split(";")[0].strip()
        m = re.match(r"^((?:v|s|ds|global|buffer|flat|scratch)_\w+)\s*(.*)$", t)
        if m:
            insts.append((re.sub(r"_e(32|64)$", "", m.group(1)), m.group(2)))
    assert len(insts) > 10000, len(insts)  # the whole step: forward pass, contacts, Newton solve, RK4
    return out, insts


def _dest(ops):
    m = re.match(r"^v(\d+)\b", ops.strip())
    return int(m.group(1)) if m else None


def _vregs(text):
    out = set()
    for m in re.finditer(r"\bv(\d+)\b|\bv\[(\d+):(\d+)\]", text):
        if m.group(1) is not None:
            out.add(int(m.group(1)))
        else:
            out.update(range(int(m.group(2)), int(m.group(3)) + 1))
    return out


def test_no_dpp_hazard_in_the_metric_instantiation(isa):
    spec = importlib.util.spec_from_file_location("check_dpp_hazards", os.path.join(ROOT, "tools", "check_dpp_hazards.py"))
    chk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    bad, ndpp = [], 0
    for f in chk.parse_compiler_s(isa[0]):
        b, n = chk.check_stream(f["name"][:60], f["insts"], f["jumps"])
        bad += b
        ndpp += n
    assert ndpp > 1500, ndpp  # the row solver and the quad forward pass: ~2300 DPP instructions
    assert not bad, "\n".join(bad[:20])


def test_row_butterflies_are_not_packed(isa):
    """No packed add fed by an unfused DPP move: `v_mov_b32_dpp a ; v_mov_b32_dpp b ; v_pk_add_f32 x, [a:b]` is the shape the SLP
    vectorizer gives two butterflies side by side — and hardly any unfused DPP move at all."""
    insts = isa[1]
    fed = []
    for i, (mn, ops) in enumerate(insts):
        if mn != "v_pk_add_f32":
            continue
        srcs = _vregs(ops.split(",", 1)[1] if "," in ops else "")
        for pmn, pops in insts[max(0, i - 3):i]:
            if pmn == "v_mov_b32_dpp" and _dest(pops) in srcs:
                fed.append((i, ops))
                break
    n_pk = sum(1 for mn, _ in insts if mn in ("v_pk_add_f32", "v_pk_mul_f32", "v_pk_fma_f32"))
    n_mov_dpp = sum(1 for mn, _ in insts if mn == "v_mov_b32_dpp")
    print(f"v_pk_add/mul/fma_f32 {n_pk}, v_mov_b32_dpp {n_mov_dpp}, packed adds fed by a DPP move {len(fed)}")
    assert not fed, fed[:5]
    assert n_mov_dpp <= 150, n_mov_dpp  # before: 670; now 26 (quad broadcasts of the forward pass)
    assert n_pk <= 640, n_pk             # before: 991; now 613 (module docstring)


def test_pivots_do_not_canonicalise_and_the_kernel_is_shorter(isa):
    insts = isa[1]
    canon = sum(1 for mn, ops in insts if mn == "v_max_f32" and re.match(r"^(v\d+), (v\d+), \2$", ops.strip()))
    print(f"canonicalising v_max_f32 x, x, x: {canon}; instructions: {len(insts)}")
    assert canon <= 44, canon              # before: 58, of which 14 in the elimination's pivots
    assert len(insts) <= 17740, len(insts)  # before: 18 073; now 17 675 (module docstring)
