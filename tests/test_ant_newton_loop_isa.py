"""Issue slots of ONE Newton iteration of the plain ant's row solver, counted on the compiled code between the two marks that
bracket the loop (`; newton loop begin` / `; newton loop end`, csrc/ant_newton_rows.h ant_solve_rows_core).  No GPU needed; skipped
without hipcc.  The kernel is `ant_step_kernel<0, 16, false, 0>`, compiled as tests/test_ant_isa_slots.py compiles it, and
tools/newton_slots.py classifies what lies between the marks and splits it by the path a wave takes (DESIGN.md 3.1 "Newton-loop
slots", profiles/newton_slots/inventory.md).

With one wave per SIMD an instruction of the loop body is paid 57 (mean wave) to 68 (slowest wave) times per step, so what the loop
spends on anything but float arithmetic must not grow back.  Figures, instructions of the region / of them not float arithmetic:

                                   parent         this change      bound (reached + 0.3 %, rounded up)
    whole region                   1822 / 457     1772 / 408       1778 / 410
    one iteration, <= 2 slots       547 / 222      521 / 197        523 / 198
    one iteration, 3 slots          628 / 235      598 / 206        600 / 207
    one iteration, 4 slots          711 / 250      678 / 218        681 / 219
(an iteration without a line search; the region also holds the line search, 181 -> 165, and the slots from 4 up, 930 -> 929.)

The float arithmetic of the loop is the parent's, mnemonic by mnemonic, but for what two items replace:
  * the limit rows' curvature on the diagonal: eight `v_cndmask` + `v_add_f32` became eight `v_fmac_f32` (5 -> 13, `v_add_f32` -8);
  * the active-set vote without its exec-mask region: the compiler pairs two of its adds, `v_add_f32` -2, `v_pk_add_f32` 16 -> 17.  The
    two spellings are the same additions, so what is held is `v_add_f32 + 2 v_pk_add_f32` = 33 + 2 * 16 - 8 = 57."""
import importlib.util
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

# float-arithmetic mnemonics between the marks in the parent of this change
PARENT_FLOAT = {"v_add_f32": 33, "v_add_f32_dpp": 224, "v_fma_f32": 14, "v_fmac_f32": 5, "v_fmac_f32_dpp": 860, "v_max_f32_dpp": 14,
                "v_mul_f32": 103, "v_mul_f32_dpp": 67, "v_pk_add_f32": 16, "v_pk_fma_f32": 2, "v_pk_mul_f32": 1, "v_rcp_f32": 15,
                "v_sqrt_f32": 2, "v_sub_f32": 9}
REPLACED = ("v_add_f32", "v_pk_add_f32", "v_fmac_f32")
REACHED = {"region": (1772, 408), "<= 2 slots": (521, 197), "3 slots": (598, 206), "4 slots": (678, 218)}


def _bound(x):
    return math.ceil(x * 1.003)


def _make_var(name):
    for line in open(os.path.join(CSRC, "Makefile")):
        m = re.match(rf"^{name}\s*=\s*(.*)$", line)
        if m:
            return m.group(1).split()
    raise AssertionError(f"{name} not set in csrc/Makefile")


@pytest.fixture(scope="module")
def slots():
    spec = importlib.util.spec_from_file_location("newton_slots", os.path.join(ROOT, "tools", "newton_slots.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def inventory(tmp_path_factory, slots):
    out = str(tmp_path_factory.mktemp("isa") / "k_0_16.s")
    base = [f.replace("$(ARCH)", "gfx950") for f in _make_var("BASE")]
    cmd = [HIPCC] + base + _make_var("FAST") + ["-DMZ_ISA_ONLY", "-DMZ_ISA_NB=0", "-DMZ_ISA_G=16", "-DMZ_ISA_PROF=false", "-DMZ_ISA_WPS=0",
                                                "--cuda-device-only", "-S", "-o", out, "ant_kernels.hip"]
    res = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    return slots.inventory(out)  # (instructions, their tags, class counts per part, float mnemonics)


def test_the_loop_is_found_and_split(inventory):
    insts, tag, table, mnem = inventory
    sizes = {k: sum(v.values()) for k, v in table.items()}
    print(sizes)
    # two slot chains (the fold into H, J . search): slot 0 holds the copy of M on top, the others one fold (52 multiply-adds) and
    # one butterfly (15) each; the elimination (81 + 14 multiply-adds, 14 reciprocals) is common
    assert sizes["slot 1"] == sizes["slot 2"] and 70 <= sizes["slot 1"] <= 90, sizes
    assert sizes["slot 0"] > sizes["slot 1"] and sizes["slots 4+"] > 800 and sizes["line search"] > 100, sizes
    assert table["common"]["float arithmetic"] >= 81 + 14 + 14 + 14, table["common"]
    assert sum(table[k]["s_waitcnt"] + table[k]["memory"] + table[k]["v_accvgpr"] for k in table) == 0  # the loop touches no memory, no accumulation register


def test_instructions_of_one_iteration(inventory, slots):
    insts, tag, table, mnem = inventory
    got = {"region": (len(insts), len(insts) - sum(mnem.values()))}
    for name, c in slots.paths(table).items():
        got[name] = (sum(c.values()), sum(c.values()) - c["float arithmetic"])
    print(got)
    for name, (n, rest) in REACHED.items():
        assert got[name][0] <= _bound(n), (name, got[name], _bound(n))
        assert got[name][1] <= _bound(rest), (name, got[name], _bound(rest))


def test_float_arithmetic_is_the_parents(inventory):
    insts, tag, table, mnem = inventory
    print(dict(sorted(mnem.items())))
    for mn in sorted(set(PARENT_FLOAT) | set(mnem)):
        if mn not in REPLACED:
            assert mnem.get(mn, 0) == PARENT_FLOAT.get(mn, 0), (mn, mnem.get(mn, 0), PARENT_FLOAT.get(mn, 0))
    assert mnem["v_fmac_f32"] == PARENT_FLOAT["v_fmac_f32"] + 8, mnem["v_fmac_f32"]  # the eight hinge positions' limit curvature
    adds = mnem["v_add_f32"] + 2 * mnem["v_pk_add_f32"]
    assert adds == PARENT_FLOAT["v_add_f32"] + 2 * PARENT_FLOAT["v_pk_add_f32"] - 8, (mnem["v_add_f32"], mnem["v_pk_add_f32"])
