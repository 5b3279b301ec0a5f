"""Wait states of the row solver's hand-placed DPP blocks, counted on the compiled code of `ant_step_kernel<0, 16, false, 0>` (no GPU
needed; skipped without hipcc).  Compiled the way tests/test_ant_isa_slots.py compiles it, with the flags of csrc/Makefile.

With one wave per SIMD an `s_nop` costs what a `v_fma` costs.  Two places of a Newton iteration spent issue slots
on wait states nothing needed, and must not again:

  * the Gauss-Jordan elimination (rows::solve_rows).  A stretch of the kernel's text from `v_max_f32_dpp ... row_newbcast:0` (the
    first pivot's clamped entry) to the next `v_fmac_f32_dpp ... row_newbcast:11` (the last pivot's elimination), no label or
    branch inside, is one elimination: 81 `v_fmac_f32_dpp` and 14 `v_rcp_f32`.  There are two (qacc_smooth; the Newton iteration).
    Before, each helper opened with `s_nop 1` whatever preceded it: 42 `s_nop` per stretch (27 `s_nop 1`, 15 `s_nop 0`), 207
    instructions.  As one scheduled sequence a pivot keeps one wait state in front of its multiply-adds, the pairs 7 -> 10 and
    10 -> 11 need three more between them, and three are left for the compiler: at most 20.  (Now: 10 and 10, 175 instructions.)
  * the "active set changed" block: `rsum2(p1, p2)` and `rsum2(sn, qn)` behind the matvec `search . M` were two two-chain
    `v_add_f32_dpp` butterflies with an `s_nop 0` between their steps (16 adds, 8 `s_nop`); as one four-chain block
    (rows::rsum4) the links sit far enough apart.  Before: two such butterflies directly behind the matvec; now none."""
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
_BUILT = {}  # path of the compiled text (fixture `text`)


def _make_var(name):
    for line in open(os.path.join(CSRC, "Makefile")):
        m = re.match(rf"^{name}\s*=\s*(.*)$", line)
        if m:
            return m.group(1).split()
    raise AssertionError(f"{name} not set in csrc/Makefile")


@pytest.fixture(scope="module")
def text(tmp_path_factory):
    """the kernel's text as a list of ("label" | "branch" | mnemonic, operands)"""
    out = str(tmp_path_factory.mktemp("isa") / "k_0_16.s")
    base = [f.replace("$(ARCH)", "gfx950") for f in _make_var("BASE")]
    cmd = [HIPCC] + base + _make_var("FAST") + ["-DMZ_ISA_ONLY", "-DMZ_ISA_NB=0", "-DMZ_ISA_G=16", "-DMZ_ISA_PROF=false", "-DMZ_ISA_WPS=0",
                                                "--cuda-device-only", "-S", "-o", out, "ant_kernels.hip"]
    res = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    items = []
    for line in open(out):
        t = line.split(";")[0].strip()
        if re.match(r"^[.\w$]+:", t):
            items.append(("label", t))
            continue
        m = re.match(r"^((?:v|s|ds|global|buffer|flat|scratch)_\w+)\s*(.*)$", t)
        if m:
            mn = re.sub(r"_e(32|64)$", "", m.group(1))
            items.append(("branch" if re.match(r"^s_c?branch|^s_setpc|^s_endpgm", mn) else mn, m.group(2)))
    assert sum(1 for k, _ in items if k not in ("label", "branch")) > 10000
    _BUILT["s"] = out
    return items


def _bcast(ops, p):
    return re.search(rf"row_newbcast:{p}\b", ops) is not None


def test_an_elimination_keeps_one_wait_state_per_pivot(text):
    stretches, i = [], 0
    while i < len(text):
        if text[i][0] == "v_max_f32_dpp" and _bcast(text[i][1], 0):
            j = i + 1
            while j < len(text) and text[j][0] not in ("label", "branch") and not (text[j][0] == "v_fmac_f32_dpp" and _bcast(text[j][1], 11)):
                j += 1
            if j < len(text) and text[j][0] == "v_fmac_f32_dpp":
                stretches.append(text[i:j + 1])
                i = j
        i += 1
    figures = [(len(s), sum(1 for k, _ in s if k == "v_fmac_f32_dpp"), sum(1 for k, _ in s if k == "v_rcp_f32"), sum(1 for k, _ in s if k == "s_nop"))
               for s in stretches]
    print(f"eliminations (instructions, v_fmac_f32_dpp, v_rcp_f32, s_nop): {figures}")
    assert len(stretches) == 2, figures
    for n, fmac, rcp, nop in figures:
        assert fmac == 81 and rcp == 14, figures  # the arithmetic is all there
        assert nop <= 20, figures                 # before: 42


def _two_chain_butterflies_with_wait_states(text, start, window):
    """index of every `add a ; add b ; s_nop ; add a ; add b ; s_nop ; add a ; add b ; s_nop ; add a ; add b` (v_add_f32_dpp, the
    adds of a step with the same DPP control) that begins within `window` instructions after `start`, no label or branch before it"""
    hits = []
    for i in range(start, min(start + window, len(text) - 11)):
        if text[i][0] in ("label", "branch"):
            break
        seq = text[i:i + 11]
        kinds = [k for k, _ in seq]
        if kinds != ["v_add_f32_dpp", "v_add_f32_dpp", "s_nop"] * 3 + ["v_add_f32_dpp", "v_add_f32_dpp"]:
            continue
        ctrl = [re.search(r"(quad_perm:\[[\d,]+\]|row_half_mirror|row_mirror)", o).group(1) for k, o in seq if k == "v_add_f32_dpp"]
        if ctrl == ["quad_perm:[1,0,3,2]"] * 2 + ["quad_perm:[2,3,0,1]"] * 2 + ["row_half_mirror"] * 2 + ["row_mirror"] * 2:
            hits.append(i)
    return hits


def test_no_two_chain_butterfly_behind_the_search_matvec(text):
    """The matvec `search . M` of the changed block: 3 v_mul_f32_dpp + 11 v_fmac_f32_dpp on three accumulators, `row_newbcast:0 .. 13`
    one after the other.  The solve has it three times (cost of the warm start, residual at the start, the changed block); only the
    changed block had row sums of PAIRS right behind it."""
    matvecs = []
    for i in range(len(text) - 14):
        seq = text[i:i + 14]
        if [k for k, _ in seq] == ["v_mul_f32_dpp"] * 3 + ["v_fmac_f32_dpp"] * 11 and all(_bcast(o, p) for p, (_, o) in enumerate(seq)):
            matvecs.append(i)
    assert len(matvecs) >= 3, matvecs
    hits = {m: _two_chain_butterflies_with_wait_states(text, m + 14, 60) for m in matvecs}
    print(f"matvecs at {matvecs}; two-chain butterflies with wait states within 60 instructions behind each: {hits}")
    assert not any(hits.values()), hits  # before: two behind the changed block's
    # ... and the four sums are still there: a matvec followed by four chains of v_add_f32_dpp, round-robin
    four = 0
    for m in matvecs:
        adds = [o for k, o in text[m + 14:m + 14 + 60] if k == "v_add_f32_dpp"]
        four += len(adds) >= 16 and all("quad_perm:[1,0,3,2]" in o for o in adds[:4]) and all("row_mirror" in o for o in adds[12:16])
    assert four >= 1, "no four-chain butterfly behind any matvec"


def test_the_strings_keep_the_rules_the_compiler_cannot_keep_for_them(text):
    """solve_rows has a v_rcp_f32, its use, a v_cmp and the selects that read its mask inside one string: a transcendental's result
    is not read in the next issue slot, a VALU-written SGPR not in the next two (tools/check_dpp_hazards.py check_asm_valu_hazards);
    the DPP rule itself is checked by tests/test_ant_isa_slots.py and, on every instantiation, tests/test_capi_and_emu.py."""
    spec = importlib.util.spec_from_file_location("check_dpp_hazards", os.path.join(ROOT, "tools", "check_dpp_hazards.py"))
    chk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    bad, nrcp = [], 0
    for f in chk.parse_compiler_s(_BUILT["s"]):
        bad += chk.check_asm_valu_hazards(f["name"][:60], f["insts"])
        nrcp += sum(1 for _, mn, _ in f["insts"] if mn == "v_rcp_f32")
    assert nrcp >= 28, nrcp
    assert not bad, "\n".join(bad[:20])
