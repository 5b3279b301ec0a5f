"""Diverged states through the kernel source under host sanitizers (no GPU).

An env whose state goes non-finite or huge (profiles/r02/README.md: they do, in soak runs) must still end its step: the kernels
take loop bounds — the maze cells under a geom — from state coordinates, and a float -> int conversion of NaN / Inf / 1e30 is
undefined in C++, INT_MIN on x86 and saturating on the device, where `for (i = i0; i <= i1; i++)` with i1 == INT_MAX never ends.
csrc/mz_maze.h `mz_cell` clamps before it converts; this module holds it there:

  * tests/emu/diverged_main.cpp — a stand-alone program (own main; nothing is preloaded, nothing is loaded into Python) built with
    -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all from the same kernel headers as libantemu.so —
    steps every engine from qpos0 with one state entry at a time set to NaN, +-Inf, +-1e12, +-1e30, +-FLT_MAX, 3 steps each, after
    200 healthy random-action steps as the control.  Any sanitizer report, a diverged result without MZ_STATUS_BAD_STATE (where the
    emulation entry computes the bit) or a loop that does not end fails the test;
  * mz_cell itself on the edge values;
  * the kernel sources hold no raw `(int)floor(...)` outside the helper but the documented device-path sites."""
import math
import os
import re
import subprocess
import time

import pytest

import mujoco_maze_amd as mm
from mujoco_maze_amd import maze_task as T
from mujoco_maze_amd import model
from tests import user_robots

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "mujoco_maze_amd", "csrc")
PROGRAM = os.path.join(EMU, "diverged_main")
MAX_GRID = 12  # MZ_MAX_GRID of include/mazestep.h

REGISTERED = ["AntUMaze-v0", "AntPush-v0", "AntFall-v0", "AntSmallBilliard-v0", "AntPushMaze-v0", "PointUMaze-v0", "PointPush-v0",
              "PointBilliard-v0", "PointFall-v0", "SwimmerUMaze-v0", "SwimmerPush-v0", "ReacherUMaze-v0"]


def _registered(env_id, **kw):
    spec = mm.REGISTRY[env_id]
    scale = spec.kwargs["maze_size_scaling"]
    return model.compile_model(spec.kwargs["model_cls"].ROBOT, spec.kwargs["maze_task"](scale), scale, **kw)


MODELS = {i: (lambda i=i: _registered(i)) for i in REGISTERED}
MODELS["PointUMaze-v0.general"] = lambda: _registered("PointUMaze-v0", engine="general")
MODELS["biped_ant"] = lambda: model.compile_model("generic", T.DistRewardPush(4.0), 4.0, robot_xml=user_robots.BIPED_ANT, frame_skip=5,
                                                  reset_qvel="normal")
# engine and state entries the program must report per model: the matrix of the module docstring, spelled out
EXPECT = {
    "AntUMaze-v0": ("ant", "x y z quat hinge"), "AntPush-v0": ("ant", "x y z quat hinge slide"), "AntFall-v0": ("ant", "x y z quat hinge slide"),
    "AntSmallBilliard-v0": ("ant", "x y z quat hinge ball"), "AntPushMaze-v0": ("ant", "x y z quat hinge slide"),
    "PointUMaze-v0": ("point", "x y hinge"), "PointPush-v0": ("point", "x y hinge slide"), "PointBilliard-v0": ("point", "x y hinge slide"),
    "PointFall-v0": ("point", "x y hinge slide"), "SwimmerUMaze-v0": ("swimmer", "x y hinge"), "SwimmerPush-v0": ("swimmer", "x y hinge slide"),
    "ReacherUMaze-v0": ("swimmer", "x y hinge"), "PointUMaze-v0.general": ("general", "x y hinge"),
    "biped_ant": ("general", "x y z quat hinge slide"),
}


@pytest.fixture(scope="module")
def program():
    subprocess.check_call(["make", "-s", "-C", EMU, "diverged_main"])
    return PROGRAM


def test_diverged_states_end_their_step_without_a_sanitizer_report(program, tmp_path):
    paths = []
    for name, make in MODELS.items():
        cm = make()
        p = tmp_path / (name + ".bin")
        p.write_bytes(bytes(cm.c))
        paths.append(str(p))
    t0 = time.perf_counter()
    # the limit exists only to catch a loop that does not end
    res = subprocess.run([program] + paths, capture_output=True, text=True, timeout=120)
    print(res.stdout)
    print(f"run time {time.perf_counter() - t0:.1f} s")
    assert res.returncode == 0, (res.returncode, res.stdout[-2000:], res.stderr[-6000:])
    lines = {os.path.basename(l.split(":")[0])[:-4]: l for l in res.stdout.splitlines() if ".bin:" in l}
    assert sorted(lines) == sorted(MODELS)
    for name, (engine, entries) in EXPECT.items():
        want = entries.split()
        want += ["v" + e for e in want]
        assert f"engine {engine}," in lines[name], lines[name]
        assert lines[name].endswith("entries: " + " ".join(want)), lines[name]
        assert f"{9 * len(want)} cases x 3 steps" in lines[name], lines[name]
        # the matrix reaches what it is for: results that really are diverged (and, off the Point, carried the status bit)
        assert int(re.search(r"\((\d+) diverged results\)", lines[name]).group(1)) >= len(want), lines[name]


def test_program_refuses_a_file_that_is_no_model(program, tmp_path):
    cm = _registered("PointUMaze-v0")
    short = tmp_path / "short.bin"
    short.write_bytes(bytes(cm.c)[:-8])
    res = subprocess.run([program, str(short)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 2 and "bytes, mz_model has" in res.stderr, (res.returncode, res.stderr)
    raw = bytearray(bytes(cm.c))
    raw[0:4] = (cm.c.abi_version + 1).to_bytes(4, "little")
    other = tmp_path / "abi.bin"
    other.write_bytes(bytes(raw))
    res = subprocess.run([program, str(other)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 2 and "abi_version" in res.stderr, (res.returncode, res.stderr)


CELL_INPUTS = ["nan", "inf", "-inf", "1e300", "-1e300", "2147483648", "-2147483648", "2147483647", "2147483649", "-2147483647", "-2147483649",
               "-2.5", "-0.5", "0", "11.49", "12", "14"]


def test_cell_helper_on_the_edges(program):
    res = subprocess.run([program, "--cells"] + CELL_INPUTS, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, (res.returncode, res.stderr[-3000:])
    rows = [l.split() for l in res.stdout.splitlines()]
    assert [r[0] for r in rows] == CELL_INPUTS
    for text, as_double, as_float in rows:
        v = float(text)
        if math.isnan(v):
            want = -2
        else:
            want = int(min(max(math.floor(v) if math.isfinite(v) else v, -2.0), MAX_GRID + 1.0))
        assert int(as_double) == want, (text, as_double, want)
        assert int(as_float) == want, (text, as_float, want)  # (every input here floors to the same cell in fp32)
        assert -2 <= int(as_double) <= MAX_GRID + 1
        if 0 <= v < MAX_GRID:
            assert int(as_double) == int(math.floor(v)) == int(as_float)
    got = {r[0]: int(r[1]) for r in rows}
    assert got["nan"] == -2 and got["-inf"] == -2 and got["inf"] == MAX_GRID + 1
    assert (got["-2.5"], got["-0.5"], got["0"], got["11.49"], got["12"], got["14"]) == (-2, -1, 0, 11, 12, 13)


# the device-path sites that keep the raw conversion (each carries a comment saying why the device form is safe there; the host
# form beside it is defined): {file: count}.  Both belong to the plain ant's benchmark kernel, whose instruction stream stays:
# the row forward pass (two lines, four conversions) and the robot-geom wall cells of geom_contacts, plain-ant device branch only
# (the kernel's staging-overflow path runs that enumerator; two lines, four conversions)
RAW_CONVERSIONS_ALLOWED = {"ant_forward_rows.h": 4, "ant_dyn.h": 4}


def test_no_raw_cell_conversion_outside_the_helper():
    pat = re.compile(r"\(int\)\s*(?:floor|floorf|rint|rintf)\s*\(")
    found = {}
    files = sorted(f for f in os.listdir(CSRC) if f.endswith((".h", ".hip")))
    assert "mz_maze.h" in files and "ant_kernels.hip" in files and len(files) >= 20
    for f in files:
        with open(os.path.join(CSRC, f), errors="replace") as fh:
            n = len(pat.findall(fh.read()))
        if n:
            found[f] = n
    assert found == RAW_CONVERSIONS_ALLOWED, found
    with open(os.path.join(CSRC, "mz_maze.h")) as fh:
        text = fh.read()
    assert "MZ_HD int mz_cell(double f)" in text and "MZ_HD int mz_cell(float f)" in text
    uses = sum(len(re.findall(r"\bmz_cell\(", open(os.path.join(CSRC, f), errors="replace").read())) for f in files)
    assert uses >= 30, uses  # the sites that used to convert raw
