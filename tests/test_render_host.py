"""The device renderer's drawing code (csrc/mz_render.h), built for the host (tests/render_host), against render.render_top_down:
every pixel equal.  Both sides evaluate the same float64 expressions with the same libm, so nothing may differ here; on the device
only the state-dependent sin / cos / atan2 may (tests/test_gpu_render.py)."""
import copy
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mujoco_maze_amd as mm
from mujoco_maze_amd import maze_task as T
from mujoco_maze_amd import model, render
from mujoco_maze_amd.model import MzModel
from tests.test_general_engine import SpinCellMaze, SpinUMaze
from tests.test_mjcf import chain_swimmer_xml
from tests.test_top_down_view import HalfBlockMaze

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "render_host")
SHAPES = [(64, 64), (97, 31), (600, 480)]
IDS = ["AntUMaze-v0", "Ant4Rooms-v0", "AntPush-v0", "AntMultiPush-v0", "AntSmallBilliard-v0", "AntFall-v0", "PointUMaze-v0",
       "PointBilliard-v0", "PointMultiPush-v0", "Point4Rooms-v2", "SwimmerUMaze-v0", "ReacherUMaze-v0"]
CUSTOM = {
    "chain5": lambda: model.compile_model("swimmer", T.DistRewardUMaze(4.0), 4.0, robot_xml=chain_swimmer_xml(5)),
    "HalfBlockMaze/ant": lambda: model.compile_model("ant", HalfBlockMaze(4.0), 4.0),
    "HalfBlockMaze/point": lambda: model.compile_model("point", HalfBlockMaze(4.0), 4.0),
    "SpinCellMaze/point": lambda: model.compile_model("point", SpinCellMaze(4.0), 4.0),
    "SpinUMaze/ant": lambda: model.compile_model("ant", SpinUMaze(8.0), 8.0),
}

_lib = None


def _load():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-s", "-C", HERE])
        lib = C.CDLL(os.path.join(HERE, "librenderhost.so"))
        vp, i32 = C.c_void_p, C.c_int
        lib.mzr_host_render.restype = i32
        lib.mzr_host_render.argtypes = [C.POINTER(MzModel), vp, vp, i32, i32, vp, vp, i32, i32, vp, C.c_char_p, i32]
        _lib = lib
    return _lib


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def host_render(cm, qpos32, shape, env_goals=None):
    """mz_render.h on the CPU: uint8 [n, H, W, 3] for the float32 qpos rows [n, nq]."""
    lib = _load()
    q = np.ascontiguousarray(np.atleast_2d(qpos32), np.float32)
    n = q.shape[0]
    rgb, size = render.goal_style(cm)
    rgb, size = np.ascontiguousarray(rgb, np.uint8), np.ascontiguousarray(size, np.float64)
    g = None if env_goals is None else np.ascontiguousarray(env_goals, np.float64)
    out = np.zeros((n, shape[1], shape[0], 3), np.uint8)
    err = C.create_string_buffer(200)
    rc = lib.mzr_host_render(C.byref(cm.c), _vp(q), _vp(g), n, len(size), _vp(rgb), _vp(size), shape[0], shape[1], _vp(out), err, 200)
    assert rc == 0, err.value.decode()
    return out


def compiled(env_id):
    if env_id in CUSTOM:
        return CUSTOM[env_id]()
    spec = mm.REGISTRY[env_id]
    kw = spec.kwargs
    scale = kw["maze_size_scaling"]
    return model.compile_model(kw["model_cls"].ROBOT, kw["maze_task"](scale), scale)


def perturbed_states(cm, k, seed):
    """qpos0 and k - 1 random perturbations of it (robot moved by up to a cell, every angle and slide moved), as float32."""
    m = cm.c
    rng = np.random.default_rng(seed)
    q0 = np.array([m.qpos0[i] for i in range(m.nq)])
    rows = [q0]
    for _ in range(k - 1):
        q = q0 + rng.normal(0.0, 0.4, m.nq)
        q[:2] += rng.uniform(-0.6, 0.6, 2) * cm.world.scale
        rows.append(q)
    return np.array(rows).astype(np.float32)


def render_with_goals(cm, pos, qpos, shape):
    """render_top_down with the task's goals drawn at pos [ngoal, 2+] (the yardstick for per-env goal rows)."""
    goals = cm.task.goals
    moved = []
    for g, p in zip(goals, pos):
        g2 = copy.copy(g)
        g2.pos = np.array(g.pos, np.float64).copy()
        g2.pos[:2] = p[:2]
        moved.append(g2)
    cm.task.goals = moved
    try:
        return render.render_top_down(cm, qpos, shape)
    finally:
        cm.task.goals = goals


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("env_id", IDS + sorted(CUSTOM))
def test_host_build_equals_render_top_down(env_id, shape):
    cm = compiled(env_id)
    qs = perturbed_states(cm, 4, hash((env_id, shape)) % 2**31)
    got = host_render(cm, qs, shape)
    for i, q in enumerate(qs):
        want = render.render_top_down(cm, q.astype(np.float64), shape)
        assert np.array_equal(got[i], want), f"{env_id} {shape} state {i}: {int((got[i] != want).any(-1).sum())} pixels differ"


def test_every_primitive_kind_is_on_the_canvas():
    """The comparison above would pass vacuously on an image of floor: the cases draw walls, chasms, blocks, balls, goals and robots."""
    seen = set()
    for env_id in ("AntFall-v0", "PointBilliard-v0", "AntPush-v0", "ReacherUMaze-v0"):
        cm = compiled(env_id)
        img = host_render(cm, perturbed_states(cm, 1, 0), (300, 240))[0]
        seen |= {tuple(c) for c in img.reshape(-1, 3)}
    for c in (render.FLOOR, render.WALL, render.CHASM, render.BLOCK, render.BALL, render.ROBOT, render.DARK):
        assert c in seen


@pytest.mark.parametrize("env_id", ["Point4Rooms-v2", "AntUMaze-v0", "PointBilliard-v0"])
def test_per_env_goal_rows(env_id):
    """With a per-env goal table (mz_bind_env_goals) each image shows its env's own goals."""
    cm = compiled(env_id)
    ng = cm.c.ngoal
    rng = np.random.default_rng(5)
    qs = perturbed_states(cm, 3, 1)
    rows = np.zeros((3, 8, 3))
    rows[:, :ng, :2] = rng.uniform(-1.0, 3.0, (3, ng, 2)) * cm.world.scale
    for shape in SHAPES:
        got = host_render(cm, qs, shape, env_goals=rows)
        for i in range(3):
            want = render_with_goals(cm, rows[i, :ng], qs[i].astype(np.float64), shape)
            assert np.array_equal(got[i], want), (env_id, shape, i)
        assert not np.array_equal(got[0], host_render(cm, qs[:1], shape)[0])  # the rows moved the goals


@pytest.mark.parametrize("env_id", ["Point4Rooms-v2", "PointBilliard-v0", "AntSmallBilliard-v0", "AntUMaze-v0"])
def test_goal_style_is_what_render_top_down_draws(env_id, monkeypatch):
    """render.goal_style: Python's round() of the task's colour and custom_size (else scale * 0.1), as the goal markers are drawn."""
    cm = compiled(env_id)
    calls = []
    orig_disc, orig_ring = render._Canvas.disc, render._Canvas.ring
    monkeypatch.setattr(render._Canvas, "disc", lambda self, cx, cy, r, colour: (calls.append(("disc", r, tuple(colour))), orig_disc(self, cx, cy, r, colour)))
    monkeypatch.setattr(render._Canvas, "ring", lambda self, cx, cy, r, colour, width=0.06: (calls.append(("ring", r, tuple(colour))), orig_ring(self, cx, cy, r, colour, width)))
    m = cm.c
    render.render_top_down(cm, np.array([m.qpos0[i] for i in range(m.nq)]), (64, 64))
    rgb, size = render.goal_style(cm)
    assert rgb.dtype == np.uint8 and rgb.shape == (len(cm.task.goals), 3) and size.shape == (len(cm.task.goals),)
    for k, g in enumerate(cm.task.goals):
        want_rgb = tuple(int(round(255 * v)) for v in (g.rgb.red, g.rgb.green, g.rgb.blue))
        want_size = g.custom_size if g.custom_size is not None else 0.1 * cm.world.scale
        assert tuple(int(v) for v in rgb[k]) == want_rgb and size[k] == want_size
        assert calls[2 * k] == ("disc", want_size, want_rgb) and calls[2 * k + 1] == ("ring", g.threshold, want_rgb)
    if env_id == "Point4Rooms-v2":
        assert len({tuple(c) for c in rgb}) == 2 and len(rgb) == 3
    if "Billiard" in env_id:
        assert any(g.custom_size is not None for g in cm.task.goals)


def test_user_robot_is_refused():
    from tests.user_robots import BIPED_ANT

    cm = model.compile_model("generic", T.DistRewardUMaze(4.0), 4.0, robot_xml=BIPED_ANT)
    with pytest.raises(AssertionError, match="user robot"):
        host_render(cm, np.zeros((1, cm.c.nq), np.float32), (64, 64))
