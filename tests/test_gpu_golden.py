"""The reference's own fixtures through the HIP kernels (C-ABI debug entries), bit for bit.

north_star: "bit-exact for termination flags and goal indices"; SURVEY §8c lists the fixtures.  Two places of the path
reproduce float64 DECISIONS of the reference: the task predicates (maze_task.py:43-47,77-81,403-407) and the Point's
manual wall rule (maze_env_utils.py:96-123,186-206; maze_env.py:457-464).  Both run here on the GPU build on ALL golden
vectors — `mz_debug_task_eval` / `mz_debug_detect` launch the very device functions the step kernels inline
(task_eval_dev of csrc/mz_task.h as compiled into the handle's translation unit; point_detect / point_bounce of csrc/point_dyn.h).
"""
import json
import os

import numpy as np
import pytest

import mujoco_maze_amd as mm
from mujoco_maze_amd import maze_task as T

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")
DET = np.load(os.path.join(G, "detect.npz"))
REW = np.load(os.path.join(G, "reward.npz"))
REW_F32 = np.load(os.path.join(G, "reward_f32.npz"))  # the reference's verdicts on float64(fp32(observations)): make_golden_r04.py
REW_META = json.load(open(os.path.join(G, "reward_meta.json")))
KAT = json.load(open(os.path.join(G, "line_kat.json")))


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


@pytest.mark.parametrize("env_id", ["PointUMaze-v0", "Point4Rooms-v0", "PointPush-v0", "PointCorridor-v0", "PointTRoom-v0", "PointBilliard-v0"])
def test_all_golden_moves_through_the_hip_detector(torch, env_id):
    """3000 moves per maze (18 000 in all): zero-length, 1e-9 (below the 1e-8 threshold), ending exactly on a wall line,
    single bounces, give-ups, collinear moves.  hit / give-up flags array_equal; collision point and final position equal
    in float64."""
    tag = env_id.replace("-", "_")
    old, new = DET[f"{tag}__old"], DET[f"{tag}__new"]
    hit, point, final = DET[f"{tag}__hit"].astype(bool), DET[f"{tag}__point"], DET[f"{tag}__final"]
    gave_up, valid = DET[f"{tag}__gave_up"].astype(bool), DET[f"{tag}__valid"].astype(bool)
    env = mm.make(env_id, num_envs=4, force_vec=True)
    h, pt, fin = [x.cpu().numpy() for x in env.debug_detect(old, new)]
    env.close()
    assert np.array_equal(h[~valid], np.full((~valid).sum(), -1))  # the reference raised ZeroDivisionError on these
    v = valid
    assert np.array_equal(h[v] > 0, hit[v])
    assert np.array_equal(fin[v], final[v])
    assert np.array_equal(pt[v & hit], point[v & hit])
    # give-up = the position was restored to the old one (maze_env.py:461-462)
    assert np.array_equal(h[v & hit] == 2, gave_up[v & hit])
    assert hit[v].sum() > 200 and gave_up[v].sum() > 5
    assert np.array_equal(h[:10], np.zeros(10, np.int32))  # rows 0-9: zero-length and 1e-9 moves


def test_hand_picked_moves_match_the_golden_pinned_host_mirror(torch):
    """Moves chosen to sit on the detector's edges — ending exactly on a wall line, starting on one, running along one
    (collinear), crossing a corner where two wall segments meet, a 1e-8 move (the `<=` threshold itself) — against the
    Python mirror of CollisionDetector (mujoco_maze_amd/maze_env_utils.py, itself bit-exact on detect.npz and on the
    known answers of the reference's tests/test_intersect.py)."""
    from mujoco_maze_amd import maze_env_utils as U
    from mujoco_maze_amd import model as M

    env = mm.make("PointUMaze-v0", num_envs=4, force_vec=True)
    w = env.model.world
    det = U.CollisionDetector(env._task.create_maze(), 4.0, w.torso_x, w.torso_y, 0.4)
    old = np.array([[0.0, 0.0], [0.0, 0.0], [0.0, 0.0], [-1.6, 0.0], [0.0, 0.0], [0.0, 0.0], [1.0, 1.0], [5.0, 1.0], [0.3, -0.2]])
    new = np.array([[-3.0, 0.0], [0.0, -3.0], [-1.6, 0.0], [-1.0, 0.5], [-1.6, -1.6], [-2.0, -2.0], [1.0 + 1e-8, 1.0], [5.0, 3.0], [0.5, 0.25]])
    h, pt, fin = [x.cpu().numpy() for x in env.debug_detect(old, new)]
    env.close()
    for k in range(len(old)):
        try:
            col = det.detect(old[k], new[k])
        except ZeroDivisionError:
            assert h[k] == -1, k
            continue
        assert (h[k] > 0) == (col is not None), k
        if col is None:
            assert np.array_equal(fin[k], new[k]), k
            continue
        assert np.array_equal(pt[k], col.point), k
        pos = col.point + 0.8 * col.rest()
        again = det.detect(old[k], pos)
        assert np.array_equal(fin[k], old[k] if again is not None else pos) and (h[k] == 2) == (again is not None), k
    assert (h > 0).sum() >= 4 and (h == 0).sum() >= 2


def _robots_for(cls, scale):
    return [r for r in ("point", "ant", "swimmer") if getattr(cls.MAZE_SIZE_SCALING, r) == scale]


@pytest.mark.parametrize("tag", sorted(REW_META))
def test_all_golden_observations_through_the_hip_task_eval(torch, tag):
    """All 400 golden observations of every task (50 tasks x the scales they are registered with), rounded to fp32 — what
    the kernels observe — through the device predicate of EVERY robot family the task is registered for (the Ant kernels are
    built with relaxed floating-point flags, the Point / Swimmer ones strictly).  Expected values: what the REFERENCE's own
    `task.reward()` / `task.termination()` / `MazeGoal.neighbor()` returned on float64(those fp32 observations) —
    tests/golden/reward_f32.npz, written by make_golden_r04.py from the imported reference (maze_task.py:43-47,77-81,110-111,
    403-407,592-604,646-658); this repository's Python mirror is not in the loop.  Rows 390 / 391 sit exactly on the
    threshold circle of the agent / object slot."""
    from mujoco_maze_amd import model as M
    from mujoco_maze_amd.agent_model import ROBOT_CLASSES

    meta = REW_META[tag]
    cls, scale = getattr(T, meta["task"]), meta["scale"]
    task = cls(scale)
    obs32 = REW[f"{tag}__obs"].astype(np.float32)
    ref_r64 = REW_F32[f"{tag}__reward"]
    exp_r = ref_r64.astype(np.float32)
    exp_t = REW_F32[f"{tag}__term"].astype(bool)
    exp_g = REW_F32[f"{tag}__goal"]
    desc = T.device_reward_descriptor(task)
    ran = 0
    for robot in _robots_for(cls, scale):
        from mujoco_maze_amd.maze_env import VecMazeEnv

        try:
            env = VecMazeEnv(ROBOT_CLASSES[robot], cls, num_envs=4, maze_size_scaling=scale)
        except NotImplementedError:
            continue
        wide = np.zeros((len(obs32), env.obs_dim), np.float32)
        k = min(env.obs_dim, obs32.shape[1])
        wide[:, :k] = obs32[:, :k]
        rew, done, gi = [x.cpu().numpy() for x in env.debug_task_eval(wide)]
        env.close()
        assert np.array_equal(done.astype(bool), exp_t), (tag, robot)
        assert np.array_equal(gi, exp_g), (tag, robot)
        assert np.array_equal(rew, exp_r) or np.max(np.abs(rew - exp_r)) <= 2e-7 * np.max(np.abs(exp_r)), (tag, robot)
        if desc[0] != T.K_NEG_DIST:
            assert np.array_equal(rew, exp_r), (tag, robot)  # goal rewards / penalties are constants: exact
        ran += 1
    if ran == 0:
        pytest.skip("maze not on the device path yet")
    if task.goals:
        assert exp_t.sum() >= 5  # (rows 390 / 391 may fall on either side once rounded to fp32: that is the point)


def test_threshold_boundary_in_float32(torch):
    """The case VERDICT r01 describes: fp32(0.6) = 0.60000002 > 0.6.  An fp32 observation at distance exactly fp32(0.6) from
    the goal is OUTSIDE for the reference (`np.linalg.norm(..) <= 0.6`, maze_task.py:43-44) — an fp32 predicate with an fp32
    threshold would call it inside.  Neighbouring fp32 values on both sides are checked as well."""
    env = mm.make("AntUMaze-v0", num_envs=4, force_vec=True)  # goal (0, 16), threshold 0.6
    penv = mm.make("PointUMaze-v0", num_envs=4, force_vec=True)  # goal (0, 8)
    thr32 = np.float32(0.6)
    xs = np.array([np.nextafter(thr32, np.float32(0)), thr32, np.nextafter(thr32, np.float32(1))], np.float32)
    for e, gy in ((env, 16.0), (penv, 8.0)):
        obs = np.zeros((3, e.obs_dim), np.float32)
        obs[:, 0] = xs
        obs[:, 1] = gy
        rew, done, gi = [x.cpu().numpy() for x in e.debug_task_eval(obs)]
        expect = np.array([float(x) <= 0.6 for x in xs])  # float64 comparison of the fp32 values
        assert expect.tolist() == [True, False, False]
        assert np.array_equal(done.astype(bool), expect) and np.array_equal(gi, np.where(expect, 0, -1))
        e.close()
