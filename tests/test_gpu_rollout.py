"""VecMazeEnv.rollout / mz_rollout against K step() calls on a twin env: same id, num_envs, seed, reset and injected states.

The fused kernels run the step kernels' device functions on the same fp32 states, so the bar is bit equality, not a tolerance:
float tensors are compared by their bit patterns (`_same`), which is torch.equal except that a NaN equals the same NaN — the
swimmers' movable block diverges by design and its rows carry non-finite values on both sides."""
import ctypes as C

import numpy as np
import pytest

import mujoco_maze_amd as mm
from mujoco_maze_amd import _capi
from tests.test_custom_task import FarGoalCross, RandomGoalCross
from tests.test_top_down_view import view_task

pytestmark = pytest.mark.gpu
MZ_ERR_ARG = -1


def _same(a, b):
    import torch

    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.float32:
        return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    return torch.equal(a, b)


def _actions(env, K, seed, drive=False):
    """[K, N, nu] uniform in the control range; `drive` (Point family): full speed ahead with a random turn, which runs the robots
    into the walls within a few steps."""
    import torch

    g = torch.Generator(device=env.device).manual_seed(seed)
    lo, hi = torch.as_tensor(env.action_space.low, device=env.device), torch.as_tensor(env.action_space.high, device=env.device)
    a = lo + (hi - lo) * torch.rand((K, env.num_envs, env.nu), device=env.device, generator=g)
    if drive:
        a[:, :, 0] = hi[0]
    return a.contiguous()


def _near_goal(env, obs0):
    """Point family: every fourth env one step in front of the first goal, heading towards it.  The Billiard tasks judge the object
    ball, not the robot (maze_task.py: obs[3:6]): there the ball of those envs — on its spawn position obs0[:, 3:5] after the reset,
    slides qpos[3:5] at zero — is put 0.2 beside the goal, inside the threshold."""
    import torch

    qpos, qvel, warm, t = env.get_state()
    gp = env.model.c.goal_pos[0]
    sel = torch.arange(env.num_envs, device=env.device) % 4 == 0
    if env.model.c.nball:
        qpos[sel, 3], qpos[sel, 4] = float(gp[0]) + 0.2 - obs0[sel, 3], float(gp[1]) - obs0[sel, 4]
    else:
        qpos[sel, 0], qpos[sel, 1], qpos[sel, 2] = float(gp[0]) + 0.9, float(gp[1]), float(np.pi)
    env.set_state(qpos=qpos)


def _twin_check(make, K, seed=11, point=False, expect_done=False, status=True, after_reset=None):
    """`after_reset(env)`: called on both envs behind the reset (state injection of other robots than the Point)"""
    import torch

    ea, eb = make(), make()
    try:
        oa, ob = ea.reset(seed=seed), eb.reset(seed=seed)
        assert _same(oa, ob)
        if point:
            _near_goal(ea, oa); _near_goal(eb, ob)
        if after_reset:
            after_reset(ea); after_reset(eb)
        acts = _actions(ea, K, seed + 1, drive=point)
        rows = {k: [] for k in ("obs", "reward", "done", "goal", "pos", "fwd", "ctrl")}
        for k in range(K):
            obs, rew, done, info = ea.step(acts[k])
            for key, v in zip(rows, (obs, rew, done, info["goal_index"], info["position"], info["reward_forward"], info["reward_ctrl"])):
                rows[key].append(v.clone())
        want = {k: torch.stack(v) for k, v in rows.items()}
        obs_b, rew_b, done_b, info_b = eb.rollout(acts, return_obs=True)
        torch.cuda.synchronize()
        assert tuple(rew_b.shape) == (K, ea.num_envs) and done_b.dtype == torch.uint8
        assert _same(rew_b, want["reward"])
        assert _same(done_b, want["done"])
        assert _same(info_b["goal_index"], want["goal"])
        assert _same(info_b["observations"], want["obs"])
        assert _same(info_b["position"], want["pos"]) and _same(info_b["reward_forward"], want["fwd"]) and _same(info_b["reward_ctrl"], want["ctrl"])
        assert _same(obs_b, obs)
        if ea._auto_reset:
            assert _same(info_b["final_observation"], info["final_observation"])
        for x, y in zip(ea.get_state(), eb.get_state()):
            assert _same(x, y)
        if status:
            assert _same(ea.status(), eb.status())
        ndone = int((want["done"] != 0).sum())
        if expect_done:
            assert ndone > 0
        return ea.launch_info(), eb.launch_info(), want
    finally:
        ea.close(); eb.close()


FUSED_IDS = ["PointUMaze-v0", "Point4Rooms-v0", "PointPush-v0", "PointBilliard-v0", "SwimmerUMaze-v0", "ReacherUMaze-v0", "SwimmerPush-v0"]


@pytest.mark.parametrize("env_id", FUSED_IDS)
def test_fused_rollout_equals_stepping(env_id):
    """1024 envs, auto-reset on, K = 300: the window crosses the 256-step split of the launches, the 120-step time limit ends every
    episode at least twice, and the Point family also runs into walls and (every fourth env) into the goal."""
    point = env_id.startswith("Point")
    la, lb, want = _twin_check(lambda: mm.make(env_id, num_envs=1024, auto_reset=True, seed=5, max_episode_steps=120), 300, point=point,
                               expect_done=True)
    assert lb["rollout_fused"] == 1 and lb["engine"] == 0
    assert int((want["done"] & 2).sum()) > 0
    if point:
        assert int((want["done"] & 1).sum()) > 0  # goals were reached, not only time limits


def test_fused_rollout_partial_group_without_auto_reset():
    """1000 envs is no multiple of the envs per workgroup; without auto-reset finished envs simply go on."""
    la, lb, want = _twin_check(lambda: mm.make("PointUMaze-v0", num_envs=1000, auto_reset=False, seed=2, max_episode_steps=30), 50, point=True,
                               expect_done=True)
    assert lb["rollout_fused"] == 1


def test_fused_rollout_at_32_lanes():
    la, lb, want = _twin_check(lambda: mm.make("PointUMaze-v0", num_envs=8192, auto_reset=True, seed=3, max_episode_steps=25), 40, point=True,
                               expect_done=True)
    assert lb["rollout_fused"] == 1 and lb["lanes_per_env"] == 32


def test_fallback_ant():
    la, lb, want = _twin_check(lambda: mm.make("AntUMaze-v0", num_envs=256, auto_reset=True, seed=4, max_episode_steps=8), 20, expect_done=True)
    assert lb["rollout_fused"] == 0


def test_fallback_top_down_view():
    from mujoco_maze_amd.maze_env import VecMazeEnv

    cls, scale = view_task("ViewPush")
    la, lb, want = _twin_check(lambda: VecMazeEnv(mm.PointEnv, cls, num_envs=64, maze_size_scaling=scale, auto_reset=True, max_episode_steps=6),
                               14, point=True, expect_done=True)
    assert lb["rollout_fused"] == 0


def test_fallback_general_engine():
    la, lb, want = _twin_check(lambda: mm.make("PointUMaze-v0", num_envs=64, engine="general", auto_reset=True, max_episode_steps=7),
                               12, point=True, expect_done=True)
    assert lb["rollout_fused"] == 0 and lb["engine"] == 1


@pytest.mark.parametrize("env_id,fused", [("PointUMaze-v0", 1), ("SwimmerUMaze-v0", 1), ("ReacherUMaze-v0", 1), ("AntUMaze-v0", 0)])
def test_path_selection(env_id, fused):
    env = mm.make(env_id, num_envs=32)
    v = C.c_double(-1.0)
    assert env._lib.mz_get_info(env._h, b"rollout_fused", C.byref(v)) == 0 and int(v.value) == fused
    assert env.launch_info()["rollout_fused"] == fused
    env.close()


@pytest.mark.parametrize("env_id", ["PointUMaze-v0", "SwimmerUMaze-v0", "AntUMaze-v0"])
def test_action_repeat(env_id):
    import torch

    K, n = 9, 128
    ea, eb = (mm.make(env_id, num_envs=n, auto_reset=True, seed=1, max_episode_steps=5) for _ in range(2))
    ea.reset(seed=8); eb.reset(seed=8)
    a = _actions(ea, 1, 3)[0].contiguous()
    oa, ra, da, ia = ea.rollout(a, repeat=K, return_obs=True)
    ob, rb, db, ib = eb.rollout(a.expand(K, n, ea.nu).contiguous(), return_obs=True)
    torch.cuda.synchronize()
    assert tuple(ra.shape) == (K, n)
    assert _same(oa, ob) and _same(ra, rb) and _same(da, db) and _same(ia["observations"], ib["observations"]) and _same(ia["goal_index"], ib["goal_index"])
    for x, y in zip(ea.get_state(), eb.get_state()):
        assert _same(x, y)
    ea.close(); eb.close()


@pytest.mark.parametrize("env_id", ["PointUMaze-v0", "ReacherUMaze-v0", "AntUMaze-v0"])
def test_record_holds_the_last_step(env_id):
    import torch

    K, n = 7, 96
    env = mm.make(env_id, num_envs=n, auto_reset=True, seed=1, max_episode_steps=4)
    rec = torch.full((n, env.obs_dim + 2), -7.0, dtype=torch.float32, device=env.device)
    env.bind_record(rec)
    env.reset(seed=2)
    obs, rew, done, info = env.rollout(_actions(env, K, 6))
    torch.cuda.synchronize()
    assert _same(rec[:, : env.obs_dim].contiguous(), obs) and _same(rec[:, env.obs_dim].contiguous(), rew[K - 1].contiguous())
    assert torch.equal(rec[:, env.obs_dim + 1], done[K - 1].to(torch.float32))
    env.bind_record(None)
    env.close()


def test_python_fallback_host_judged_task():
    from mujoco_maze_amd.maze_env import VecMazeEnv

    def make():
        env = VecMazeEnv(mm.PointEnv, FarGoalCross, maze_size_scaling=4.0, num_envs=48, auto_reset=True, max_episode_steps=6)
        assert env._host_rewards
        return env

    _twin_check(make, 10, point=True, expect_done=True)


def test_python_fallback_per_env_goals_under_auto_reset():
    import torch

    from mujoco_maze_amd.maze_env import VecMazeEnv

    envs = []

    def make():
        env = VecMazeEnv(mm.PointEnv, RandomGoalCross, maze_size_scaling=4.0, num_envs=64, auto_reset=True, inner_reward_scaling=0.0,
                         max_episode_steps=6)
        envs.append(env)
        return env

    la, lb, want = _twin_check(make, 10, point=True, expect_done=True)
    assert envs[0].env_goals is not None and torch.equal(envs[0].env_goals, envs[1].env_goals)


def test_refusals():
    import torch

    env = mm.make("PointUMaze-v0", num_envs=16)
    env.reset(seed=1)
    n, nu, lib, h = env.num_envs, env.nu, env._lib, env._h
    a = torch.zeros((3, n, nu), dtype=torch.float32, device=env.device)
    rew, done = torch.zeros((3, n), device=env.device), torch.zeros((3, n), dtype=torch.uint8, device=env.device)
    p = lambda t: C.c_void_p(t.data_ptr())
    call = lambda k, stride: lib.mz_rollout(h, k, p(a), stride, p(env._obs), p(rew), p(done), None, None, None, env._stream())
    assert call(0, n * nu) == MZ_ERR_ARG and b"n_steps" in lib.mz_last_error(h)
    assert call(65537, 0) == MZ_ERR_ARG
    assert call(3, n * nu + 1) == MZ_ERR_ARG and b"stride" in lib.mz_last_error(h)
    assert call(3, nu) == MZ_ERR_ARG
    assert lib.mz_rollout(h, 3, p(a), n * nu, p(env._obs), None, p(done), None, None, None, env._stream()) == MZ_ERR_ARG
    assert call(3, n * nu) == 0 and call(3, 0) == 0
    with pytest.raises(ValueError):
        env.rollout(torch.zeros((n, nu), device=env.device))  # [N, nu] needs repeat
    with pytest.raises(ValueError):
        env.rollout(torch.zeros((3, n, nu), device=env.device), repeat=3)
    with pytest.raises(ValueError):
        env.rollout(torch.zeros((3, n + 1, nu), device=env.device))
    with pytest.raises(ValueError):
        env.rollout(torch.zeros((n, nu), device=env.device), repeat=0)
    torch.cuda.synchronize()
    env.close()
