"""VecMazeEnv.policy_act / rollout_policy (mz_policy_act / mz_rollout_policy) on the device.

policy_act goes against mujoco_maze_amd.policy.reference (affine: bit equal) and a float64 evaluation within the derived bound of
tests/test_policy_api.py (tanh paths).  rollout_policy goes against K times (policy_act, step) on a twin env — same id, num_envs,
seed, reset and injected states — by bit patterns (`_same` of tests/test_gpu_rollout.py): the fused kernels run the same unit
functions on the same fp32 observation rows as the stand-alone policy kernel, so nothing may differ."""
import ctypes as C

import numpy as np
import pytest

import mujoco_maze_amd as mm
from mujoco_maze_amd import policy
from tests.test_custom_task import FarGoalCross, RandomGoalCross
from tests.test_gpu_rollout import FUSED_IDS, _near_goal, _same
from tests.test_policy_api import SCALE, f64_and_bound, random_policy
from tests.test_top_down_view import view_task

pytestmark = pytest.mark.gpu
MZ_ERR_ARG = -1
# (per-env params, hidden, squash): one shared affine policy, and one tanh policy per env at a narrow and at the widest hidden layer
POLICIES = [(False, 0, False), (True, 5, True), (True, 64, True)]
POLICY_IDS = ["shared-affine", "per-env-H5-squash", "per-env-H64-squash"]
ACTION_SCALE = 0.9  # no power of two: the squashed output is a rounded product


def _policy(env, per_env, hidden, squash, seed, drive=False):
    """kwargs of policy_act / rollout_policy with random parameters on the env's device.  `drive` (Point family): a small output
    layer and a bias on the first action that drives forward, so that the robots run into walls and goals."""
    import torch

    rng = np.random.default_rng(seed)
    p = random_policy(rng, env.obs_dim, env.nu, hidden, rows=env.num_envs if per_env else None)
    if drive:
        last = env.nu + (hidden if hidden else env.obs_dim) * env.nu  # the output layer: its weights and biases
        p[..., -last:] *= 0.1
        p[..., -env.nu] = 2.0 if squash else 1.0
    return dict(params=torch.as_tensor(p, device=env.device), hidden=hidden, squash=squash, action_scale=ACTION_SCALE)


def _current_obs(env):
    """every env's observation of its present state, nothing reset (set_state does not refresh the observation buffer)"""
    import torch

    return env.reset(mask=torch.zeros(env.num_envs, dtype=torch.uint8, device=env.device))


KEYS = ("act", "obs", "reward", "done", "goal", "pos", "fwd", "ctrl")


def _loop(env, pol, K):
    """K times (policy_act, step): the stacked rows, the last step's obs and info"""
    import torch

    rows = {k: [] for k in KEYS}
    for k in range(K):
        a = env.policy_act(**pol)
        obs, rew, done, info = env.step(a)
        for key, v in zip(KEYS, (a, obs, rew, done, info["goal_index"], info["position"], info["reward_forward"], info["reward_ctrl"])):
            rows[key].append(v.clone())
    return {k: torch.stack(v) for k, v in rows.items()}, obs, info


def _assert_equal(ea, eb, want, obs_a, info_a, out_b, K, status=True):
    import torch

    obs_b, rew_b, done_b, info_b = out_b
    torch.cuda.synchronize()
    assert tuple(rew_b.shape) == (K, ea.num_envs) and done_b.dtype == torch.uint8
    assert tuple(info_b["actions"].shape) == (K, ea.num_envs, ea.nu) and tuple(info_b["observations"].shape) == (K, ea.num_envs, ea.obs_dim)
    assert _same(info_b["actions"], want["act"])
    assert _same(rew_b, want["reward"])
    assert _same(done_b, want["done"])
    assert _same(info_b["goal_index"], want["goal"])
    assert _same(info_b["observations"], want["obs"])
    assert _same(info_b["position"], want["pos"]) and _same(info_b["reward_forward"], want["fwd"]) and _same(info_b["reward_ctrl"], want["ctrl"])
    assert _same(obs_b, obs_a)
    if ea._auto_reset:
        assert _same(info_b["final_observation"], info_a["final_observation"])
    for x, y in zip(ea.get_state(), eb.get_state()):
        assert _same(x, y)
    if status:
        assert _same(ea.status(), eb.status())


def _twin_check(make, K, pol_spec, seed=11, point=False, prepare=None):
    """env A: K x (policy_act, step); env B: one rollout_policy.  Returns (launch info of B, the loop's rows, the policy)."""
    ea, eb = make(), make()
    try:
        for e in (ea, eb):
            if prepare:
                prepare(e)
            o = e.reset(seed=seed)
            if point:
                _near_goal(e, o)
                _current_obs(e)
        assert _same(ea._obs, eb._obs)
        pol = _policy(ea, *pol_spec, seed=seed + 1, drive=point)
        want, obs_a, info_a = _loop(ea, pol, K)
        out_b = eb.rollout_policy(steps=K, return_obs=True, return_actions=True, **pol)
        _assert_equal(ea, eb, want, obs_a, info_a, out_b, K)
        return eb.launch_info(), want, pol
    finally:
        ea.close(); eb.close()


# ---------------------------------------------------------------------------------------------- 1. policy_act against the model
@pytest.mark.parametrize("env_id", ["PointUMaze-v0", "AntUMaze-v0"])
def test_policy_act_against_the_model(env_id):
    import torch

    env = mm.make(env_id, num_envs=130, seed=3)
    try:
        env.reset(seed=4)
        g = torch.Generator(device=env.device).manual_seed(1)
        lo, hi = torch.as_tensor(env.action_space.low, device=env.device), torch.as_tensor(env.action_space.high, device=env.device)
        for _ in range(3):  # observations of moving robots
            obs, _, _, _ = env.step(lo + (hi - lo) * torch.rand((130, env.nu), device=env.device, generator=g))
        x = obs.cpu().numpy()
        rng = np.random.default_rng(7)
        p0 = random_policy(rng, env.obs_dim, env.nu, 0, rows=130)
        got = env.policy_act(torch.as_tensor(p0, device=env.device)).cpu().numpy()
        want = policy.reference(p0, x, env.nu)
        assert got.shape == (130, env.nu) and np.array_equal(got.view(np.int32), want.view(np.int32))
        # the same rows passed explicitly, and one shared policy
        got2 = env.policy_act(torch.as_tensor(p0[5], device=env.device), obs=obs.clone()).cpu().numpy()
        assert np.array_equal(got2.view(np.int32), policy.reference(p0[5], x, env.nu).view(np.int32))
        for hidden in (5, 64):
            p = random_policy(rng, env.obs_dim, env.nu, hidden, rows=130)
            got = env.policy_act(torch.as_tensor(p, device=env.device), hidden=hidden, squash=True, action_scale=SCALE).cpu().numpy()
            val, bound = f64_and_bound(p, x, env.nu, hidden, True, SCALE)
            err = np.abs(got.astype(np.float64) - val)
            print(f"{env_id} H {hidden}: max err {err.max():.3e}, max err / bound {(err / bound).max():.3f}")
            assert np.all(err <= bound)
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------- 2. fused equals the loop
@pytest.mark.parametrize("pol_spec", POLICIES, ids=POLICY_IDS)
@pytest.mark.parametrize("env_id", FUSED_IDS)
def test_fused_rollout_policy_equals_the_loop(env_id, pol_spec):
    """130 envs (no multiple of the envs per workgroup), auto-reset, K = 260: the second launch picks its first observation up
    from the observation buffer, and the 40-step time limit ends every episode several times, so the policy acts on new-episode rows."""
    point = env_id.startswith("Point")
    lb, want, _ = _twin_check(lambda: mm.make(env_id, num_envs=130, auto_reset=True, seed=5, max_episode_steps=40), 260, pol_spec, point=point)
    assert lb["rollout_fused"] == 1 and lb["engine"] == 0
    assert int((want["done"] & 2).sum()) > 0
    if point:
        assert int((want["done"] & 1).sum()) > 0  # goals were reached, not only time limits


def test_fused_rollout_policy_at_32_lanes():
    lb, want, _ = _twin_check(lambda: mm.make("PointUMaze-v0", num_envs=130, auto_reset=True, seed=3, max_episode_steps=40), 260, POLICIES[1],
                              point=True, prepare=lambda e: e.set_option("lanes_per_env", 32))
    assert lb["rollout_fused"] == 1 and lb["lanes_per_env"] == 32
    assert int((want["done"] & 1).sum()) > 0 and int((want["done"] & 2).sum()) > 0


@pytest.mark.parametrize("env_id", ["PointUMaze-v0", "SwimmerUMaze-v0"])
def test_fused_rollout_policy_without_auto_reset(env_id):
    """finished envs simply go on, and the policy with them"""
    point = env_id.startswith("Point")
    lb, want, _ = _twin_check(lambda: mm.make(env_id, num_envs=130, auto_reset=False, seed=2, max_episode_steps=30), 260, POLICIES[1], point=point)
    assert lb["rollout_fused"] == 1 and int((want["done"] & 2).sum()) > 0


# ---------------------------------------------------------------------------------------------- 3. replay through rollout()
@pytest.mark.parametrize("env_id", ["PointUMaze-v0", "PointPush-v0", "SwimmerUMaze-v0"])
def test_replaying_the_actions_through_rollout(env_id):
    """the actions rollout_policy returned, fed to the open-loop rollout() on a third twin: everything equal — the new path tied to
    the existing, already pinned one"""
    import torch

    point, K = env_id.startswith("Point"), 260
    eb, ec = (mm.make(env_id, num_envs=130, auto_reset=True, seed=5, max_episode_steps=40) for _ in range(2))
    try:
        for e in (eb, ec):
            o = e.reset(seed=9)
            if point:
                _near_goal(e, o)
                _current_obs(e)
        pol = _policy(eb, True, 5, True, seed=10, drive=point)
        obs_b, rew_b, done_b, info_b = eb.rollout_policy(steps=K, return_obs=True, return_actions=True, **pol)
        obs_c, rew_c, done_c, info_c = ec.rollout(info_b["actions"], return_obs=True)
        torch.cuda.synchronize()
        assert _same(obs_b, obs_c) and _same(rew_b, rew_c) and _same(done_b, done_c)
        for key in ("observations", "goal_index", "position", "reward_forward", "reward_ctrl", "final_observation"):
            assert _same(info_b[key], info_c[key]), key
        for x, y in zip(eb.get_state(), ec.get_state()):
            assert _same(x, y)
        assert _same(eb.status(), ec.status())
        assert int((done_b != 0).sum()) > 0
    finally:
        eb.close(); ec.close()


# ---------------------------------------------------------------------------------------------- 4. degenerate policy
@pytest.mark.parametrize("env_id", ["PointUMaze-v0", "SwimmerUMaze-v0", "AntUMaze-v0"])
def test_constant_policy_is_action_repeat(env_id):
    import torch

    K, n = 30, 130
    ea, eb = (mm.make(env_id, num_envs=n, auto_reset=True, seed=1, max_episode_steps=12) for _ in range(2))
    try:
        ea.reset(seed=8); eb.reset(seed=8)
        c = torch.as_tensor((0.35 * ea.action_space.high).astype(np.float32), device=ea.device)
        params = torch.cat([torch.zeros(ea.obs_dim * ea.nu, device=ea.device), c])
        oa, ra, da, ia = ea.rollout_policy(params, K, return_obs=True, return_actions=True)
        ob, rb, db, ib = eb.rollout(c.expand(n, ea.nu).contiguous(), repeat=K, return_obs=True)
        torch.cuda.synchronize()
        assert _same(ia["actions"], c.expand(K, n, ea.nu).contiguous())
        assert _same(oa, ob) and _same(ra, rb) and _same(da, db) and _same(ia["observations"], ib["observations"]) and _same(ia["goal_index"], ib["goal_index"])
        for x, y in zip(ea.get_state(), eb.get_state()):
            assert _same(x, y)
    finally:
        ea.close(); eb.close()


# ---------------------------------------------------------------------------------------------- 5. unfused handles
def test_unfused_ant():
    lb, want, _ = _twin_check(lambda: mm.make("AntUMaze-v0", num_envs=64, auto_reset=True, seed=4, max_episode_steps=8), 20, POLICIES[1])
    assert lb["rollout_fused"] == 0 and int((want["done"] != 0).sum()) > 0


def test_unfused_top_down_view():
    from mujoco_maze_amd.maze_env import VecMazeEnv

    cls, scale = view_task("ViewPush")
    dims = []

    def make():
        env = VecMazeEnv(mm.PointEnv, cls, num_envs=64, maze_size_scaling=scale, auto_reset=True, max_episode_steps=6)
        dims.append(env.obs_dim)
        return env

    lb, want, pol = _twin_check(make, 14, POLICIES[1], point=True)
    assert lb["rollout_fused"] == 0
    assert dims[0] > 75 and pol["params"].shape[1] == policy.param_count(dims[0], 2, 5)  # the policy reads the 75 view entries too
    assert int((want["done"] != 0).sum()) > 0


def test_unfused_general_engine():
    lb, want, _ = _twin_check(lambda: mm.make("PointUMaze-v0", num_envs=32, engine="general", auto_reset=True, max_episode_steps=7), 12,
                              POLICIES[2], point=True)
    assert lb["rollout_fused"] == 0 and lb["engine"] == 1


@pytest.mark.parametrize("env_id", ["PointUMaze-v0", "AntUMaze-v0"])
def test_record_holds_the_last_step(env_id):
    import torch

    K, n = 7, 96
    env = mm.make(env_id, num_envs=n, auto_reset=True, seed=1, max_episode_steps=4)
    try:
        rec = torch.full((n, env.obs_dim + 2), -7.0, dtype=torch.float32, device=env.device)
        env.bind_record(rec)
        env.reset(seed=2)
        obs, rew, done, info = env.rollout_policy(steps=K, **_policy(env, True, 5, True, seed=6))
        torch.cuda.synchronize()
        assert "actions" not in info and "observations" not in info
        assert _same(rec[:, : env.obs_dim].contiguous(), obs) and _same(rec[:, env.obs_dim].contiguous(), rew[K - 1].contiguous())
        assert torch.equal(rec[:, env.obs_dim + 1], done[K - 1].to(torch.float32))
        env.bind_record(None)
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------- 6. host-side fallbacks, arguments
def test_python_loop_host_judged_task():
    from mujoco_maze_amd.maze_env import VecMazeEnv

    def make():
        env = VecMazeEnv(mm.PointEnv, FarGoalCross, maze_size_scaling=4.0, num_envs=48, auto_reset=True, max_episode_steps=6)
        assert env._host_rewards
        return env

    lb, want, _ = _twin_check(make, 10, POLICIES[1], point=True)
    assert tuple(want["act"].shape) == (10, 48, 2) and int((want["done"] != 0).sum()) > 0


def test_python_loop_per_env_goals_under_auto_reset():
    import torch

    from mujoco_maze_amd.maze_env import VecMazeEnv

    envs = []

    def make():
        env = VecMazeEnv(mm.PointEnv, RandomGoalCross, maze_size_scaling=4.0, num_envs=64, auto_reset=True, inner_reward_scaling=0.0,
                         max_episode_steps=6)
        envs.append(env)
        return env

    lb, want, _ = _twin_check(make, 10, POLICIES[0], point=True)
    assert envs[0].env_goals is not None and torch.equal(envs[0].env_goals, envs[1].env_goals)
    assert tuple(want["reward"].shape) == (10, 64) and int((want["done"] != 0).sum()) > 0


def test_refusals():
    import torch

    env = mm.make("PointUMaze-v0", num_envs=16)
    try:
        env.reset(seed=1)
        n, nu, od, lib, h, dev = env.num_envs, env.nu, env.obs_dim, env._lib, env._h, env.device
        npar0, npar5 = policy.param_count(od, nu, 0), policy.param_count(od, nu, 5)
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
        for bad in (dict(params=z(npar0 + 1), steps=3), dict(params=z(n + 1, npar0), steps=3), dict(params=z(npar0), steps=3, hidden=5),
                    dict(params=z(n, npar5, 1), steps=3, hidden=5), dict(params=z(npar0), steps=3, hidden=65), dict(params=z(npar0), steps=3, hidden=-1),
                    dict(params=z(npar0), steps=0), dict(params=z(npar0), steps=65537), dict(params=z(npar0), steps=3, obs=z(n, od + 1))):
            with pytest.raises(ValueError):
                env.rollout_policy(**bad)
        with pytest.raises(ValueError):
            env.policy_act(z(npar0 + 1))
        with pytest.raises(ValueError):
            env.policy_act(z(npar0), hidden=65)
        with pytest.raises(ValueError):
            env.policy_act(z(npar0), obs=z(n, od + 1))
        # straight through the C-ABI
        par, act = z(n, npar5), z(3, n, nu)
        rew, done = z(3, n), torch.zeros((3, n), dtype=torch.uint8, device=dev)
        p = lambda t: C.c_void_p(t.data_ptr())
        roll = lambda k, stride, hidden=5, squash=1: lib.mz_rollout_policy(h, k, p(par), stride, hidden, squash, 1.0, p(env._obs), p(rew), p(done), None,
                                                                            None, None, p(act), env._stream())
        assert roll(0, npar5) == MZ_ERR_ARG and b"n_steps" in lib.mz_last_error(h)
        assert roll(65537, 0) == MZ_ERR_ARG
        assert roll(3, npar5 + 1) == MZ_ERR_ARG and b"stride" in lib.mz_last_error(h)
        assert roll(3, npar0) == MZ_ERR_ARG and roll(3, 1) == MZ_ERR_ARG
        assert roll(3, 0, hidden=65) == MZ_ERR_ARG and b"hidden" in lib.mz_last_error(h)
        assert roll(3, 0, hidden=-1) == MZ_ERR_ARG
        assert roll(3, 0, squash=2) == MZ_ERR_ARG and b"squash" in lib.mz_last_error(h)
        assert lib.mz_rollout_policy(h, 3, None, 0, 5, 1, 1.0, p(env._obs), p(rew), p(done), None, None, None, None, env._stream()) == MZ_ERR_ARG
        assert lib.mz_rollout_policy(h, 3, p(par), 0, 5, 1, 1.0, p(env._obs), None, p(done), None, None, None, None, env._stream()) == MZ_ERR_ARG
        assert lib.mz_rollout_policy(h, 3, p(par), 0, 5, 1, 1.0, None, p(rew), p(done), None, None, None, None, env._stream()) == MZ_ERR_ARG
        pact = lambda stride, hidden=5, squash=1, o=env._obs, a=act: lib.mz_policy_act(h, p(par), stride, hidden, squash, 1.0, p(o) if o is not None else None,
                                                                                       p(a) if a is not None else None, env._stream())
        assert pact(npar5 - 1) == MZ_ERR_ARG and pact(0, hidden=65) == MZ_ERR_ARG and pact(0, squash=-1) == MZ_ERR_ARG
        assert pact(0, o=None) == MZ_ERR_ARG and pact(0, a=None) == MZ_ERR_ARG
        assert lib.mz_policy_act(h, None, 0, 5, 1, 1.0, p(env._obs), p(act), env._stream()) == MZ_ERR_ARG
        assert roll(3, npar5) == 0 and roll(3, 0) == 0 and pact(npar5) == 0 and pact(0) == 0
        # after the refused calls the env still steps
        obs, rew1, done1, _ = env.step(z(n, nu))
        torch.cuda.synchronize()
        assert torch.isfinite(obs).all() and tuple(rew1.shape) == (n,)
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------- 7. stale observation
@pytest.mark.parametrize("env_id", ["PointUMaze-v0", "SwimmerUMaze-v0", "AntUMaze-v0"])
def test_observation_after_set_state(env_id):
    """set_state leaves the observation buffer as it was; reset(mask=zeros) returns every env's current observation without resetting
    any, and rollout_policy then acts on it — as a twin does that is handed that observation as obs="""
    import torch

    K, n = 12, 130
    ea, eb = (mm.make(env_id, num_envs=n, auto_reset=False, seed=1) for _ in range(2))
    try:
        for e in (ea, eb):
            stale = e.reset(seed=6).clone()
            qpos, qvel, warm, t = e.get_state()
            qpos[:, 0] += 0.25
            qpos[:, 1] -= 0.125
            t += 3
            e.set_state(qpos=qpos, qvel=qvel, t=t)
        assert _same(ea._obs, stale)  # not refreshed
        cur = _current_obs(ea).clone()
        q2, v2, w2, t2 = ea.get_state()
        assert _same(q2, qpos) and _same(v2, qvel) and torch.equal(t2, t)  # nothing was reset
        assert torch.equal(cur[:, :2], qpos[:, :2]) and not torch.equal(cur[:, :2], stale[:, :2])
        assert torch.allclose(cur[:, -1], torch.full((n,), 0.003, device=ea.device))  # the time entry follows t
        pol = _policy(ea, True, 5, True, seed=3)
        want, obs_a, info_a = _loop(ea, pol, K)
        assert _same(eb._obs, stale)
        out_b = eb.rollout_policy(steps=K, obs=cur, return_obs=True, return_actions=True, **pol)
        _assert_equal(ea, eb, want, obs_a, info_a, out_b, K)
        # the stale row would have given other actions
        assert not _same(want["act"][0], ea.policy_act(obs=stale, **pol))
    finally:
        ea.close(); eb.close()
