"""VecMazeEnv.policy_sample / rollout_policy_sample (mz_policy_sample / mz_rollout_policy_sample) on the device.

The noise goes against mujoco_maze_amd.policy.noise at the suite's 1e-5 (the two sides share the fp32 u1, u2 and angle and differ by
libm ulps on a radius <= 5.77: below 2e-6) and, by bit patterns, against itself under another batch size and env_index_offset.
rollout_policy_sample goes against K times (policy_sample(noise_step + k), step) on a twin env — same id, num_envs, seed, reset and
injected states — by bit patterns: the fused kernels run the unit functions of the stand-alone kernel on the same fp32 rows with the
same four integers per draw, so nothing may differ.  The helpers are those of tests/test_gpu_policy_rollout.py."""
import ctypes as C

import numpy as np
import pytest

import mujoco_maze_amd as mm
from mujoco_maze_amd import policy
from tests.test_custom_task import FarGoalCross, RandomGoalCross
from tests.test_gpu_policy_rollout import KEYS, POLICIES, POLICY_IDS, _assert_equal, _current_obs, _policy
from tests.test_gpu_rollout import FUSED_IDS, _near_goal, _same
from tests.test_top_down_view import view_task

pytestmark = pytest.mark.gpu
MZ_ERR_ARG = -1
SEED, STEP0 = 77, 1000


def _spolicy(env, per_env, hidden, squash, seed, drive=False, log_std=None):
    """_policy with log_std [nu] behind the network: U(-1, 0) per unit (and per env) unless given"""
    import torch

    pol = _policy(env, per_env, hidden, squash, seed, drive=drive)
    net = pol["params"]
    if log_std is None:
        ls = np.random.default_rng(seed + 1000).uniform(-1.0, 0.0, tuple(net.shape[:-1]) + (env.nu,)).astype(np.float32)
    else:
        ls = np.full(tuple(net.shape[:-1]) + (env.nu,), log_std, np.float32)
    pol["params"] = torch.cat([net, torch.as_tensor(ls, device=env.device)], dim=-1).contiguous()
    return pol


def _loop(env, pol, K, seed=SEED, step0=STEP0):
    """K times (policy_sample(noise_step = step0 + k), step): the stacked rows, the last step's obs and info"""
    import torch

    rows = {k: [] for k in KEYS + ("logp",)}
    for k in range(K):
        a, lp = env.policy_sample(noise_seed=seed, noise_step=step0 + k, **pol)
        obs, rew, done, info = env.step(a)
        for key, v in zip(KEYS + ("logp",), (a, obs, rew, done, info["goal_index"], info["position"], info["reward_forward"], info["reward_ctrl"], lp)):
            rows[key].append(v.clone())
    return {k: torch.stack(v) for k, v in rows.items()}, obs, info


def _twin_check(make, K, pol_spec, seed=11, point=False, prepare=None):
    """env A: K x (policy_sample, step); env B: one rollout_policy_sample.  Returns (launch info of B, the loop's rows, the policy)."""
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
        pol = _spolicy(ea, *pol_spec, seed=seed + 1, drive=point)
        want, obs_a, info_a = _loop(ea, pol, K)
        out_b = eb.rollout_policy_sample(steps=K, noise_seed=SEED, noise_step=STEP0, return_obs=True, return_actions=True, **pol)
        _assert_equal(ea, eb, want, obs_a, info_a, out_b, K)
        assert tuple(out_b[3]["logp"].shape) == (K, ea.num_envs) and _same(out_b[3]["logp"], want["logp"])
        import torch

        assert torch.isfinite(want["logp"][0]).all() and torch.isfinite(want["act"][0]).all()  # (an unsquashed policy may drive a chain to NaN later on)
        return eb.launch_info(), want, pol
    finally:
        ea.close(); eb.close()


# ---------------------------------------------------------------------------------------------- 1. the noise itself
def _zero_policy(env, log_std=0.0):
    import torch

    p = torch.zeros(policy.param_count(env.obs_dim, env.nu, 0, stochastic=True), dtype=torch.float32, device=env.device)
    p[-env.nu:] = log_std
    return p


@pytest.mark.parametrize("env_id", ["AntUMaze-v0", "PointUMaze-v0"])
def test_policy_sample_returns_the_noise(env_id):
    """all weights and biases zero, log_std 0, no squash: the action IS eps"""
    n = 130
    env = mm.make(env_id, num_envs=n, seed=3)
    try:
        env.reset(seed=4)
        nu = env.nu
        act, logp = env.policy_sample(_zero_policy(env), noise_seed=1234, noise_step=7)
        eps, lp = act.cpu().numpy(), logp.cpu().numpy()
        want = policy.noise(1234, 7, range(n), nu)
        err = np.abs(eps.astype(np.float64) - want)
        print(f"{env_id}: max |device eps - policy.noise| = {err.max():.3e}")
        assert eps.shape == (n, nu) and lp.shape == (n,) and err.max() < 1e-5
        e64 = eps.astype(np.float64)
        lp64 = np.sum(-0.5 * e64 ** 2 - 0.9189385332046727, axis=1)
        bound = (4 * nu + 2) * 2.0 ** -23 * np.sum(0.5 * e64 ** 2 + 0.919, axis=1)
        print(f"{env_id}: max logp err / bound = {(np.abs(lp - lp64) / bound).max():.3f}")
        assert np.all(np.abs(lp - lp64) <= bound)
        # another step and another seed are other numbers
        other, _ = env.policy_sample(_zero_policy(env), noise_seed=1234, noise_step=8)
        assert not _same(other, act)
    finally:
        env.close()


@pytest.mark.parametrize("env_id", ["AntUMaze-v0", "PointUMaze-v0"])
def test_noise_is_keyed_by_the_global_slot(env_id):
    small, big = mm.make(env_id, num_envs=3, seed=3), mm.make(env_id, num_envs=8, seed=3)
    try:
        small.set_option("env_index_offset", 5)
        small.reset(seed=4); big.reset(seed=4)
        a3, l3 = small.policy_sample(_zero_policy(small), noise_seed=9, noise_step=2)
        a8, l8 = big.policy_sample(_zero_policy(big), noise_seed=9, noise_step=2)
        assert _same(a3, a8[5:8].contiguous()) and _same(l3, l8[5:8].contiguous())
        assert not _same(a3, a8[0:3].contiguous())
    finally:
        small.close(); big.close()


# ---------------------------------------------------------------------------------------------- 2. fused equals the loop
@pytest.mark.parametrize("pol_spec", POLICIES, ids=POLICY_IDS)
@pytest.mark.parametrize("env_id", FUSED_IDS)
def test_fused_rollout_policy_sample_equals_the_loop(env_id, pol_spec):
    """130 envs (idle groups in the last workgroup), auto-reset, K = 260: two launches — the second continues at noise_step + 256 on
    the observation the first left — and the 40-step time limit ends every episode several times"""
    point = env_id.startswith("Point")
    lb, want, _ = _twin_check(lambda: mm.make(env_id, num_envs=130, auto_reset=True, seed=5, max_episode_steps=40), 260, pol_spec, point=point)
    assert lb["rollout_fused"] == 1 and lb["engine"] == 0
    assert int((want["done"] & 2).sum()) > 0
    if point:
        assert int((want["done"] & 1).sum()) > 0  # goals were reached, not only time limits


def test_fused_rollout_policy_sample_at_32_lanes():
    lb, want, _ = _twin_check(lambda: mm.make("PointUMaze-v0", num_envs=130, auto_reset=True, seed=3, max_episode_steps=40), 260, POLICIES[1],
                              point=True, prepare=lambda e: e.set_option("lanes_per_env", 32))
    assert lb["rollout_fused"] == 1 and lb["lanes_per_env"] == 32
    assert int((want["done"] & 1).sum()) > 0 and int((want["done"] & 2).sum()) > 0


def test_fused_rollout_policy_sample_without_auto_reset():
    lb, want, _ = _twin_check(lambda: mm.make("SwimmerUMaze-v0", num_envs=130, auto_reset=False, seed=2, max_episode_steps=30), 260, POLICIES[1])
    assert lb["rollout_fused"] == 1 and int((want["done"] & 2).sum()) > 0


# ---------------------------------------------------------------------------------------------- 3. unfused handles
def test_unfused_ant():
    lb, want, _ = _twin_check(lambda: mm.make("AntUMaze-v0", num_envs=64, auto_reset=True, seed=4, max_episode_steps=8), 20, POLICIES[1])
    assert lb["rollout_fused"] == 0 and int((want["done"] != 0).sum()) > 0


def test_unfused_top_down_view():
    from mujoco_maze_amd.maze_env import VecMazeEnv

    cls, scale = view_task("ViewPush")
    lb, want, pol = _twin_check(lambda: VecMazeEnv(mm.PointEnv, cls, num_envs=64, maze_size_scaling=scale, auto_reset=True, max_episode_steps=6), 14,
                                POLICIES[1], point=True)
    assert lb["rollout_fused"] == 0 and int((want["done"] != 0).sum()) > 0


def test_unfused_general_engine():
    lb, want, _ = _twin_check(lambda: mm.make("PointUMaze-v0", num_envs=32, engine="general", auto_reset=True, max_episode_steps=7), 12,
                              POLICIES[2], point=True)
    assert lb["rollout_fused"] == 0 and lb["engine"] == 1


# ---------------------------------------------------------------------------------------------- 4. Python fallbacks
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
    assert int((want["done"] != 0).sum()) > 0


# ---------------------------------------------------------------------------------------------- 5. ties to what is already pinned
@pytest.mark.parametrize("env_id", ["PointUMaze-v0", "PointPush-v0", "SwimmerUMaze-v0"])
def test_replaying_the_sampled_actions_through_rollout(env_id):
    import torch

    point, K = env_id.startswith("Point"), 260
    eb, ec = (mm.make(env_id, num_envs=130, auto_reset=True, seed=5, max_episode_steps=40) for _ in range(2))
    try:
        for e in (eb, ec):
            o = e.reset(seed=9)
            if point:
                _near_goal(e, o)
                _current_obs(e)
        pol = _spolicy(eb, True, 5, True, seed=10, drive=point)
        obs_b, rew_b, done_b, info_b = eb.rollout_policy_sample(steps=K, noise_seed=SEED, noise_step=STEP0, return_obs=True, return_actions=True, **pol)
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


@pytest.mark.parametrize("env_id", ["PointUMaze-v0", "SwimmerUMaze-v0", "AntUMaze-v0"])
def test_zero_std_is_the_deterministic_policy(env_id):
    """log_std = -inf: s = 0 and z = m + (+-0) — the actions of rollout_policy by value (-0 + 0 is +0), every step output by bits"""
    import torch

    point, K, n = env_id.startswith("Point"), 60, 130
    ea, eb = (mm.make(env_id, num_envs=n, auto_reset=True, seed=5, max_episode_steps=25) for _ in range(2))
    try:
        for e in (ea, eb):
            o = e.reset(seed=9)
            if point:
                _near_goal(e, o)
                _current_obs(e)
        pol = _spolicy(ea, True, 5, True, seed=10, drive=point, log_std=-np.inf)
        det = dict(pol, params=pol["params"][:, : -ea.nu].contiguous())
        obs_a, rew_a, done_a, info_a = ea.rollout_policy(steps=K, return_obs=True, return_actions=True, **det)
        obs_b, rew_b, done_b, info_b = eb.rollout_policy_sample(steps=K, noise_seed=SEED, noise_step=STEP0, return_obs=True, return_actions=True, **pol)
        torch.cuda.synchronize()
        assert torch.equal(info_a["actions"], info_b["actions"])
        assert _same(obs_a, obs_b) and _same(rew_a, rew_b) and _same(done_a, done_b)
        for key in ("observations", "goal_index", "position", "reward_forward", "reward_ctrl", "final_observation"):
            assert _same(info_a[key], info_b[key]), key
        for x, y in zip(ea.get_state(), eb.get_state()):
            assert _same(x, y)
        assert torch.isposinf(info_b["logp"]).all() and int((done_b != 0).sum()) > 0
    finally:
        ea.close(); eb.close()


# ---------------------------------------------------------------------------------------------- 6. counter semantics
@pytest.mark.parametrize("env_id", ["PointUMaze-v0", "AntUMaze-v0"])
def test_counter_semantics(env_id):
    import torch

    n = 48
    ea, eb = (mm.make(env_id, num_envs=n, auto_reset=True, seed=21, max_episode_steps=7) for _ in range(2))
    try:
        pol = _spolicy(ea, True, 5, True, seed=10)
        # no reset(seed=): the constructor's seed and a counter at 0 — two default calls of 5 equal one of 10
        ea.reset(); eb.reset()
        first = [t.clone() if torch.is_tensor(t) else {k: v.clone() for k, v in t.items()} for t in ea.rollout_policy_sample(steps=5, return_actions=True, **pol)]
        second = ea.rollout_policy_sample(steps=5, return_actions=True, **pol)
        whole = eb.rollout_policy_sample(steps=10, return_actions=True, **pol)
        torch.cuda.synchronize()
        assert ea._noise_step == eb._noise_step == 10 and ea._noise_seed == 21
        assert _same(torch.cat([first[3]["actions"], second[3]["actions"]]), whole[3]["actions"])
        assert _same(torch.cat([first[3]["logp"], second[3]["logp"]]), whole[3]["logp"])
        assert _same(torch.cat([first[1], second[1]]), whole[1]) and _same(second[0], whole[0])
        # ... which is the explicit (21, 0 .. 9); policy_sample advances the counter by one
        a10, _ = ea.policy_sample(**pol)
        b10, _ = eb.policy_sample(noise_seed=21, noise_step=10, **pol)
        assert _same(a10, b10) and ea._noise_step == 11 and eb._noise_step == 10
        # a repeated explicit noise_step reproduces the draw from the same state, another seed changes it
        x1, l1 = ea.policy_sample(noise_seed=5, noise_step=3, **pol)
        x2, l2 = ea.policy_sample(noise_seed=5, noise_step=3, **pol)
        x3, _ = ea.policy_sample(noise_seed=6, noise_step=3, **pol)
        assert _same(x1, x2) and _same(l1, l2) and not _same(x1, x3) and ea._noise_step == 11
        # reset(seed=) is the new default seed and starts the counter again
        ea.reset(seed=33); eb.reset(seed=33)
        assert ea._noise_seed == 33 and ea._noise_step == 0
        r1 = ea.rollout_policy_sample(steps=4, return_actions=True, **pol)
        r2 = eb.rollout_policy_sample(steps=4, noise_seed=33, noise_step=0, return_actions=True, **pol)
        torch.cuda.synchronize()
        assert _same(r1[3]["actions"], r2[3]["actions"]) and ea._noise_step == 4 and eb._noise_step == 0
    finally:
        ea.close(); eb.close()


# ---------------------------------------------------------------------------------------------- 7. refusals, NaN
def test_refusals():
    import torch

    env = mm.make("PointUMaze-v0", num_envs=16)
    try:
        env.reset(seed=1)
        n, nu, od, lib, h, dev = env.num_envs, env.nu, env.obs_dim, env._lib, env._h, env.device
        npar5, npar5s = policy.param_count(od, nu, 5), policy.param_count(od, nu, 5, stochastic=True)
        assert npar5s == npar5 + nu
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
        for bad in (dict(params=z(npar5), steps=3, hidden=5), dict(params=z(n, npar5), steps=3, hidden=5), dict(params=z(npar5s), steps=0, hidden=5),
                    dict(params=z(npar5s), steps=65537, hidden=5), dict(params=z(npar5s), steps=3, hidden=5, obs=z(n, od + 1))):
            with pytest.raises(ValueError):
                env.rollout_policy_sample(**bad)
        with pytest.raises(ValueError):
            env.policy_sample(z(npar5), hidden=5)
        # straight through the C-ABI
        par, act, lp = z(n, npar5s), z(3, n, nu), z(3, n)
        rew, done = z(3, n), torch.zeros((3, n), dtype=torch.uint8, device=dev)
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        roll = lambda k, stride, params=par, obs=env._obs, r=rew, d=done: lib.mz_rollout_policy_sample(
            h, k, p(params), stride, 5, 1, 1.0, 1, 2, p(obs), p(r), p(d), None, None, None, p(act), p(lp), env._stream())
        smp = lambda stride, params=par, obs=env._obs, a=act: lib.mz_policy_sample(h, p(params), stride, 5, 1, 1.0, 1, 2, p(obs), p(a), p(lp), env._stream())
        assert roll(0, npar5s) == MZ_ERR_ARG and b"n_steps" in lib.mz_last_error(h)
        assert roll(3, npar5) == MZ_ERR_ARG and b"stride" in lib.mz_last_error(h)  # the deterministic policy's stride
        assert smp(npar5) == MZ_ERR_ARG and b"stride" in lib.mz_last_error(h)
        assert roll(3, 0, params=None) == MZ_ERR_ARG and b"null" in lib.mz_last_error(h)
        assert roll(3, 0, obs=None) == MZ_ERR_ARG and roll(3, 0, r=None) == MZ_ERR_ARG and roll(3, 0, d=None) == MZ_ERR_ARG
        assert b"null" in lib.mz_last_error(h)
        assert smp(0, params=None) == MZ_ERR_ARG and smp(0, obs=None) == MZ_ERR_ARG and smp(0, a=None) == MZ_ERR_ARG
        assert roll(3, npar5s) == 0 and roll(3, 0) == 0 and smp(npar5s) == 0 and smp(0) == 0
        # logp is optional
        assert lib.mz_policy_sample(h, p(par), 0, 5, 1, 1.0, 1, 2, p(env._obs), p(act), None, env._stream()) == 0
        assert lib.mz_rollout_policy_sample(h, 3, p(par), 0, 5, 1, 1.0, 1, 2, p(env._obs), p(rew), p(done), None, None, None, None, None, env._stream()) == 0
        obs, rew1, done1, _ = env.step(z(n, nu))
        torch.cuda.synchronize()
        assert torch.isfinite(obs).all() and tuple(rew1.shape) == (n,)
    finally:
        env.close()


@pytest.mark.parametrize("env_id", ["PointUMaze-v0", "SwimmerUMaze-v0", "AntUMaze-v0"])
def test_nan_log_std_stays_in_its_env(env_id):
    import torch

    K, n, bad = 6, 130, 37
    ea, eb = (mm.make(env_id, num_envs=n, auto_reset=False, seed=1) for _ in range(2))
    try:
        ea.reset(seed=6); eb.reset(seed=6)
        pol = _spolicy(ea, True, 5, False, seed=3)
        dirty = dict(pol, params=pol["params"].clone())
        dirty["params"][bad, -1] = float("nan")  # log_std of the last unit of env `bad`
        _, rew_a, _, info_a = ea.rollout_policy_sample(steps=K, noise_seed=SEED, noise_step=STEP0, return_obs=True, return_actions=True, **pol)
        _, rew_b, _, info_b = eb.rollout_policy_sample(steps=K, noise_seed=SEED, noise_step=STEP0, return_obs=True, return_actions=True, **dirty)
        torch.cuda.synchronize()
        assert torch.isnan(info_b["actions"][:, bad, -1]).all() and torch.isnan(info_b["logp"][:, bad]).all()
        keep = torch.arange(n, device=ea.device) != bad
        for key in ("actions", "logp", "observations"):
            assert _same(info_a[key][:, keep].contiguous(), info_b[key][:, keep].contiguous()), key
        assert _same(rew_a[:, keep].contiguous(), rew_b[:, keep].contiguous())
        a1, l1 = eb.policy_sample(noise_seed=1, noise_step=1, obs=info_a["observations"][0].contiguous(), **dirty)
        assert torch.isnan(a1[bad, -1]) and torch.isnan(l1[bad]) and torch.isfinite(a1[keep]).all() and torch.isfinite(l1[keep]).all()
    finally:
        ea.close(); eb.close()
