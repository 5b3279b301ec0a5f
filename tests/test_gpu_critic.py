"""VecMazeEnv.value / gae and the critic of rollout_policy / rollout_policy_sample (mz_value, mz_gae, mz_rollout_actor_critic) on the
device.

`value` goes against mujoco_maze_amd.policy.value_reference (affine: by bits; tanh: the suite's 1e-5).  A rollout with a critic goes
against its defining loop on a twin env — same id, num_envs, seed, reset and injected states —

    values[k] = value(obs);  a = policy(obs);  obs, reward, done = step(a)
    next_values[k] = value(final_observation) where the env finished under auto-reset, value(obs) elsewhere

by bit patterns: the fused kernels run the unit functions of the stand-alone kernels on the same fp32 rows, so nothing may differ.
The helpers are those of tests/test_gpu_policy_rollout.py and tests/test_gpu_policy_sample.py."""
import ctypes as C

import numpy as np
import pytest

import mujoco_maze_amd as mm
from mujoco_maze_amd import _capi, policy
from tests.test_custom_task import FarGoalCross, RandomGoalCross
from tests.test_gpu_policy_rollout import KEYS, POLICIES, _assert_equal, _current_obs, _policy
from tests.test_gpu_policy_sample import SEED, STEP0, _spolicy
from tests.test_gpu_rollout import FUSED_IDS, _near_goal, _same
from tests.test_policy_api import random_policy
from tests.test_top_down_view import view_task

pytestmark = pytest.mark.gpu
MZ_ERR_ARG = -1
# (per-env parameters, hidden): one shared affine critic, and one tanh critic per env at a narrow and at the widest hidden layer
CRITICS = [(False, 0), (True, 5), (True, 64)]
CRITIC_IDS = ["shared-affine", "per-env-Hv5", "per-env-Hv64"]
MODES = [False, True]
MODE_IDS = ["deterministic", "sampled"]


def _critic(env, per_env, hidden, seed):
    """kwargs value_params / value_hidden of the rollouts, random parameters on the env's device"""
    import torch

    p = random_policy(np.random.default_rng(seed), env.obs_dim, 1, hidden, rows=env.num_envs if per_env else None)
    return dict(value_params=torch.as_tensor(p, device=env.device), value_hidden=hidden)


def _value(env, crt, obs=None):
    return env.value(crt["value_params"], obs=obs, hidden=crt["value_hidden"])


def _loop(env, pol, crt, K, sample):
    """the defining loop: the stacked rows, the last step's obs and info"""
    import torch

    keys = KEYS + ("values", "next_values") + (("logp",) if sample else ())
    rows = {k: [] for k in keys}
    for k in range(K):
        v = _value(env, crt)
        if sample:
            a, lp = env.policy_sample(noise_seed=SEED, noise_step=STEP0 + k, **pol)
        else:
            a = env.policy_act(**pol)
        obs, rew, done, info = env.step(a)
        nv = _value(env, crt)
        if env._auto_reset:
            nv = torch.where(done != 0, _value(env, crt, info["final_observation"]), nv)
        vals = (a, obs, rew, done, info["goal_index"], info["position"], info["reward_forward"], info["reward_ctrl"], v, nv) + ((lp,) if sample else ())
        for key, x in zip(keys, vals):
            rows[key].append(x.clone())
    return {k: torch.stack(v) for k, v in rows.items()}, obs, info


def _rollout(env, pol, crt, K, sample, **kw):
    if sample:
        return env.rollout_policy_sample(steps=K, noise_seed=SEED, noise_step=STEP0, return_obs=True, return_actions=True, **pol, **crt, **kw)
    return env.rollout_policy(steps=K, return_obs=True, return_actions=True, **pol, **crt, **kw)


def _make_policy(env, sample, spec, seed, drive):
    return _spolicy(env, *spec, seed=seed, drive=drive) if sample else _policy(env, *spec, seed=seed, drive=drive)


def _twin_check(make, K, crt_spec, sample, pol_spec=POLICIES[1], seed=11, point=False, prepare=None):
    """env A: the defining loop; env B: one rollout with a critic.  Returns (launch info of B, the loop's rows)."""
    import torch

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
        pol = _make_policy(ea, sample, pol_spec, seed + 1, point)
        crt = _critic(ea, *crt_spec, seed=seed + 2)
        want, obs_a, info_a = _loop(ea, pol, crt, K, sample)
        out_b = _rollout(eb, pol, crt, K, sample)
        _assert_equal(ea, eb, want, obs_a, info_a, out_b, K)
        info_b = out_b[3]
        n = ea.num_envs
        assert tuple(info_b["values"].shape) == tuple(info_b["next_values"].shape) == (K, n)
        assert _same(info_b["values"], want["values"]) and _same(info_b["next_values"], want["next_values"])
        if sample:
            assert _same(info_b["logp"], want["logp"])
        assert torch.isfinite(want["values"][0]).all()
        # one evaluation, stored twice, wherever the episode goes on ...
        if K > 1:
            on = want["done"][:-1] == 0
            nvb, vb = info_b["next_values"][:-1].contiguous().view(torch.int32), info_b["values"][1:].contiguous().view(torch.int32)
            assert torch.equal(nvb[on], vb[on])
            # ... and under auto-reset the value of the TERMINAL row, not of the new episode's first row, where it ended
            if ea._auto_reset:
                assert int((~on).sum()) > 0 and int((nvb[~on] != vb[~on]).sum()) > 0
            else:
                assert torch.equal(nvb, vb)
        return eb.launch_info(), want
    finally:
        ea.close(); eb.close()


# ---------------------------------------------------------------------------------------------- 1. value against the model
@pytest.mark.parametrize("env_id", ["PointUMaze-v0", "AntUMaze-v0"])
def test_value_against_the_model(env_id):
    import torch

    n = 130
    env = mm.make(env_id, num_envs=n, seed=3)
    try:
        env.reset(seed=4)
        g = torch.Generator(device=env.device).manual_seed(1)
        lo, hi = torch.as_tensor(env.action_space.low, device=env.device), torch.as_tensor(env.action_space.high, device=env.device)
        for _ in range(3):  # observations of moving robots
            obs, _, _, _ = env.step(lo + (hi - lo) * torch.rand((n, env.nu), device=env.device, generator=g))
        x = obs.cpu().numpy()
        rng = np.random.default_rng(7)
        for per_env in (True, False):
            p0 = random_policy(rng, env.obs_dim, 1, 0, rows=n if per_env else None)
            got = env.value(torch.as_tensor(p0, device=env.device)).cpu().numpy()
            want = policy.value_reference(p0, x)
            assert got.shape == (n,) and got.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32))
            # the same rows passed explicitly
            got2 = env.value(p0, obs=obs.clone()).cpu().numpy()
            assert np.array_equal(got2.view(np.int32), want.view(np.int32))
            for hidden in (5, 64):
                p = random_policy(rng, env.obs_dim, 1, hidden, rows=n if per_env else None)
                got = env.value(torch.as_tensor(p, device=env.device), hidden=hidden).cpu().numpy()
                err = np.abs(got.astype(np.float64) - policy.value_reference(p, x, hidden).astype(np.float64))
                print(f"{env_id} per-env {per_env} Hv {hidden}: max |device value - policy.value_reference| = {err.max():.3e}")
                assert err.max() < 1e-5
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------- 2. fused equals the defining loop
@pytest.mark.parametrize("sample", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("crt_spec", CRITICS, ids=CRITIC_IDS)
@pytest.mark.parametrize("env_id", FUSED_IDS)
def test_fused_actor_critic_equals_the_defining_loop(env_id, crt_spec, sample):
    """130 envs (idle groups in the last workgroup), auto-reset, K = 260: two launches — the second values the row the first left in the
    observation buffer again — and the 40-step time limit ends every episode several times"""
    point = env_id.startswith("Point")
    lb, want = _twin_check(lambda: mm.make(env_id, num_envs=130, auto_reset=True, seed=5, max_episode_steps=40), 260, crt_spec, sample, point=point)
    assert lb["rollout_fused"] == 1 and lb["engine"] == 0
    assert int((want["done"] & 2).sum()) > 0
    if point:
        assert int((want["done"] & 1).sum()) > 0  # goals were reached, not only time limits


@pytest.mark.parametrize("sample", MODES, ids=MODE_IDS)
def test_fused_actor_critic_at_32_lanes(sample):
    lb, want = _twin_check(lambda: mm.make("PointUMaze-v0", num_envs=130, auto_reset=True, seed=3, max_episode_steps=40), 260, CRITICS[1], sample,
                           point=True, prepare=lambda e: e.set_option("lanes_per_env", 32))
    assert lb["rollout_fused"] == 1 and lb["lanes_per_env"] == 32
    assert int((want["done"] & 1).sum()) > 0 and int((want["done"] & 2).sum()) > 0


@pytest.mark.parametrize("env_id", ["SwimmerUMaze-v0", "PointUMaze-v0"])
def test_fused_actor_critic_without_auto_reset(env_id):
    lb, want = _twin_check(lambda: mm.make(env_id, num_envs=130, auto_reset=False, seed=2, max_episode_steps=30), 260, CRITICS[1], True)
    assert lb["rollout_fused"] == 1 and int((want["done"] & 2).sum()) > 0


# ---------------------------------------------------------------------------------------------- 3. unfused handles
@pytest.mark.parametrize("sample", MODES, ids=MODE_IDS)
def test_unfused_ant(sample):
    lb, want = _twin_check(lambda: mm.make("AntUMaze-v0", num_envs=64, auto_reset=True, seed=4, max_episode_steps=8), 20, CRITICS[1], sample)
    assert lb["rollout_fused"] == 0 and int((want["done"] != 0).sum()) > 0


def test_unfused_general_engine():
    lb, want = _twin_check(lambda: mm.make("PointUMaze-v0", num_envs=32, engine="general", auto_reset=True, max_episode_steps=7), 12,
                           CRITICS[2], True, pol_spec=POLICIES[2], point=True)
    assert lb["rollout_fused"] == 0 and lb["engine"] == 1


def test_unfused_top_down_view():
    """the critic reads the view entries of both rows: the terminal row's are filled in final_observation by the step's view kernel"""
    from mujoco_maze_amd.maze_env import VecMazeEnv

    cls, scale = view_task("ViewPush")
    lb, want = _twin_check(lambda: VecMazeEnv(mm.PointEnv, cls, num_envs=64, maze_size_scaling=scale, auto_reset=True, max_episode_steps=6), 14,
                           CRITICS[1], True, point=True)
    assert lb["rollout_fused"] == 0 and int((want["done"] != 0).sum()) > 0


# ---------------------------------------------------------------------------------------------- 4. Python fallbacks
def test_python_loop_host_judged_task():
    from mujoco_maze_amd.maze_env import VecMazeEnv

    def make():
        env = VecMazeEnv(mm.PointEnv, FarGoalCross, maze_size_scaling=4.0, num_envs=48, auto_reset=True, max_episode_steps=6)
        assert env._host_rewards
        return env

    lb, want = _twin_check(make, 10, CRITICS[1], True, point=True)
    assert tuple(want["values"].shape) == (10, 48) and int((want["done"] != 0).sum()) > 0


def test_python_loop_per_env_goals_under_auto_reset():
    import torch

    from mujoco_maze_amd.maze_env import VecMazeEnv

    envs = []

    def make():
        env = VecMazeEnv(mm.PointEnv, RandomGoalCross, maze_size_scaling=4.0, num_envs=64, auto_reset=True, inner_reward_scaling=0.0,
                         max_episode_steps=6)
        envs.append(env)
        return env

    lb, want = _twin_check(make, 10, CRITICS[0], False, pol_spec=POLICIES[0], point=True)
    assert envs[0].env_goals is not None and torch.equal(envs[0].env_goals, envs[1].env_goals)
    assert int((want["done"] != 0).sum()) > 0


# ---------------------------------------------------------------------------------------------- 5. the critic is inert
@pytest.mark.parametrize("sample", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("env_id", ["PointUMaze-v0", "SwimmerUMaze-v0", "AntUMaze-v0"])
def test_the_critic_is_inert(env_id, sample):
    """env A: the rollout without a critic; env B: with one; env C: mz_rollout_actor_critic with critic = NULL straight through the
    C-ABI.  Everything the three share is equal by bits."""
    import torch

    point, n = env_id.startswith("Point"), 130
    K = 20 if env_id.startswith("Ant") else 260
    ea, eb, ec = (mm.make(env_id, num_envs=n, auto_reset=True, seed=5, max_episode_steps=8 if K == 20 else 40) for _ in range(3))
    try:
        for e in (ea, eb, ec):
            o = e.reset(seed=9)
            if point:
                _near_goal(e, o)
                _current_obs(e)
        pol = _make_policy(ea, sample, POLICIES[1], 10, point)
        crt = _critic(ea, True, 5, seed=12)
        none = dict(value_params=None, value_hidden=0)
        obs_a, rew_a, done_a, info_a = _rollout(ea, pol, none, K, sample)
        obs_b, rew_b, done_b, info_b = _rollout(eb, pol, crt, K, sample)
        assert "values" not in info_a and "values" in info_b
        # env C
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=ec.device)
        rew_c, done_c, goal_c, inf_c = z(K, n), z(K, n, dt=torch.uint8), z(K, n, dt=torch.int32), z(K, n, 4)
        oseq_c, act_c, logp_c = z(K, n, ec.obs_dim), z(K, n, ec.nu), z(K, n)
        par = pol["params"]
        rc = ec._lib.mz_rollout_actor_critic(ec._h, K, p(par), par.shape[-1] if par.dim() == 2 else 0, pol["hidden"], 1 if pol["squash"] else 0,
                                             float(pol["action_scale"]), 1 if sample else 0, SEED, STEP0, None, p(ec._obs), p(rew_c), p(done_c),
                                             p(goal_c), p(inf_c), p(oseq_c), p(act_c), p(logp_c) if sample else None, ec._stream())
        assert rc == 0, ec._lib.mz_last_error(ec._h)
        torch.cuda.synchronize()
        for obs_x, rew_x, done_x, act_x, oseq_x, goal_x, e in ((obs_b, rew_b, done_b, info_b["actions"], info_b["observations"], info_b["goal_index"], eb),
                                                               (ec._obs, rew_c, done_c, act_c, oseq_c, goal_c, ec)):
            assert _same(obs_a, obs_x) and _same(rew_a, rew_x) and _same(done_a, done_x)
            assert _same(info_a["actions"], act_x) and _same(info_a["observations"], oseq_x) and _same(info_a["goal_index"], goal_x)
            assert _same(ea._final_obs, e._final_obs)
            for x, y in zip(ea.get_state(), e.get_state()):
                assert _same(x, y)
        for key in ("position", "reward_forward", "reward_ctrl", "final_observation") + (("logp",) if sample else ()):
            assert _same(info_a[key], info_b[key]), key
        if sample:
            assert _same(info_a["logp"], logp_c)
        sa, sb, sc = ea.status(), eb.status(), ec.status()
        assert _same(sa, sb) and _same(sa, sc)
        assert int((done_a != 0).sum()) > 0
    finally:
        ea.close(); eb.close(); ec.close()


# ---------------------------------------------------------------------------------------------- 6. gae
@pytest.mark.parametrize("env_id", ["PointUMaze-v0", "AntUMaze-v0"])
def test_gae_of_a_device_rollout_against_the_model(env_id):
    import torch

    point, n = env_id.startswith("Point"), 130
    K = 20 if env_id.startswith("Ant") else 100
    env = mm.make(env_id, num_envs=n, auto_reset=True, seed=5, max_episode_steps=8 if K == 20 else 40)
    try:
        o = env.reset(seed=9)
        if point:
            _near_goal(env, o)
            _current_obs(env)
        pol = _spolicy(env, True, 5, True, seed=10, drive=point)
        crt = _critic(env, True, 5, seed=12)
        _, rew, done, info = _rollout(env, pol, crt, K, True, gae=(0.99, 0.95))
        torch.cuda.synchronize()
        r, d, v, nv = (t.cpu().numpy() for t in (rew, done, info["values"], info["next_values"]))
        assert (d & 2).any() and (not point or (d & 1).any())
        want_adv, want_ret = policy.gae_reference(r, d, v, nv, 0.99, 0.95)
        adv, ret = info["advantages"].cpu().numpy(), info["returns"].cpu().numpy()
        assert adv.shape == ret.shape == (K, n) and np.isfinite(adv).all()
        assert np.array_equal(adv.view(np.int32), want_adv.view(np.int32)) and np.array_equal(ret.view(np.int32), want_ret.view(np.int32))
        # the method on its own, other coefficients, and NaN next_values behind true terminations
        nv2 = info["next_values"].clone()
        nv2[(done & 1) != 0] = float("nan")
        adv2, ret2 = env.gae(rew, done, info["values"], nv2, gamma=0.9, lam=0.5)
        want2 = policy.gae_reference(r, d, v, nv2.cpu().numpy(), 0.9, 0.5)
        assert torch.isfinite(adv2).all()
        assert np.array_equal(adv2.cpu().numpy().view(np.int32), want2[0].view(np.int32))
        assert np.array_equal(ret2.cpu().numpy().view(np.int32), want2[1].view(np.int32))
        # K = 1, and K no multiple of the scan's load depth
        for k in (1, 13):
            a, _ = env.gae(rew[:k], done[:k], info["values"][:k], info["next_values"][:k])
            assert np.array_equal(a.cpu().numpy().view(np.int32), policy.gae_reference(r[:k], d[:k], v[:k], nv[:k])[0].view(np.int32))
        with pytest.raises(ValueError):
            env.gae(rew, done[:3], info["values"], info["next_values"])
        with pytest.raises(ValueError):
            env.rollout_policy_sample(steps=3, gae=(0.99, 0.95), **pol)  # advantages need a critic
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------- 7. refusals
def test_refusals():
    import torch

    env = mm.make("PointUMaze-v0", num_envs=16, auto_reset=True)
    try:
        env.reset(seed=1)
        n, nu, od, lib, h, dev = env.num_envs, env.nu, env.obs_dim, env._lib, env._h, env.device
        npar5, nvpar5 = policy.param_count(od, nu, 5), policy.param_count(od, 1, 5)
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
        with pytest.raises(ValueError):
            env.value(z(nvpar5 + 1), hidden=5)
        with pytest.raises(ValueError):
            env.value(z(nvpar5), hidden=65)
        with pytest.raises(ValueError):
            env.rollout_policy(z(npar5), steps=3, hidden=5, value_params=z(n, nvpar5 + 1), value_hidden=5)
        # straight through the C-ABI
        par, vpar, vals, nvals = z(n, npar5), z(n, nvpar5), z(3, n), z(3, n)
        rew, done = z(3, n), torch.zeros((3, n), dtype=torch.uint8, device=dev)
        p = lambda t: t.data_ptr() if t is not None else None

        def roll(sample=0, params=vpar, stride=nvpar5, hidden=5, reserved=0, nv=nvals):
            crt = _capi.MzCritic(p(params), stride, hidden, reserved, p(vals), p(nv))
            return lib.mz_rollout_actor_critic(h, 3, p(par), npar5, 5, 1, 1.0, sample, 1, 2, C.byref(crt), p(env._obs), p(rew), p(done), None, None,
                                               None, None, None, env._stream())

        err = lambda: lib.mz_last_error(h)
        assert roll(hidden=65) == MZ_ERR_ARG and b"critic" in err() and b"hidden" in err()
        assert roll(hidden=-1) == MZ_ERR_ARG and b"hidden" in err()
        assert roll(stride=nvpar5 - 1) == MZ_ERR_ARG and b"critic" in err() and b"env_stride" in err()
        assert roll(reserved=1) == MZ_ERR_ARG and b"reserved" in err()
        assert roll(sample=2) == MZ_ERR_ARG and b"sample" in err()
        assert roll(sample=-1) == MZ_ERR_ARG and b"sample" in err()
        assert roll(params=None) == MZ_ERR_ARG and b"critic" in err() and b"params_dev" in err()
        val = lambda params=vpar, stride=nvpar5, hidden=5, obs=env._obs, out=vals: lib.mz_value(h, p(params), stride, hidden, p(obs), p(out), env._stream())
        assert val(hidden=65) == MZ_ERR_ARG and b"hidden" in err()
        assert val(stride=3) == MZ_ERR_ARG and b"env_stride" in err()
        assert val(params=None) == MZ_ERR_ARG and val(obs=None) == MZ_ERR_ARG and val(out=None) == MZ_ERR_ARG
        assert lib.mz_gae(h, 0, p(rew), p(done), p(vals), p(nvals), 0.99, 0.95, p(vals), None, env._stream()) == MZ_ERR_ARG and b"n_steps" in err()
        assert lib.mz_gae(h, 3, p(rew), p(done), p(vals), None, 0.99, 0.95, p(vals), None, env._stream()) == MZ_ERR_ARG and b"null" in err()
        # auto-reset on, next values requested, no final_obs buffer bound: refused on every handle, fused or not
        assert lib.mz_bind_final_obs(h, None) == 0
        assert roll() == MZ_ERR_ARG and b"final_obs" in err() and b"next_value_seq_dev" in err()
        assert roll(nv=None) == 0  # values alone need no terminal row
        assert lib.mz_bind_final_obs(h, p(env._final_obs)) == 0
        assert roll() == 0 and roll(stride=0) == 0 and val() == 0 and val(stride=0) == 0
        assert roll(sample=1, stride=0) == MZ_ERR_ARG and b"param_env_stride" in err()  # the actor's vector lacks log_std
        # afterwards the env still steps
        obs, rew1, done1, _ = env.step(z(n, nu))
        torch.cuda.synchronize()
        assert torch.isfinite(obs).all() and tuple(rew1.shape) == (n,)
    finally:
        env.close()


def test_refusal_without_final_obs_on_an_unfused_handle():
    import torch

    env = mm.make("AntUMaze-v0", num_envs=8, auto_reset=True)
    try:
        env.reset(seed=1)
        n, lib, h, dev = env.num_envs, env._lib, env._h, env.device
        npar, nvpar = policy.param_count(env.obs_dim, env.nu, 0), policy.param_count(env.obs_dim, 1, 0)
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
        par, vpar, vals, nvals, rew, done = z(npar), z(nvpar), z(2, n), z(2, n), z(2, n), torch.zeros((2, n), dtype=torch.uint8, device=dev)
        crt = _capi.MzCritic(vpar.data_ptr(), 0, 0, 0, vals.data_ptr(), nvals.data_ptr())
        roll = lambda: lib.mz_rollout_actor_critic(h, 2, par.data_ptr(), 0, 0, 0, 1.0, 0, 0, 0, C.byref(crt), env._obs.data_ptr(), rew.data_ptr(),
                                                   done.data_ptr(), None, None, None, None, None, env._stream())
        assert env.launch_info()["rollout_fused"] == 0
        assert lib.mz_bind_final_obs(h, None) == 0
        assert roll() == MZ_ERR_ARG and b"final_obs" in lib.mz_last_error(h)
        assert lib.mz_bind_final_obs(h, env._final_obs.data_ptr()) == 0
        assert roll() == 0
        torch.cuda.synchronize()
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------- 8. NaN isolation
@pytest.mark.parametrize("env_id", ["PointUMaze-v0", "SwimmerUMaze-v0", "AntUMaze-v0"])
def test_nan_critic_parameters_stay_in_their_env(env_id):
    import torch

    K, n, bad = 6, 130, 37
    ea, eb = (mm.make(env_id, num_envs=n, auto_reset=True, seed=1, max_episode_steps=4) for _ in range(2))
    try:
        ea.reset(seed=6); eb.reset(seed=6)
        pol = _spolicy(ea, True, 5, True, seed=3)
        crt = _critic(ea, True, 5, seed=4)
        dirty = dict(crt, value_params=crt["value_params"].clone())
        dirty["value_params"][bad, 2] = float("nan")  # a first-layer weight of env `bad`
        _, rew_a, done_a, info_a = _rollout(ea, pol, crt, K, True, gae=(0.99, 0.95))
        _, rew_b, done_b, info_b = _rollout(eb, pol, dirty, K, True, gae=(0.99, 0.95))
        torch.cuda.synchronize()
        assert torch.isnan(info_b["values"][:, bad]).all() and torch.isnan(info_b["next_values"][:, bad]).all()
        keep = torch.arange(n, device=ea.device) != bad
        for key in ("values", "next_values", "advantages", "returns"):
            assert torch.isfinite(info_b[key][:, keep]).all(), key
            assert _same(info_a[key][:, keep].contiguous(), info_b[key][:, keep].contiguous()), key
        # ... and nothing but the values sees it
        for key in ("actions", "logp", "observations", "final_observation"):
            assert _same(info_a[key], info_b[key]), key
        assert _same(rew_a, rew_b) and _same(done_a, done_b) and int((done_a != 0).sum()) > 0
        v1 = eb.value(dirty["value_params"], hidden=5)
        assert torch.isnan(v1[bad]) and torch.isfinite(v1[keep]).all()
    finally:
        ea.close(); eb.close()
