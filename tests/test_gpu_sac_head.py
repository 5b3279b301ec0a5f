"""Stochastic actors with a state-dependent log-std head on the device (policy_sample / rollout_policy_sample with log_std="state";
mz_net_sample_head / mz_rollout_head).

A rollout goes against its defining loop on a twin env — same id, num_envs, seed, reset and injected states —

    [value]; a, logp = policy_sample(log_std="state", noise_step + k); obs, reward, done, info = step(a); [value of the terminal / new row]

by bit patterns: actions, logp, rewards, dones, observations, next observations, values, get_state() and the status words afterwards,
and a second call that continues where the first stopped.  The fused kernels of the Point, Swimmer and Reacher evaluate the head
with the unit functions the stand-alone kernel runs (chains of five or six links, like every unfused handle, run the loop inside the
call), so nothing may differ.  The single draw goes against the existing entries by bits where the head is a
constant or switched off, and against the numpy model at the bars of tests/test_gpu_transitions.py (actions) and of
tests/test_sac_head_api.py (logp), whose helpers these are."""
import ctypes as C

import numpy as np
import pytest

import mujoco_maze_amd as mm
from mujoco_maze_amd import _capi, policy
from tests.test_custom_task import FarGoalCross
from tests.test_deep_policy_api import random_net
from tests.test_gpu_deep_policy import _critic as _deep_critic
from tests.test_gpu_deep_policy import _moving_obs, _view_env
from tests.test_gpu_policy_rollout import ACTION_SCALE, _current_obs
from tests.test_gpu_policy_sample import SEED, STEP0
from tests.test_gpu_rollout import _near_goal, _same
from tests.test_gpu_transitions import _bufs, _p, _same_state
from tests.test_mjcf import chain_swimmer_xml
from tests.test_sac_head_api import BOUNDS, constant_head, f64_head_and_bounds

pytestmark = pytest.mark.gpu
MZ_ERR_ARG = -1
FUSED = ["PointUMaze-v0", "SwimmerUMaze-v0", "ReacherUMaze-v0", "PointPush-v0"]
# (per env, hidden, activation): per-env ReLU (64, 64) actors and a shared tanh-5 actor
ACTORS = {"relu64-per-env": (True, (64, 64), "relu"), "tanh5-shared": (False, 5, "tanh")}
KEYS = ("act", "logp", "obs", "next_obs", "reward", "done", "goal", "pos", "fwd", "ctrl", "values", "next_values")
INFO_OF = {"act": "actions", "logp": "logp", "obs": "observations", "next_obs": "next_observations", "goal": "goal_index", "pos": "position",
           "fwd": "reward_forward", "ctrl": "reward_ctrl", "values": "values", "next_values": "next_values"}


def _head_actor(env, per_env, hidden, activation, seed, squashed_logp, drive=False, bounds=BOUNDS):
    """kwargs of policy_sample / rollout_policy_sample for a random head actor on the env's device: squashed to ACTION_SCALE (0.9, no
    power of two), raw log-stds around -1 (biases U(-1.5, -0.5) on small weights).  `drive` (Point family): a small output layer and a
    bias on the first mean that drives forward, so that the robots run into walls and goals."""
    import torch

    rng = np.random.default_rng(seed)
    nu = env.nu
    p = random_net(rng, env.obs_dim, 2 * nu, hidden, rows=env.num_envs if per_env else None)
    widths = policy.net_shape(hidden)[0]
    last = 2 * nu + (widths[-1] if widths else env.obs_dim) * 2 * nu  # the output layer: its weights and biases
    p[..., -last:] *= 0.1
    if drive:
        p[..., -2 * nu] = 2.0
    p[..., -nu:] += rng.uniform(-1.5, -0.5, p.shape[:-1] + (nu,)).astype(np.float32)
    return dict(params=torch.as_tensor(p, device=env.device), hidden=hidden, squash=True, action_scale=ACTION_SCALE, activation=activation,
                log_std="state", log_std_bounds=bounds, squashed_logp=squashed_logp)


def _value(env, crt, obs=None):
    return env.value(crt["value_params"], obs=obs, hidden=crt["value_hidden"], activation=crt["value_activation"])


def _loop(env, K, pol, crt, step0=STEP0):
    """the defining loop: the stacked rows, the last step's obs and info"""
    import torch

    rows = {}
    for k in range(K):
        r = {}
        if crt:
            r["values"] = _value(env, crt)
        a, r["logp"] = env.policy_sample(noise_seed=SEED, noise_step=step0 + k, **pol)
        obs, rew, done, info = env.step(a)
        fin = (done != 0) if env._auto_reset else None
        r["next_obs"] = torch.where(fin.unsqueeze(1), info["final_observation"], obs) if env._auto_reset else obs
        if crt:
            nv = _value(env, crt)
            r["next_values"] = torch.where(fin, _value(env, crt, info["final_observation"]), nv) if env._auto_reset else nv
        r.update(act=a, obs=obs, reward=rew, done=done, goal=info["goal_index"], pos=info["position"], fwd=info["reward_forward"],
                 ctrl=info["reward_ctrl"])
        for key, x in r.items():
            rows.setdefault(key, []).append(x.clone())
    return {k: torch.stack(v) for k, v in rows.items()}, obs, info


def _call(env, K, pol, crt, step0=STEP0, return_next_obs=True):
    return env.rollout_policy_sample(steps=K, noise_seed=SEED, noise_step=step0, return_obs=True, return_actions=True, return_next_obs=return_next_obs,
                                     **pol, **(crt or {}))


def _out(out, key):
    obs, rew, done, info = out
    return rew if key == "reward" else (done if key == "done" else info.get(INFO_OF[key]))


def _assert_call_equals_loop(ea, eb, want, obs_a, info_a, out_b):
    for key in KEYS:
        if key in want:
            got = _out(out_b, key)
            assert got is not None and _same(got.contiguous(), want[key]), key
    assert _same(out_b[0], obs_a)
    if ea._auto_reset:
        assert _same(out_b[3]["final_observation"], info_a["final_observation"])
    return _same_state(ea, eb)


def _head_check(make, K, actor, squashed_logp, critic=False, seed=11, point=False, prepare=None, K2=3, fused=None, expect_done=True):
    """env A: the defining loop; env B: one call; then K2 more steps on both, B in a second call that continues.  Returns (the loop's
    rows, the first call's output, the actor, the critic, B's status words after the first call)."""
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
        pol = _head_actor(ea, *actor, seed=seed + 1, squashed_logp=squashed_logp, drive=point)
        crt = _deep_critic(ea, True, (64, 64), "relu", seed + 2) if critic else None
        want, obs_a, info_a = _loop(ea, K, pol, crt)
        out_b = _call(eb, K, pol, crt)
        torch.cuda.synchronize()
        if fused is not None:
            assert eb.launch_info()["rollout_fused"] == fused
        status = _assert_call_equals_loop(ea, eb, want, obs_a, info_a, out_b)
        assert torch.isfinite(want["act"]).all() and torch.isfinite(want["logp"]).all() and float(want["act"].abs().max()) <= ACTION_SCALE
        if expect_done:
            assert int((want["done"] != 0).sum()) > 0
        first = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in out_b[3].items()}
        out_first = (out_b[0].clone(), out_b[1].clone(), out_b[2].clone(), first)
        # the second call continues: the noise at STEP0 + K, the observation buffer and the state where the first left them
        want2, obs_a2, info_a2 = _loop(ea, K2, pol, crt, step0=STEP0 + K)
        out_b2 = _call(eb, K2, pol, crt, step0=STEP0 + K)
        torch.cuda.synchronize()
        _assert_call_equals_loop(ea, eb, want2, obs_a2, info_a2, out_b2)
        return want, out_first, pol, crt, status
    finally:
        ea.close(); eb.close()


# ---------------------------------------------------------------------------------------------- 1. the fused kernels
@pytest.mark.parametrize("squashed_logp", [False, True], ids=["logp-z", "logp-action"])
@pytest.mark.parametrize("actor", list(ACTORS))
@pytest.mark.parametrize("env_id", FUSED)
def test_fused_rollout_equals_the_defining_loop(env_id, actor, squashed_logp):
    """130 envs: no multiple of the envs per wave, idle groups run; K = 260 crosses the 256-step split of the launches;
    max_episode_steps = 40 resets every env six times"""
    point = env_id.startswith("Point")
    want, out, pol, _, _ = _head_check(lambda: mm.make(env_id, num_envs=130, auto_reset=True, seed=5, max_episode_steps=40), 260, ACTORS[actor],
                                       squashed_logp, point=point, fused=1)
    assert int((want["done"] != 0).sum(dim=0).min()) >= 6


@pytest.mark.parametrize("env_id", FUSED)
def test_fused_one_env_one_step(env_id):
    point = env_id.startswith("Point")
    _head_check(lambda: mm.make(env_id, num_envs=1, force_vec=True, auto_reset=True, seed=5, max_episode_steps=1), 1, ACTORS["relu64-per-env"], True,
                point=point, fused=1, K2=1)


@pytest.mark.parametrize("env_id", ["PointUMaze-v0", "SwimmerUMaze-v0"])
def test_fused_with_critic_normaliser_and_next_observations(env_id):
    """a ReLU (64, 64) critic, a bound normaliser (clip = 5) and return_next_obs compose with the head; a third env runs the call on
    the same binding without the critic and the extra rows: nothing else the call returns may change"""
    import torch

    point = env_id.startswith("Point")

    def prepare(env):
        rng = np.random.default_rng(3)
        env.bind_obs_norm(torch.as_tensor(rng.normal(0.0, 0.3, env.obs_dim).astype(np.float32), device=env.device),
                          torch.as_tensor(rng.uniform(0.5, 2.0, env.obs_dim).astype(np.float32), device=env.device), 5.0)

    make = lambda: mm.make(env_id, num_envs=130, auto_reset=True, seed=5, max_episode_steps=20)
    K = 45
    want, out, pol, crt, status = _head_check(make, K, ACTORS["relu64-per-env"], True, critic=True, point=point, prepare=prepare, fused=1)
    # the rows stay raw, and the critic valued the terminal rows
    fin = out[2] != 0
    nb, sb = out[3]["next_observations"].view(torch.int32), out[3]["observations"].view(torch.int32)
    assert torch.equal(nb[~fin], sb[~fin]) and int((nb[fin] != sb[fin]).any(dim=-1).sum()) > 0
    ec = make()
    try:
        prepare(ec)
        o = ec.reset(seed=11)
        if point:
            _near_goal(ec, o)
            _current_obs(ec)
        out_c = _call(ec, K, pol, None, return_next_obs=False)
        torch.cuda.synchronize()
        assert set(out_c[3]) == set(out[3]) - {"next_observations", "values", "next_values"}
        assert _same(out[0], out_c[0]) and _same(out[1], out_c[1]) and _same(out[2], out_c[2])
        for key in out_c[3]:
            assert _same(out[3][key].contiguous(), out_c[3][key].contiguous()), key
    finally:
        ec.close()
    # without the binding the actions are others: the normaliser is what the actor read
    ed = make()
    try:
        o = ed.reset(seed=11)
        if point:
            _near_goal(ed, o)
            _current_obs(ed)
        out_d = _call(ed, 1, pol, None, return_next_obs=False)
        assert not _same(out_d[3]["actions"][0].contiguous(), out[3]["actions"][0].contiguous())
    finally:
        ed.close()


# ---------------------------------------------------------------------------------------------- 2. the handles that run the loop inside the call
@pytest.mark.parametrize("squashed_logp", [False, True], ids=["logp-z", "logp-action"])
def test_unfused_ant(squashed_logp):
    """nu = 8: an output layer of 16 units"""
    _head_check(lambda: mm.make("AntUMaze-v0", num_envs=64, auto_reset=True, seed=4, max_episode_steps=8), 20, ACTORS["relu64-per-env"], squashed_logp,
                critic=squashed_logp, fused=0)


def test_unfused_general_engine():
    make = lambda: mm.make("PointUMaze-v0", num_envs=32, engine="general", auto_reset=True, max_episode_steps=7)
    _head_check(make, 12, ACTORS["tanh5-shared"], True, point=True, fused=0)


def test_unfused_top_down_view():
    _head_check(lambda: _view_env(64, auto_reset=True, max_episode_steps=6), 14, ACTORS["relu64-per-env"], True, point=True, fused=0)


@pytest.mark.parametrize("nlink", [4, 5, 6])
def test_user_chains(nlink):
    """user chains (the generator of tests/test_mjcf.py, which the planar ladder's tests use): four links sample inside the fused kernel
    <4, 0, 4>; five- and six-link chains are fused handles whose head plans run the defining loop inside the call (rollout_run)"""
    make = lambda: mm.make("SwimmerUMaze-v0", num_envs=66, robot_xml=chain_swimmer_xml(nlink), auto_reset=True, seed=5, max_episode_steps=9)
    _head_check(make, 20, ACTORS["relu64-per-env"], True, critic=True, fused=1)


def test_python_fallback_host_judged_task():
    from mujoco_maze_amd.maze_env import VecMazeEnv

    def make():
        env = VecMazeEnv(mm.PointEnv, FarGoalCross, maze_size_scaling=4.0, num_envs=48, auto_reset=True, max_episode_steps=6)
        assert env._host_rewards
        return env

    _head_check(make, 10, ACTORS["tanh5-shared"], True, critic=True, point=True)


# ---------------------------------------------------------------------------------------------- 3. one draw against the existing entries
@pytest.mark.parametrize("env_id", ["PointUMaze-v0", "AntUMaze-v0"])
def test_constant_head_and_switched_off_head_are_the_existing_entries_by_bits(env_id):
    import torch

    n = 130
    env = mm.make(env_id, num_envs=n, seed=3)
    try:
        obs = _moving_obs(env)
        od, nu = env.obs_dim, env.nu
        rng = np.random.default_rng(5)
        t = lambda a: torch.as_tensor(a, device=env.device)
        for hidden, activation in ((0, "tanh"), (5, "tanh"), ((5, 3), "relu"), ((64, 64), "relu")):
            for per_env in (True, False):
                net = random_net(rng, od, nu, hidden, rows=n if per_env else None)
                kw = dict(hidden=hidden, activation=activation, noise_seed=SEED, noise_step=STEP0)
                # zero weights into the log-std units, a bias inside the bounds: policy_sample with log_std = b behind the network
                b = rng.uniform(-1.5, 0.5, net.shape[:-1] + (nu,)).astype(np.float32)
                for squash in (False, True):
                    a, lp = env.policy_sample(t(constant_head(net, od, nu, hidden, b)), log_std="state", squash=squash, action_scale=ACTION_SCALE, **kw)
                    ra, rlp = env.policy_sample(t(np.concatenate([net, b], axis=-1)), squash=squash, action_scale=ACTION_SCALE, **kw)
                    assert _same(a, ra) and _same(lp, rlp) and torch.isfinite(a).all() and torch.isfinite(lp).all()
                # biases +-50 are the clamp's ends
                sign = np.where(np.arange(nu) % 2 == 0, 1.0, -1.0).astype(np.float32)
                a, lp = env.policy_sample(t(constant_head(net, od, nu, hidden, 50.0 * sign)), log_std="state", squash=True, squashed_logp=True, **kw)
                ra, rlp = env.policy_sample(t(constant_head(net, od, nu, hidden, np.where(sign > 0, 2.0, -20.0))), log_std="state", squash=True,
                                            squashed_logp=True, **kw)
                assert _same(a, ra) and _same(lp, rlp) and torch.isfinite(lp).all()
                # bounds (-inf, 2) with a bias of -inf: the deterministic actor on the means' columns
                head = constant_head(net, od, nu, hidden, -np.inf)
                for squash in (False, True):
                    a, lp = env.policy_sample(t(head), log_std="state", log_std_bounds=(-np.inf, 2.0), squash=squash, action_scale=ACTION_SCALE, **kw)
                    want = env.policy_act(t(policy.mean_actor(head, od, nu, hidden)), obs, hidden, squash, ACTION_SCALE, activation)
                    assert not bool(((want == 0) & torch.signbit(want)).any())
                    assert _same(a, want) and bool(torch.isposinf(lp).all())
    finally:
        env.close()


@pytest.mark.parametrize("env_id", ["PointUMaze-v0", "AntUMaze-v0"], ids=["fused", "unfused"])
def test_a_null_head_is_the_existing_entries_by_bits(env_id):
    import torch

    point, K, n = env_id.startswith("Point"), 20, 64
    envs = [mm.make(env_id, num_envs=n, auto_reset=True, seed=5, max_episode_steps=8) for _ in range(2)]
    try:
        for e in envs:
            o = e.reset(seed=3)
            if point:
                _near_goal(e, o)
                _current_obs(e)
        e0, e1 = envs
        lib = e0._lib
        rng = np.random.default_rng(21)
        par = torch.as_tensor(random_net(rng, e0.obs_dim, e0.nu, (64, 64), rows=n, log_std=True), device=e0.device)
        vpar = torch.as_tensor(random_net(rng, e0.obs_dim, 1, (5, 3), rows=n), device=e0.device)
        actor = lambda: _capi.make_net(_p(par), par.shape[1], (64, 64), _capi.ACT_RELU, True, ACTION_SCALE)
        critic = lambda: _capi.make_net(_p(vpar), vpar.shape[1], (5, 3), _capi.ACT_RELU)
        # mz_net_sample against mz_net_sample_head with head == NULL, in both noise modes
        for mode in (_capi.NOISE_PRE_SQUASH, _capi.NOISE_ACTION):
            outs = []
            for e, head_entry in ((e0, False), (e1, True)):
                a, lp = torch.zeros((n, e.nu), device=e.device), torch.zeros(n, device=e.device)
                net, nz = actor(), _capi.make_noise(mode, SEED, STEP0)
                if head_entry:
                    rc = lib.mz_net_sample_head(e._h, C.byref(net), None, C.byref(nz), _p(e._obs), _p(a), _p(lp), e._stream())
                else:
                    rc = lib.mz_net_sample(e._h, C.byref(net), C.byref(nz), _p(e._obs), _p(a), _p(lp), e._stream())
                assert rc == 0, lib.mz_last_error(e._h)
                outs.append((a, lp))
            torch.cuda.synchronize()
            assert _same(outs[0][0], outs[1][0]) and _same(outs[0][1], outs[1][1]) and torch.isfinite(outs[0][0]).all()
        # mz_rollout_ex against mz_rollout_head with head == NULL: an actor with a trailing log_std, a critic, the extra rows
        bufs = []
        for e, head_entry in ((e0, False), (e1, True)):
            b = _bufs(e, K)
            b["next"] = torch.zeros((K, n, e.obs_dim), device=e.device)
            io = _capi.make_rollout_io(K, actor=actor(), noise=_capi.make_noise(_capi.NOISE_ACTION, SEED, STEP0), critic=critic(), obs_dev=_p(e._obs),
                                       reward_dev=_p(b["reward"]), done_dev=_p(b["done"]), goal_idx_dev=_p(b["goal"]), info_dev=_p(b["info"]),
                                       obs_seq_dev=_p(b["obs_seq"]), actions_seq_dev=_p(b["act"]), logp_seq_dev=_p(b["logp"]),
                                       value_seq_dev=_p(b["values"]), next_value_seq_dev=_p(b["next_values"]), next_obs_seq_dev=_p(b["next"]))
            rc = lib.mz_rollout_head(e._h, C.byref(io), None, e._stream()) if head_entry else lib.mz_rollout_ex(e._h, C.byref(io), e._stream())
            assert rc == 0, lib.mz_last_error(e._h)
            bufs.append(b)
        torch.cuda.synchronize()
        for key in bufs[0]:
            assert _same(bufs[0][key], bufs[1][key]), key
        assert _same(e0._obs, e1._obs) and int((bufs[0]["done"] != 0).sum()) > 0
        _same_state(e0, e1)
    finally:
        for e in envs:
            e.close()


def test_noise_is_keyed_by_the_global_slot():
    """the same shared actor and observations on 130 envs and on 64: the first 64 rows agree by bits"""
    import torch

    big, small = mm.make("PointUMaze-v0", num_envs=130, seed=3), mm.make("PointUMaze-v0", num_envs=64, seed=3)
    try:
        obs = _moving_obs(big)
        pol = _head_actor(big, False, (64, 64), "relu", 9, True)
        a, lp = big.policy_sample(obs=obs, noise_seed=SEED, noise_step=STEP0, **pol)
        b, lq = small.policy_sample(obs=obs[:64].contiguous(), noise_seed=SEED, noise_step=STEP0, **pol)
        assert _same(a[:64].contiguous(), b) and _same(lp[:64].contiguous(), lq) and torch.isfinite(a).all()
        c, _ = big.policy_sample(obs=obs, noise_seed=SEED, noise_step=STEP0 + 1, **pol)
        assert not _same(a, c)
    finally:
        big.close(); small.close()


# ---------------------------------------------------------------------------------------------- 4. against the numpy model
@pytest.mark.parametrize("env_id", ["PointUMaze-v0", "AntUMaze-v0"])
def test_device_against_the_model(env_id):
    """actions at the bar tests/test_gpu_transitions.py holds sampled squashed actions to (1e-5: the suite's bar on eps with s <= 1, the
    device's libm behind it), logp inside the bound tests/test_sac_head_api.py derives / measures, on the device's own rows"""
    import torch

    n = 130
    env = mm.make(env_id, num_envs=n, seed=3)
    try:
        obs = _moving_obs(env)
        x = obs.cpu().numpy()
        od, nu = env.obs_dim, env.nu
        slots = np.arange(n)
        eps = policy.noise(9, 4, slots, nu).astype(np.float64)
        rng = np.random.default_rng(7)
        worst = 0.0
        for per_env in (True, False):
            for hidden, activation in ((0, "tanh"), (5, "tanh"), ((5, 3), "relu"), ((64, 64), "relu")):
                par = random_net(rng, od, 2 * nu, hidden, rows=n if per_env else None)
                par[..., -nu:] += rng.uniform(-3.0, 1.0, par.shape[:-1] + (nu,)).astype(np.float32)
                for bounds, squashed in (((-2.0, 0.0), False), ((-2.0, 0.0), True), (BOUNDS, True)):
                    kw = dict(hidden=hidden, activation=activation, squash=True, action_scale=0.5, noise_seed=9, noise_step=4)
                    got, glp = env.policy_sample(torch.as_tensor(par, device=env.device), obs=obs, log_std="state", log_std_bounds=bounds,
                                                 squashed_logp=squashed, **kw)
                    ref, rlp = policy.sample_reference(par, x, nu, slots=slots, log_std="state", log_std_bounds=bounds, squashed_logp=squashed, **kw)
                    got, glp = got.cpu().numpy(), glp.cpu().numpy()
                    val, e_a, lp64, e_lp, _ = f64_head_and_bounds(par, x, nu, hidden, activation, True, 0.5, bounds, squashed, eps)
                    err = np.abs(got.astype(np.float64) - ref).max()
                    el = np.abs(glp.astype(np.float64) - lp64)
                    worst = max(worst, float((el / e_lp).max()))
                    print(f"{env_id} per_env {per_env} hidden {hidden} {activation} bounds {bounds} squashed_logp {squashed}: max |action - model| = "
                          f"{err:.3e}, max |logp - float64| = {el.max():.3e} (bound {e_lp[el.argmax()]:.3e}), |logp - model| = "
                          f"{np.abs(glp.astype(np.float64) - rlp).max():.3e}")
                    assert np.isfinite(glp).all() and float(np.abs(got).max()) <= 0.5
                    if bounds[1] <= 0.0:  # s <= 1: the bar of the sampled squashed actions
                        assert err <= 1e-5
                    assert np.all(np.abs(got.astype(np.float64) - val) <= e_a)
                    assert np.all(el <= e_lp)
        print(f"{env_id}: worst logp error / bound = {worst:.3f}")
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------- 5. isolation
@pytest.mark.parametrize("env_id", ["PointUMaze-v0", "AntUMaze-v0"], ids=["fused", "unfused"])
def test_nan_parameters_stay_in_their_env(env_id):
    import torch

    n, K, bad_env = 66, 6, 7
    ea, eb = (mm.make(env_id, num_envs=n, auto_reset=True, seed=5, max_episode_steps=4) for _ in range(2))
    try:
        ea.reset(seed=6); eb.reset(seed=6)
        pol = _head_actor(ea, True, (64, 64), "relu", 13, True)
        bad = dict(pol, params=pol["params"].clone())
        bad["params"][bad_env, :] = float("nan")
        kw = dict(steps=K, noise_seed=SEED, noise_step=STEP0, return_actions=True, return_obs=True, return_next_obs=True)
        oa, ra, da, ia = ea.rollout_policy_sample(**pol, **kw)
        ob, rb, db, ib = eb.rollout_policy_sample(**bad, **kw)
        torch.cuda.synchronize()
        keep = torch.arange(n, device=ea.device) != bad_env
        assert bool(torch.isnan(ib["actions"][:, bad_env]).all()) and bool(torch.isnan(ib["logp"][:, bad_env]).all())
        for x, y in ((ia["actions"], ib["actions"]), (ia["logp"], ib["logp"]), (ra, rb), (da, db), (ia["observations"], ib["observations"]),
                     (ia["next_observations"], ib["next_observations"])):
            assert _same(x[:, keep].contiguous(), y[:, keep].contiguous())
        assert _same(oa[keep].contiguous(), ob[keep].contiguous())
        for x, y in zip(ea.get_state(), eb.get_state()):
            assert _same(x[keep].contiguous(), y[keep].contiguous())
    finally:
        ea.close(); eb.close()


# ---------------------------------------------------------------------------------------------- 6. refusals
@pytest.mark.parametrize("env_id", ["PointUMaze-v0", "AntUMaze-v0"], ids=["fused", "unfused"])
def test_refusals_name_the_argument_and_leave_the_handle_as_it_was(env_id):
    import torch

    K, n = 3, 16
    env, twin = (mm.make(env_id, num_envs=n, auto_reset=True, seed=1) for _ in range(2))
    try:
        env.reset(seed=1); twin.reset(seed=1)
        lib, h = env._lib, env._h
        b = _bufs(env, K)
        acts = torch.zeros((K, n, env.nu), device=env.device)
        count = policy.param_count(env.obs_dim, env.nu, 0, log_std="state")
        par = torch.zeros(count, device=env.device)
        actor = lambda squash=True: _capi.make_net(_p(par), 0, (), _capi.ACT_TANH, squash, ACTION_SCALE)
        noise = lambda mode=_capi.NOISE_PRE_SQUASH: _capi.make_noise(mode, 1, 2)
        head = lambda **kw: _capi.make_head(kw.pop("lo", -20.0), kw.pop("hi", 2.0), kw.pop("squashed", True))
        base = dict(obs_dev=_p(env._obs), reward_dev=_p(b["reward"]), done_dev=_p(b["done"]))
        out, lp = torch.zeros((n, env.nu), device=env.device), torch.zeros(n, device=env.device)

        def refused(word, hd=None, actor_=None, noise_=None, sample_only=False, rollout_only=False, io=None):
            """through both entries: the head `hd` with the actor and the noise given (defaults: valid ones)"""
            hd = head() if hd is None else hd
            a = actor() if actor_ is None else actor_
            nz = noise() if noise_ is None else noise_
            if not rollout_only:
                rc = lib.mz_net_sample_head(h, C.byref(a) if a != "null" else None, C.byref(hd), C.byref(nz) if nz != "null" else None, _p(env._obs),
                                            _p(out), _p(lp), env._stream())
                assert rc == MZ_ERR_ARG and word in lib.mz_last_error(h), (word, rc, lib.mz_last_error(h))
                assert lib.mz_last_error(h).startswith(b"mz_net_sample_head:"), lib.mz_last_error(h)  # the entry the caller used
            if not sample_only:
                io = io or _capi.make_rollout_io(K, actor=None if a == "null" else a, noise=None if nz == "null" else nz, **base)
                rc = lib.mz_rollout_head(h, C.byref(io), C.byref(hd), env._stream())
                assert rc == MZ_ERR_ARG and word in lib.mz_last_error(h), (word, rc, lib.mz_last_error(h))
                assert lib.mz_last_error(h).startswith(b"mz_rollout_head:"), lib.mz_last_error(h)

        hd = head(); hd.struct_size += 8
        refused(b"head->struct_size", hd)
        hd = head(); hd.struct_size -= 8
        refused(b"head->struct_size", hd)
        hd = head(); hd.kind = 0
        refused(b"head->kind", hd)
        hd = head(); hd.kind = 2
        refused(b"head->kind", hd)
        hd = head(); hd.reserved = 1
        refused(b"head->reserved", hd)
        hd = head(); hd.logp_squashed = 2
        refused(b"head->logp_squashed", hd)
        hd = head(); hd.logp_squashed = -1
        refused(b"head->logp_squashed", hd)
        refused(b"squash", head(squashed=True), actor_=actor(False))  # the density of the squashed action needs a squash
        refused(b"NaN", head(lo=float("nan")))
        refused(b"NaN", head(hi=float("nan")))
        refused(b"log_std_min", head(lo=1.0, hi=-1.0))
        refused(b"noise", noise_="null", sample_only=True)  # a head samples
        refused(b"noise", noise_="null", rollout_only=True)
        refused(b"actor", actor_="null", sample_only=True)
        refused(b"actor", rollout_only=True,
                io=_capi.make_rollout_io(K, actions_dev=_p(acts), action_step_stride=n * env.nu, **base))  # a head without an actor
        refused(b"noise->mode", noise_=noise(_capi.NOISE_ACTION))
        refused(b"noise->mode", noise_=noise(2))
        strided = actor(); strided.env_stride = policy.param_count(env.obs_dim, env.nu, 0, stochastic=True)  # the parametrised count
        refused(b"actor->env_stride", actor_=strided)
        strided = actor(); strided.env_stride = 3
        refused(b"actor->env_stride", actor_=strided)
        # what the underlying entries refuse
        bad = actor(); bad.struct_size += 8
        refused(b"actor->struct_size", actor_=bad)
        wide = actor(); wide.n_hidden, wide.hidden[0] = 1, 65
        refused(b"actor->hidden[0]", actor_=wide)
        nz = noise(); nz.struct_size -= 8
        refused(b"noise->struct_size", noise_=nz)
        refused(b"n_steps", rollout_only=True, io=_capi.make_rollout_io(0, actor=actor(), noise=noise(), **base))
        io = _capi.make_rollout_io(K, actor=actor(), noise=noise(), **base); io.struct_size += 8
        refused(b"io->struct_size", rollout_only=True, io=io)
        hd = head()
        assert lib.mz_rollout_head(h, None, C.byref(hd), env._stream()) == MZ_ERR_ARG and b"io" in lib.mz_last_error(h)
        a, nz = actor(), noise()
        assert lib.mz_net_sample_head(h, C.byref(a), C.byref(hd), C.byref(nz), None, _p(out), _p(lp), env._stream()) == MZ_ERR_ARG
        assert b"null array" in lib.mz_last_error(h)
        # a per-env stride of the head count is accepted
        per_env = torch.zeros((n, count), device=env.device)
        a = _capi.make_net(_p(per_env), count, (), _capi.ACT_TANH, True, ACTION_SCALE)
        assert lib.mz_net_sample_head(h, C.byref(a), C.byref(hd), C.byref(nz), _p(env._obs), _p(out), _p(lp), env._stream()) == 0, lib.mz_last_error(h)
        # the Python side
        for kw in (dict(log_std="learned"), dict(log_std="state", noise="action"), dict(log_std="state", squashed_logp=True, squash=False),
                   dict(squashed_logp=True, squash=True), dict(log_std="state", log_std_bounds=(1.0, -1.0)),
                   dict(log_std="state", log_std_bounds=(float("nan"), 1.0))):
            p = par if kw.get("log_std") == "state" else torch.zeros(policy.param_count(env.obs_dim, env.nu, 0, stochastic=True), device=env.device)
            with pytest.raises(ValueError):
                env.policy_sample(p, **kw)
            with pytest.raises(ValueError):
                env.rollout_policy_sample(p, K, **kw)
        with pytest.raises(ValueError):  # a parametrised vector is no head vector
            env.policy_sample(torch.zeros(count - env.nu, device=env.device), log_std="state")
        # after all of it the next accepted call equals a twin's that never saw a refusal
        pol = _head_actor(env, True, (5, 3), "relu", 3, True)
        kw = dict(steps=K, noise_seed=SEED, noise_step=STEP0, return_actions=True, return_obs=True, return_next_obs=True)
        oa, ra, da, ia = env.rollout_policy_sample(**pol, **kw)
        ob, rb, db, ib = twin.rollout_policy_sample(**pol, **kw)
        torch.cuda.synchronize()
        assert _same(oa, ob) and _same(ra, rb) and _same(da, db)
        for key in ia:
            assert _same(ia[key].contiguous(), ib[key].contiguous()), key
        _same_state(env, twin)
    finally:
        env.close(); twin.close()
