"""Off-policy collection on the device: info["next_observations"] of rollout / rollout_policy / rollout_policy_sample (mz_rollout_ex
next_obs_seq_dev) and exploration noise on the action (noise="action": mz_net_sample, mz_noise.mode = MZ_NOISE_ACTION).

next_observations goes against its defining loop on a twin env — same id, num_envs, seed, reset and injected states —

    obs, reward, done, info = step(a);  next_obs[k] = where(done != 0, info["final_observation"], obs)      (auto-reset; else obs)

by bit patterns: the fused kernels store the row they hand to final_obs and obs_seq, the other handles select between the two
buffers, so nothing may differ.  A third env runs the same call without return_next_obs: every other output and the state afterwards
must be its bits.  A rollout with noise="action" goes against K x (policy_sample(noise="action", noise_step + k), step) the same way.
The helpers are those of the rollout, policy, critic, deep-policy and normaliser modules."""
import ctypes as C

import numpy as np
import pytest

import mujoco_maze_amd as mm
from mujoco_maze_amd import _capi, policy
from tests.test_custom_task import FarGoalCross, RandomGoalCross
from tests.test_gpu_critic import _critic as _shallow_critic
from tests.test_gpu_deep_policy import _actor as _deep_actor
from tests.test_gpu_deep_policy import _critic as _deep_critic
from tests.test_gpu_deep_policy import _view_env
from tests.test_gpu_policy_rollout import _current_obs, _policy
from tests.test_gpu_policy_sample import SEED, STEP0, _spolicy
from tests.test_gpu_rollout import FUSED_IDS, _actions, _near_goal, _same

pytestmark = pytest.mark.gpu
MZ_ERR_ARG = -1
MODES = ["open", "deterministic", "sampled", "sampled-critic"]
OUT_KEYS = ("act", "obs", "next_obs", "reward", "done", "goal", "pos", "fwd", "ctrl", "values", "next_values", "logp")
INFO_OF = {"act": "actions", "obs": "observations", "next_obs": "next_observations", "goal": "goal_index", "pos": "position", "fwd": "reward_forward",
           "ctrl": "reward_ctrl", "values": "values", "next_values": "next_values", "logp": "logp"}


def _value(env, crt, obs=None):
    return env.value(crt["value_params"], obs=obs, hidden=crt["value_hidden"], activation=crt.get("value_activation", "tanh"))


def _setup(mode, env, point, seed, net="tanh5", critic=None):
    """(pol, crt, sample) of a mode: pol None for the open loop; net "tanh5": one tanh layer of 5 units per env, squashed; "relu64": 64-64
    ReLU per env, squashed; critic: None / "shallow" / "relu64" (default: shallow where the mode has one)"""
    sample = mode.startswith("sampled")
    if mode == "open":
        return None, {}, False
    if net == "tanh5":
        pol = _spolicy(env, True, 5, True, seed=seed, drive=point) if sample else _policy(env, True, 5, True, seed=seed, drive=point)
    else:
        pol = _deep_actor(env, True, (64, 64), "relu", True, seed, sample, drive=point)
    if critic is None and mode.endswith("critic"):
        critic = "shallow"
    crt = {} if critic is None else (_shallow_critic(env, True, 5, seed=seed + 1) if critic == "shallow" else _deep_critic(env, True, (64, 64), "relu", seed + 1))
    return pol, crt, sample


def _loop(env, K, pol, crt, sample, acts, noise="pre_squash"):
    """the defining loop: the stacked rows, the last step's obs and info"""
    import torch

    rows = {}
    for k in range(K):
        r = {}
        if crt:
            r["values"] = _value(env, crt)
        if pol is None:
            a = acts[k]
        elif sample:
            a, r["logp"] = env.policy_sample(noise_seed=SEED, noise_step=STEP0 + k, noise=noise, **pol)
        else:
            a = env.policy_act(**pol)
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


def _call(env, K, pol, crt, sample, acts, noise="pre_squash", **kw):
    if pol is None:
        return env.rollout(acts, return_obs=True, **kw)
    if sample:
        return env.rollout_policy_sample(steps=K, noise_seed=SEED, noise_step=STEP0, return_obs=True, return_actions=True, noise=noise, **pol, **crt, **kw)
    return env.rollout_policy(steps=K, return_obs=True, return_actions=True, **pol, **crt, **kw)


def _out(out, key):
    obs, rew, done, info = out
    return rew if key == "reward" else (done if key == "done" else info.get(INFO_OF[key]))


def _same_state(ea, eb, status_a=None):
    """state and status words of two envs; status() clears what it reads: a third env is compared with the words read before
    (status_a).  Returns eb's words."""
    for x, y in zip(ea.get_state(), eb.get_state()):
        assert _same(x, y)
    sa, sb = ea.status() if status_a is None else status_a, eb.status()
    assert _same(sa, sb)
    return sb


def _transitions_check(make, K, mode, seed=11, point=False, net="tanh5", critic=None, prepare=None, noise="pre_squash", third=True,
                       expect_done=True, after_reset=None):
    """env A: the defining loop; env B: one call with return_next_obs; env C: the same call without.  Returns (rows of the loop, the
    call's output, B's launch info, the critic).  `prepare(env)` runs in front of the reset, `after_reset(env)` behind it (state
    injection of other robots than the Point; the observation buffer is refreshed afterwards)."""
    import torch

    envs = [make() for _ in range(3 if third else 2)]
    try:
        for e in envs:
            if prepare:
                prepare(e)
            o = e.reset(seed=seed)
            if point:
                _near_goal(e, o)
                _current_obs(e)
            if after_reset:
                after_reset(e)
                _current_obs(e)
        ea, eb = envs[:2]
        assert _same(ea._obs, eb._obs)
        pol, crt, sample = _setup(mode, ea, point, seed + 1, net, critic)
        acts = _actions(ea, K, seed + 1, drive=point) if pol is None else None
        want, obs_a, info_a = _loop(ea, K, pol, crt, sample, acts, noise)
        out_b = _call(eb, K, pol, crt, sample, acts, noise, return_next_obs=True)
        torch.cuda.synchronize()
        n, od = ea.num_envs, ea.obs_dim
        nxt, seq, done = out_b[3]["next_observations"], out_b[3]["observations"], out_b[2]
        assert tuple(nxt.shape) == (K, n, od) and nxt.dtype == torch.float32
        # 1. the defining loop, by bits: the new rows and everything else the call returns
        for key in OUT_KEYS:
            if key in want and not (key == "act" and pol is None):  # (the open loop was given its actions)
                assert _same(_out(out_b, key), want[key]), key
        assert _same(out_b[0], obs_a)
        if ea._auto_reset:
            assert _same(out_b[3]["final_observation"], info_a["final_observation"])
        status_b = _same_state(ea, eb)
        # 2. against the call's own observations
        fin = done != 0
        nb, sb = nxt.view(torch.int32), seq.view(torch.int32)
        if ea._auto_reset:
            assert torch.equal(nb[~fin], sb[~fin])
            if expect_done:
                assert int(fin.sum()) > 0 and int((nb[fin] != sb[fin]).any(dim=-1).sum()) > 0
        else:
            assert torch.equal(nb, sb)
            if expect_done:
                assert int(fin.sum()) > 0
        # 3. the same call without the new rows: every other output and the state afterwards
        if third:
            ec = envs[2]
            out_c = _call(ec, K, pol, crt, sample, acts, noise)
            torch.cuda.synchronize()
            assert "next_observations" not in out_c[3]
            assert _same(out_b[0], out_c[0]) and _same(out_b[1], out_c[1]) and _same(out_b[2], out_c[2])
            assert set(out_c[3]) == set(out_b[3]) - {"next_observations"}
            for key in out_c[3]:
                assert _same(out_b[3][key].contiguous(), out_c[3][key].contiguous()), key
            _same_state(eb, ec, status_b)
        return want, out_b, eb.launch_info(), crt
    finally:
        for e in envs:
            e.close()


# ---------------------------------------------------------------------------------------------- 1. the fused kernels
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("env_id", FUSED_IDS)
def test_fused_next_observations_equal_the_defining_loop(env_id, mode):
    """130 envs: a partial wave; K = 260 crosses the 256-step split of the launches; max_episode_steps = 40 ends six episodes per env,
    of which the bound final_obs buffer keeps one"""
    point = env_id.startswith("Point")
    want, out, li, _ = _transitions_check(lambda: mm.make(env_id, num_envs=130, auto_reset=True, seed=5, max_episode_steps=40), 260, mode, point=point)
    assert li["rollout_fused"] == 1
    assert int((want["done"] != 0).sum(dim=0).min()) >= 6  # (260 steps under a 40-step limit; a goal reached early only adds episodes)


@pytest.mark.parametrize("mode", ["open", "sampled-critic"])
@pytest.mark.parametrize("env_id", FUSED_IDS)
def test_fused_without_auto_reset_the_rows_are_the_observations(env_id, mode):
    point = env_id.startswith("Point")
    _transitions_check(lambda: mm.make(env_id, num_envs=130, auto_reset=False, seed=5, max_episode_steps=30), 260, mode, point=point, third=False)


@pytest.mark.parametrize("n,K", [(130, 1), (1, 45)])
@pytest.mark.parametrize("mode", ["open", "sampled"])
@pytest.mark.parametrize("env_id", ["PointUMaze-v0", "SwimmerUMaze-v0"])
def test_fused_one_step_and_one_env(env_id, mode, n, K):
    point = env_id.startswith("Point")
    _transitions_check(lambda: mm.make(env_id, num_envs=n, force_vec=True, auto_reset=True, seed=5, max_episode_steps=1 if K == 1 else 20), K, mode,
                       point=point)


# ---------------------------------------------------------------------------------------------- 2. with a critic
@pytest.mark.parametrize("bound", [False, True], ids=["raw", "obs-norm"])
@pytest.mark.parametrize("net", ["tanh5", "relu64"])
@pytest.mark.parametrize("env_id", ["PointUMaze-v0", "SwimmerUMaze-v0", "AntUMaze-v0"])
def test_the_critic_values_the_rows_returned(env_id, net, bound):
    """value(next_observations[k]) is next_values[k], for every k — with a normaliser bound too, while the rows themselves stay raw"""
    import torch

    point = env_id.startswith("Point")
    norm = {}

    def prepare(env):
        if bound:
            rng = np.random.default_rng(3)
            m = torch.as_tensor(rng.normal(0.0, 0.3, env.obs_dim).astype(np.float32), device=env.device)
            s = torch.as_tensor(rng.uniform(0.5, 2.0, env.obs_dim).astype(np.float32), device=env.device)
            env.bind_obs_norm(m, s, 1.5)
            norm[id(env)] = (m, s)

    n, K, mes = (64, 20, 8) if env_id.startswith("Ant") else (130, 45, 20)
    want, out, li, crt = _transitions_check(lambda: mm.make(env_id, num_envs=n, auto_reset=True, seed=5, max_episode_steps=mes), K, "sampled-critic",
                                            point=point, net=net, critic="shallow" if net == "tanh5" else "relu64", prepare=prepare)
    # (the check above compared next_observations with the twin's RAW step outputs; here the critic, on a fresh env with the binding)
    env = mm.make(env_id, num_envs=n, seed=5)
    try:
        prepare(env)
        nxt, nv = out[3]["next_observations"], out[3]["next_values"]
        for k in range(K):
            assert _same(_value(env, crt, nxt[k].contiguous()), nv[k].contiguous()), k
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------- 3. the handles that step launch by launch
@pytest.mark.parametrize("mode", MODES)
def test_unfused_ant(mode):
    want, out, li, _ = _transitions_check(lambda: mm.make("AntUMaze-v0", num_envs=64, auto_reset=True, seed=4, max_episode_steps=8), 20, mode)
    assert li["rollout_fused"] == 0


@pytest.mark.parametrize("mode", MODES)
def test_unfused_general_engine(mode):
    want, out, li, _ = _transitions_check(lambda: mm.make("PointUMaze-v0", num_envs=32, engine="general", auto_reset=True, max_episode_steps=7), 12, mode,
                                          point=True)
    assert li["rollout_fused"] == 0 and li["engine"] == 1


@pytest.mark.parametrize("mode", MODES)
def test_unfused_top_down_view(mode):
    """the view entries of the terminal rows are part of the rows"""
    import torch

    want, out, li, _ = _transitions_check(lambda: _view_env(64, auto_reset=True, max_episode_steps=6), 14, mode, point=True)
    assert li["rollout_fused"] == 0
    nxt, fin = out[3]["next_observations"], out[2] != 0
    view = nxt[..., -1 - 75: -1]  # MZ_VIEW_DIM entries in front of the trailing time entry
    assert float(view[fin].abs().sum()) > 0
    assert bool((nxt[fin][:, -1] > 0).all())  # terminal rows carry their own step count, not the new episode's t = 0


@pytest.mark.parametrize("env_id", ["AntUMaze-v0", "view"])
def test_unfused_without_auto_reset(env_id):
    make = (lambda: _view_env(64, auto_reset=False, max_episode_steps=6)) if env_id == "view" else (
        lambda: mm.make(env_id, num_envs=64, auto_reset=False, seed=4, max_episode_steps=8))
    _transitions_check(make, 14, "sampled-critic", point=env_id == "view", third=False)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("task", ["host-judged", "per-env-goals"])
def test_python_fallback(task, mode):
    from mujoco_maze_amd.maze_env import VecMazeEnv

    def make():
        if task == "host-judged":
            env = VecMazeEnv(mm.PointEnv, FarGoalCross, maze_size_scaling=4.0, num_envs=48, auto_reset=True, max_episode_steps=6)
            assert env._host_rewards
        else:
            env = VecMazeEnv(mm.PointEnv, RandomGoalCross, maze_size_scaling=4.0, num_envs=64, auto_reset=True, inner_reward_scaling=0.0,
                             max_episode_steps=6)
        return env

    _transitions_check(make, 10, mode, point=True)


# ---------------------------------------------------------------------------------------------- 4. mz_rollout_ex through ctypes
def _p(t):
    return None if t is None else t.data_ptr()


def _bufs(env, K):
    import torch

    n, dev = env.num_envs, env.device
    return dict(reward=torch.zeros((K, n), device=dev), done=torch.zeros((K, n), dtype=torch.uint8, device=dev),
                goal=torch.zeros((K, n), dtype=torch.int32, device=dev), info=torch.zeros((K, n, 4), device=dev),
                obs_seq=torch.zeros((K, n, env.obs_dim), device=dev), act=torch.zeros((K, n, env.nu), device=dev), logp=torch.zeros((K, n), device=dev),
                values=torch.zeros((K, n), device=dev), next_values=torch.zeros((K, n), device=dev))


@pytest.mark.parametrize("env_id", ["PointUMaze-v0", "SwimmerUMaze-v0", "AntUMaze-v0"])
def test_rollout_ex_without_the_new_arguments_is_the_existing_entries(env_id):
    import torch

    point, K, n = env_id.startswith("Point"), 20, 64
    envs = [mm.make(env_id, num_envs=n, auto_reset=True, seed=5, max_episode_steps=8) for _ in range(4)]
    try:
        for e in envs:
            o = e.reset(seed=3)
            if point:
                _near_goal(e, o)
                _current_obs(e)
        e0, e1, e2, e3 = envs
        lib = e0._lib
        # open loop: mz_rollout against mz_rollout_ex with actions_dev
        acts = _actions(e0, K, 9, drive=point)
        b0, b1 = _bufs(e0, K), _bufs(e1, K)
        rc = lib.mz_rollout(e0._h, K, _p(acts), n * e0.nu, _p(e0._obs), _p(b0["reward"]), _p(b0["done"]), _p(b0["goal"]), _p(b0["info"]), _p(b0["obs_seq"]),
                            e0._stream())
        assert rc == 0
        io = _capi.make_rollout_io(K, actions_dev=_p(acts), action_step_stride=n * e1.nu, obs_dev=_p(e1._obs), reward_dev=_p(b1["reward"]),
                                   done_dev=_p(b1["done"]), goal_idx_dev=_p(b1["goal"]), info_dev=_p(b1["info"]), obs_seq_dev=_p(b1["obs_seq"]))
        assert lib.mz_rollout_ex(e1._h, C.byref(io), e1._stream()) == 0, lib.mz_last_error(e1._h)
        torch.cuda.synchronize()
        for key in ("reward", "done", "goal", "info", "obs_seq"):
            assert _same(b0[key], b1[key]), key
        assert _same(e0._obs, e1._obs)
        _same_state(e0, e1)
        # closed loop: mz_rollout_net against mz_rollout_ex with an actor, mode 0 noise and a critic
        pol = _deep_actor(e2, True, (64, 64), "relu", True, 21, True, drive=point)
        crt = _deep_critic(e2, True, (5, 3), "relu", 22)
        b2, b3 = _bufs(e2, K), _bufs(e3, K)

        def nets(e):
            a = _capi.make_net(_p(pol["params"]), pol["params"].shape[1], (64, 64), _capi.ACT_RELU, True, pol["action_scale"])
            c = _capi.make_net(_p(crt["value_params"]), crt["value_params"].shape[1], (5, 3), _capi.ACT_RELU)
            return a, c

        a2, c2 = nets(e2)
        rc = lib.mz_rollout_net(e2._h, K, C.byref(a2), 1, SEED, STEP0, C.byref(c2), _p(b2["values"]), _p(b2["next_values"]), _p(e2._obs),
                                _p(b2["reward"]), _p(b2["done"]), _p(b2["goal"]), _p(b2["info"]), _p(b2["obs_seq"]), _p(b2["act"]), _p(b2["logp"]),
                                e2._stream())
        assert rc == 0, lib.mz_last_error(e2._h)
        a3, c3 = nets(e3)
        io = _capi.make_rollout_io(K, actor=a3, noise=_capi.make_noise(_capi.NOISE_PRE_SQUASH, SEED, STEP0), critic=c3, obs_dev=_p(e3._obs),
                                   reward_dev=_p(b3["reward"]), done_dev=_p(b3["done"]), goal_idx_dev=_p(b3["goal"]), info_dev=_p(b3["info"]),
                                   obs_seq_dev=_p(b3["obs_seq"]), actions_seq_dev=_p(b3["act"]), logp_seq_dev=_p(b3["logp"]),
                                   value_seq_dev=_p(b3["values"]), next_value_seq_dev=_p(b3["next_values"]))
        assert lib.mz_rollout_ex(e3._h, C.byref(io), e3._stream()) == 0, lib.mz_last_error(e3._h)
        torch.cuda.synchronize()
        for key in b2:
            assert _same(b2[key], b3[key]), key
        assert _same(e2._obs, e3._obs) and int((b2["done"] != 0).sum()) > 0
        _same_state(e2, e3)
    finally:
        for e in envs:
            e.close()


@pytest.mark.parametrize("env_id", ["PointUMaze-v0", "AntUMaze-v0"], ids=["fused", "unfused"])
def test_rollout_ex_refusals_name_the_argument_and_leave_the_handle_usable(env_id):
    import torch

    K, n = 3, 16
    env = mm.make(env_id, num_envs=n, auto_reset=True, seed=1)
    try:
        env.reset(seed=1)
        lib, h = env._lib, env._h
        b = _bufs(env, K)
        nxt = torch.zeros((K, n, env.obs_dim), device=env.device)
        acts = torch.zeros((K, n, env.nu), device=env.device)
        par = torch.zeros(policy.param_count(env.obs_dim, env.nu, 0, stochastic=True), device=env.device)
        vpar = torch.zeros(policy.param_count(env.obs_dim, 1, 0), device=env.device)
        actor = lambda: _capi.make_net(_p(par), 0, (), _capi.ACT_TANH, True, 1.0)
        critic = lambda: _capi.make_net(_p(vpar), 0, (), _capi.ACT_TANH)
        base = dict(obs_dev=_p(env._obs), reward_dev=_p(b["reward"]), done_dev=_p(b["done"]))

        def refused(word, io):
            assert lib.mz_rollout_ex(h, C.byref(io), env._stream()) == MZ_ERR_ARG, word
            assert word in lib.mz_last_error(h), (word, lib.mz_last_error(h))

        assert lib.mz_rollout_ex(h, None, env._stream()) == MZ_ERR_ARG and b"io" in lib.mz_last_error(h)
        io = _capi.make_rollout_io(K, actions_dev=_p(acts), action_step_stride=n * env.nu, **base)
        io.struct_size += 8
        refused(b"struct_size", io)
        nz = _capi.make_noise(_capi.NOISE_ACTION, 1, 2)
        nz.struct_size -= 8
        refused(b"noise->struct_size", _capi.make_rollout_io(K, actor=actor(), noise=nz, **base))
        refused(b"noise->mode", _capi.make_rollout_io(K, actor=actor(), noise=_capi.make_noise(2, 1, 2), **base))
        refused(b"noise->mode", _capi.make_rollout_io(K, actor=actor(), noise=_capi.make_noise(-1, 1, 2), **base))
        bad_actor = actor()
        bad_actor.struct_size += 8
        refused(b"actor->struct_size", _capi.make_rollout_io(K, actor=bad_actor, **base))
        refused(b"io->actions_dev", _capi.make_rollout_io(K, actions_dev=_p(acts), action_step_stride=n * env.nu, actor=actor(), **base))
        refused(b"io->actor", _capi.make_rollout_io(K, **base))
        refused(b"io->noise", _capi.make_rollout_io(K, actions_dev=_p(acts), action_step_stride=n * env.nu, noise=_capi.make_noise(0, 1, 2), **base))
        refused(b"io->critic", _capi.make_rollout_io(K, actions_dev=_p(acts), action_step_stride=n * env.nu, critic=critic(), **base))
        # what the two older entries refuse
        refused(b"n_steps", _capi.make_rollout_io(0, actions_dev=_p(acts), action_step_stride=n * env.nu, **base))
        refused(b"n_steps", _capi.make_rollout_io(65537, actor=actor(), **base))
        refused(b"stride", _capi.make_rollout_io(K, actions_dev=_p(acts), action_step_stride=n * env.nu + 1, **base))
        refused(b"null array", _capi.make_rollout_io(K, actions_dev=_p(acts), action_step_stride=0, obs_dev=_p(env._obs), done_dev=_p(b["done"])))
        refused(b"null array", _capi.make_rollout_io(K, actor=actor(), obs_dev=_p(env._obs), reward_dev=_p(b["reward"])))
        wide = actor()
        wide.n_hidden, wide.hidden[0] = 1, 65
        refused(b"actor->hidden[0]", _capi.make_rollout_io(K, actor=wide, **base))
        squashed = critic()
        squashed.squash = 1
        refused(b"critic->squash", _capi.make_rollout_io(K, actor=actor(), critic=squashed, **base))
        strided = actor()
        strided.env_stride = 3
        refused(b"actor->env_stride", _capi.make_rollout_io(K, actor=strided, noise=_capi.make_noise(1, 1, 2), **base))
        # mz_net_sample
        out, lp = torch.zeros((n, env.nu), device=env.device), torch.zeros(n, device=env.device)
        a = actor()
        assert lib.mz_net_sample(h, C.byref(a), None, _p(env._obs), _p(out), _p(lp), env._stream()) == MZ_ERR_ARG and b"noise" in lib.mz_last_error(h)
        bad = _capi.make_noise(3, 1, 2)
        assert lib.mz_net_sample(h, C.byref(a), C.byref(bad), _p(env._obs), _p(out), _p(lp), env._stream()) == MZ_ERR_ARG
        assert b"noise->mode" in lib.mz_last_error(h)
        assert lib.mz_net_sample(h, C.byref(a), C.byref(nz), _p(env._obs), _p(out), _p(lp), env._stream()) == MZ_ERR_ARG
        assert b"noise->struct_size" in lib.mz_last_error(h)
        ok = _capi.make_noise(1, 1, 2)
        assert lib.mz_net_sample(h, C.byref(a), C.byref(ok), None, _p(out), _p(lp), env._stream()) == MZ_ERR_ARG
        assert lib.mz_net_sample(h, None, C.byref(ok), _p(env._obs), _p(out), _p(lp), env._stream()) == MZ_ERR_ARG and b"actor" in lib.mz_last_error(h)
        # next_obs_seq_dev under auto-reset without a final_obs buffer: refused on every handle, open and closed loop
        assert lib.mz_bind_final_obs(h, None) == 0
        refused(b"next_obs_seq_dev", _capi.make_rollout_io(K, actions_dev=_p(acts), action_step_stride=n * env.nu, next_obs_seq_dev=_p(nxt), **base))
        refused(b"next_obs_seq_dev", _capi.make_rollout_io(K, actor=actor(), next_obs_seq_dev=_p(nxt), **base))
        io = _capi.make_rollout_io(K, actions_dev=_p(acts), action_step_stride=n * env.nu, **base)  # (without the rows the call goes through)
        assert lib.mz_rollout_ex(h, C.byref(io), env._stream()) == 0
        assert lib.mz_bind_final_obs(h, _p(env._final_obs)) == 0
        io = _capi.make_rollout_io(K, actor=actor(), noise=_capi.make_noise(1, 1, 2), critic=critic(), next_obs_seq_dev=_p(nxt), **base)
        assert lib.mz_rollout_ex(h, C.byref(io), env._stream()) == 0, lib.mz_last_error(h)
        # the Python side
        with pytest.raises(ValueError):
            env.policy_sample(par, noise="post_squash")
        with pytest.raises(ValueError):
            env.rollout_policy_sample(par, 3, noise="tanh")
        # the env still steps, and a rollout with the rows still works
        obs, rew, done, info = env.step(acts[0])
        obs, rew, done, info = env.rollout_policy_sample(par, K, squash=True, noise="action", return_next_obs=True)
        torch.cuda.synchronize()
        assert torch.isfinite(obs).all() and torch.isfinite(info["next_observations"]).all()
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------- 5. noise on the action
ACTION_CASES = [("tanh5", None, False), ("relu64", None, False), ("relu64", None, True), ("tanh5", "shallow", False), ("relu64", "relu64", True)]
ACTION_IDS = ["tanh5", "relu64", "relu64-obs-norm", "tanh5-critic", "relu64-critic-obs-norm"]


@pytest.mark.parametrize("net,critic,bound", ACTION_CASES, ids=ACTION_IDS)
@pytest.mark.parametrize("env_id", ["PointUMaze-v0", "SwimmerUMaze-v0", "ReacherUMaze-v0", "AntUMaze-v0"])
def test_action_noise_rollout_equals_the_loop(env_id, net, critic, bound):
    """K x (policy_sample(noise="action", noise_step + k), step); the one-layer case crosses the 256-step split on the fused handles"""
    import torch

    point, ant = env_id.startswith("Point"), env_id.startswith("Ant")

    def prepare(env):
        if bound:
            rng = np.random.default_rng(3)
            env.bind_obs_norm(torch.as_tensor(rng.normal(0.0, 0.3, env.obs_dim).astype(np.float32), device=env.device),
                              torch.as_tensor(rng.uniform(0.5, 2.0, env.obs_dim).astype(np.float32), device=env.device), 1.5)

    n, K, mes = (64, 20, 8) if ant else ((130, 260, 40) if (net, critic) == ("tanh5", None) else (130, 45, 20))
    want, out, li, _ = _transitions_check(lambda: mm.make(env_id, num_envs=n, auto_reset=True, seed=5, max_episode_steps=mes), K,
                                          "sampled-critic" if critic else "sampled", point=point, net=net, critic=critic, prepare=prepare,
                                          noise="action", third=False)
    assert li["rollout_fused"] == (0 if ant else 1)
    assert torch.isfinite(want["act"][0]).all() and float(want["act"].abs().max()) <= 0.9  # ACTION_SCALE of the helpers: the clip


def _clip_policy(env, squash, log_std, seed=31, per_env=True, hidden=(64, 64)):
    import torch

    from tests.test_deep_policy_api import random_net

    p = random_net(np.random.default_rng(seed), env.obs_dim, env.nu, hidden, rows=env.num_envs if per_env else None)
    ls = np.full(p.shape[:-1] + (env.nu,), log_std, np.float32)
    return dict(params=torch.as_tensor(np.concatenate([p, ls], axis=-1), device=env.device), hidden=hidden, squash=squash, action_scale=1.0,
                activation="relu" if np.ndim(hidden) else "tanh")


@pytest.mark.parametrize("env_id", ["PointUMaze-v0", "AntUMaze-v0"])
def test_action_noise_modes_clip_and_logp(env_id):
    import torch

    env = mm.make(env_id, num_envs=130, seed=2)
    try:
        env.reset(seed=2)
        kw = dict(noise_seed=SEED, noise_step=STEP0)
        # without squash the two modes are the same operations
        pol = _clip_policy(env, False, -0.5)
        (a0, l0), (a1, l1) = env.policy_sample(noise="pre_squash", **pol, **kw), env.policy_sample(noise="action", **pol, **kw)
        assert _same(a0, a1) and _same(l0, l1) and torch.isfinite(a0).all()
        # the default is "pre_squash", which takes the entries it took
        ad, ld = env.policy_sample(**pol, **kw)
        assert _same(a0, ad) and _same(l0, ld)
        # squash, log_std 2, action_scale 1: clipped to +-1 exactly, logp that of the other mode
        pol = _clip_policy(env, True, 2.0)
        (a0, l0), (a1, l1) = env.policy_sample(noise="pre_squash", **pol, **kw), env.policy_sample(noise="action", **pol, **kw)
        assert bool((a1.abs() <= 1.0).all()) and int((a1.abs() == 1.0).sum()) > 0 and int((a1.abs() < 1.0).sum()) > 0
        assert bool((a1 == 1.0).any()) and bool((a1 == -1.0).any())
        assert _same(l0, l1) and not _same(a0, a1)
        # the same through a rollout
        obs, rew, done, info = env.rollout_policy_sample(steps=5, noise="action", return_actions=True, **pol, **kw)
        assert _same(info["actions"][0].contiguous(), a1) and _same(info["logp"][0].contiguous(), l1)
        assert bool((info["actions"].abs() <= 1.0).all()) and int((info["actions"].abs() == 1.0).sum()) > 0
    finally:
        env.close()


@pytest.mark.parametrize("env_id", ["PointUMaze-v0", "AntUMaze-v0"])
def test_action_noise_against_the_model(env_id):
    import torch

    from tests.test_deep_policy_api import random_net

    n = 130
    env = mm.make(env_id, num_envs=n, seed=3)
    try:
        env.reset(seed=4)
        g = torch.Generator(device=env.device).manual_seed(1)
        lo, hi = torch.as_tensor(env.action_space.low, device=env.device), torch.as_tensor(env.action_space.high, device=env.device)
        for _ in range(3):  # observations of moving robots
            obs, _, _, _ = env.step(lo + (hi - lo) * torch.rand((n, env.nu), device=env.device, generator=g))
        x = obs.cpu().numpy()
        slots = np.arange(n)
        rng = np.random.default_rng(7)
        for per_env in (True, False):
            # affine, unsquashed, expf exact (log_std -inf: z = m + (+-0)): by bits
            net = random_net(rng, env.obs_dim, env.nu, 0, rows=n if per_env else None)
            p = np.concatenate([net, np.full(net.shape[:-1] + (env.nu,), -np.inf, np.float32)], axis=-1)
            got, glp = env.policy_sample(torch.as_tensor(p, device=env.device), noise="action", noise_seed=9, noise_step=4)
            ref, rlp = policy.sample_reference(p, x, env.nu, noise="action", noise_seed=9, noise_step=4, slots=slots)
            assert np.array_equal(got.cpu().numpy().view(np.int32), ref.view(np.int32)) and bool(torch.isposinf(glp).all())
            # affine, unsquashed, a general log_std: the device's own eps (libm) — the suite's 1e-5 on eps, times s <= 1
            p = np.concatenate([net, rng.uniform(-1, 0, net.shape[:-1] + (env.nu,)).astype(np.float32)], axis=-1)
            got, glp = env.policy_sample(torch.as_tensor(p, device=env.device), noise="action", noise_seed=9, noise_step=4)
            ref, rlp = policy.sample_reference(p, x, env.nu, noise="action", noise_seed=9, noise_step=4, slots=slots)
            # (the eps bar times s, expf to 2 ulp on |p| and the sum's rounding on |z|: 4 EPS |z|)
            assert np.abs(got.cpu().numpy().astype(np.float64) - ref).max() <= 1e-5 + 4 * 2.0 ** -23 * float(np.abs(ref).max())
            # squashed networks: the suite's 1e-5
            for hidden, activation in ((0, "tanh"), (5, "tanh"), ((64, 64), "relu")):
                net = random_net(rng, env.obs_dim, env.nu, hidden, rows=n if per_env else None, log_std=True)
                kw = dict(hidden=hidden, activation=activation, squash=True, action_scale=0.5, noise_seed=9, noise_step=4)
                got, glp = env.policy_sample(torch.as_tensor(net, device=env.device), noise="action", **kw)
                ref, rlp = policy.sample_reference(net, x, env.nu, noise="action", slots=slots, **kw)
                err = np.abs(got.cpu().numpy().astype(np.float64) - ref).max()
                print(f"{env_id} per_env {per_env} hidden {hidden} {activation}: max |device - model| = {err:.3e}")
                assert err <= 1e-5 and float(got.abs().max()) <= 0.5
    finally:
        env.close()


@pytest.mark.parametrize("env_id", ["PointUMaze-v0", "AntUMaze-v0"])
def test_action_noise_nan_log_std_stays_in_its_env(env_id):
    import torch

    n, K = 66, 6
    ea, eb = (mm.make(env_id, num_envs=n, auto_reset=True, seed=5, max_episode_steps=4) for _ in range(2))
    try:
        ea.reset(seed=6); eb.reset(seed=6)
        pol = _clip_policy(ea, True, -1.0, hidden=5)
        bad = dict(pol, params=pol["params"].clone())
        bad["params"][7, -1] = float("nan")  # log_std of the last action of env 7
        kw = dict(steps=K, noise_seed=SEED, noise_step=STEP0, noise="action", return_actions=True, return_next_obs=True)
        oa, ra, da, ia = ea.rollout_policy_sample(**pol, **kw)
        ob, rb, db, ib = eb.rollout_policy_sample(**bad, **kw)
        torch.cuda.synchronize()
        keep = torch.arange(n, device=ea.device) != 7
        assert bool(torch.isnan(ib["actions"][:, 7, -1]).all()) and bool(torch.isnan(ib["logp"][:, 7]).all())
        assert bool(torch.isfinite(ib["actions"][0, 7, :-1]).all())  # (from the second step on env 7 acts on the row its NaN action produced)
        for x, y in ((ia["actions"], ib["actions"]), (ia["logp"], ib["logp"]), (ra, rb), (ia["next_observations"], ib["next_observations"])):
            assert _same(x[:, keep].contiguous(), y[:, keep].contiguous())
        assert _same(oa[keep].contiguous(), ob[keep].contiguous())
    finally:
        ea.close(); eb.close()
