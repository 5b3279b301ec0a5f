"""Networks of up to two hidden layers with tanh or ReLU units on the device: VecMazeEnv.policy_act / policy_sample / value with
`hidden=(H1, H2)` and `activation=`, the rollouts with them, and mz_net_act / mz_net_value / mz_rollout_net straight through the C-ABI.

ReLU networks without squash go against mujoco_maze_amd.policy by bit patterns (a select adds no rounding), tanh networks against a
float64 evaluation within the derived bound of tests/test_deep_policy_api.py.  The rollouts go against the defining loop on a twin env
— same id, num_envs, seed, reset and injected states — by bit patterns (`_same` of tests/test_gpu_rollout.py): the fused kernels run
the unit functions of the stand-alone kernels on the same fp32 rows.  Shapes: 130 envs (no multiple of any group count: shadow groups
exist), hidden (5, 3) (narrower than a lane group, unequal widths: a stride mix-up shows) and (64, 64) (every lane owns several units
of both layers)."""
import ctypes as C

import numpy as np
import pytest

import mujoco_maze_amd as mm
from mujoco_maze_amd import _capi, policy
from tests.test_custom_task import FarGoalCross
from tests.test_deep_policy_api import f64_and_bound_net, random_net
from tests.test_gpu_policy_rollout import ACTION_SCALE, KEYS, _assert_equal, _current_obs
from tests.test_gpu_policy_sample import SEED, STEP0
from tests.test_gpu_rollout import FUSED_IDS, _near_goal, _same
from tests.test_policy_api import SCALE
from tests.test_top_down_view import view_task

pytestmark = pytest.mark.gpu
MZ_ERR_ARG = -1
N = 130
DEEP = [(5, 3), (64, 64)]


def _actor(env, per_env, hidden, activation, squash, seed, sample, drive=False):
    """kwargs of policy_act / policy_sample / the rollouts with random parameters on the env's device; `sample`: log_std [nu] in
    [-1, 0] behind the network.  `drive` (Point family): a small output layer and a bias on the first action that drives forward, so
    that the robots run into walls and goals."""
    import torch

    p = random_net(np.random.default_rng(seed), env.obs_dim, env.nu, hidden, rows=env.num_envs if per_env else None, log_std=sample)
    if drive:
        widths = policy.net_shape(hidden)[0]
        tail = env.nu if sample else 0
        last = env.nu + (widths[-1] if widths else env.obs_dim) * env.nu  # the output layer: its weights and biases
        p[..., p.shape[-1] - tail - last: p.shape[-1] - tail] *= 0.1
        p[..., p.shape[-1] - tail - env.nu] = 2.0 if squash else 1.0
    return dict(params=torch.as_tensor(p, device=env.device), hidden=hidden, squash=squash, action_scale=ACTION_SCALE, activation=activation)


def _critic(env, per_env, hidden, activation, seed):
    import torch

    p = random_net(np.random.default_rng(seed), env.obs_dim, 1, hidden, rows=env.num_envs if per_env else None)
    return dict(value_params=torch.as_tensor(p, device=env.device), value_hidden=hidden, value_activation=activation)


def _value(env, crt, obs=None):
    return env.value(crt["value_params"], obs=obs, hidden=crt["value_hidden"], activation=crt["value_activation"])


def _loop(env, pol, crt, K, sample):
    """the defining loop (crt: None for none): the stacked rows, the last step's obs and info"""
    import torch

    keys = KEYS + (("values", "next_values") if crt else ()) + (("logp",) if sample else ())
    rows = {k: [] for k in keys}
    for k in range(K):
        v = _value(env, crt) if crt else None
        if sample:
            a, lp = env.policy_sample(noise_seed=SEED, noise_step=STEP0 + k, **pol)
        else:
            a = env.policy_act(**pol)
        obs, rew, done, info = env.step(a)
        vals = (a, obs, rew, done, info["goal_index"], info["position"], info["reward_forward"], info["reward_ctrl"])
        if crt:
            nv = _value(env, crt)
            if env._auto_reset:
                nv = torch.where(done != 0, _value(env, crt, info["final_observation"]), nv)
            vals += (v, nv)
        for key, x in zip(keys, vals + ((lp,) if sample else ())):
            rows[key].append(x.clone())
    return {k: torch.stack(v) for k, v in rows.items()}, obs, info


def _rollout(env, pol, crt, K, sample, **kw):
    if sample:
        return env.rollout_policy_sample(steps=K, noise_seed=SEED, noise_step=STEP0, return_obs=True, return_actions=True, **pol, **(crt or {}), **kw)
    return env.rollout_policy(steps=K, return_obs=True, return_actions=True, **pol, **(crt or {}), **kw)


def _twin_check(make, K, actor_spec, critic_spec, sample, seed=11, point=False, prepare=None):
    """env A: the defining loop; env B: one rollout.  actor_spec: (per_env, hidden, activation, squash); critic_spec: (per_env, hidden,
    activation) or None.  Returns (launch info of B, the loop's rows)."""
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
        pol = _actor(ea, *actor_spec, seed=seed + 1, sample=sample, drive=point)
        crt = _critic(ea, *critic_spec, seed=seed + 2) if critic_spec else None
        want, obs_a, info_a = _loop(ea, pol, crt, K, sample)
        out_b = _rollout(eb, pol, crt, K, sample)
        _assert_equal(ea, eb, want, obs_a, info_a, out_b, K)
        info_b = out_b[3]
        assert ("values" in info_b) == bool(crt) and ("logp" in info_b) == bool(sample)
        if crt:
            assert tuple(info_b["values"].shape) == tuple(info_b["next_values"].shape) == (K, ea.num_envs)
            assert _same(info_b["values"], want["values"]) and _same(info_b["next_values"], want["next_values"])
            assert torch.isfinite(want["values"][0]).all()
            if K > 1 and ea._auto_reset:  # the value of the TERMINAL row, not of the new episode's first row, where an episode ended
                off = want["done"][:-1] != 0
                nvb, vb = info_b["next_values"][:-1].contiguous().view(torch.int32), info_b["values"][1:].contiguous().view(torch.int32)
                assert torch.equal(nvb[~off], vb[~off]) and int(off.sum()) > 0 and int((nvb[off] != vb[off]).sum()) > 0
        if sample:
            assert _same(info_b["logp"], want["logp"]) and torch.isfinite(want["logp"][0]).all()
        assert torch.isfinite(want["act"][0]).all()
        return eb.launch_info(), want
    finally:
        ea.close(); eb.close()


def _view_env(num_envs, **kw):
    from mujoco_maze_amd.maze_env import VecMazeEnv

    cls, scale = view_task("ViewPush")
    return VecMazeEnv(mm.PointEnv, cls, num_envs=num_envs, maze_size_scaling=scale, **kw)


def _moving_obs(env):
    import torch

    env.reset(seed=4)
    g = torch.Generator(device=env.device).manual_seed(1)
    lo, hi = torch.as_tensor(env.action_space.low, device=env.device), torch.as_tensor(env.action_space.high, device=env.device)
    for _ in range(3):  # observations of moving robots
        obs, _, _, _ = env.step(lo + (hi - lo) * torch.rand((env.num_envs, env.nu), device=env.device, generator=g))
    return obs


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ---------------------------------------------------------------------------------------------- 1. against numpy
@pytest.mark.parametrize("hidden", DEEP, ids=str)
@pytest.mark.parametrize("env_id", ["PointUMaze-v0", "AntUMaze-v0", "view"])
def test_act_and_value_against_the_model(env_id, hidden):
    import torch

    env = _view_env(N, seed=3) if env_id == "view" else mm.make(env_id, num_envs=N, seed=3)
    try:
        obs = _moving_obs(env)
        x, od, nu = obs.cpu().numpy(), env.obs_dim, env.nu
        rng = np.random.default_rng(7)
        for per_env in (True, False):
            rows = N if per_env else None
            p, vp = random_net(rng, od, nu, hidden, rows), random_net(rng, od, 1, hidden, rows)
            tp, tvp = torch.as_tensor(p, device=env.device), torch.as_tensor(vp, device=env.device)
            # ReLU, unsquashed: bit for bit
            got = env.policy_act(tp, hidden=hidden, activation="relu").cpu().numpy()
            assert got.shape == (N, nu) and got.dtype == np.float32
            assert np.array_equal(_bits(got), _bits(policy.reference(p, x, nu, hidden, activation="relu")))
            gv = env.value(tvp, hidden=hidden, activation="relu").cpu().numpy()
            assert gv.shape == (N,) and np.array_equal(_bits(gv), _bits(policy.value_reference(vp, x, hidden, activation="relu")))
            # the same rows passed explicitly
            assert np.array_equal(_bits(env.policy_act(p, obs=obs.clone(), hidden=hidden, activation="relu").cpu().numpy()), _bits(got))
            # tanh, plain and squashed: the derived bound
            for squash in (False, True):
                ref, bound = f64_and_bound_net(p, x, nu, hidden, "tanh", squash, SCALE)
                got = env.policy_act(tp, hidden=hidden, squash=squash, action_scale=SCALE).cpu().numpy()
                ratio = np.abs(got.astype(np.float64) - ref) / bound
                print(f"{env_id} {hidden} per-env {per_env} squash {squash}: max err / bound = {ratio.max():.3f}")
                assert (ratio <= 1.0).all()
            vref, vbound = f64_and_bound_net(vp, x, 1, hidden, "tanh", False, 1.0)
            gv = env.value(tvp, hidden=hidden).cpu().numpy()
            assert (np.abs(gv.astype(np.float64) - vref[:, 0]) <= vbound[:, 0]).all()
    finally:
        env.close()


def test_relu_on_the_device_keeps_negative_zero_and_a_nan():
    import torch

    env = mm.make("PointUMaze-v0", num_envs=N, seed=3)
    try:
        od, nu, hidden = env.obs_dim, env.nu, (3, 2)
        p = policy.pack_mlp([(np.ones((o, i), np.float32), np.full(o, -0.0, np.float32)) for i, o in ((od, 3), (3, 2), (2, nu))])
        x = np.full((N, od), -0.0, np.float32)
        x[1, 0] = np.nan
        got = env.policy_act(p, obs=torch.as_tensor(x, device=env.device), hidden=hidden, activation="relu").cpu().numpy()
        assert np.array_equal(_bits(got), _bits(policy.reference(p, x, nu, hidden, activation="relu")))
        assert np.isnan(got[1]).all() and (np.delete(got, 1, axis=0) == 0).all() and np.signbit(np.delete(got, 1, axis=0)).all()
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------- 2. sampling
@pytest.mark.parametrize("hidden", DEEP, ids=str)
@pytest.mark.parametrize("env_id", ["PointUMaze-v0", "AntUMaze-v0"])
def test_policy_sample_with_two_layers(env_id, hidden):
    """logp depends on (noise_seed, noise_step, slot) and log_std alone: today's policy_sample with an affine policy and the same
    log_std returns the same bits.  The actions: the mean is bit-equal to numpy's (ReLU, unsquashed), s = exp(log_std) <= 1 and the
    device's eps is within 1e-5 of policy.noise (the bar of tests/test_gpu_policy_sample.py); the sum adds roundings of the size of z."""
    import torch

    env = mm.make(env_id, num_envs=N, seed=3)
    try:
        obs = _moving_obs(env)
        x, od, nu = obs.cpu().numpy(), env.obs_dim, env.nu
        rng = np.random.default_rng(17)
        for per_env in (True, False):
            p = random_net(rng, od, nu, hidden, N if per_env else None, log_std=True)
            act, logp = env.policy_sample(torch.as_tensor(p, device=env.device), hidden=hidden, activation="relu", noise_seed=1234, noise_step=7)
            affine = np.zeros(p.shape[:-1] + (policy.param_count(od, nu, 0, stochastic=True),), np.float32)
            affine[..., -nu:] = p[..., -nu:]
            _, logp0 = env.policy_sample(torch.as_tensor(affine, device=env.device), noise_seed=1234, noise_step=7)
            assert _same(logp, logp0)
            want, wlp = policy.sample_reference(p, x, nu, hidden, noise_seed=1234, noise_step=7, activation="relu")
            got = act.cpu().numpy().astype(np.float64)
            bar = 1e-5 + 4 * 2.0 ** -23 * (np.abs(want) + 6.0)
            print(f"{env_id} {hidden} per-env {per_env}: max |device action - sample_reference| = {np.abs(got - want).max():.3e}")
            assert (np.abs(got - want) <= bar).all()
    finally:
        env.close()


def test_draws_do_not_depend_on_the_batch():
    import torch

    small, big = mm.make("PointUMaze-v0", num_envs=3, seed=3), mm.make("PointUMaze-v0", num_envs=8, seed=3)
    try:
        small.set_option("env_index_offset", 5)
        small.reset(seed=4)
        obs = big.reset(seed=4)
        p = torch.as_tensor(random_net(np.random.default_rng(2), big.obs_dim, big.nu, (64, 64), log_std=True), device=big.device)
        kw = dict(hidden=(64, 64), activation="relu", squash=True, action_scale=ACTION_SCALE, noise_seed=9, noise_step=2)
        a8, l8 = big.policy_sample(p, **kw)
        a3, l3 = small.policy_sample(p, obs=obs[5:8].contiguous(), **kw)
        assert _same(a3, a8[5:8].contiguous()) and _same(l3, l8[5:8].contiguous())
        a0, _ = small.policy_sample(p, obs=obs[0:3].contiguous(), **kw)
        assert not _same(a0, a8[0:3].contiguous())  # other slots, other noise
    finally:
        small.close(); big.close()


# ---------------------------------------------------------------------------------------------- 3. fused equals the defining loop
@pytest.mark.parametrize("env_id", FUSED_IDS)
def test_fused_rollout_equals_the_defining_loop(env_id):
    """130 envs, auto-reset, K = 260 (two launches), a 40-step time limit that ends every episode several times: a sampled tanh
    (64, 64) actor with a ReLU (5, 3) critic per env"""
    point = env_id.startswith("Point")
    lb, want = _twin_check(lambda: mm.make(env_id, num_envs=N, auto_reset=True, seed=5, max_episode_steps=40), 260,
                           (False, (64, 64), "tanh", True), (True, (5, 3), "relu"), True, point=point)
    assert lb["rollout_fused"] == 1 and lb["engine"] == 0
    assert int((want["done"] & 2).sum()) > 0
    if point:
        assert int((want["done"] & 1).sum()) > 0  # goals were reached, not only time limits


@pytest.mark.parametrize("hidden", DEEP, ids=str)
@pytest.mark.parametrize("critic", [False, True], ids=["no-critic", "critic"])
@pytest.mark.parametrize("sample", [False, True], ids=["deterministic", "sampled"])
def test_fused_matrix_on_the_point(sample, critic, hidden):
    """every SMP / CRT instantiation with both shapes, per-env actors: (5, 3) ReLU with a tanh critic of the mirrored widths, (64, 64)
    tanh with a ReLU critic"""
    act, vact = ("relu", "tanh") if hidden == (5, 3) else ("tanh", "relu")
    lb, want = _twin_check(lambda: mm.make("PointUMaze-v0", num_envs=N, auto_reset=True, seed=5, max_episode_steps=12), 40,
                           (True, hidden, act, True), (True, hidden[::-1], vact) if critic else None, sample, point=True)
    assert lb["rollout_fused"] == 1 and int((want["done"] & 1).sum()) > 0 and int((want["done"] & 2).sum()) > 0


def test_fused_at_32_lanes():
    lb, want = _twin_check(lambda: mm.make("PointUMaze-v0", num_envs=N, auto_reset=True, seed=3, max_episode_steps=12), 40,
                           (True, (64, 64), "relu", True), (True, (5, 3), "tanh"), True, point=True,
                           prepare=lambda e: e.set_option("lanes_per_env", 32))
    assert lb["rollout_fused"] == 1 and lb["lanes_per_env"] == 32
    assert int((want["done"] & 1).sum()) > 0 and int((want["done"] & 2).sum()) > 0


@pytest.mark.parametrize("env_id", ["SwimmerUMaze-v0", "PointUMaze-v0"])
def test_fused_without_auto_reset(env_id):
    lb, want = _twin_check(lambda: mm.make(env_id, num_envs=N, auto_reset=False, seed=2, max_episode_steps=30), 40,
                           (True, (5, 3), "relu", True), (False, (64, 64), "tanh"), True)
    assert lb["rollout_fused"] == 1 and int((want["done"] & 2).sum()) > 0


# ---------------------------------------------------------------------------------------------- 4. unfused handles, Python loops
@pytest.mark.parametrize("sample", [False, True], ids=["deterministic", "sampled"])
def test_unfused_ant(sample):
    lb, want = _twin_check(lambda: mm.make("AntUMaze-v0", num_envs=64, auto_reset=True, seed=4, max_episode_steps=8), 20,
                           (True, (64, 64), "tanh", True), (True, (5, 3), "relu"), sample)
    assert lb["rollout_fused"] == 0 and int((want["done"] != 0).sum()) > 0


def test_unfused_general_engine():
    lb, want = _twin_check(lambda: mm.make("PointUMaze-v0", num_envs=32, engine="general", auto_reset=True, max_episode_steps=7), 12,
                           (True, (5, 3), "relu", True), (True, (64, 64), "tanh"), True, point=True)
    assert lb["rollout_fused"] == 0 and lb["engine"] == 1


def test_unfused_top_down_view():
    lb, want = _twin_check(lambda: _view_env(64, auto_reset=True, max_episode_steps=6), 14, (False, (64, 64), "relu", True), (True, (5, 3), "tanh"),
                           True, point=True)
    assert lb["rollout_fused"] == 0 and int((want["done"] != 0).sum()) > 0


def test_python_loop_host_judged_task():
    from mujoco_maze_amd.maze_env import VecMazeEnv

    def make():
        env = VecMazeEnv(mm.PointEnv, FarGoalCross, maze_size_scaling=4.0, num_envs=48, auto_reset=True, max_episode_steps=6)
        assert env._host_rewards
        return env

    lb, want = _twin_check(make, 10, (True, (5, 3), "relu", True), (True, (64, 64), "tanh"), True, point=True)
    assert tuple(want["values"].shape) == (10, 48) and int((want["done"] != 0).sum()) > 0


# ---------------------------------------------------------------------------------------------- 5. compatibility
def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _c_rollout_net(env, K, actor, sample, critic):
    """mz_rollout_net straight through the C-ABI on env; returns the outputs as a dict"""
    import torch

    n = env.num_envs
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=env.device)
    out = dict(reward=z(K, n), done=z(K, n, dt=torch.uint8), goal=z(K, n, dt=torch.int32), info=z(K, n, 4), obs_seq=z(K, n, env.obs_dim),
               actions=z(K, n, env.nu), logp=z(K, n), values=z(K, n), next_values=z(K, n))
    rc = env._lib.mz_rollout_net(env._h, K, C.byref(actor), sample, SEED, STEP0, C.byref(critic) if critic else None, _p(out["values"]),
                                 _p(out["next_values"]), _p(env._obs), _p(out["reward"]), _p(out["done"]), _p(out["goal"]), _p(out["info"]),
                                 _p(out["obs_seq"]), _p(out["actions"]), _p(out["logp"]), env._stream())
    assert rc == 0, env._lib.mz_last_error(env._h)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("hidden", [0, 5, 64])
@pytest.mark.parametrize("env_id", ["PointUMaze-v0", "AntUMaze-v0"])
def test_shallow_tanh_networks_return_the_bits_of_the_existing_entries(env_id, hidden):
    """env A: today's entries through VecMazeEnv (an int `hidden`, tanh); env B: mz_net_act / mz_net_value / mz_rollout_net with
    n_hidden <= 1 and MZ_ACT_TANH straight through the C-ABI"""
    import torch

    point = env_id.startswith("Point")
    K = 20 if env_id.startswith("Ant") else 40
    ea, eb = (mm.make(env_id, num_envs=N, auto_reset=True, seed=5, max_episode_steps=8 if K == 20 else 12) for _ in range(2))
    try:
        for e in (ea, eb):
            o = e.reset(seed=9)
            if point:
                _near_goal(e, o)
                _current_obs(e)
        widths = (hidden,) if hidden else ()
        det = _actor(ea, True, hidden, "tanh", True, 10, False, drive=point)
        smp = _actor(ea, True, hidden, "tanh", True, 10, True, drive=point)
        crt = _critic(ea, True, hidden, "tanh", 12)
        for d in (det, smp):
            del d["activation"]  # env A takes today's path
        vkw = dict(value_params=crt["value_params"], value_hidden=hidden)
        net = lambda kw, stochastic: _capi.make_net(_p(kw["params"]), kw["params"].shape[-1], widths, _capi.ACT_TANH, kw["squash"], kw["action_scale"])
        vnet = _capi.make_net(_p(crt["value_params"]), crt["value_params"].shape[-1], widths, _capi.ACT_TANH)
        lib, n, nu = eb._lib, N, eb.nu
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device=eb.device)
        # the three stand-alone entries on the same rows
        a_b, lp_b, v_b = z(n, nu), z(n), z(n)
        assert lib.mz_net_act(eb._h, C.byref(net(det, False)), 0, 0, 0, _p(eb._obs), _p(a_b), None, eb._stream()) == 0
        assert _same(a_b, ea.policy_act(**det))
        assert lib.mz_net_act(eb._h, C.byref(net(smp, True)), 1, SEED, STEP0, _p(eb._obs), _p(a_b), _p(lp_b), eb._stream()) == 0
        a_a, lp_a = ea.policy_sample(noise_seed=SEED, noise_step=STEP0, **smp)
        assert _same(a_b, a_a) and _same(lp_b, lp_a)
        assert lib.mz_net_value(eb._h, C.byref(vnet), _p(eb._obs), _p(v_b), eb._stream()) == 0
        assert _same(v_b, ea.value(crt["value_params"], hidden=hidden))
        # the rollouts: deterministic, sampled, sampled with a critic — each continues where the one before ended on both envs
        for sample, pol, critic in ((0, det, None), (1, smp, None), (1, smp, vnet), (0, det, vnet)):
            kw = dict(return_obs=True, return_actions=True, **(vkw if critic else {}))
            if sample:
                obs_a, rew_a, done_a, info_a = ea.rollout_policy_sample(steps=K, noise_seed=SEED, noise_step=STEP0, **pol, **kw)
            else:
                obs_a, rew_a, done_a, info_a = ea.rollout_policy(steps=K, **pol, **kw)
            out = _c_rollout_net(eb, K, net(pol, bool(sample)), sample, critic)
            assert _same(eb._obs, obs_a) and _same(out["reward"], rew_a) and _same(out["done"], done_a) and _same(out["goal"], info_a["goal_index"])
            assert _same(out["actions"], info_a["actions"]) and _same(out["obs_seq"], info_a["observations"])
            assert _same(out["info"][:, :, :2].contiguous(), info_a["position"].contiguous())
            if sample:
                assert _same(out["logp"], info_a["logp"])
            if critic:
                assert _same(out["values"], info_a["values"]) and _same(out["next_values"], info_a["next_values"])
            assert _same(ea._final_obs, eb._final_obs) and _same(ea.status(), eb.status())
            for x, y in zip(ea.get_state(), eb.get_state()):
                assert _same(x, y)
            assert int((done_a != 0).sum()) > 0
    finally:
        ea.close(); eb.close()


# ---------------------------------------------------------------------------------------------- 6. isolation
@pytest.mark.parametrize("where", ["actor", "critic"])
def test_nan_in_layer_two_stays_in_its_env(where):
    import torch

    K, n, bad = 6, N, 37
    ea, eb = (mm.make("PointUMaze-v0", num_envs=n, auto_reset=True, seed=1, max_episode_steps=4) for _ in range(2))
    try:
        ea.reset(seed=6); eb.reset(seed=6)
        hidden = (5, 3)
        pol = _actor(ea, True, hidden, "relu", True, 3, True)
        crt = _critic(ea, True, hidden, "tanh", 4)
        dpol, dcrt = dict(pol, params=pol["params"].clone()), dict(crt, value_params=crt["value_params"].clone())
        w2 = ea.obs_dim * 5 + 5 + 4  # an entry of W2t, the second hidden layer's weights
        (dpol["params"] if where == "actor" else dcrt["value_params"])[bad, w2] = float("nan")
        _, rew_a, done_a, info_a = _rollout(ea, pol, crt, K, True)
        _, rew_b, done_b, info_b = _rollout(eb, dpol, dcrt, K, True)
        torch.cuda.synchronize()
        keep = torch.arange(n, device=ea.device) != bad
        if where == "actor":
            assert torch.isnan(info_b["actions"][:, bad]).all()
        else:  # nothing but the values sees a critic
            assert torch.isnan(info_b["values"][:, bad]).all() and torch.isnan(info_b["next_values"][:, bad]).all()
            for key in ("actions", "observations", "final_observation"):
                assert _same(info_a[key], info_b[key]), key
            assert _same(rew_a, rew_b) and _same(done_a, done_b)
        assert _same(info_a["logp"], info_b["logp"])  # the log-prob depends on the noise and log_std alone
        for key in ("values", "next_values", "actions", "observations", "position"):
            assert _same(info_a[key][:, keep].contiguous(), info_b[key][:, keep].contiguous()), key
            assert torch.isfinite(info_b[key][:, keep]).all(), key
        assert _same(rew_a[:, keep].contiguous(), rew_b[:, keep].contiguous()) and _same(done_a[:, keep].contiguous(), done_b[:, keep].contiguous())
        assert _same(info_a["final_observation"][keep].contiguous(), info_b["final_observation"][keep].contiguous())
        for x, y in zip(ea.get_state(), eb.get_state()):
            assert _same(x[keep].contiguous(), y[keep].contiguous())
        assert int((done_a != 0).sum()) > 0
    finally:
        ea.close(); eb.close()


# ---------------------------------------------------------------------------------------------- 7. refusals
def test_refusals():
    import torch

    env = mm.make("PointUMaze-v0", num_envs=16, auto_reset=True)
    try:
        env.reset(seed=1)
        n, nu, od, lib, h, dev = env.num_envs, env.nu, env.obs_dim, env._lib, env._h, env.device
        count, vcount = policy.param_count(od, nu, (5, 3)), policy.param_count(od, 1, (5, 3))
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
        # the Python side: ValueErrors that name the argument
        with pytest.raises(ValueError, match="hidden"):
            env.policy_act(z(count), hidden=(5, 3, 2))
        with pytest.raises(ValueError, match="hidden"):
            env.policy_act(z(count), hidden=(5, 0))
        with pytest.raises(ValueError, match="hidden"):
            env.value(z(vcount), hidden=(65, 3))
        with pytest.raises(ValueError, match="activation"):
            env.policy_act(z(count), hidden=(5, 3), activation="gelu")
        with pytest.raises(ValueError, match="activation"):
            env.rollout_policy(z(count), steps=3, hidden=(5, 3), value_params=z(vcount), value_hidden=(5, 3), value_activation="elu")
        with pytest.raises(ValueError, match="params must have shape"):
            env.policy_sample(z(count), hidden=(5, 3))  # no log_std behind the network
        with pytest.raises(ValueError, match="params must have shape"):
            env.rollout_policy(z(count), steps=3, hidden=(3, 5))
        with pytest.raises(ValueError, match="value_params must have shape"):
            env.rollout_policy(z(count), steps=3, hidden=(5, 3), value_params=z(n, vcount + 1), value_hidden=(5, 3))
        # straight through the C-ABI
        par, spar, vpar = z(n, count), z(n, count + nu), z(n, vcount)
        vals, nvals, rew, done, act, logp = z(3, n), z(3, n), z(3, n), torch.zeros((3, n), dtype=torch.uint8, device=dev), z(n, nu), z(n)
        p = lambda t: t.data_ptr() if t is not None else None
        err = lambda: lib.mz_last_error(h)

        def mk(params, stride, **over):
            net = _capi.make_net(p(params), stride, (5, 3), _capi.ACT_RELU)
            for k, v in over.items():
                if k == "hidden":
                    net.hidden[0], net.hidden[1] = v
                else:
                    setattr(net, k, v)
            return net

        def roll(sample=0, actor=None, critic=None, with_critic=True, nv=nvals, null_actor=False, K=3):
            a = actor or mk(spar if sample == 1 else par, (count + nu) if sample == 1 else count, squash=1)
            c = critic or mk(vpar, vcount)
            return lib.mz_rollout_net(h, K, None if null_actor else C.byref(a), sample, 1, 2, C.byref(c) if with_critic else None, p(vals), p(nv),
                                      p(env._obs), p(rew), p(done), None, None, None, None, None, env._stream())

        def act_(net, sample=0, null=False):
            return lib.mz_net_act(h, None if null else C.byref(net), sample, 1, 2, p(env._obs), p(act), p(logp), env._stream())

        def val(net, null=False):
            return lib.mz_net_value(h, None if null else C.byref(net), p(env._obs), p(vals), env._stream())

        # every case through all three entries (the critic's through the two that take one)
        cases = [(dict(struct_size=40), b"struct_size"), (dict(n_hidden=3), b"n_hidden"), (dict(n_hidden=-1), b"n_hidden"),
                 (dict(hidden=(0, 3)), b"hidden[0]"), (dict(hidden=(5, 65)), b"hidden[1]"), (dict(n_hidden=1), b"hidden[1]"),
                 (dict(n_hidden=0, hidden=(5, 0)), b"hidden[0]"), (dict(activation=2), b"activation"), (dict(activation=-1), b"activation"),
                 (dict(squash=2), b"squash"), (dict(env_stride=count - 1), b"env_stride"), (dict(params_dev=None), b"params_dev")]
        for over, word in cases:
            bad = mk(par, count, **over)
            assert act_(bad) == MZ_ERR_ARG and b"actor" in err() and word in err(), (over, err())
            assert roll(actor=bad) == MZ_ERR_ARG and b"actor" in err() and word in err(), (over, err())
            if "env_stride" in over:
                over = dict(env_stride=vcount - 1)
            badc = mk(vpar, vcount, **over)
            assert val(badc) == MZ_ERR_ARG and b"critic" in err() and word in err(), (over, err())
            assert roll(critic=badc) == MZ_ERR_ARG and b"critic" in err() and word in err(), (over, err())
        squashed = mk(vpar, vcount, squash=1)
        assert val(squashed) == MZ_ERR_ARG and b"critic" in err() and b"squash" in err()
        assert roll(critic=squashed) == MZ_ERR_ARG and b"critic" in err() and b"squash" in err()
        assert act_(None, null=True) == MZ_ERR_ARG and b"actor" in err()
        assert val(None, null=True) == MZ_ERR_ARG and b"critic" in err()
        assert roll(null_actor=True) == MZ_ERR_ARG and b"actor" in err()
        for s in (2, -1):
            assert act_(mk(par, count), sample=s) == MZ_ERR_ARG and b"sample" in err()
            assert roll(sample=s) == MZ_ERR_ARG and b"sample" in err()
        # a sampling call counts log_std: the deterministic stride is refused, and the other way round
        assert act_(mk(par, count), sample=1) == MZ_ERR_ARG and b"env_stride" in err()
        assert act_(mk(spar, count + nu), sample=0) == MZ_ERR_ARG and b"env_stride" in err()
        # what the existing rollout entries refuse
        assert roll(K=0) == MZ_ERR_ARG and b"n_steps" in err()
        assert roll(K=65537) == MZ_ERR_ARG and b"n_steps" in err()
        assert lib.mz_rollout_net(h, 3, C.byref(mk(par, count)), 0, 1, 2, None, None, None, None, p(rew), p(done), None, None, None, None, None,
                                  env._stream()) == MZ_ERR_ARG and b"null" in err()
        assert lib.mz_bind_final_obs(h, None) == 0
        assert roll() == MZ_ERR_ARG and b"final_obs" in err() and b"next_value_seq_dev" in err()
        assert roll(nv=None) == 0 and roll(with_critic=False) == 0  # values alone, or no critic, need no terminal row
        assert lib.mz_bind_final_obs(h, p(env._final_obs)) == 0
        # the good calls pass, shared parameters too
        assert roll() == 0 and roll(sample=1) == 0 and roll(actor=mk(par, 0), critic=mk(vpar, 0)) == 0
        assert act_(mk(par, count)) == 0 and act_(mk(spar, count + nu), sample=1) == 0 and val(mk(vpar, vcount)) == 0
        # afterwards the env still steps
        obs, rew1, done1, _ = env.step(z(n, nu))
        torch.cuda.synchronize()
        assert torch.isfinite(obs).all() and tuple(rew1.shape) == (n,)
    finally:
        env.close()
