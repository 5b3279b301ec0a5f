"""Context inputs on the device: `context=` on policy_act / policy_sample / value / rollout_policy / rollout_policy_sample
(mz_net_eval_ctx, mz_net_value_ctx, mz_rollout_ctx).

Everything is compared by bit patterns.  The single calls go against numpy for affine and ReLU networks without squash
(policy.reference on policy.context_row); a rollout goes against its defining loop on a twin env — same id, num_envs, seed and
reset —

    contexts[k] = c;  [value(context=c)];  a, logp = policy_sample(context=c, noise_step + k);  step(a);
    the transition in torch where dones == 0;  [value(context=c) of the terminal / new row]

with the next value behind the transition: next_values[k] reads the context after it, which makes it values[k + 1] wherever the
episode goes on.  N = 70 leaves idle lane groups and a partial block, max_episode_steps = 7 with auto-reset resets every env
inside the K = 12 window; one case runs K = 260."""
import ctypes as C

import numpy as np
import pytest

import mujoco_maze_amd as mm
from mujoco_maze_amd import _capi, policy
from tests.test_deep_policy_api import random_net
from tests.test_gpu_deep_policy import _view_env
from tests.test_gpu_rollout import _same

pytestmark = pytest.mark.gpu
MZ_ERR_ARG = -1
N, T, K, CDIM, D = 70, 7, 12, 5, 2
SEED, STEP0 = 1234, 40
ACTION_SCALE = 0.9


def _make(env_id, n=N):
    if env_id == "view":
        return _view_env(n, auto_reset=True, seed=5, max_episode_steps=T)
    return mm.make(env_id, num_envs=n, auto_reset=True, seed=5, max_episode_steps=T)


def _t(env, a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a), device=env.device)


def torch_zeros(env, count):
    import torch

    return torch.zeros(count, dtype=torch.float32, device=env.device)


def _ctx(env, seed=7, cdim=CDIM):
    return _t(env, (2 * np.random.default_rng(seed).normal(size=(env.num_envs, cdim))).astype(np.float32))


def _norm(env, clip=5.0):
    rng = np.random.default_rng(3)
    mean, inv = rng.normal(0.0, 0.3, env.obs_dim).astype(np.float32), rng.uniform(0.5, 2.0, env.obs_dim).astype(np.float32)
    env.bind_obs_norm(_t(env, mean), _t(env, inv), clip)
    return mean, inv, clip


def _actor(env, hidden, activation, per_env, seed, cdim=CDIM, sample=True, squash=False, head=False, **extra):
    """kwargs of the policy methods for a random actor on [obs | context]; log_std around -1"""
    rng = np.random.default_rng(seed)
    nu = env.nu
    rows = env.num_envs if per_env else None
    if head:
        p = random_net(rng, env.obs_dim + cdim, 2 * nu, hidden, rows=rows)
        p[..., -nu:] += rng.uniform(-1.5, -0.5, p.shape[:-1] + (nu,)).astype(np.float32)
        extra = dict(extra, log_std="state")
    else:
        p = random_net(rng, env.obs_dim + cdim, nu, hidden, rows=rows, log_std=sample)
    return dict(params=_t(env, p), hidden=hidden, activation=activation, squash=squash, action_scale=ACTION_SCALE if squash else 1.0, **extra)


def _critic(env, hidden, activation, per_env, seed, cdim=CDIM):
    p = random_net(np.random.default_rng(seed), env.obs_dim + cdim, 1, hidden, rows=env.num_envs if per_env else None)
    return dict(value_params=_t(env, p), value_hidden=hidden, value_activation=activation)


def _value(env, crt, c, obs=None):
    return env.value(crt["value_params"], obs=obs, hidden=crt["value_hidden"], activation=crt["value_activation"], context=c)


def _loop(env, steps, pol, crt, c, dims, sample=True, step0=STEP0):
    """the defining loop on env with the context c (updated in place): the stacked rows and the last observation"""
    import torch

    rows = {}
    for k in range(steps):
        r = {"contexts": c.clone()}
        s_old = env._obs[:, :dims].clone() if dims else None
        if crt:
            r["values"] = _value(env, crt, c)
        if sample:
            a, r["logp"] = env.policy_sample(noise_seed=SEED, noise_step=step0 + k, context=c, **pol)
        else:
            a = env.policy_act(context=c, **pol)
        obs, rew, done, info = env.step(a)
        fin = done != 0
        r["next_observations"] = torch.where(fin.unsqueeze(1), info["final_observation"], obs)
        if dims:  # a sum, then a difference: two roundings
            tmp = c[:, :dims] + s_old
            new = tmp - r["next_observations"][:, :dims]
            c[:, :dims] = torch.where(fin.unsqueeze(1), c[:, :dims], new)
        if crt:
            r["next_values"] = torch.where(fin, _value(env, crt, c, info["final_observation"]), _value(env, crt, c))
        r.update(actions=a, observations=obs, reward=rew, done=done, goal_index=info["goal_index"], position=info["position"],
                 reward_forward=info["reward_forward"], reward_ctrl=info["reward_ctrl"])
        for key, x in r.items():
            rows.setdefault(key, []).append(x.clone())
    return {k: torch.stack(v) for k, v in rows.items()}, obs.clone(), info["final_observation"].clone()


def _call(env, steps, pol, crt, c, dims, sample=True, step0=STEP0):
    kw = dict(steps=steps, return_obs=True, return_actions=True, return_next_obs=True, context=c, return_contexts=True,
              context_update="relative" if dims else None, context_dims=dims if dims else None, **pol, **(crt or {}))
    if sample:
        return env.rollout_policy_sample(noise_seed=SEED, noise_step=step0, **kw)
    return env.rollout_policy(**kw)


def _assert_equal(want, obs_a, fin_a, out, ca, cb, ea, eb):
    obs, rew, done, info = out
    got = dict(info, reward=rew, done=done)
    for key, x in want.items():
        assert key in got and _same(got[key].contiguous(), x), key
    assert _same(obs, obs_a) and _same(info["final_observation"], fin_a)
    assert _same(ca, cb), "the context afterwards"
    for x, y in zip(ea.get_state(), eb.get_state()):
        assert _same(x, y)
    assert _same(ea.status(), eb.status())


def _twin(env_id, dims, steps=K, n=N, sample=True, critic=True, prepare=None, actor=None, seed=11):
    """env A: the defining loop; env B: one call.  Returns the loop's rows."""
    import torch

    ea, eb = _make(env_id, n), _make(env_id, n)
    try:
        for e in (ea, eb):
            if prepare:
                prepare(e)
            e.reset(seed=seed)
        assert _same(ea._obs, eb._obs)
        pol = (actor or (lambda e: _actor(e, (64, 64), "relu", True, seed + 1, sample=sample)))(ea)
        crt = _critic(ea, (64, 64), "relu", True, seed + 2) if critic else None
        ca, cb = _ctx(ea), _ctx(eb)
        c0 = ca.clone()
        want, obs_a, fin_a = _loop(ea, steps, pol, crt, ca, dims, sample)
        out = _call(eb, steps, pol, crt, cb, dims, sample)
        torch.cuda.synchronize()
        _assert_equal(want, obs_a, fin_a, out, ca, cb, ea, eb)
        assert _same(want["contexts"][0], c0)
        assert int((want["done"] != 0).sum(dim=0).min()) >= 1 or steps < T, "every env resets inside the window"
        if dims:
            moved = (want["contexts"][1:].view(torch.int32) != want["contexts"][:-1].view(torch.int32))
            assert bool(moved[:, :, :dims].any()) and not bool(moved[:, :, dims:].any())
            # no transition crosses an episode end
            ended = want["done"][:-1] != 0
            assert not bool(moved[ended].any())
            if crt:  # the next value reads the context behind the transition: it is the next step's value where the episode goes on
                assert torch.equal(want["next_values"][:-1][~ended].view(torch.int32), want["values"][1:][~ended].view(torch.int32))
        else:
            assert _same(ca, c0)
        return want
    finally:
        ea.close(); eb.close()


# ---------------------------------------------------------------------------------------------- 1. the single calls against numpy
@pytest.mark.parametrize("bound", [False, True], ids=["unbound", "bound"])
@pytest.mark.parametrize("per_env", [False, True], ids=["shared", "per-env"])
@pytest.mark.parametrize("hidden,activation", [(0, "tanh"), ((64, 64), "relu")], ids=["affine", "relu64x64"])
def test_single_calls_equal_numpy(hidden, activation, per_env, bound):
    env = _make("PointUMaze-v0")
    try:
        obs = env.reset(seed=3).clone()
        norm = _norm(env) if bound else ()
        c = _ctx(env)
        row = policy.context_row(obs.cpu().numpy(), c.cpu().numpy(), *norm)
        det = _actor(env, hidden, activation, per_env, 21, sample=False)
        a = env.policy_act(context=c, **det)
        assert np.array_equal(a.cpu().numpy().view(np.int32), policy.reference(det["params"].cpu().numpy(), row, env.nu, hidden, activation=activation).view(np.int32))
        # policy_sample: the device's eps is its own libm's (logf, cosf: within 1e-5 of numpy's, tests/test_gpu_policy_sample.py, never
        # its bits), so the draw is taken from the device — an all-zero network with log_std 0 returns eps itself — and numpy does
        # everything else: with log_std 0, s = expf(0) = 1 and p = s * eps = eps exactly, so a = m + eps in one rounding, and the
        # log-prob is four float32 operations per unit on eps
        f = np.float32
        nu = env.nu
        zero = torch_zeros(env, policy.param_count(env.obs_dim + CDIM, nu, 0, stochastic=True))
        eps_t, lp0 = env.policy_sample(zero, noise_seed=SEED, noise_step=STEP0, context=c)
        eps = eps_t.cpu().numpy()
        sto = _actor(env, hidden, activation, per_env, 22)
        sto["params"][..., -nu:] = 0.0
        a, lp = env.policy_sample(noise_seed=SEED, noise_step=STEP0, context=c, **sto)
        m = policy.reference(sto["params"][..., :-nu].cpu().numpy(), row, nu, hidden, activation=activation)
        wa = (m + eps).astype(f)
        wlp = np.zeros(N, f)
        for u in range(nu):
            t = ((f(-0.5) * (eps[:, u] * eps[:, u]).astype(f)).astype(f) - f(0.0)).astype(f)
            wlp = (wlp + (t - f(0.9189385)).astype(f)).astype(f)
        assert np.array_equal(a.cpu().numpy().view(np.int32), wa.view(np.int32)) and np.array_equal(lp.cpu().numpy().view(np.int32), wlp.view(np.int32))
        assert _same(lp, lp0) and np.abs(eps - policy.noise(SEED, STEP0, range(N), nu)).max() < 1e-5
        crt = _critic(env, hidden, activation, per_env, 23)
        v = _value(env, crt, c)
        assert np.array_equal(v.cpu().numpy().view(np.int32), policy.value_reference(crt["value_params"].cpu().numpy(), row, hidden, activation=activation).view(np.int32))
        # an explicit observation tensor, and a context given as numpy
        v2 = _value(env, crt, c.cpu().numpy(), obs=obs)
        assert _same(v, v2)
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------- 2. zero weights on the context columns
def _widen(small, obs_dim, cdim, first_width):
    """the packed vector(s) of the network with `cdim` zero rows behind the obs_dim rows of its first layer"""
    cut = obs_dim * first_width
    zeros = np.zeros(small.shape[:-1] + (cdim * first_width,), np.float32)
    return np.concatenate([small[..., :cut], zeros, small[..., cut:]], axis=-1)


@pytest.mark.parametrize("hidden,activation", [(0, "tanh"), (5, "tanh"), ((64, 64), "relu")], ids=["affine", "tanh5", "relu64x64"])
def test_zero_context_weights_return_the_bits_of_the_call_without_a_context(hidden, activation):
    import torch

    ea, eb = _make("PointUMaze-v0"), _make("PointUMaze-v0")
    try:
        for e in (ea, eb):
            e.reset(seed=3)
        rng = np.random.default_rng(31)
        od, nu = ea.obs_dim, ea.nu
        widths = policy.net_shape(hidden)[0]
        small = random_net(rng, od, nu, hidden, rows=N, log_std=True)
        vsmall = random_net(rng, od, 1, hidden, rows=N)
        wide = _widen(small, od, CDIM, widths[0] if widths else nu)
        vwide = _widen(vsmall, od, CDIM, widths[0] if widths else 1)
        net = dict(hidden=hidden, activation=activation, squash=True, action_scale=ACTION_SCALE)
        c = _ctx(eb)
        ndet = policy.param_count(od, nu, hidden)
        assert _same(eb.policy_act(_t(eb, wide[:, : wide.shape[1] - nu]), context=c, **net), ea.policy_act(_t(ea, small[:, :ndet]), **net))
        xa, xb = ea.policy_sample(_t(ea, small), noise_seed=SEED, noise_step=STEP0, **net), eb.policy_sample(_t(eb, wide), noise_seed=SEED, noise_step=STEP0,
                                                                                                              context=c, **net)
        assert _same(xa[0], xb[0]) and _same(xa[1], xb[1])
        assert _same(ea.value(_t(ea, vsmall), hidden=hidden, activation=activation), eb.value(_t(eb, vwide), hidden=hidden, activation=activation, context=c))
        crit = dict(value_hidden=hidden, value_activation=activation)
        for sample in (True, False):
            pa, pb = (small, wide) if sample else (small[:, :ndet], wide[:, : wide.shape[1] - nu])
            kw = dict(steps=K, return_obs=True, return_actions=True, return_next_obs=True, **net, **crit)
            if sample:
                kw.update(noise_seed=SEED, noise_step=STEP0)
            fa, fb = (ea.rollout_policy_sample, eb.rollout_policy_sample) if sample else (ea.rollout_policy, eb.rollout_policy)
            oa = fa(_t(ea, pa), value_params=_t(ea, vsmall), **kw)
            ob = fb(_t(eb, pb), value_params=_t(eb, vwide), context=c, context_update="relative", context_dims=D, **kw)
            torch.cuda.synchronize()
            assert _same(oa[0], ob[0]) and _same(oa[1], ob[1]) and _same(oa[2], ob[2])
            for key in oa[3]:
                assert _same(oa[3][key].contiguous(), ob[3][key].contiguous()), key
            for x, y in zip(ea.get_state(), eb.get_state()):
                assert _same(x, y)
    finally:
        ea.close(); eb.close()


# ---------------------------------------------------------------------------------------------- 3. a rollout against its defining loop
ENVS = ["PointUMaze-v0", "PointPush-v0", "SwimmerUMaze-v0", "ReacherUMaze-v0", "view"]


@pytest.mark.parametrize("dims", [0, D], ids=["hold", "relative"])
@pytest.mark.parametrize("env_id", ENVS)
def test_rollout_equals_the_defining_loop(env_id, dims):
    """a per-env ReLU (64, 64) actor and critic, return_next_obs"""
    _twin(env_id, dims)


@pytest.mark.parametrize("dims", [0, D], ids=["hold", "relative"])
def test_ant_rollout_equals_the_defining_loop(dims):
    _twin("AntUMaze-v0", dims, steps=4)


def test_rollout_across_the_launch_split():
    want = _twin("PointUMaze-v0", D, steps=260)
    assert int((want["done"] != 0).sum(dim=0).min()) >= 260 // T


def test_rollout_with_a_bound_normaliser():
    _twin("PointUMaze-v0", D, prepare=_norm)
    _twin("SwimmerUMaze-v0", 0, prepare=_norm)


def test_rollout_with_the_sac_head():
    _twin("PointUMaze-v0", D, actor=lambda e: _actor(e, (64, 64), "relu", True, 12, squash=True, head=True, squashed_logp=True))


def test_rollout_with_noise_on_the_action():
    _twin("PointUMaze-v0", D, actor=lambda e: _actor(e, 5, "tanh", False, 12, squash=True, noise="action"))


def test_deterministic_rollout():
    _twin("PointUMaze-v0", D, sample=False)
    _twin("ReacherUMaze-v0", D, sample=False, critic=False, actor=lambda e: _actor(e, 5, "tanh", False, 12, sample=False, squash=True))


# ---------------------------------------------------------------------------------------------- 4. two calls equal one
@pytest.mark.parametrize("env_id", ["PointUMaze-v0", "AntUMaze-v0"])
def test_two_calls_equal_one(env_id):
    import torch

    steps = 12 if env_id.startswith("Point") else 4
    ea, eb = _make(env_id), _make(env_id)
    try:
        for e in (ea, eb):
            e.reset(seed=11)
        pol, crt = _actor(ea, (64, 64), "relu", True, 12), _critic(ea, (64, 64), "relu", True, 13)
        ca, cb = _ctx(ea), _ctx(eb)
        one = _call(ea, steps, pol, crt, ca, D)
        one = (one[0].clone(), one[1].clone(), one[2].clone(), {k: v.clone() for k, v in one[3].items()})
        h = steps // 2
        first = _call(eb, h, pol, crt, cb, D)
        first = (first[1].clone(), first[2].clone(), {k: v.clone() for k, v in first[3].items()})
        second = _call(eb, h, pol, crt, cb, D, step0=STEP0 + h)
        torch.cuda.synchronize()
        assert _same(one[0], second[0]) and _same(ca, cb)
        assert _same(one[1], torch.cat([first[0], second[1]])) and _same(one[2], torch.cat([first[1], second[2]]))
        for key in one[3]:
            if key != "final_observation":
                assert _same(one[3][key].contiguous(), torch.cat([first[2][key], second[3][key]]).contiguous()), key
        for x, y in zip(ea.get_state(), eb.get_state()):
            assert _same(x, y)
    finally:
        ea.close(); eb.close()


# ---------------------------------------------------------------------------------------------- 5. a NaN stays in its env
@pytest.mark.parametrize("env_id", ["PointUMaze-v0", "AntUMaze-v0"])
def test_a_nan_context_reaches_its_own_env_only(env_id):
    import torch

    steps = K if env_id.startswith("Point") else 4
    ea, eb = _make(env_id), _make(env_id)
    try:
        for e in (ea, eb):
            e.reset(seed=11)
        pol = _actor(ea, (64, 64), "relu", True, 12, squash=True, head=True)  # a head: the log-prob depends on the network
        crt = _critic(ea, (64, 64), "relu", True, 13)
        ca, cb = _ctx(ea), _ctx(eb)
        cb[3, CDIM - 1] = float("nan")  # a column that holds
        oa, ob = _call(ea, steps, pol, crt, ca, D), _call(eb, steps, pol, crt, cb, D)
        torch.cuda.synchronize()
        keep = torch.arange(N, device=ea.device) != 3
        assert _same(oa[0][keep], ob[0][keep]) and _same(oa[1][:, keep], ob[1][:, keep]) and _same(oa[2][:, keep], ob[2][:, keep])
        for key in oa[3]:
            x, y = oa[3][key], ob[3][key]
            assert _same(x[keep], y[keep]) if key == "final_observation" else _same(x[:, keep].contiguous(), y[:, keep].contiguous()), key
        for key in ("actions", "logp", "values", "next_values"):
            assert bool(torch.isnan(ob[3][key][0, 3]).any()) and not bool(torch.isnan(oa[3][key][:, 3]).any()), key
        assert _same(ca[keep], cb[keep])
        for x, y in zip(ea.get_state(), eb.get_state()):
            assert _same(x[keep], y[keep])
        assert _same(ea.status()[keep], eb.status()[keep])
    finally:
        ea.close(); eb.close()


# ---------------------------------------------------------------------------------------------- 6. Q(s, a)
def test_value_with_the_actions_as_context_is_q():
    env = _make("AntUMaze-v0")
    try:
        s = env.reset(seed=3).clone()
        rng = np.random.default_rng(41)
        a = _t(env, rng.uniform(-1, 1, (N, env.nu)).astype(np.float32))
        for per_env in (False, True):
            q = random_net(rng, env.obs_dim + env.nu, 1, (64, 64), rows=N if per_env else None)
            got = env.value(_t(env, q), obs=s, hidden=(64, 64), activation="relu", context=a)
            want = policy.value_reference(q, np.concatenate([s.cpu().numpy(), a.cpu().numpy()], axis=1), (64, 64), activation="relu")
            assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32))
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------- 7. without a context nothing changes
def _raw_rollout(env, entry, steps, pol, crt, ctx=None):
    """one rollout through `entry` (mz_rollout_head or mz_rollout_ctx with a NULL context) on buffers of its own"""
    import torch

    n, dev = env.num_envs, env.device
    f = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=dev)
    out = dict(reward=f(steps, n), done=torch.zeros((steps, n), dtype=torch.uint8, device=dev), goal=torch.zeros((steps, n), dtype=torch.int32, device=dev),
               info=f(steps, n, 4), obs_seq=f(steps, n, env.obs_dim), actions=f(steps, n, env.nu), logp=f(steps, n), values=f(steps, n),
               next_values=f(steps, n), next_obs=f(steps, n, env.obs_dim))
    widths, act = policy.net_shape(pol["hidden"], pol["activation"])
    p, vp = pol["params"], crt["value_params"]
    io = _capi.make_rollout_io(steps, actor=_capi.make_net(p.data_ptr(), p.shape[1], widths, act, pol["squash"], pol["action_scale"]),
                               noise=_capi.make_noise(_capi.NOISE_PRE_SQUASH, SEED, STEP0), critic=_capi.make_net(vp.data_ptr(), vp.shape[1], widths, act),
                               obs_dev=env._obs.data_ptr(), reward_dev=out["reward"].data_ptr(), done_dev=out["done"].data_ptr(),
                               goal_idx_dev=out["goal"].data_ptr(), info_dev=out["info"].data_ptr(), obs_seq_dev=out["obs_seq"].data_ptr(),
                               actions_seq_dev=out["actions"].data_ptr(), logp_seq_dev=out["logp"].data_ptr(), value_seq_dev=out["values"].data_ptr(),
                               next_value_seq_dev=out["next_values"].data_ptr(), next_obs_seq_dev=out["next_obs"].data_ptr())
    if entry == "mz_rollout_ctx":
        rc = env._lib.mz_rollout_ctx(env._h, C.byref(io), None, ctx, env._stream())
    else:
        rc = env._lib.mz_rollout_head(env._h, C.byref(io), None, env._stream())
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize("env_id", ["PointUMaze-v0", "SwimmerUMaze-v0", "AntUMaze-v0"])
def test_a_null_context_is_the_existing_entry(env_id):
    steps = K if not env_id.startswith("Ant") else 4
    ea, eb = _make(env_id), _make(env_id)
    try:
        for e in (ea, eb):
            e.reset(seed=11)
        pol, crt = _actor(ea, (64, 64), "relu", True, 12, cdim=0), _critic(ea, (64, 64), "relu", True, 13, cdim=0)
        rca, oa = _raw_rollout(ea, "mz_rollout_head", steps, pol, crt)
        rcb, ob = _raw_rollout(eb, "mz_rollout_ctx", steps, pol, crt)
        assert rca == rcb == 0
        for key in oa:
            assert _same(oa[key], ob[key]), key
        assert _same(ea._obs, eb._obs) and _same(ea._final_obs, eb._final_obs)
        for x, y in zip(ea.get_state(), eb.get_state()):
            assert _same(x, y)
        assert _same(ea.status(), eb.status())
        # and the Python methods without context= take the paths they took: the same call through rollout_policy_sample
        ec = _make(env_id)
        try:
            ec.reset(seed=11)
            oc = ec.rollout_policy_sample(steps=steps, noise_seed=SEED, noise_step=STEP0, return_obs=True, return_actions=True, return_next_obs=True, **pol, **crt)
            assert _same(oc[1], oa["reward"]) and _same(oc[2], oa["done"]) and _same(oc[3]["actions"], oa["actions"]) and _same(oc[3]["logp"], oa["logp"])
            assert _same(oc[3]["values"], oa["values"]) and _same(oc[3]["next_values"], oa["next_values"]) and _same(oc[0], ea._obs)
        finally:
            ec.close()
    finally:
        ea.close(); eb.close()


# ---------------------------------------------------------------------------------------------- refusals that need a handle
def test_the_library_refuses_a_bad_context_and_leaves_the_handle_alone():
    import torch

    env = _make("PointUMaze-v0")
    try:
        env.reset(seed=11)
        pol, crt = _actor(env, (64, 64), "relu", True, 12), _critic(env, (64, 64), "relu", True, 13)
        c = _ctx(env)
        before = [x.clone() for x in env.get_state()] + [env._obs.clone(), c.clone()]
        ok = dict(struct_size=C.sizeof(_capi.MzContext), dim=CDIM, update=_capi.CTX_RELATIVE, rel_dims=D, reserved=0, ctx_dev=c.data_ptr(), ctx_seq_dev=None)
        bad = [(dict(struct_size=36), "struct_size"), (dict(dim=0), "dim"), (dict(dim=33), "dim"), (dict(update=2), "update"),
               (dict(rel_dims=0), "rel_dims"), (dict(rel_dims=CDIM + 1), "rel_dims"), (dict(update=_capi.CTX_HOLD), "rel_dims"),
               (dict(reserved=1), "reserved"), (dict(ctx_dev=None), "ctx_dev"), (dict(dim=CDIM - 1), "env_stride")]
        for change, names in bad:
            ctx = _capi.MzContext(**dict(ok, **change))
            rc, _ = _raw_rollout(env, "mz_rollout_ctx", 3, pol, crt, C.byref(ctx))
            msg = env._lib.mz_last_error(env._h).decode()
            assert rc == MZ_ERR_ARG and names in msg and msg.startswith("mz_rollout_ctx"), (change, msg)
        # the single calls: the same struct checks, and no transition or sequence there
        widths, act = policy.net_shape(pol["hidden"], pol["activation"])
        net = _capi.make_net(pol["params"].data_ptr(), pol["params"].shape[1], widths, act)
        vnet = _capi.make_net(crt["value_params"].data_ptr(), crt["value_params"].shape[1], widths, act)
        nz = _capi.make_noise(_capi.NOISE_PRE_SQUASH, SEED, STEP0)
        out, lp = torch.empty((N, env.nu), device=env.device), torch.empty(N, device=env.device)
        hold = dict(ok, update=_capi.CTX_HOLD, rel_dims=0)
        for change, names in [(dict(struct_size=0), "struct_size"), (dict(dim=-1), "dim"), (dict(update=_capi.CTX_RELATIVE, rel_dims=D), "update"),
                              (dict(rel_dims=1), "rel_dims"), (dict(reserved=-1), "reserved"), (dict(ctx_dev=None), "ctx_dev"),
                              (dict(ctx_seq_dev=c.data_ptr()), "ctx_seq_dev"), (dict(dim=1), "env_stride")]:
            ctx = _capi.MzContext(**dict(hold, **change))
            rc = env._lib.mz_net_eval_ctx(env._h, C.byref(net), None, C.byref(nz), C.byref(ctx), env._obs.data_ptr(), out.data_ptr(), lp.data_ptr(), env._stream())
            msg = env._lib.mz_last_error(env._h).decode()
            assert rc == MZ_ERR_ARG and names in msg and msg.startswith("mz_net_eval_ctx"), (change, msg)
            rc = env._lib.mz_net_value_ctx(env._h, C.byref(vnet), C.byref(ctx), env._obs.data_ptr(), lp.data_ptr(), env._stream())
            msg = env._lib.mz_last_error(env._h).decode()
            assert rc == MZ_ERR_ARG and names in msg and msg.startswith("mz_net_value_ctx"), (change, msg)
        torch.cuda.synchronize()
        after = [x.clone() for x in env.get_state()] + [env._obs.clone(), c.clone()]
        assert all(_same(x, y) for x, y in zip(before, after))
        # the Python side: raised before any device call
        for kw in (dict(context=c[:, :0]), dict(context=c[:-1]), dict(context=torch.zeros((N, 33), device=env.device)), dict(context=c[:, :3])):
            with pytest.raises(ValueError):
                env.policy_sample(noise_seed=SEED, noise_step=STEP0, **dict(pol, **kw))
        for kw in (dict(context_update="relative"), dict(context_update="relative", context_dims=CDIM + 1), dict(context_dims=2),
                   dict(context_update="absolute", context_dims=2)):
            with pytest.raises(ValueError):
                env.rollout_policy_sample(steps=3, context=c, **pol, **kw)
        with pytest.raises(ValueError):  # a rollout updates the context in place: no copy is made behind the caller's back
            env.rollout_policy_sample(steps=3, context=c.cpu().numpy(), **pol)
        with pytest.raises(ValueError):
            env.rollout_policy_sample(steps=3, return_contexts=True, **_actor(env, (64, 64), "relu", True, 12, cdim=0))
    finally:
        env.close()
