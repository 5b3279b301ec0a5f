"""K = 64 steps as 64 `env.step` calls against one `env.rollout` of the same [64, N, nu] action tensor, at 4096 envs under auto-reset:
PointUMaze-v0, SwimmerUMaze-v0, ReacherUMaze-v0, PointPush-v0 (fused kernels) and AntUMaze-v0 (the step's launches in a loop inside
mz_rollout).  Both legs run in one process, alternating, three repeats each after a warm-up of both; a leg repeats its window until
at least `--seconds` of work has passed, with a device synchronise around the host clock.  Whole-call wall clock, inputs resident.
    python tools/rollout_bench.py [--envs N] [--steps K] [--seconds S] [--repeats R] [--ids a,b,..] [--out FILE]
With --policy H the three closed-loop ways to run the same K steps of one shared policy (H = 0: affine; else one tanh hidden layer of H
units) are timed instead, same protocol: K x (torch policy + env.step), K x (env.policy_act + env.step), one env.rollout_policy.
    python tools/rollout_bench.py --policy 32 [--ids PointUMaze-v0,SwimmerUMaze-v0,AntUMaze-v0]
With --policy H --sample the same K steps with a sampled action each (log_std = -0.5 on every unit): K x (env.policy_sample + env.step),
one env.rollout_policy_sample, and the deterministic env.rollout_policy at the same shape beside them.
    python tools/rollout_bench.py --policy 32 --sample
With --policy H --sample --critic HV one actor-critic collection window (a shared critic with HV hidden units, 0 = affine; gamma 0.99,
lambda 0.95): K x (env.policy_sample + env.step) with the rows kept, a torch critic over the [K, N, obs_dim] rows and a torch GAE loop
of K iterations; one env.rollout_policy_sample(..., value_params=, gae=); and the one-call rollout without a critic beside them.  (The
torch leg bootstraps every row from the value of the NEXT row it holds: the terminal rows are gone, which is the gap the one-call path
closes — its cost is what this compares, not its result.)
    python tools/rollout_bench.py --policy 32 --sample --critic 32 --steps 128 --ids PointUMaze-v0,SwimmerUMaze-v0,AntUMaze-v0
--policy and --critic also take two widths, `64,64`: a network with two hidden layers (mz_net_act / mz_rollout_net), the torch legs then
run a two-layer torch MLP; --activation tanh|relu chooses the hidden units of both networks (relu goes through the same entries).
    python tools/rollout_bench.py --policy 64,64 --sample --critic 64,64 --activation relu --steps 128
With --obs-norm every --policy mode binds an observation normaliser first (env.bind_obs_norm: mean and 1 / (std + 0.1) of the rows of
a few random steps, clip 5), so that all its legs evaluate their networks on normalised rows; a torch network normalises and clamps
in torch.
    python tools/rollout_bench.py --policy 64,64 --sample --critic 64,64 --steps 128 --obs-norm --ids PointUMaze-v0,SwimmerUMaze-v0
With --policy H --sample --next-obs one off-policy collection window, the transitions (s, a, r, s', d) of K steps: K x (env.policy_sample +
env.step + torch.where(done, final_observation, obs)) with the rows kept — the only way to the per-step terminal rows without
return_next_obs —; one env.rollout_policy_sample(..., return_obs, return_actions, return_next_obs); and the same call without the next
rows beside them.  --noise action puts the noise on the action in every leg (TD3 / DDPG exploration; log_std = log(0.1) on every unit).
    python tools/rollout_bench.py --policy 64,64 --activation relu --sample --next-obs --noise action --steps 128 --ids PointUMaze-v0,SwimmerUMaze-v0,AntUMaze-v0
With --policy H --head state one SAC collection window: the actor's output layer carries the raw log-stds (clamped to (-20, 2); the
second nn.Linear of a SAC actor, small weights, bias -0.5), squashed actions, and with --squashed-logp the log-probability of the
squashed action.  K x (env.policy_sample(log_std="state") + env.step + torch.where on the terminal rows) with the rows kept against
one env.rollout_policy_sample(..., log_std="state", return_obs, return_actions, return_next_obs), and that call without the next rows.
    python tools/rollout_bench.py --policy 64,64 --activation relu --head state --squashed-logp --steps 128 --ids PointUMaze-v0,SwimmerUMaze-v0,AntUMaze-v0
With --policy H --sample --context C [--relative D] one goal-conditioned collection window: a [N, C] context behind the observation
(both the torch-free legs below read [obs | context]; --relative D applies HIRO's goal transition to the first D entries after every
step).  K x (env.policy_sample(context=) + env.step + the transition in torch) with the rows kept against one
env.rollout_policy_sample(..., context=, context_update=, return_next_obs, return_contexts), and the call without a context at the
same shape (a network on obs_dim inputs) beside them.
    python tools/rollout_bench.py --policy 64,64 --activation relu --sample --context 15 --relative 3 --steps 10 --ids PointUMaze-v0,SwimmerUMaze-v0,AntUMaze-v0
With --policy H --head state --critic HV one SAC-style window with a critic: K x (torch actor with its head + torch critic + env.step) —
the loop a user runs without the device networks — against one rollout_policy_sample(log_std="state", value_params=) call, and the cost
of one actor evaluation, one critic evaluation and one env.step.  Widths above 64 (`256,256`) set option "wide_nets" = 1 on every env
by themselves; --wide-nets 2 puts narrower networks on the tiled kernel as well (the A/B of the two kernel families); --per-env gives
every env its own network:
    python tools/rollout_bench.py --policy 256,256 --activation relu --head state --critic 256,256 --ids AntUMaze-v0,PointUMaze-v0
    python tools/rollout_bench.py --policy 64,64 --activation relu --head state --critic 64,64 --wide-nets 2 [--per-env] --ids AntUMaze-v0
Kernel durations come from a run of their own:  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/rollout_bench.py --seconds 0.2"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import mujoco_maze_amd as mm  # noqa: E402

IDS = ["PointUMaze-v0", "SwimmerUMaze-v0", "ReacherUMaze-v0", "PointPush-v0", "AntUMaze-v0"]


def leg(fn, windows_min, seconds, dev):
    """env-steps per second of `fn` (one K-step window per call): windows until `seconds` have passed, at least `windows_min`."""
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    done = 0
    while True:
        for _ in range(windows_min):
            fn()
        done += windows_min
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return done, dt


WIDE_NETS = 0  # option "wide_nets" of every env of this run (main: from the widths and --wide-nets)


def make_env(env_id, n, dev):
    env = mm.make(env_id, num_envs=n, auto_reset=True, device=dev, force_vec=True)
    if WIDE_NETS:
        env.set_option("wide_nets", WIDE_NETS)
    return env


def max_width():
    from mujoco_maze_amd import policy

    return policy.MAX_WIDTH if WIDE_NETS else policy.MAX_HIDDEN


def hidden_arg(text):
    """`32` -> 32, `64,64` -> (64, 64)"""
    w = tuple(int(x) for x in text.split(","))
    return w[0] if len(w) == 1 else w


def build_net(lin, obs_dim, nout, hidden, activation, dev, log_std=None):
    """One network as (packed params on the device, the same network as a torch function of [R, obs_dim] rows); lin(out, fan_in)
    draws one layer's (W, b), first layer first."""
    from mujoco_maze_amd import policy

    sizes = (obs_dim,) + policy.net_shape(hidden, activation, max_width=max_width())[0] + (nout,)
    layers = [lin(o, i) for i, o in zip(sizes[:-1], sizes[1:])]
    params = torch.as_tensor(policy.pack_mlp(layers, log_std=log_std, max_width=max_width()), device=dev)
    wts = [(W.T.contiguous(), b) for W, b in layers]
    f = torch.tanh if activation == "tanh" else torch.relu

    def fn(obs):
        for Wt, b in wts[:-1]:
            obs = f(torch.addmm(b, obs, Wt))
        return torch.addmm(wts[-1][1], obs, wts[-1][0])

    return params, fn


def bind_norm(env, on, dev, g):
    """With `on`: binds a normaliser built from the rows of four random steps and returns what a torch network applies to its rows;
    else the identity.  The env is reset afterwards, so that every leg starts as it does without a normaliser."""
    if not on:
        return lambda obs: obs
    lo, hi = torch.as_tensor(env.action_space.low, device=dev), torch.as_tensor(env.action_space.high, device=dev)
    rows = torch.stack([env.step(lo + (hi - lo) * torch.rand((env.num_envs, env.nu), device=dev, generator=g))[0].clone() for _ in range(4)])
    rows = torch.nan_to_num(rows.view(-1, env.obs_dim))
    mean, inv_std, clip = rows.mean(dim=0).contiguous(), (1.0 / (rows.std(dim=0) + 0.1)).contiguous(), 5.0
    env.bind_obs_norm(mean, inv_std, clip)
    env.reset(seed=20260928)
    return lambda obs: torch.clamp((obs - mean) * inv_std, -clip, clip)


def bench(env_id, n, K, seconds, repeats):
    dev = torch.device("cuda", 0)
    env = make_env(env_id, n, dev)
    env.reset(seed=20260928)
    g = torch.Generator(device=dev).manual_seed(1234)
    lo, hi = torch.as_tensor(env.action_space.low, device=dev), torch.as_tensor(env.action_space.high, device=dev)
    acts = (lo + (hi - lo) * torch.rand((K, n, env.nu), device=dev, generator=g)).contiguous()
    rows = [acts[k] for k in range(K)]

    def stepping():
        for k in range(K):
            env.step(rows[k])

    def rollout():
        env.rollout(acts)

    for _ in range(4):  # warm-up of both legs: code objects loaded, output tensors of this K allocated, episodes in their steady mix
        stepping(); rollout()
    res = {"step": [], "rollout": []}
    for _ in range(repeats):
        for name, fn in (("step", stepping), ("rollout", rollout)):
            w, dt = leg(fn, 4, seconds, dev)
            res[name].append(n * K * w / dt)
    bad = int((env.status() & 3).ne(0).sum())
    fused = env.launch_info()["rollout_fused"]
    env.close()
    return {"env": env_id, "envs": n, "steps_per_window": K, "fused": fused, "flagged_envs": bad,
            "step_env_steps_per_s": res["step"], "rollout_env_steps_per_s": res["rollout"]}


def bench_policy(env_id, n, K, H, seconds, repeats, ACT="tanh", obs_norm=False):
    """K closed-loop steps of one shared policy, three ways: torch policy + step, policy_act + step, one rollout_policy."""
    dev = torch.device("cuda", 0)
    env = make_env(env_id, n, dev)
    env.reset(seed=20260928)
    g = torch.Generator(device=dev).manual_seed(1234)
    nrm = bind_norm(env, obs_norm, dev, g)

    def lin(out, fan_in):
        k = fan_in ** -0.5
        return (2 * torch.rand((out, fan_in), device=dev, generator=g) - 1) * k, (2 * torch.rand(out, device=dev, generator=g) - 1) * k

    params, torch_policy = build_net(lin, env.obs_dim, env.nu, H, ACT, dev)
    state = {"obs": env._obs}

    def torch_step():
        for k in range(K):
            state["obs"] = env.step(torch_policy(nrm(state["obs"])))[0]

    def act_step():
        for k in range(K):
            env.step(env.policy_act(params, hidden=H, activation=ACT))

    def fused():
        env.rollout_policy(params, K, hidden=H, activation=ACT)

    legs = (("torch_step", torch_step), ("act_step", act_step), ("rollout_policy", fused))
    for _ in range(4):
        for _, fn in legs:
            fn()
    res = {name: [] for name, _ in legs}
    for _ in range(repeats):
        for name, fn in legs:
            w, dt = leg(fn, 4, seconds, dev)
            res[name].append(n * K * w / dt)
    bad = int((env.status() & 3).ne(0).sum())
    fused_flag = env.launch_info()["rollout_fused"]
    env.close()
    return {"env": env_id, "envs": n, "steps_per_window": K, "hidden": H, "activation": ACT, "obs_norm": bool(obs_norm), "fused": fused_flag, "flagged_envs": bad,
            **{name + "_env_steps_per_s": v for name, v in res.items()}}


def bench_sample(env_id, n, K, H, seconds, repeats, ACT="tanh", obs_norm=False):
    """K closed-loop steps of one shared Gaussian policy: policy_sample + step, one rollout_policy_sample; the deterministic
    rollout_policy of the same network as the yardstick."""
    dev = torch.device("cuda", 0)
    env = make_env(env_id, n, dev)
    env.reset(seed=20260928)
    g = torch.Generator(device=dev).manual_seed(1234)
    bind_norm(env, obs_norm, dev, g)  # (no torch network in this mode)

    def lin(out, fan_in):
        k = fan_in ** -0.5
        return (2 * torch.rand((out, fan_in), device=dev, generator=g) - 1) * k, (2 * torch.rand(out, device=dev, generator=g) - 1) * k

    log_std = torch.full((env.nu,), -0.5)
    params, _ = build_net(lin, env.obs_dim, env.nu, H, ACT, dev, log_std=log_std)
    det = params[: -env.nu].contiguous()

    def sample_step():
        for k in range(K):
            env.step(env.policy_sample(params, hidden=H, activation=ACT)[0])

    def fused():
        env.rollout_policy_sample(params, K, hidden=H, activation=ACT)

    def fused_det():
        env.rollout_policy(det, K, hidden=H, activation=ACT)

    legs = (("sample_step", sample_step), ("rollout_policy_sample", fused), ("rollout_policy", fused_det))
    for _ in range(4):
        for _, fn in legs:
            fn()
    res = {name: [] for name, _ in legs}
    for _ in range(repeats):
        for name, fn in legs:
            w, dt = leg(fn, 4, seconds, dev)
            res[name].append(n * K * w / dt)
    bad = int((env.status() & 3).ne(0).sum())
    fused_flag = env.launch_info()["rollout_fused"]
    env.close()
    return {"env": env_id, "envs": n, "steps_per_window": K, "hidden": H, "activation": ACT, "obs_norm": bool(obs_norm), "sample": True, "fused": fused_flag, "flagged_envs": bad,
            **{name + "_env_steps_per_s": v for name, v in res.items()}}


def bench_context(env_id, n, K, H, cdim, rel, seconds, repeats, ACT="tanh", obs_norm=False):
    """K closed-loop steps of one shared Gaussian policy on [obs | context]: policy_sample(context=) + step + the transition in torch,
    one rollout_policy_sample(context=); the same call without a context as the yardstick."""
    dev = torch.device("cuda", 0)
    env = make_env(env_id, n, dev)
    env.reset(seed=20260928)
    g = torch.Generator(device=dev).manual_seed(1234)
    bind_norm(env, obs_norm, dev, g)  # (no torch network in this mode)

    def lin(out, fan_in):
        k = fan_in ** -0.5
        return (2 * torch.rand((out, fan_in), device=dev, generator=g) - 1) * k, (2 * torch.rand(out, device=dev, generator=g) - 1) * k

    log_std = torch.full((env.nu,), -0.5)
    params, _ = build_net(lin, env.obs_dim + cdim, env.nu, H, ACT, dev, log_std=log_std)
    plain, _ = build_net(lin, env.obs_dim, env.nu, H, ACT, dev, log_std=log_std)
    ctx0 = torch.randn((n, cdim), device=dev, generator=g).contiguous()
    ctx = ctx0.clone()
    upd = dict(context_update="relative", context_dims=rel) if rel else {}
    rows = torch.empty((K, n, env.obs_dim), device=dev)
    crow = torch.empty((K, n, cdim), device=dev)

    def sample_step():
        ctx.copy_(ctx0)
        for k in range(K):
            crow[k] = ctx
            s_old = env._obs[:, :rel].clone() if rel else None
            obs, _, done, info = env.step(env.policy_sample(params, hidden=H, activation=ACT, context=ctx)[0])
            nxt = torch.where((done != 0).unsqueeze(1), info["final_observation"], obs)
            rows[k] = nxt
            if rel:
                new = (ctx[:, :rel] + s_old) - nxt[:, :rel]
                ctx[:, :rel] = torch.where((done != 0).unsqueeze(1), ctx[:, :rel], new)

    def one_call():
        ctx.copy_(ctx0)
        env.rollout_policy_sample(params, K, hidden=H, activation=ACT, context=ctx, return_next_obs=True, return_contexts=True, **upd)

    def no_context():
        env.rollout_policy_sample(plain, K, hidden=H, activation=ACT, return_next_obs=True)

    legs = (("sample_step", sample_step), ("rollout_context", one_call), ("rollout_plain", no_context))
    for _ in range(4):
        for _, fn in legs:
            fn()
    res = {name: [] for name, _ in legs}
    for _ in range(repeats):
        for name, fn in legs:
            w, dt = leg(fn, 4, seconds, dev)
            res[name].append(n * K * w / dt)
    bad = int((env.status() & 3).ne(0).sum())
    fused_flag = env.launch_info()["rollout_fused"]
    env.close()
    return {"env": env_id, "envs": n, "steps_per_window": K, "hidden": H, "activation": ACT, "obs_norm": bool(obs_norm), "context": cdim, "relative": rel,
            "fused": fused_flag, "flagged_envs": bad, **{name + "_env_steps_per_s": v for name, v in res.items()}}


def bench_critic(env_id, n, K, H, HV, seconds, repeats, ACT="tanh", obs_norm=False):
    """One actor-critic collection window of K steps: policy_sample + step + torch critic + torch GAE loop; one
    rollout_policy_sample with value_params and gae; the same call without a critic."""
    dev = torch.device("cuda", 0)
    env = make_env(env_id, n, dev)
    env.reset(seed=20260928)
    g = torch.Generator(device=dev).manual_seed(1234)
    nrm = bind_norm(env, obs_norm, dev, g)
    gamma, lam = 0.99, 0.95

    def lin(out, fan_in):
        k = fan_in ** -0.5
        return (2 * torch.rand((out, fan_in), device=dev, generator=g) - 1) * k, (2 * torch.rand(out, device=dev, generator=g) - 1) * k

    log_std = torch.full((env.nu,), -0.5)
    params, _ = build_net(lin, env.obs_dim, env.nu, H, ACT, dev, log_std=log_std)
    vparams, torch_critic = build_net(lin, env.obs_dim, 1, HV, ACT, dev)
    rows = torch.empty((K + 1, n, env.obs_dim), device=dev)
    rew, done = torch.empty((K, n), device=dev), torch.empty((K, n), dtype=torch.uint8, device=dev)
    adv = torch.empty((K, n), device=dev)

    def torch_path():
        rows[0] = env._obs
        for k in range(K):
            o, r, d, _ = env.step(env.policy_sample(params, hidden=H, activation=ACT)[0])
            rows[k + 1], rew[k], done[k] = o, r, d
        v = torch_critic(nrm(rows.view((K + 1) * n, env.obs_dim))).view(K + 1, n)
        carry = torch.zeros(n, device=dev)
        term, end = (done & 1) != 0, done != 0
        for k in range(K - 1, -1, -1):
            delta = rew[k] + torch.where(term[k], 0.0, gamma * v[k + 1]) - v[k]
            carry = delta + torch.where(end[k], 0.0, gamma * lam * carry)
            adv[k] = carry
        return adv, adv + v[:K]

    def one_call():
        env.rollout_policy_sample(params, K, hidden=H, value_params=vparams, value_hidden=HV, gae=(gamma, lam), activation=ACT, value_activation=ACT)

    def no_critic():
        env.rollout_policy_sample(params, K, hidden=H, activation=ACT)

    legs = (("torch_critic_gae", torch_path), ("rollout_actor_critic_gae", one_call), ("rollout_policy_sample", no_critic))
    for _ in range(4):
        for _, fn in legs:
            fn()
    res = {name: [] for name, _ in legs}
    for _ in range(repeats):
        for name, fn in legs:
            w, dt = leg(fn, 4, seconds, dev)
            res[name].append(n * K * w / dt)
    bad = int((env.status() & 3).ne(0).sum())
    fused_flag = env.launch_info()["rollout_fused"]
    env.close()
    return {"env": env_id, "envs": n, "steps_per_window": K, "hidden": H, "critic_hidden": HV, "activation": ACT, "obs_norm": bool(obs_norm), "sample": True, "fused": fused_flag, "flagged_envs": bad,
            **{name + "_env_steps_per_s": v for name, v in res.items()}}


def bench_transitions(env_id, n, K, H, seconds, repeats, ACT="tanh", obs_norm=False, noise="pre_squash"):
    """One off-policy collection window of K steps: policy_sample + step + torch.where on the terminal rows; one
    rollout_policy_sample with return_next_obs; the same call without the next rows."""
    import math

    dev = torch.device("cuda", 0)
    env = make_env(env_id, n, dev)
    env.reset(seed=20260928)
    g = torch.Generator(device=dev).manual_seed(1234)
    bind_norm(env, obs_norm, dev, g)  # (no torch network in this mode)

    def lin(out, fan_in):
        k = fan_in ** -0.5
        return (2 * torch.rand((out, fan_in), device=dev, generator=g) - 1) * k, (2 * torch.rand(out, device=dev, generator=g) - 1) * k

    log_std = torch.full((env.nu,), math.log(0.1) if noise == "action" else -0.5)
    params, _ = build_net(lin, env.obs_dim, env.nu, H, ACT, dev, log_std=log_std)
    kw = dict(hidden=H, activation=ACT, squash=True, noise=noise)
    obs_rows, next_rows = torch.empty((K, n, env.obs_dim), device=dev), torch.empty((K, n, env.obs_dim), device=dev)
    act_rows = torch.empty((K, n, env.nu), device=dev)
    rew, done = torch.empty((K, n), device=dev), torch.empty((K, n), dtype=torch.uint8, device=dev)

    def step_where():
        for k in range(K):
            a = env.policy_sample(params, **kw)[0]
            o, r, d, info = env.step(a)
            act_rows[k], obs_rows[k], rew[k], done[k] = a, o, r, d
            next_rows[k] = torch.where((d != 0).unsqueeze(1), info["final_observation"], o)

    def one_call():
        env.rollout_policy_sample(params, K, return_obs=True, return_actions=True, return_next_obs=True, **kw)

    def no_next():
        env.rollout_policy_sample(params, K, return_obs=True, return_actions=True, **kw)

    legs = (("sample_step_where", step_where), ("rollout_next_obs", one_call), ("rollout_no_next_obs", no_next))
    for _ in range(4):
        for _, fn in legs:
            fn()
    res = {name: [] for name, _ in legs}
    for _ in range(repeats):
        for name, fn in legs:
            w, dt = leg(fn, 4, seconds, dev)
            res[name].append(n * K * w / dt)
    bad = int((env.status() & 3).ne(0).sum())
    fused_flag = env.launch_info()["rollout_fused"]
    env.close()
    return {"env": env_id, "envs": n, "steps_per_window": K, "hidden": H, "activation": ACT, "obs_norm": bool(obs_norm), "noise": noise, "fused": fused_flag,
            "flagged_envs": bad, **{name + "_env_steps_per_s": v for name, v in res.items()}}


def bench_head(env_id, n, K, H, seconds, repeats, ACT="tanh", obs_norm=False, squashed_logp=False):
    """One SAC collection window of K steps with a state-dependent log-std head: policy_sample(log_std="state") + step + torch.where
    on the terminal rows; one rollout_policy_sample(log_std="state") with return_next_obs; the same call without the next rows."""
    from mujoco_maze_amd import policy

    dev = torch.device("cuda", 0)
    env = make_env(env_id, n, dev)
    env.reset(seed=20260928)
    g = torch.Generator(device=dev).manual_seed(1234)
    bind_norm(env, obs_norm, dev, g)  # (no torch network in this mode)

    def lin(out, fan_in):
        k = fan_in ** -0.5
        return (2 * torch.rand((out, fan_in), device=dev, generator=g) - 1) * k, (2 * torch.rand(out, device=dev, generator=g) - 1) * k

    sizes = (env.obs_dim,) + policy.net_shape(H, ACT, max_width=max_width())[0] + (env.nu,)
    layers = [lin(o, i) for i, o in zip(sizes[:-1], sizes[1:])]
    Wh, bh = lin(env.nu, sizes[-2])
    params = torch.as_tensor(policy.pack_mlp(layers, log_std_head=(0.1 * Wh, torch.full_like(bh, -0.5)), max_width=max_width()), device=dev)
    kw = dict(hidden=H, activation=ACT, squash=True, log_std="state", squashed_logp=squashed_logp)
    obs_rows, next_rows = torch.empty((K, n, env.obs_dim), device=dev), torch.empty((K, n, env.obs_dim), device=dev)
    act_rows, logp_rows = torch.empty((K, n, env.nu), device=dev), torch.empty((K, n), device=dev)
    rew, done = torch.empty((K, n), device=dev), torch.empty((K, n), dtype=torch.uint8, device=dev)

    def step_where():
        for k in range(K):
            a, lp = env.policy_sample(params, **kw)
            o, r, d, info = env.step(a)
            act_rows[k], logp_rows[k], obs_rows[k], rew[k], done[k] = a, lp, o, r, d
            next_rows[k] = torch.where((d != 0).unsqueeze(1), info["final_observation"], o)

    def one_call():
        env.rollout_policy_sample(params, K, return_obs=True, return_actions=True, return_next_obs=True, **kw)

    def no_next():
        env.rollout_policy_sample(params, K, return_obs=True, return_actions=True, **kw)

    legs = (("head_step_where", step_where), ("rollout_head_next_obs", one_call), ("rollout_head_no_next_obs", no_next))
    for _ in range(4):
        for _, fn in legs:
            fn()
    res = {name: [] for name, _ in legs}
    for _ in range(repeats):
        for name, fn in legs:
            w, dt = leg(fn, 4, seconds, dev)
            res[name].append(n * K * w / dt)
    bad = int((env.status() & 3).ne(0).sum())
    fused_flag = env.launch_info()["rollout_fused"]
    env.close()
    return {"env": env_id, "envs": n, "steps_per_window": K, "hidden": H, "activation": ACT, "obs_norm": bool(obs_norm), "head": "state",
            "squashed_logp": bool(squashed_logp), "fused": fused_flag, "flagged_envs": bad, **{name + "_env_steps_per_s": v for name, v in res.items()}}


def bench_head_critic(env_id, n, K, H, HV, seconds, repeats, ACT="tanh", per_env=False):
    """One SAC-style window of K steps with a head actor and a critic (the 256-256 networks of SB3 / CleanRL with `--policy 256,256
    --critic 256,256`): what a user runs without the device networks — K x (torch actor with its head and sampling, torch critic,
    env.step) —, against one rollout_policy_sample(log_std="state", value_params=) call; and, one launch each, an actor evaluation
    (policy_sample), a critic evaluation (value) and an env.step.  per_env: one network per env ([N, count] parameters; no torch leg)."""
    from mujoco_maze_amd import policy

    dev = torch.device("cuda", 0)
    env = make_env(env_id, n, dev)
    env.reset(seed=20260928)
    g = torch.Generator(device=dev).manual_seed(1234)

    def lin(out, fan_in):
        k = fan_in ** -0.5
        return (2 * torch.rand((out, fan_in), device=dev, generator=g) - 1) * k, (2 * torch.rand(out, device=dev, generator=g) - 1) * k

    sizes = (env.obs_dim,) + policy.net_shape(H, ACT, max_width=max_width())[0] + (env.nu,)
    layers = [lin(o, i) for i, o in zip(sizes[:-1], sizes[1:])]
    Wh, bh = lin(env.nu, sizes[-2])
    Wh, bh = 0.1 * Wh, torch.full_like(bh, -0.5)
    params = torch.as_tensor(policy.pack_mlp(layers, log_std_head=(Wh, bh), max_width=max_width()), device=dev)
    vparams, torch_critic = build_net(lin, env.obs_dim, 1, HV, ACT, dev)
    if per_env:
        params, vparams = params.repeat(n, 1).contiguous(), vparams.repeat(n, 1).contiguous()
    f = torch.tanh if ACT == "tanh" else torch.relu
    body = [(W.T.contiguous(), b) for W, b in layers[:-1]]
    Wm, bm, Ws, bs = layers[-1][0].T.contiguous(), layers[-1][1], Wh.T.contiguous(), bh
    kw = dict(hidden=H, activation=ACT, squash=True, log_std="state", squashed_logp=True)
    vals = torch.empty((K, n), device=dev)

    def torch_loop():
        obs = env._obs
        for k in range(K):
            x = obs
            for Wt, b in body:
                x = f(torch.addmm(b, x, Wt))
            m, ls = torch.addmm(bm, x, Wm), torch.clamp(torch.addmm(bs, x, Ws), -20.0, 2.0)
            z = m + ls.exp() * torch.randn(m.shape, device=dev, generator=g)
            vals[k] = torch_critic(obs).squeeze(1)
            obs = env.step(torch.tanh(z))[0]

    def one_call():
        env.rollout_policy_sample(params, K, value_params=vparams, value_hidden=HV, value_activation=ACT, **kw)

    def actor_eval():
        for _ in range(K):
            env.policy_sample(params, **kw)

    def critic_eval():
        for _ in range(K):
            env.value(vparams, hidden=HV, activation=ACT)

    zero = torch.zeros((n, env.nu), device=dev)

    def step_only():
        for _ in range(K):
            env.step(zero)

    legs = (() if per_env else (("torch_loop", torch_loop),)) + (("rollout_head_critic", one_call), ("actor_eval", actor_eval),
                                                                 ("critic_eval", critic_eval), ("step", step_only))
    for _ in range(4):
        for _, fn in legs:
            fn()
    res = {name: [] for name, _ in legs}
    for _ in range(repeats):
        for name, fn in legs:
            w, dt = leg(fn, 2, seconds, dev)
            res[name].append(n * K * w / dt)
    bad = int((env.status() & 3).ne(0).sum())
    info = env.launch_info()
    env.close()
    return {"env": env_id, "envs": n, "steps_per_window": K, "hidden": H, "critic_hidden": HV, "activation": ACT, "head": "state", "per_env": bool(per_env),
            "wide_nets": info["wide_nets"], "fused": info["rollout_fused"], "flagged_envs": bad, **{name + "_env_steps_per_s": v for name, v in res.items()}}


def main_head_critic(args):
    out = []
    med = lambda v: sorted(v)[len(v) // 2]
    print(f"SAC-style window with a critic: head actor (hidden {args.policy}) and critic (hidden {args.critic}), {args.activation} units, "
          f"{'one network per env' if args.per_env else 'shared networks'}, wide_nets = {WIDE_NETS}, {args.steps} steps per window, {args.envs} envs, "
          f"auto-reset, >= {args.seconds} s per leg, {args.repeats} alternating repeats; M env-steps/s, median (max - min); the last three "
          "columns: ms per launch of one actor evaluation, one critic evaluation, one env.step (median)")
    print("%-16s %26s %26s %10s %10s %10s" % ("env", "torch nets + step, K x", "one call", "actor ms", "critic ms", "step ms"))
    for env_id in args.ids.split(","):
        r = bench_head_critic(env_id, args.envs, args.steps, args.policy, args.critic, args.seconds, args.repeats, args.activation, args.per_env)
        out.append(r)
        cell = lambda v: "%10.3f (%6.3f)" % (med(v) / 1e6, (max(v) - min(v)) / 1e6)
        ms = lambda v: 1e3 * args.envs / med(v)
        print("%-16s %26s %26s %10.4f %10.4f %10.4f" % (env_id, cell(r["torch_loop_env_steps_per_s"]) if "torch_loop_env_steps_per_s" in r else "-",
                                                        cell(r["rollout_head_critic_env_steps_per_s"]), ms(r["actor_eval_env_steps_per_s"]),
                                                        ms(r["critic_eval_env_steps_per_s"]), ms(r["step_env_steps_per_s"])), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for r in out:
                f.write(json.dumps(r) + "\n")


def main_head(args):
    out = []
    med = lambda v: sorted(v)[len(v) // 2]
    print(f"SAC window (s, a, logp, r, s', d), shared squashed actor with a log-std head (hidden {args.policy}, {args.activation} units, logp of the "
          f"{'action' if args.squashed_logp else 'pre-squash sample'}), {args.steps} steps per window, {args.envs} envs, auto-reset, >= {args.seconds} s per leg, "
          f"{args.repeats} alternating repeats; M env-steps/s, median (max - min)")
    print("%-18s %5s %26s %26s %26s" % ("env", "fused", "sample + step + where", "one call, next rows", "one call, no next rows"))
    for env_id in args.ids.split(","):
        r = bench_head(env_id, args.envs, args.steps, args.policy, args.seconds, args.repeats, args.activation, args.obs_norm, args.squashed_logp)
        out.append(r)
        cell = lambda v: "%10.3f (%6.3f)" % (med(v) / 1e6, (max(v) - min(v)) / 1e6)
        print("%-18s %5d %26s %26s %26s" % (env_id, r["fused"], cell(r["head_step_where_env_steps_per_s"]), cell(r["rollout_head_next_obs_env_steps_per_s"]),
                                            cell(r["rollout_head_no_next_obs_env_steps_per_s"])), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for r in out:
                f.write(json.dumps(r) + "\n")


def main_transitions(args):
    out = []
    med = lambda v: sorted(v)[len(v) // 2]
    print(f"off-policy window (s, a, r, s', d), shared squashed Gaussian policy (hidden {args.policy}, {args.activation} units, noise {args.noise}), {args.steps} steps per "
          f"window, {args.envs} envs, auto-reset, >= {args.seconds} s per leg, {args.repeats} alternating repeats; M env-steps/s, median (max - min)")
    print("%-18s %5s %26s %26s %26s" % ("env", "fused", "sample + step + where", "one call, next rows", "one call, no next rows"))
    for env_id in args.ids.split(","):
        r = bench_transitions(env_id, args.envs, args.steps, args.policy, args.seconds, args.repeats, args.activation, args.obs_norm, args.noise)
        out.append(r)
        cell = lambda v: "%10.3f (%6.3f)" % (med(v) / 1e6, (max(v) - min(v)) / 1e6)
        print("%-18s %5d %26s %26s %26s" % (env_id, r["fused"], cell(r["sample_step_where_env_steps_per_s"]), cell(r["rollout_next_obs_env_steps_per_s"]),
                                            cell(r["rollout_no_next_obs_env_steps_per_s"])), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for r in out:
                f.write(json.dumps(r) + "\n")


def main_critic(args):
    out = []
    med = lambda v: sorted(v)[len(v) // 2]
    print(f"actor-critic window, shared Gaussian policy (hidden {args.policy}) and critic (hidden {args.critic}), {args.activation} units, GAE(0.99, 0.95), {args.steps} steps per "
          f"window, {args.envs} envs, auto-reset, >= {args.seconds} s per leg, {args.repeats} alternating repeats; M env-steps/s, median (max - min)")
    print("%-18s %5s %26s %26s %26s" % ("env", "fused", "sample+step, torch V, GAE", "one call, critic + gae", "one call, no critic"))
    for env_id in args.ids.split(","):
        r = bench_critic(env_id, args.envs, args.steps, args.policy, args.critic, args.seconds, args.repeats, args.activation, args.obs_norm)
        out.append(r)
        cell = lambda v: "%10.3f (%6.3f)" % (med(v) / 1e6, (max(v) - min(v)) / 1e6)
        print("%-18s %5d %26s %26s %26s" % (env_id, r["fused"], cell(r["torch_critic_gae_env_steps_per_s"]), cell(r["rollout_actor_critic_gae_env_steps_per_s"]),
                                            cell(r["rollout_policy_sample_env_steps_per_s"])), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for r in out:
                f.write(json.dumps(r) + "\n")


def main_context(args):
    out = []
    med = lambda v: sorted(v)[len(v) // 2]
    print(f"goal-conditioned window, one shared Gaussian policy on [obs | context] (hidden {args.policy}, {args.activation} units, context {args.context}, "
          f"{'relative ' + str(args.relative) if args.relative else 'hold'}), {args.steps} steps per window, {args.envs} envs, auto-reset, >= {args.seconds} s per leg, "
          f"{args.repeats} alternating repeats; M env-steps/s, median (max - min)")
    print("%-18s %5s %30s %26s %26s" % ("env", "fused", "policy_sample(context) + step", "rollout(context=)", "rollout without a context"))
    for env_id in args.ids.split(","):
        r = bench_context(env_id, args.envs, args.steps, args.policy, args.context, args.relative, args.seconds, args.repeats, args.activation, args.obs_norm)
        out.append(r)
        cell = lambda v: "%10.3f (%6.3f)" % (med(v) / 1e6, (max(v) - min(v)) / 1e6)
        print("%-18s %5d %30s %26s %26s" % (env_id, r["fused"], cell(r["sample_step_env_steps_per_s"]), cell(r["rollout_context_env_steps_per_s"]),
                                            cell(r["rollout_plain_env_steps_per_s"])), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for r in out:
                f.write(json.dumps(r) + "\n")


def main_sample(args):
    out = []
    med = lambda v: sorted(v)[len(v) // 2]
    print(f"closed loop, one shared Gaussian policy (hidden {args.policy}, {args.activation} units, log_std -0.5), {args.steps} steps per window, {args.envs} envs, auto-reset, "
          f">= {args.seconds} s per leg, {args.repeats} alternating repeats; M env-steps/s, median (max - min)")
    print("%-18s %5s %24s %24s %24s" % ("env", "fused", "policy_sample + step", "rollout_policy_sample", "rollout_policy (det.)"))
    for env_id in args.ids.split(","):
        r = bench_sample(env_id, args.envs, args.steps, args.policy, args.seconds, args.repeats, args.activation, args.obs_norm)
        out.append(r)
        cell = lambda v: "%10.3f (%6.3f)" % (med(v) / 1e6, (max(v) - min(v)) / 1e6)
        print("%-18s %5d %24s %24s %24s" % (env_id, r["fused"], cell(r["sample_step_env_steps_per_s"]), cell(r["rollout_policy_sample_env_steps_per_s"]),
                                            cell(r["rollout_policy_env_steps_per_s"])), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for r in out:
                f.write(json.dumps(r) + "\n")


def main_policy(args):
    out = []
    med = lambda v: sorted(v)[len(v) // 2]
    print(f"closed loop, one shared policy (hidden {args.policy}, {args.activation} units), {args.steps} steps per window, {args.envs} envs, auto-reset, >= {args.seconds} s per leg, "
          f"{args.repeats} alternating repeats; M env-steps/s, median (max - min)")
    print("%-18s %5s %24s %24s %24s" % ("env", "fused", "torch policy + step", "policy_act + step", "rollout_policy"))
    for env_id in args.ids.split(","):
        r = bench_policy(env_id, args.envs, args.steps, args.policy, args.seconds, args.repeats, args.activation, args.obs_norm)
        out.append(r)
        cell = lambda v: "%10.3f (%6.3f)" % (med(v) / 1e6, (max(v) - min(v)) / 1e6)
        print("%-18s %5d %24s %24s %24s" % (env_id, r["fused"], cell(r["torch_step_env_steps_per_s"]), cell(r["act_step_env_steps_per_s"]),
                                            cell(r["rollout_policy_env_steps_per_s"])), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for r in out:
                f.write(json.dumps(r) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=1.0, help="least duration of one timed leg")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--ids", type=str, default=",".join(IDS))
    ap.add_argument("--out", type=str, default=None, help="also write the rows as JSON lines")
    ap.add_argument("--policy", type=hidden_arg, default=None, metavar="H", help="closed-loop mode: hidden units of the policy (0 = affine), or two widths H1,H2")
    ap.add_argument("--sample", action="store_true", help="with --policy: Gaussian policies, a sampled action every step")
    ap.add_argument("--critic", type=hidden_arg, default=None, metavar="HV", help="with --policy H --sample: a critic with HV hidden units (0 = affine; or HV1,HV2) and GAE")
    ap.add_argument("--activation", choices=("tanh", "relu"), default="tanh", help="with --policy: the hidden units of policy and critic")
    ap.add_argument("--obs-norm", action="store_true", help="with --policy: bind an observation normaliser (env.bind_obs_norm) in every leg")
    ap.add_argument("--next-obs", action="store_true", help="with --policy H --sample: the off-policy window, with every step's pre-reset row")
    ap.add_argument("--noise", choices=("pre_squash", "action"), default="pre_squash", help="with --next-obs: where the exploration noise goes")
    ap.add_argument("--head", choices=("state",), default=None, help="with --policy H: a state-dependent log-std head on the actor (the SAC window)")
    ap.add_argument("--squashed-logp", action="store_true", help="with --head state: the log-probability of the squashed action")
    ap.add_argument("--context", type=int, default=None, metavar="C", help="with --policy H --sample: a [N, C] context behind the observation (1 .. 32)")
    ap.add_argument("--wide-nets", type=int, choices=(0, 1, 2), default=None, help="option wide_nets of every env (default: 1 where --policy or "
                    "--critic is wider than 64, else 0; 2 puts narrower networks on the tiled kernel too)")
    ap.add_argument("--per-env", action="store_true", help="with --policy H --head state --critic HV: one network per env")
    ap.add_argument("--relative", type=int, default=0, metavar="D", help="with --context C: HIRO's goal transition on the first D entries after every step")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "rollout_bench.py measures on the GPU only"
    if args.sample and args.policy is None:
        ap.error("--sample goes with --policy H")
    if args.critic is not None and not args.sample and args.head is None:
        ap.error("--critic goes with --policy H --sample, or with --policy H --head state")
    global WIDE_NETS
    widths = [w for h in (args.policy, args.critic) if h is not None for w in (h if isinstance(h, tuple) else (h,))]
    WIDE_NETS = args.wide_nets if args.wide_nets is not None else int(any(w > 64 for w in widths))
    if args.per_env and (args.head is None or args.critic is None):
        ap.error("--per-env goes with --policy H --head state --critic HV")
    if args.obs_norm and args.policy is None:
        ap.error("--obs-norm goes with --policy H")
    if args.obs_norm:
        print("observation normaliser bound (clip 5): every network below reads normalised rows")
    if args.next_obs and (not args.sample or args.critic is not None):
        ap.error("--next-obs goes with --policy H --sample, without --critic")
    if args.noise != "pre_squash" and not args.next_obs:
        ap.error("--noise goes with --next-obs")
    if args.head is not None and (args.policy is None or args.next_obs or args.sample):
        ap.error("--head goes with --policy H alone (it samples and returns the next rows by itself), or with --critic HV as well")
    if args.squashed_logp and args.head is None:
        ap.error("--squashed-logp goes with --head state")
    if args.context is not None and (not args.sample or args.critic is not None or args.next_obs or args.head is not None):
        ap.error("--context goes with --policy H --sample alone")
    if args.relative and args.context is None:
        ap.error("--relative goes with --context C")
    if args.context is not None:
        return main_context(args)
    if args.head is not None and args.critic is not None:
        return main_head_critic(args)
    if args.head is not None:
        return main_head(args)
    if args.next_obs:
        return main_transitions(args)
    if args.critic is not None:
        return main_critic(args)
    if args.policy is not None:
        return main_sample(args) if args.sample else main_policy(args)
    out = []
    print(f"{args.steps} x env.step against one env.rollout, {args.envs} envs, auto-reset, >= {args.seconds} s per leg, {args.repeats} alternating repeats")
    print("%-18s %5s %14s %10s %14s %10s %7s" % ("env", "fused", "step M/s", "spread", "rollout M/s", "spread", "ratio"))
    for env_id in args.ids.split(","):
        r = bench(env_id, args.envs, args.steps, args.seconds, args.repeats)
        out.append(r)
        s, ro = r["step_env_steps_per_s"], r["rollout_env_steps_per_s"]
        med = lambda v: sorted(v)[len(v) // 2]
        print("%-18s %5d %12.3f M %8.3f M %12.3f M %8.3f M %7.2f" % (env_id, r["fused"], med(s) / 1e6, (max(s) - min(s)) / 1e6, med(ro) / 1e6,
                                                                  (max(ro) - min(ro)) / 1e6, med(ro) / med(s)), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for r in out:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
