"""What the rollout entries share, pinned from outside: which C entry every VecMazeEnv rollout call makes, and the packed record
(mz_bind_record) after a call through each closed-loop entry — on a handle that takes the fused kernels and on one that steps launch
by launch.  tests/test_gpu_rollout.py and tests/test_gpu_policy_rollout.py pin the record for mz_rollout and mz_rollout_policy."""
import numpy as np
import pytest

import mujoco_maze_amd as mm
from mujoco_maze_amd import policy
from tests.test_gpu_rollout import _same

pytestmark = pytest.mark.gpu
HIDDEN = 4


class _Recorder:
    """env._lib with the names of the mz_rollout* calls written down"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("mz_rollout"):
            return fn

        def call(*args):
            self.calls.append(name)
            return fn(*args)

        return call


def _params(env, nout, hidden, seed, stochastic=False):
    """a random network with nout outputs on the env's device (stochastic: log_std[nu] behind it)"""
    import torch

    count = policy.param_count(env.obs_dim, nout, hidden, stochastic)
    return torch.as_tensor(0.3 * np.random.default_rng(seed).standard_normal(count).astype(np.float32), device=env.device)


def test_entry_choice():
    import torch

    n, K = 8, 3
    env = mm.make("PointUMaze-v0", num_envs=n, auto_reset=True, seed=1, max_episode_steps=5)
    try:
        env.reset(seed=2)
        rec = env._lib = _Recorder(env._lib)
        act = torch.zeros((K, n, env.nu), dtype=torch.float32, device=env.device)
        pol, spol = _params(env, env.nu, HIDDEN, 3), _params(env, env.nu, HIDDEN, 4, stochastic=True)
        deep, sdeep = _params(env, env.nu, (HIDDEN, HIDDEN), 5), _params(env, env.nu, (HIDDEN, HIDDEN), 6, stochastic=True)
        critic = dict(value_params=_params(env, 1, HIDDEN, 7), value_hidden=HIDDEN)
        table = [
            (lambda: env.rollout(act), "mz_rollout"),
            (lambda: env.rollout(act, return_next_obs=True), "mz_rollout_ex"),
            (lambda: env.rollout(act[0], repeat=K, return_obs=True, return_next_obs=True), "mz_rollout_ex"),
            (lambda: env.rollout_policy(pol, K, hidden=HIDDEN), "mz_rollout_policy"),
            (lambda: env.rollout_policy_sample(spol, K, hidden=HIDDEN), "mz_rollout_policy_sample"),
            (lambda: env.rollout_policy(pol, K, hidden=HIDDEN, **critic), "mz_rollout_actor_critic"),
            (lambda: env.rollout_policy_sample(spol, K, hidden=HIDDEN, gae=(0.99, 0.95), **critic), "mz_rollout_actor_critic"),
            (lambda: env.rollout_policy(deep, K, hidden=(HIDDEN, HIDDEN)), "mz_rollout_net"),
            (lambda: env.rollout_policy_sample(sdeep, K, hidden=(HIDDEN, HIDDEN), **critic), "mz_rollout_net"),
            (lambda: env.rollout_policy(pol, K, hidden=HIDDEN, activation="relu"), "mz_rollout_net"),
            (lambda: env.rollout_policy_sample(spol, K, hidden=HIDDEN, activation="relu"), "mz_rollout_net"),
            (lambda: env.rollout_policy(pol, K, hidden=HIDDEN, value_activation="relu", **critic), "mz_rollout_net"),
            (lambda: env.rollout_policy(pol, K, hidden=HIDDEN, return_next_obs=True), "mz_rollout_ex"),
            (lambda: env.rollout_policy_sample(spol, K, hidden=HIDDEN, return_next_obs=True, **critic), "mz_rollout_ex"),
            (lambda: env.rollout_policy_sample(spol, K, hidden=HIDDEN, noise="action"), "mz_rollout_ex"),
            (lambda: env.rollout_policy_sample(sdeep, K, hidden=(HIDDEN, HIDDEN), noise="action", return_next_obs=True), "mz_rollout_ex"),
        ]
        for i, (call, entry) in enumerate(table):
            rec.calls.clear()
            call()
            assert rec.calls == [entry], f"row {i}: {rec.calls} instead of one {entry}"
        torch.cuda.synchronize()
    finally:
        env.close()


@pytest.mark.parametrize("env_id,n,K", [("PointUMaze-v0", 8, 3), ("AntUMaze-v0", 4, 2)], ids=["fused", "launch-by-launch"])
def test_record_row_on_every_entry(env_id, n, K):
    """after a call through any closed-loop entry the record is [obs | rewards[K - 1] | dones[K - 1]]: one pack_record_kernel launch
    behind the fused kernels, the step kernel's own stores on the Ant"""
    import torch

    env = mm.make(env_id, num_envs=n, auto_reset=True, seed=1, max_episode_steps=2)
    try:
        assert env.launch_info()["rollout_fused"] == (1 if env_id.startswith("Point") else 0)
        od = env.obs_dim
        record = torch.empty((n, od + 2), dtype=torch.float32, device=env.device)
        env.bind_record(record)
        env.reset(seed=2)
        lib = env._lib = _Recorder(env._lib)
        spol = _params(env, env.nu, HIDDEN, 3, stochastic=True)
        critic = dict(value_params=_params(env, 1, HIDDEN, 4), value_hidden=HIDDEN)
        variants = [
            (lambda: env.rollout_policy_sample(spol, K, hidden=HIDDEN, squash=True, **critic), "mz_rollout_actor_critic"),
            (lambda: env.rollout_policy(_params(env, env.nu, (HIDDEN, HIDDEN), 5), K, hidden=(HIDDEN, HIDDEN)), "mz_rollout_net"),
            (lambda: env.rollout_policy(_params(env, env.nu, HIDDEN, 6), K, hidden=HIDDEN, return_next_obs=True), "mz_rollout_ex"),
        ]
        for call, entry in variants:
            record.fill_(-7.0)
            lib.calls.clear()
            obs, rew, done, _ = call()
            torch.cuda.synchronize()
            assert lib.calls == [entry]
            assert _same(record[:, :od].contiguous(), obs), entry
            assert _same(record[:, od].contiguous(), rew[K - 1].contiguous()), entry
            assert torch.equal(record[:, od + 1], done[K - 1].to(torch.float32)), entry
        env.bind_record(None)
    finally:
        env.close()
