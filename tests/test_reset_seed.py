"""The episode seed without a GPU: csrc/mz_rng.h's episode_seed, built for the host under tests/policy_sample_host, against the numpy
mirror of tests/reset_ref.py — integers on both sides, so bit equality — and `expected_reset`, the reference of
tests/test_gpu_reset_parity.py, against the plain oracle reset."""
import ctypes as C

import numpy as np

from mujoco_maze_amd import maze_task as T
from mujoco_maze_amd import model
from tests import reset_ref
from tests.test_policy_sample_api import _load

U64 = (1 << 64) - 1


def _host_episode_seed():
    lib = _load()
    lib.mzp_host_episode_seed.restype = C.c_ulonglong
    lib.mzp_host_episode_seed.argtypes = [C.c_ulonglong, C.c_uint]
    return lib.mzp_host_episode_seed


def test_episode_seed_mirror_equals_the_header():
    host = _host_episode_seed()
    for seed in (0, 1, 1 << 63, U64):
        assert reset_ref.episode_seed(seed, 0) == host(seed, 0) == seed  # episode 0 is what mz_reset draws: the seed itself
        for episode in (0, 1, 2, 1 << 31, (1 << 32) - 1):
            assert reset_ref.episode_seed(seed, episode) == host(seed, episode), (seed, episode)
    rng = np.random.default_rng(0)
    seeds = rng.integers(0, 1 << 64, 1000, dtype=np.uint64)
    episodes = rng.integers(0, 1 << 32, 1000, dtype=np.uint64)
    got = [reset_ref.episode_seed(int(s), int(e)) for s, e in zip(seeds, episodes)]
    assert got == [host(int(s), int(e)) for s, e in zip(seeds, episodes)]
    assert len(set(got)) == 1000
    # the counter is the multiplier's argument, not a plain offset of the seed: neighbours in either argument share no value
    assert len({reset_ref.episode_seed(s, e) for s in range(8) for e in range(8)}) == 64


def test_expected_reset_separates_episodes_and_slots(oracle):
    n, seed = 12, 77
    for robot, task in (("ant", T.DistRewardUMaze), ("point", T.DistRewardPush), ("swimmer", T.DistRewardUMaze)):
        cm = model.compile_model(robot, task(4.0), 4.0)
        plain_st, plain_obs = oracle.reset(cm, n, seed, env0=1000)
        st0, obs0 = reset_ref.expected_reset(oracle, cm, n, seed, np.zeros(n, np.int64), 1000)
        assert np.array_equal(obs0, plain_obs) and all(np.array_equal(st0[k], plain_st[k]) for k in plain_st)
        nr = cm.c.nq_robot
        # every episode its own draw, and the rows are those of the episode each env is in
        episodes = np.arange(n) % 3
        st, obs = reset_ref.expected_reset(oracle, cm, n, seed, episodes, 1000)
        per_k = [oracle.reset(cm, n, reset_ref.episode_seed(seed, k), env0=1000) for k in range(3)]
        for e in range(n):
            k = int(episodes[e])
            assert np.array_equal(st["qpos"][e], per_k[k][0]["qpos"][e]) and np.array_equal(obs[e], per_k[k][1][e])
            for other in range(3):
                if other != k:
                    assert np.all(st["qpos"][e, :nr] != per_k[other][0]["qpos"][e, :nr]) and np.all(st["qvel"][e, :cm.c.nv_robot] != per_k[other][0]["qvel"][e, :cm.c.nv_robot])
        assert np.array_equal(st["qpos"][episodes == 0], plain_st["qpos"][episodes == 0])
        # the global slot keys the draw: another env0 gives other rows, and slot 1000 + e is slot 1003 + (e - 3)
        st3, _ = reset_ref.expected_reset(oracle, cm, n, seed, episodes, 1003)
        assert np.all(st3["qpos"][:, :nr] != st["qpos"][:, :nr])
        same = episodes[3:] == episodes[:-3]
        assert same.all() and np.array_equal(st3["qpos"][:-3], st["qpos"][3:])
        # coordinates outside the robot's carry no noise in any episode
        assert np.array_equal(st["qpos"][:, nr:], np.tile(np.array(cm.c.qpos0[nr:cm.c.nq]), (n, 1)))
