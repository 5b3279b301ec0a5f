"""The row solver's hand-placed DPP blocks open with the wait states their call site needs, and the Gauss-Jordan elimination is one
scheduled sequence (csrc/ant_newton_rows.h solve_rows: the pivot's reciprocal, its lane compare and both selects inside the string,
the hinge pivots' heads in each other's gaps).  A wait state that was needed and is gone gives a stale operand — wrong numbers, not
a fault — so this runs the kernels on states that use every part of the solver and compares with the float64 oracle.

States of the plain ant: the oracle's reset plus 200 random-action steps over 1024 envs (tests/test_gpu_parity.py _rollout_states),
64 of them picked by contact count into 16 waves of four and the last eight moved in front of the east wall face of the UMaze's
first corridor — five and more contact slots — as tests/test_gpu_ant_slot_guards.py does.  The one-block ant (AntPush-v0, the
16-column elimination and `resolve_rows`): 32 envs after 20 random-action steps.  For each of four kernels — the plain ant with one
and with two waves per SIMD, AntPush-v0 at 16 and at 32 lanes per env:
  (a) the same step twice from the same state: equal bits;
  (b) one step against the float64 oracle, `_assert_step_parity` of tests/test_gpu_parity.py with its tolerances — a stale DPP operand in
      a pivot is a wrong search direction and shows here;
  (c) 20 further steps: no status bit set, everything finite.
The parent of this change passes as well (profiles/wait_states/ab.md): the wait states that went did no work."""
import numpy as np
import pytest

import mujoco_maze_amd as mm
from tests.test_gpu_ant_slot_guards import N, N_ROLL, SEED, STEP, WALL_ENVS, pick_arrangement
from tests.test_gpu_parity import _assert_step_parity, _close, _rollout_states

pytestmark = pytest.mark.gpu

NAMES = ("obs", "reward", "done", "qpos", "qvel", "warm", "t")
MORE_STEPS = 20


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def _step_from(torch, env, start, act):
    env.set_state(start["qpos"], start["qvel"], start["warm"], start["t"])
    obs, rew, done, info = env.step(torch.as_tensor(act, device=env.device))
    out = [x.cpu().numpy().copy() for x in (obs, rew, done, *env.get_state())]
    return out, env.status().cpu().numpy().copy()


def _check(torch, oracle, env, start, act, max_outlier_frac):
    cm = env.model
    # (a)
    first, status = _step_from(torch, env, start, act)
    second, _ = _step_from(torch, env, start, act)
    for name, a, b in zip(NAMES, first, second):
        assert np.array_equal(a, b), f"(a) {name}: the same step from the same state gave different bits"
    # (b)
    assert np.all(status == 0), np.unique(status)
    ref_state = {k: v.copy() for k, v in start.items()}
    ref = oracle.step(cm, ref_state, act.astype(np.float64), nthreads=8)
    obs, rew, done, qpos, qvel = first[:5]
    good = _assert_step_parity(oracle, cm, start, act, qpos, qvel, ref_state, max_outlier_frac=max_outlier_frac, dev_out=(obs, rew, done))
    assert np.all(_close(obs[good], ref["obs"][good]))
    assert np.all(_close(rew[good], ref["reward"][good], atol=1e-6))
    assert np.array_equal(done, ref["done"])
    # (c) on from the state the second step left
    rng = np.random.default_rng(3)
    for k in range(MORE_STEPS):
        a = rng.uniform(-30, 30, act.shape).astype(np.float32)
        obs, rew, done, info = env.step(torch.as_tensor(a, device=env.device))
        st = env.status().cpu().numpy()
        assert np.all(st == 0), (k, np.unique(st))
        for name, x in zip(NAMES, (obs, rew, done, *env.get_state())):
            assert bool(torch.isfinite(x.float()).all()), (k, name)


@pytest.fixture(scope="module")
def plain_ant(torch, oracle):
    """(env at 16 lanes, start state as the device holds it, actions)"""
    env = mm.make("AntUMaze-v0", num_envs=N)
    env.set_option("lanes_per_env", 16)
    cm = env.model
    st = _rollout_states(oracle, cm, N_ROLL, SEED, {STEP})[STEP]
    nc_roll = oracle.forward(cm, st["qpos"], st["qvel"], None, st["warm"])["counts"][:, 0]
    pick = pick_arrangement(nc_roll)
    env.set_state(st["qpos"][pick], st["qvel"][pick], st["warm"][pick], st["t"][pick])
    rng = np.random.default_rng(6)
    xy = env.wrapped_env.get_xy().cpu().numpy()
    xy[-WALL_ENVS:, 0] = rng.uniform(19.45, 19.75, WALL_ENVS)
    xy[-WALL_ENVS:, 1] = rng.uniform(-1.0, 1.0, WALL_ENVS)
    env.wrapped_env.set_xy(xy)
    dq, dv, dw, dt = [x.cpu().numpy() for x in env.get_state()]
    start = dict(qpos=dq.astype(np.float64), qvel=dv.astype(np.float64), warm=dw.astype(np.float64), t=dt.copy())
    act = np.random.default_rng(1).uniform(-30, 30, (N, 8)).astype(np.float32)
    nc = oracle.forward(cm, start["qpos"], start["qvel"], act.astype(np.float64), start["warm"])["counts"][:, 0].astype(int)
    print(f"oracle contact counts by wave: {nc.reshape(-1, 4).tolist()}")
    assert (nc.reshape(-1, 4).max(1) >= 5).any() and nc.max() <= 16, nc  # five and more slots occur, nobody beyond the kernel's 16
    yield env, start, act
    env.close()


@pytest.mark.parametrize("waves", [1, 2])
def test_plain_ant(torch, oracle, plain_ant, waves):
    env, start, act = plain_ant
    env.set_option("waves_per_simd", waves)
    assert env.launch_info()["lanes_per_env"] == 16 and env.launch_info()["waves_per_simd"] == waves
    # outlier cap, the rule of tests/test_gpu_ant_slot_guards.py: 0.08 x the share of the batch placed at the wall
    _check(torch, oracle, env, start, act, max_outlier_frac=0.08 * WALL_ENVS / N)


@pytest.fixture(scope="module")
def push_states(oracle):
    n = 32
    env = mm.make("AntPush-v0", num_envs=n)
    st = _rollout_states(oracle, env.model, n, 21, {20})[20]
    env.close()
    return st, np.random.default_rng(9).uniform(-30, 30, (n, 8)).astype(np.float32)


@pytest.mark.parametrize("lanes", [16, 32])
def test_one_block_ant(torch, oracle, push_states, lanes):
    st, act = push_states
    env = mm.make("AntPush-v0", num_envs=len(act))
    env.set_option("lanes_per_env", lanes)
    assert env.launch_info()["lanes_per_env"] == lanes
    _check(torch, oracle, env, st, act, max_outlier_frac=0.005)  # the cap of tests/test_gpu_parity.py test_ant_push_movable_block
    env.close()
