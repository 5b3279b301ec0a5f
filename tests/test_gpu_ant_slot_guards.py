"""The row solver runs only the contact slots some env of the wave uses (csrc/ant_newton_rows.h each_contact: for the plain ant one
wave-uniform guard per slot 0 .. 3, the groups of 4 | 6 | 8 | 12 | 16 behind them; the one-block ant guards the first four as a
block).  A skipped slot holds zero columns in every row of the wave, so skipping it must not move one bit — and what a wave skips
depends on its env's WAVE-MATES, which the result of an env must not.

States: the oracle's reset plus 200 random-action steps over 1024 envs (tests/test_gpu_parity.py _rollout_states), 64 of them
picked by the oracle's contact count into 16 waves of four (arrangement A, `pick_arrangement`), the last eight moved with
`wrapped_env.set_xy` in front of the east wall face (x = 20) of the UMaze's first corridor as tests/test_gpu_ant_row_slots.py does:
five and more contacts.  Asserted from the oracle alone: A holds a wave whose largest count is exactly 1, one at 2, 3, 4 and one at
5 or more, a wave that mixes a 0-contact env with a 3- or 4-contact env, and nobody beyond the kernel's 16 slots.

  (a) the same step twice from the same state: bitwise equal;
  (b) wave-mate independence: arrangement B = A permuted by i -> (i % W) * 4 + i // W (W waves: the four envs of a wave of A land
      in four different waves of B, every env gets three other wave-mates), states and actions permuted alike — obs, reward, done,
      qpos, qvel and warm start of each env after one step bitwise equal to A's.  A guard that skips a slot some row needs shows
      here, and so does a guard tested per env instead of per wave;
  (c) one step against the float64 oracle, tolerances and outlier proof of tests/test_gpu_parity.py.
(a) and (b) again with two waves per SIMD (the fold on the matrix cores) and on AntPush-v0 at 16 lanes (the NB = 1 row solver)."""
import numpy as np
import pytest

import mujoco_maze_amd as mm
from tests.test_gpu_parity import _assert_step_parity, _close, _rollout_states

pytestmark = pytest.mark.gpu

N = 64           # 16 waves at 16 lanes per env
N_ROLL = 1024    # envs of the rollout the 64 are picked from
STEP = 200
SEED = 23
WALL_ENVS = 8    # the last two waves of arrangement A
NAMES = ("obs", "reward", "done", "qpos", "qvel", "warm", "t")


def pick_arrangement(nc):
    """64 env indices of the rollout, by contact count `nc`: rows = waves of arrangement A.  -1: any env not yet taken."""
    waves = [(1, 1, 0, 1), (2, 1, 2, 0), (3, 2, 1, 3), (4, 1, 2, 3), (0, 3, 0, 3), (0, 0, 0, 0), (4, 0, 2, 1), (2, 2, 2, 2),
             (1, 0, 0, 0), (3, 3, 1, 0), (2, 0, 1, 1), (1, 2, 3, 2), (0, 1, 2, 3), (1, 1, 1, 1), (-1, -1, -1, -1), (-1, -1, -1, -1)]
    pools = {c: list(np.flatnonzero(nc == c)) for c in range(5)}
    out = []
    for w in waves:
        for c in w:
            if c >= 0:
                assert pools[c], f"the rollout holds too few envs with {c} contacts: {np.bincount(nc).tolist()}"
                out.append(pools[c].pop(0))
    rest = [i for i in range(len(nc)) if i not in set(out)]
    out += rest[: N - len(out)]
    return np.array(out)


def _regroup(w):
    """arrangement A -> B for 4 w envs in w waves: the env at index i of A sits at index (i % w) * 4 + i // w of B"""
    i = np.arange(4 * w)
    return (i % w) * 4 + i // w


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


def _assert_repeatable_and_mate_independent(torch, env, start, act):
    """(a) and (b); returns the first step's outputs and status words"""
    w = len(act) // 4
    first, status = _step_from(torch, env, start, act)
    second, _ = _step_from(torch, env, start, act)
    for name, a, b in zip(NAMES, first, second):
        assert np.array_equal(a, b), f"(a) {name}: the same step from the same state gave different bits"
    to_b = _regroup(w)
    assert len(set((i // 4, to_b[i] // 4) for i in range(4 * w))) == 4 * w  # no two envs share a wave in both arrangements
    from_a = np.argsort(to_b)  # B[j] = A[from_a[j]]
    start_b = {k: v[from_a] for k, v in start.items()}
    third, _ = _step_from(torch, env, start_b, act[from_a])
    for name, a, b in zip(NAMES, first, third):
        diff = a != b[to_b]
        assert not diff.any(), f"(b) {name}: {int(diff.reshape(len(a), -1).any(1).sum())} envs step differently with other wave-mates"
    return first, status


@pytest.fixture(scope="module")
def plain_ant(torch, oracle):
    """(env at 16 lanes, start state of arrangement A as the device holds it, actions, oracle contact counts)"""
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
    top = nc.reshape(-1, 4).max(1)
    print(f"oracle contact counts of arrangement A, by wave: {nc.reshape(-1, 4).tolist()}")
    for want in (1, 2, 3, 4):
        assert (top == want).any(), (want, top)
    assert (top >= 5).any(), top
    assert any((w == 0).any() and w.max() in (3, 4) for w in nc.reshape(-1, 4)), nc.reshape(-1, 4)
    assert nc.max() <= 16, nc.max()
    yield env, start, act, nc
    env.close()


def test_plain_ant_one_wave_per_simd(torch, oracle, plain_ant):
    env, start, act, nc = plain_ant
    env.set_option("waves_per_simd", 1)
    assert env.launch_info()["lanes_per_env"] == 16 and env.launch_info()["waves_per_simd"] == 1
    first, status = _assert_repeatable_and_mate_independent(torch, env, start, act)
    # (c) against the oracle
    cm = env.model
    ref_state = {k: v.copy() for k, v in start.items()}
    ref = oracle.step(cm, ref_state, act.astype(np.float64), nthreads=8)
    obs, rew, done, qpos, qvel = first[:5]
    assert np.all((status & 7) == 0), np.unique(status)  # no NaN, no contact overflow, no solve at the iteration cap
    # outlier cap, the rule of tests/test_gpu_ant_row_slots.py: 0.08 x the share of the batch placed at the wall
    good = _assert_step_parity(oracle, cm, start, act, qpos, qvel, ref_state, max_outlier_frac=0.08 * WALL_ENVS / N, dev_out=(obs, rew, done))
    assert np.all(_close(obs[good], ref["obs"][good]))
    assert np.all(_close(rew[good], ref["reward"][good], atol=1e-6))
    assert np.array_equal(done, ref["done"])


def test_plain_ant_two_waves_per_simd(torch, plain_ant):
    env, start, act, nc = plain_ant
    env.set_option("waves_per_simd", 2)
    assert env.launch_info()["waves_per_simd"] == 2
    _, status = _assert_repeatable_and_mate_independent(torch, env, start, act)
    assert np.all((status & 7) == 0), np.unique(status)


def test_one_block_ant_at_16_lanes(torch, oracle):
    n = 32
    env = mm.make("AntPush-v0", num_envs=n)
    env.set_option("lanes_per_env", 16)
    assert env.launch_info()["lanes_per_env"] == 16
    st = _rollout_states(oracle, env.model, n, 21, {20})[20]
    act = np.random.default_rng(9).uniform(-30, 30, (n, 8)).astype(np.float32)
    nc = oracle.forward(env.model, st["qpos"], st["qvel"], act.astype(np.float64), st["warm"])["counts"][:, 0].astype(int)
    print(f"oracle contact counts (block's and robot's), by wave: {nc.reshape(-1, 4).tolist()}")
    _, status = _assert_repeatable_and_mate_independent(torch, env, st, act)
    assert np.all((status & 3) == 0), np.unique(status)
    env.close()
