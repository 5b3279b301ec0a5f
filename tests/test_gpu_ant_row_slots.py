"""The row solver's hand-scheduled DPP blocks on crowded contact sets (csrc/ant_newton_rows.h: rsum3 / rsum3_scaled in jdot3, the
pivot's v_max_f32_dpp): ants leaning on a wall hold five to thirteen contacts, so the contact slots beyond the first four — which
a rollout under random actions hardly reaches — and every guard level of `each_contact` run.

State: the oracle's reset plus 30 random-action steps (tests/test_gpu_parity.py _rollout_states), then half of the envs moved with
`wrapped_env.set_xy` to 0.25 .. 0.55 m in front of the east wall face (x = 20) of the UMaze's first corridor: legs reach 1.1 m
from the torso, so several leg capsules and often the torso sphere touch the wall on top of the floor contacts.

  (a) one step against the float64 oracle, tolerances and outlier proof of tests/test_gpu_parity.py;
  (b) the same step again from the same state through mz_set_state: bitwise equal.  Nothing in a step is random or depends on
      another env, so any difference is a read of a register before its write has landed — what a DPP hazard looks like."""
import numpy as np
import pytest

import mujoco_maze_amd as mm
from tests.test_gpu_parity import _assert_step_parity, _close, _rollout_states

pytestmark = pytest.mark.gpu

N = 256


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def test_crowded_contact_slots_step_parity_and_repeatability(torch, oracle):
    env = mm.make("AntUMaze-v0", num_envs=N)
    env.set_option("lanes_per_env", 16)  # one DPP row per env: the instantiation the benchmark runs
    assert env.launch_info()["lanes_per_env"] == 16
    cm = env.model
    st = _rollout_states(oracle, cm, N, 17, {30})[30]
    env.set_state(st["qpos"], st["qvel"], st["warm"], st["t"])
    rng = np.random.default_rng(6)
    xy = env.wrapped_env.get_xy().cpu().numpy()
    xy[: N // 2, 0] = rng.uniform(19.45, 19.75, N // 2)
    xy[: N // 2, 1] = rng.uniform(-1.0, 1.0, N // 2)
    env.wrapped_env.set_xy(xy)
    # the fp32 state the device now holds is the start of both sides
    dq, dv, dw, dt = [x.cpu().numpy() for x in env.get_state()]
    start = dict(qpos=dq.astype(np.float64), qvel=dv.astype(np.float64), warm=dw.astype(np.float64), t=dt.copy())
    assert np.array_equal(start["qpos"][:, :2], xy.astype(np.float64)) and np.array_equal(start["qvel"], st["qvel"])
    act = np.random.default_rng(1).uniform(-30, 30, (N, 8)).astype(np.float32)

    # condition of the fixture, from the float64 oracle alone: at least 5 contacts in at least 16 envs (measured: 115, up to 13)
    nc = oracle.forward(cm, start["qpos"], start["qvel"], act.astype(np.float64), start["warm"])["counts"][:, 0]
    print(f"oracle contact counts: {np.bincount(nc.astype(int)).tolist()}")
    assert (nc >= 5).sum() >= 16, np.bincount(nc.astype(int))
    assert nc.max() <= 16  # nobody beyond the kernel's contact slots: every env is a parity case

    def step_from_start():
        env.set_state(start["qpos"], start["qvel"], start["warm"], start["t"])
        obs, rew, done, info = env.step(torch.as_tensor(act, device=env.device))
        out = [obs, rew, done, *env.get_state()]
        return [x.cpu().numpy().copy() for x in out]

    first = step_from_start()
    status = env.status().cpu().numpy()
    second = step_from_start()

    # (a) against the oracle
    ref_state = {k: v.copy() for k, v in start.items()}
    ref = oracle.step(cm, ref_state, act.astype(np.float64), nthreads=8)
    obs, rew, done, qpos, qvel = first[0], first[1], first[2], first[3], first[4]
    worst = np.abs(qvel - ref_state["qvel"]).max(1)
    print(f"|qvel - oracle|: median {np.median(worst):.2e}, 99 % {np.quantile(worst, 0.99):.2e}, max {worst.max():.2e}; "
          f"envs outside 1e-5: {int((worst > 1e-5 + 1e-5 * np.abs(ref_state['qvel']).max(1)).sum())}")
    assert np.all((status & 7) == 0), np.unique(status)  # no NaN, no contact overflow, no solve at the iteration cap
    # Outlier cap: ants dropped INTO two walls of a corner are allowed 8 % of the batch on the oracle-proven discontinuity route
    # (test_ant_corner_contacts_overflow_the_staging: every env placed, two walls).  Here half of the batch is placed, against one
    # wall: 0.08 / 2.  Each such env must still be matched with the oracle's value on its side of the discontinuity.
    good = _assert_step_parity(oracle, cm, start, act, qpos, qvel, ref_state, max_outlier_frac=0.04, dev_out=(obs, rew, done))
    assert np.all(_close(obs[good], ref["obs"][good]))
    assert np.all(_close(rew[good], ref["reward"][good], atol=1e-6))
    assert np.array_equal(done, ref["done"])

    # (b) bitwise repeatable
    for name, a, b in zip(("obs", "reward", "done", "qpos", "qvel", "warm", "t"), first, second):
        assert np.array_equal(a, b), f"{name}: the same step from the same state gave different bits in {int((a != b).any(axis=-1).sum()) if a.ndim > 1 else int((a != b).sum())} envs"
    env.close()
