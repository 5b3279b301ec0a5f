"""The Newton loop of the Ant row solver after its non-arithmetic issue slots went (csrc/ant_newton_rows.h ant_solve_rows_core,
DESIGN.md 3.1 "Newton-loop slots"): the slot guards' votes are taken once per solve, the active-set vote has no exec-mask region,
the limit rows' curvature enters the diagonal as one multiply-add with a lane constant, the solver's settings are unpacked in front of
the loop.  None of it changes an arithmetic result; what could go wrong is control flow — a slot skipped that a row needs, a vote
that misses a lane, a one-hot constant on the wrong lane — and that gives wrong numbers, not a fault.  So small batches that take
each of those paths are stepped against the float64 oracle.

States come from the oracle alone: its reset plus 200 random-action steps over 64 envs (tests/test_gpu_parity.py _rollout_states),
of which a few are picked by index; the properties the cases rely on are asserted below from the oracle's counts on the state the
device holds.
  * `two_waves`: 8 envs of AntUMaze-v0 at 16 lanes — two waves.  The first holds envs with 1, 2, 3 and 2 contacts (the guards of
    slots 1 and 2 taken and not taken within one launch), in the second two of the four envs are lifted by a metre: their contact
    rows are empty while their wave-mates' are not.
  * `six_envs`: the first six of them — the second wave's last two DPP rows hold no env at all.
  * `foot_at_wall`: 8 envs, in each wave one env moved in front of the east wall face (x = 20) of the UMaze's first corridor so
    that a foot touches it — three contacts in one wave, four in the other — next to wave-mates with one or two.
  * `hinge_beyond_limit`: one env (a wave with three empty rows) whose first hip is set to 33 degrees, three beyond its range: the
    limit row is active, its curvature on the diagonal is not zero.
Each case: three consecutive steps; every step of every env against the oracle stepped from the state the device held in front of
that step, inside the plain Ant tolerance of tests/test_gpu_parity.py (`_close`: 1e-5 absolute on qpos, 1e-5 + 1e-5 |x| on qvel
and the observation) with NO env on the discontinuity route; status words zero on the device as the oracle's solver flags are
(`forward_report`: status 0 at every start state), the oracle's iteration count below its cap and the device's cap bit clear.

Checked on the CPU before this test was written: the fp32 emulation of the step (tests/emu_lib.py) along the same three steps is at
most 1.2e-6 (qvel) / 6.0e-7 (qpos) off the oracle in every case, no status bit."""
import numpy as np
import pytest

import mujoco_maze_amd as mm
from tests.test_gpu_parity import POS_RTOL, _close, _rollout_states

pytestmark = pytest.mark.gpu

N_ROLL, SEED, STEP = 64, 23, 200
STEPS = 3
WALL_X = np.float32(19.2)


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def rollout(oracle):
    """the 64 rollout states (computed once, never written to) and the model they belong to"""
    env = mm.make("AntUMaze-v0", num_envs=1, force_vec=True)
    cm = env.model
    st = _rollout_states(oracle, cm, N_ROLL, SEED, {STEP})[STEP]
    env.close()
    for v in st.values():
        v.setflags(write=False)
    return st


def _take(st, idx):
    return {k: st[k][idx].copy() for k in ("qpos", "qvel", "warm", "t")}


def _two_waves(st):
    s = _take(st, [1, 3, 2, 4, 7, 5, 11, 12])
    s["qpos"][[5, 7], 2] = s["qpos"][[5, 7], 2].astype(np.float32) + np.float32(1.0)
    return s


def _six_envs(st):
    return _take(st, [1, 3, 2, 4, 7, 5])


def _foot_at_wall(st):
    s = _take(st, [1, 5, 4, 12, 3, 7, 11, 14])
    s["qpos"][0, :2] = (WALL_X, np.float32(0.0))
    s["qpos"][4, :2] = (WALL_X, np.float32(0.5))
    return s


def _hinge_beyond_limit(st):
    s = _take(st, [9])
    s["qpos"][0, 7] = np.float32(np.radians(33.0))
    return s


def _counts(oracle, cm, s, act):
    cnt = oracle.forward(cm, s["qpos"], s["qvel"], act.astype(np.float64), s["warm"])["counts"].astype(int)
    return cnt[:, 0], cnt[:, 1] - 4 * cnt[:, 0]  # contacts, active limit rows (a contact is four pyramid rows, a limit one)


def _expect_two_waves(nc, nlim):
    assert nc[:4].tolist() == [1, 2, 3, 2] and nc[5] == 0 and nc[7] == 0 and nc[4] > 0 and nc[6] > 0, nc


def _expect_six_envs(nc, nlim):
    assert nc[:4].tolist() == [1, 2, 3, 2] and len(nc) == 6, nc


def _expect_foot_at_wall(nc, nlim):
    assert nc[0] == 3 and nc[4] == 4, nc
    assert all(1 <= c <= 2 for c in np.delete(nc, [0, 4])), nc


def _expect_hinge_beyond_limit(nc, nlim):
    assert nlim[0] >= 1, nlim


CASES = {"two_waves": (_two_waves, _expect_two_waves, 1), "six_envs": (_six_envs, _expect_six_envs, 1),
         "foot_at_wall": (_foot_at_wall, _expect_foot_at_wall, 4), "hinge_beyond_limit": (_hinge_beyond_limit, _expect_hinge_beyond_limit, 2)}


@pytest.mark.parametrize("case", list(CASES))
def test_three_steps_against_the_oracle(torch, oracle, rollout, case):
    build, expect, act_seed = CASES[case]
    start = build(rollout)
    n = len(start["t"])
    env = mm.make("AntUMaze-v0", num_envs=n, force_vec=True)
    env.set_option("lanes_per_env", 16)
    env.set_option("waves_per_simd", 1)
    assert env.launch_info()["lanes_per_env"] == 16 and env.launch_info()["waves_per_simd"] == 1
    cm = env.model
    acts = np.random.default_rng(act_seed).uniform(-30, 30, (STEPS, n, 8)).astype(np.float32)
    env.set_state(start["qpos"], start["qvel"], start["warm"], start["t"])
    for k in range(STEPS):
        dq, dv, dw, dt = [x.cpu().numpy() for x in env.get_state()]
        ref_state = dict(qpos=dq.astype(np.float64), qvel=dv.astype(np.float64), warm=dw.astype(np.float64), t=dt.copy())
        nc, nlim = _counts(oracle, cm, ref_state, acts[k])
        print(f"{case} step {k}: oracle contacts {nc.tolist()}, active limit rows {nlim.tolist()}")
        if k == 0:
            expect(nc, nlim)
        for e in range(n):  # the oracle's own solver flags at the state the device starts from
            rep, _ = oracle.forward_report(cm, ref_state["qpos"][e], ref_state["qvel"][e], acts[k][e].astype(np.float64), ref_state["warm"][e])
            assert int(rep["status"]) == 0 and rep["iters"] < 100, (k, e, rep)
        obs, rew, done, info = env.step(torch.as_tensor(acts[k], device=env.device))
        status = env.status().cpu().numpy()
        assert np.all(status == 0), (k, status.tolist())  # no NaN, no contact overflow, no solve at the iteration cap: the oracle's flags
        ref = oracle.step(cm, ref_state, acts[k].astype(np.float64), nthreads=8)  # advances ref_state in place
        qpos, qvel = [x.cpu().numpy() for x in env.get_state()[:2]]
        eq, ev = np.abs(qpos - ref_state["qpos"]).max(), np.abs(qvel - ref_state["qvel"]).max()
        print(f"{case} step {k}: |qpos - oracle| {eq:.1e}, |qvel - oracle| {ev:.1e}")
        assert np.all(_close(qpos, ref_state["qpos"], rtol=POS_RTOL)), (k, eq)
        assert np.all(_close(qvel, ref_state["qvel"])), (k, ev)
        assert np.all(_close(obs.cpu().numpy(), ref["obs"]))
        assert np.all(_close(rew.cpu().numpy(), ref["reward"], atol=1e-6))
        assert np.array_equal(done.cpu().numpy(), ref["done"])
    env.close()
