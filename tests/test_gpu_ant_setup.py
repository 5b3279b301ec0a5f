"""The set-up of the Ant row solver takes the env's contact counts from the forward pass's registers, and `wr_col` decides from a
per-lane bit table which contacts a dof sees (csrc/ant_newton_rows.h ant_solve_rows_core, csrc/ant_forward_rows.h).  The cases in
which that can go wrong are waves whose envs take different paths through the forward pass:

  * a MIXED FALL-BACK wave: one env has a geom with four contacts (a foot in the south-east corner of the UMaze's first corridor:
    floor and two wall faces), so its wave takes the two-pass enumeration, which writes its own counts to LDS — the one case where
    registers and LDS disagree — while its three wave-mates keep theirs;
  * a MIXED AIRBORNE wave: one env has no contact and no active limit row (the `!has` path: qacc = qacc_smooth), its mates have
    contacts;
  * LIMIT ROWS: hinges beyond their range.

States: arrangement A of tests/test_gpu_ant_wait_states.py (64 envs of the oracle's 200-step rollout picked by contact count into
16 waves of four, the last eight in front of the east wall face), with two envs replaced on the host: slot 28 (a wave of envs with
two contacts each) by rollout state 136 put into the corridor's corner, slot 52 (a wave of envs with one contact each) by rollout
state 131 lifted by one metre.  Both were chosen on the CPU with the oracle: state 136 at this place has a geom with four contacts,
five in all, and the fp32 emulation of the step (tests/emu_lib.py) is 6.0e-7 / 4.0e-7 (qpos / qvel) off the float64 oracle there,
inside `_assert_step_parity`'s 1e-5; state 131 has no active limit and, lifted, no contact.  Every property is asserted below from
the oracle on the state the device holds.

For one and two waves per SIMD: (a) the same step twice gives equal bits; (b) one step against the float64 oracle
(`_assert_step_parity`, its tolerances, the outlier cap of tests/test_gpu_ant_wait_states.py); (c) the same env states dealt into
other waves (i -> (i % 16) * 4 + i // 16: every env gets three other wave-mates) give every env equal bits; (d) 20 further steps: no
status bit, everything finite.  AntPush-v0, 32 envs at 16 and at 32 lanes: (a), (b), (d).  The parent of this change passes this file
as well (profiles/solve_setup/ab.md)."""
import numpy as np
import pytest

import mujoco_maze_amd as mm
from tests.test_gpu_ant_slot_guards import N, N_ROLL, SEED, STEP, WALL_ENVS, _assert_repeatable_and_mate_independent, pick_arrangement
from tests.test_gpu_ant_wait_states import _check
from tests.test_gpu_parity import _rollout_states

pytestmark = pytest.mark.gpu

FALLBACK_SLOT, FALLBACK_STATE, FALLBACK_XY = 28, 136, (19.277790069580078, -3.2281203269958496)  # (float32 values)
AIR_SLOT, AIR_STATE, AIR_LIFT = 52, 131, 1.0


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def _geom_counts(oracle, cm, qpos):
    """contacts per robot geom (ids 1 .. 13; 0 is the floor, -1 a maze box) at one configuration"""
    c = oracle.contacts(cm, qpos)
    if len(c) == 0:
        return np.zeros(14, int)
    g1, g2 = c[:, 7].astype(int), c[:, 8].astype(int)
    return np.bincount(np.where((g1 >= 1) & (g1 <= 13), g1, g2), minlength=14)


@pytest.fixture(scope="module")
def plain_ant(torch, oracle):
    """(env at 16 lanes, start state, actions)"""
    env = mm.make("AntUMaze-v0", num_envs=N)
    env.set_option("lanes_per_env", 16)
    cm = env.model
    st = _rollout_states(oracle, cm, N_ROLL, SEED, {STEP})[STEP]
    nc_roll = oracle.forward(cm, st["qpos"], st["qvel"], None, st["warm"])["counts"][:, 0]
    pick = pick_arrangement(nc_roll)
    assert FALLBACK_STATE not in pick and AIR_STATE not in pick
    env.set_state(st["qpos"][pick], st["qvel"][pick], st["warm"][pick], st["t"][pick])
    rng = np.random.default_rng(6)
    xy = env.wrapped_env.get_xy().cpu().numpy()
    xy[-WALL_ENVS:, 0] = rng.uniform(19.45, 19.75, WALL_ENVS)
    xy[-WALL_ENVS:, 1] = rng.uniform(-1.0, 1.0, WALL_ENVS)
    env.wrapped_env.set_xy(xy)
    dq, dv, dw, dt = [x.cpu().numpy() for x in env.get_state()]
    start = dict(qpos=dq.astype(np.float64), qvel=dv.astype(np.float64), warm=dw.astype(np.float64), t=dt.copy())
    for slot, src in ((FALLBACK_SLOT, FALLBACK_STATE), (AIR_SLOT, AIR_STATE)):
        for k in ("qpos", "qvel", "warm", "t"):
            start[k][slot] = st[k][src]  # (fp32 values: _rollout_states rounds)
    start["qpos"][FALLBACK_SLOT, :2] = FALLBACK_XY
    start["qpos"][AIR_SLOT, 2] = np.float32(start["qpos"][AIR_SLOT, 2] + AIR_LIFT)
    act = np.random.default_rng(1).uniform(-30, 30, (N, 8)).astype(np.float32)

    cnt = oracle.forward(cm, start["qpos"], start["qvel"], act.astype(np.float64), start["warm"])["counts"].astype(int)
    nc, nlim = cnt[:, 0], cnt[:, 1] - 4 * cnt[:, 0]  # (a contact is four pyramid rows, a limit one)
    per_geom = np.array([_geom_counts(oracle, cm, q).max() for q in start["qpos"]])
    print(f"oracle contact counts by wave: {nc.reshape(-1, 4).tolist()}\nactive limits by wave: {nlim.reshape(-1, 4).tolist()}\n"
          f"largest count of one geom by wave: {per_geom.reshape(-1, 4).tolist()}")
    assert (nc.reshape(-1, 4).max(1) >= 5).any() and nc.max() <= 16, nc
    fw = FALLBACK_SLOT // 4 * 4
    assert per_geom[FALLBACK_SLOT] >= 4 and all(per_geom[i] <= 3 for i in range(fw, fw + 4) if i != FALLBACK_SLOT), per_geom[fw:fw + 4]
    aw = AIR_SLOT // 4 * 4
    assert nc[AIR_SLOT] == 0 and nlim[AIR_SLOT] == 0 and all(nc[i] > 0 for i in range(aw, aw + 4) if i != AIR_SLOT), (nc[aw:aw + 4], nlim[aw:aw + 4])
    assert (nlim > 0).sum() >= 8, nlim
    yield env, start, act
    env.close()


@pytest.mark.parametrize("waves", [1, 2])
def test_plain_ant(torch, oracle, plain_ant, waves):
    env, start, act = plain_ant
    env.set_option("waves_per_simd", waves)
    assert env.launch_info()["lanes_per_env"] == 16 and env.launch_info()["waves_per_simd"] == waves
    _assert_repeatable_and_mate_independent(torch, env, start, act)  # (a), (c)
    _check(torch, oracle, env, start, act, max_outlier_frac=0.08 * WALL_ENVS / N)  # (a), (b), (d)


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
