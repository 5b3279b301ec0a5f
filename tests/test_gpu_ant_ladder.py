"""The Ant ladder, rung by rung: ant_config / ant_rung_lanes of csrc/ant_kernels.hip turn a handle into one instantiation
ant_step_kernel<NB, G> — NB the configuration of movable bodies (0 plain, 1 one two-slide block, 2 / 3 two / three blocks, 4 one
three-slide block, 5 the object ball), G the lanes per env — and the step, mz_debug_forward and launch_info() all go through that
one rule.  Nineteen rungs are compiled (G in 16 / 32 / 64 for every NB, and (0, 8)); every one can be selected with the option
"lanes_per_env".  The other GPU modules run the default rungs and the plain and one-block ant's other widths; this module runs the
nine that nothing ran (DESIGN.md section 3.1 holds the table of rungs and tests):

    (1, 64)  AntPush-v0 + 64                     (4, 16) (4, 32)  AntMultiFall-v0 + 16 / 32
    (2, 16) (2, 32)  AntMultiPush-v0 + 16 / 32   (5, 16) (5, 32)  AntSmallBilliard-v0 + 16 / 32
    (3, 16) (3, 32)  AntPushMaze-v0 + 16 / 32

Every test first asserts, from the model constants and launch_info(), that it is on the rung it names (`_on_rung`): the rungs of one
configuration agree to fp32 round-off, so a ladder that sent one lane count to another rung's kernel would show nowhere else.

For NB >= 2 the kernels run the lane-group solver (ant_solve, the merged con_enum_item / con_map_item with the re-enumeration on
overflow: csrc/ant_dyn.h).  At 64 lanes an env has a wavefront to itself; at 16 / 32 lanes four / two envs with blocks share one,
a converged env sits through its mates' Newton iterations and the re-enumeration runs for some lanes of a wave only.

The comparisons are those of tests/test_gpu_parity.py and nothing is looser: one step from injected fp32 states against the float64
oracle through `_assert_step_parity` at ATOL / POS_RTOL / BRANCH_ATOL, with the cap on envs taking the discontinuity route that the
maze's pinned test has (0.005 one block, 0.006 multi-block, 0.01 Fall / Billiard: one env of 66 per checkpoint).  The cap is a
condition on the states, not a measurement: each case first sends the same states through the maze's default rung — pinned by the
tests of the other modules — under the same cap, and a new rung gets no more than that control.  States are taken as the pinned test
of the same maze takes them (seeds, placements and checkpoints of test_ant_push_movable_block, test_ant_multi_block_mazes,
test_ant_fall_maze, test_ant_small_billiard_free_joint_ball), at N = 66: sixteen full waves and a half wave at 16 lanes, 33 waves
at 32, 66 at 64.  On those seeds no env of a control or of a rung leaves the plain tolerance, and every rung returns its control's
observation bit for bit (profiles/ant_ladder/parity.md) — parity cannot tell the rungs of one configuration apart, `_on_rung` and
the rows of tests/test_gpu_env_isolation.py in which blocks share a wave do."""
import numpy as np
import pytest

import mujoco_maze_amd as mm
from mujoco_maze_amd import _capi
from tests.test_gpu_parity import _assert_step_parity, _close, _f32

pytestmark = pytest.mark.gpu
N = 66


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


# ---------------------------------------------------------------------------------------------- 0. the rungs
def _ant_rung(env_id, lanes=None, **options):
    def make(n, **kw):
        env = mm.make(env_id, num_envs=n, **kw)
        if lanes:
            env.set_option("lanes_per_env", lanes)
        for key, v in options.items():
            env.set_option(key, v)
        return env
    return make


# the maze that reaches configuration NB (ant_config of csrc/ant_kernels.hip), and the G its handle takes by default at N envs
MAZE = {0: ("AntUMaze-v0", 16), 1: ("AntPush-v0", 32), 2: ("AntMultiPush-v0", 64), 3: ("AntPushMaze-v0", 64), 4: ("AntMultiFall-v0", 64),
        5: ("AntSmallBilliard-v0", 64)}
# name -> (make(n, **kw), (NB, G)); a default rung is made without the option, so that the table holds the defaults as well
RUNGS = {f"ant-{nb}-{g}": (_ant_rung(env_id, None if g == default else g), (nb, g))
         for nb, (env_id, default) in MAZE.items() for g in ((8, 16, 32, 64) if nb == 0 else (16, 32, 64))}
RUNGS["ant-0-16-wps2"] = (_ant_rung("AntUMaze-v0", 16, waves_per_simd=2), (0, 16))  # the kernel held to two waves per SIMD
NEW = ["ant-1-64", "ant-2-16", "ant-2-32", "ant-3-16", "ant-3-32", "ant-4-16", "ant-4-32", "ant-5-16", "ant-5-32"]


def _config(m):
    """ant_config of csrc/ant_kernels.hip from the model constants: 0-3 two-slide blocks, 4 one three-slide block, 5 the ball"""
    slides = m.body_jntnum[m.block_bodyid[0]] if m.nblock else 0
    assert slides in ((0,) if m.nblock == 0 else (2, 3)) and m.nball <= 1 and not (m.nball and m.nblock)
    assert m.nv == 14 + (slides if m.nblock == 1 else 2 * m.nblock) + 6 * m.nball, (m.nv, m.nblock, m.nball)
    return 5 if m.nball else (4 if (m.nblock == 1 and slides == 3) else m.nblock)


def _on_rung(env, name):
    """the env is on the rung `name`: movable bodies of the model, the Ant's specialised engine, lanes per env and waves per SIMD of
    the instantiation the next step launches"""
    want = RUNGS[name][1]
    m, li = env.model.c, env.launch_info()
    assert li["engine"] == 0, (name, li)
    got = (_config(m), li["lanes_per_env"])
    assert got == want, (name, got, want)
    assert li["waves_per_simd"] == (2 if name.endswith("wps2") else 1), (name, li)


def _make(name, n=N, **kw):
    env = RUNGS[name][0](n, **kw)
    try:
        _on_rung(env, name)
    except BaseException:
        env.close()
        raise
    return env


# the instantiations of csrc/ant_kernels.hip: G in 16 / 32 / 64 for every configuration, and (0, 8); the twentieth row of the table is
# the plain ant's 16-lane kernel at two waves per SIMD
assert {r for _, r in RUNGS.values()} == {(nb, g) for nb in range(6) for g in (16, 32, 64)} | {(0, 8)} and len(RUNGS) == 20
assert {RUNGS[name][1] for name in NEW} == {(1, 64)} | {(nb, g) for nb in (2, 3, 4, 5) for g in (16, 32)}


@pytest.mark.parametrize("name", list(RUNGS))
def test_every_rung_has_a_constructor(torch, name):
    env = _make(name)
    env.close()


@pytest.mark.parametrize("nb", [1, 2, 3, 4, 5])
def test_block_ants_refuse_8_lanes(torch, nb):
    """8 lanes per env exist for the plain ant alone.  An Ant with movable bodies refuses the value (MZ_ERR_UNSUPPORTED, a message
    that names the configuration) instead of stepping on another width while reporting 8; the handle keeps its rung and steps."""
    default = f"ant-{nb}-{MAZE[nb][1]}"
    env = _make(default)
    try:
        with pytest.raises(_capi.MazeStepError, match=r"code -3.*plain Ant only"):
            env.set_option("lanes_per_env", 8)
        _on_rung(env, default)
        env.set_option("lanes_per_env", 16)
        _on_rung(env, f"ant-{nb}-16")
        with pytest.raises(_capi.MazeStepError, match=r"code -3"):
            env.set_option("lanes_per_env", 8)
        _on_rung(env, f"ant-{nb}-16")
        env.reset(seed=1)
        obs, *_ = env.step(torch.zeros((N, env.nu), device=env.device))
        assert torch.isfinite(obs).all() and int((env.status() & 7).sum()) == 0
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------- 1. states, as the pinned tests take them
def _place_nothing(st, rng, cm):
    pass


def _place_push(st, rng, cm):  # test_ant_push_movable_block: a third of the ants in front of the block, walking into it
    n = len(st["t"])
    st["qpos"][: n // 3, 1] = 3.0 + rng.uniform(0.2, 0.6, n // 3)
    st["qvel"][: n // 3, 1] = 1.5


def _place_blocks(st, rng, cm):  # test_ant_multi_block_mazes: random block velocities
    st["qvel"][:, 14:] = rng.uniform(-3, 3, (len(st["t"]), 2 * cm.c.nblock))


def _place_billiard(st, rng, cm):  # test_ant_small_billiard_free_joint_ball: half of the ants sent into the ball, a few balls on the goal
    n = len(st["t"])
    st["qpos"][: n // 2, 1] = -0.9 + rng.uniform(-0.1, 0.1, n // 2)
    st["qvel"][: n // 2, 1] = -2.0
    goal = np.array(cm.task.goals[0].pos[:2])
    st["qpos"][-4:, 15:17] = goal + rng.uniform(-0.3, 0.3, (4, 2))


# per configuration: make keywords, reset seed, action / placement seed, placement, checkpoints, the cap of the maze's pinned test,
# the reward's absolute tolerance in that test
CASES = {
    1: dict(kw={}, seed=5, rng=0, place=_place_push, ks=(2, 11), frac=0.005, rew_atol=1e-6),
    2: dict(kw=dict(maze_size_scaling=2.0), seed=5, rng=0, place=_place_blocks, ks=(0, 5, 20), frac=0.006, rew_atol=1e-6),
    3: dict(kw=dict(maze_size_scaling=2.0), seed=5, rng=0, place=_place_blocks, ks=(0, 5, 20), frac=0.006, rew_atol=1e-6),
    4: dict(kw={}, seed=1, rng=0, place=_place_nothing, ks=(0, 1, 3, 10, 40), frac=0.01, rew_atol=1e-6),
    5: dict(kw={}, seed=17, rng=3, place=_place_billiard, ks=(0, 2, 10, 40, 80), frac=0.01, rew_atol=1e-5),
}


def _touching(oracle, cm, qpos):
    """per env: does the oracle's contact set hold a pair of a robot geom and a movable body's geom"""
    m = cm.c
    movable = {m.block_geomid[k] for k in range(m.nblock)} | {m.ball_geomid[k] for k in range(m.nball)}
    mbody = {m.block_bodyid[k] for k in range(m.nblock)} | {m.ball_bodyid[k] for k in range(m.nball)}
    robot = {g for g in range(m.ngeom) if m.geom_bodyid[g] != 0 and m.geom_bodyid[g] not in mbody}
    out = np.zeros(len(qpos), bool)
    for e in range(len(qpos)):
        for c in oracle.contacts(cm, qpos[e]):
            g1, g2 = int(c[7]), int(c[8])
            out[e] |= (g1 in movable and g2 in robot) or (g2 in movable and g1 in robot)
    return out


def _block_limit_rows(cm, qpos):
    """per env: the active joint-limit rows of the movable blocks' slides (falling blocks: limited slides with a margin).  MuJoCo and
    the oracle count them among the constraint rows, not among the contacts; the kernels enumerate them with the block's contacts
    (kind 6 of geom_contacts, csrc/ant_dyn.h), so debug_forward's count holds them: the oracle's contact count plus this"""
    m, rows = cm.c, np.zeros(len(qpos), int)
    for k in range(m.nblock):
        b = m.block_bodyid[k]
        for j in range(m.body_jntadr[b], m.body_jntadr[b] + m.body_jntnum[b]):
            if m.jnt_limited[j]:
                q = qpos[:, m.jnt_qposadr[j]]
                rows += (q - m.jnt_range[j][0] < m.jnt_margin[j]).astype(int) + (m.jnt_range[j][1] - q < m.jnt_margin[j]).astype(int)
    return rows


def _oracle_count(oracle, cm, qpos, qvel, act, warm):
    """what debug_forward's count is compared with: the oracle's contacts, and the blocks' slide-limit rows at that state"""
    return oracle.forward(cm, qpos, qvel, act.astype(np.float64), warm)["counts"][:, 0].astype(int) + _block_limit_rows(cm, qpos)


def build_states(oracle, cm, nb, n=N):
    """CPU only: the checkpoints of configuration `nb` — per checkpoint the fp32 start state, the action, the oracle's step from it
    and the oracle's contact counts.  The preconditions are asserted here, from the oracle alone: the batch holds an env with an
    ant-block / ant-ball contact, and one whose count is beyond the movable bodies' resting contacts (four corners of a block, one
    point of a ball) by 4 or more."""
    case = CASES[nb]
    st, _ = oracle.reset(cm, n, case["seed"])
    rng = np.random.default_rng(case["rng"])
    case["place"](st, rng, cm)
    out = []
    for k in range(max(case["ks"]) + 1):
        act = rng.uniform(-30, 30, (n, 8)).astype(np.float32)
        if k in case["ks"]:
            start = _f32(st)
            after = {key: v.copy() for key, v in start.items()}
            ref = oracle.step(cm, after, act.astype(np.float64), nthreads=8)
            nc = oracle.forward(cm, start["qpos"], start["qvel"], act.astype(np.float64), start["warm"])["counts"][:, 0].astype(int)
            out.append(dict(k=k, start=start, act=act, after=after, ref=ref, nc=nc, touching=_touching(oracle, cm, start["qpos"]),
                            nc_dev=_oracle_count(oracle, cm, start["qpos"], start["qvel"], act, start["warm"])))
        oracle.step(cm, st, act.astype(np.float64), nthreads=8)
    rest = 4 * cm.c.nblock + cm.c.nball
    assert any(c["touching"].any() for c in out), "no env of the batch has an ant-block / ant-ball contact"
    assert max(int(c["nc"].max()) for c in out) >= rest + 4, [np.bincount(c["nc"]).tolist() for c in out]
    assert all(np.isfinite(c["ref"]["obs"]).all() for c in out)
    return out


_states, _control = {}, {}


def _states_of(oracle, cm, nb):
    if nb not in _states:
        _states[nb] = build_states(oracle, cm, nb)
    return _states[nb]


def _count_is_a_tie(oracle, cm, c, e):
    """the one excuse of test_ant_corner_contacts_overflow_the_staging: the float64 oracle's own count for env e changes under a
    perturbation of the state at 1e-6"""
    prng = np.random.default_rng(77)
    st, seen = c["start"], set()
    for _ in range(24):
        q = st["qpos"][e:e + 1] + prng.uniform(-1e-6, 1e-6, (1, st["qpos"].shape[1])) * np.maximum(1.0, np.abs(st["qpos"][e:e + 1]))
        seen.add(int(_oracle_count(oracle, cm, q, st["qvel"][e:e + 1], c["act"][e:e + 1], st["warm"][e:e + 1])[0]))
    return len(seen) > 1


def _run(torch, oracle, env, nb, label):
    """every checkpoint of configuration nb on `env`: the assertions of the module docstring; returns per checkpoint the observation,
    the mask of the envs inside the plain tolerance and the error figures"""
    case, cm, rows = CASES[nb], env.model, []
    for c in _states_of(oracle, cm, nb):
        s, act, after, ref = c["start"], c["act"], c["after"], c["ref"]
        env.set_state(s["qpos"], s["qvel"], s["warm"], s["t"])
        env.status()  # (cleared on read: what follows is this checkpoint's)
        _, counts = env.debug_forward(act)
        dc = counts.cpu().numpy()[:, 0].astype(int)
        for e in np.flatnonzero(dc != c["nc_dev"]):
            assert _count_is_a_tie(oracle, cm, c, e), f"{label} k={c['k']} env {e}: device {dc[e]} contacts, oracle {c['nc_dev'][e]}, and the oracle's count is stable"
        obs, rew, done, info = env.step(torch.as_tensor(act, device=env.device))
        obs, rew, done, goal = obs.cpu().numpy().copy(), rew.cpu().numpy().copy(), done.cpu().numpy().copy(), info["goal_index"].cpu().numpy().copy()
        qpos, qvel, _, t = [x.cpu().numpy() for x in env.get_state()]
        status = env.status().cpu().numpy()
        err = np.maximum(np.abs(qpos - after["qpos"]).max(1), (np.abs(qvel - after["qvel"]) / (1.0 + np.abs(after["qvel"]))).max(1))
        plain = np.all(_close(qpos, after["qpos"], rtol=0.0), axis=1) & np.all(_close(qvel, after["qvel"]), axis=1)
        print(f"LADDER {label} NB={nb} k={c['k']}: {int((~plain).sum())} of {N} envs outside the plain tolerance (cap {max(1, int(case['frac'] * N))}), "
              f"worst in-tolerance error {err[plain].max():.3e}, median {np.median(err):.3e}, worst of all {err.max():.3e}; "
              f"oracle counts {int(c['nc'].min())}..{int(c['nc'].max())}, {int(c['touching'].sum())} envs touch a movable body, device counts differ in {int((dc != c['nc_dev']).sum())}")
        ok = _assert_step_parity(oracle, cm, s, act, qpos, qvel, after, max_outlier_frac=case["frac"], dev_out=(obs, rew, done), ref_done=ref["done"])
        assert np.array_equal(ok, plain)
        assert np.array_equal(done, ref["done"]) and np.array_equal(goal, ref["goal_idx"]), (label, c["k"])
        assert np.all(_close(obs[ok], ref["obs"][ok])), (label, c["k"])
        assert np.all(_close(rew[ok], ref["reward"][ok], atol=case["rew_atol"])), (label, c["k"])
        assert np.array_equal(t, after["t"])
        assert np.all((status & 7) == 0), (label, c["k"], status[status != 0])
        rows.append(dict(k=c["k"], obs=obs, ok=ok))
    return rows


def _control_rows(torch, oracle, nb):
    """the same states on the configuration's default rung, under the same cap — run once per configuration"""
    if nb not in _control:
        name = f"ant-{nb}-{MAZE[nb][1]}"
        env = _make(name, **CASES[nb]["kw"])
        try:
            _control[nb] = _run(torch, oracle, env, nb, f"control {name}")
        finally:
            env.close()
    return _control[nb]


# ---------------------------------------------------------------------------------------------- 2. the nine rungs against the oracle
@pytest.mark.parametrize("name", NEW)
def test_new_rung_steps_like_the_oracle(torch, oracle, name):
    """One step from every checkpoint on a rung that no other test runs: `_assert_step_parity` with the device's outputs, flags and
    goal indices equal to the oracle's, observation and reward of the in-tolerance envs at the suite's bars, no status bit, and the
    contact counts of debug_forward equal to oracle.forward's (an env whose oracle count itself changes under a 1e-6 perturbation
    is the one excuse; the kernels count an active limit row of a falling block's slide as a contact of the block, the oracle as a
    constraint row: `_block_limit_rows` adds those to the oracle's side — one per env of AntMultiFall-v0, whose block rests at the
    upper end of its z slide).  The control comes first; the difference between the rung's observation and the control's is printed, not
    bounded (profiles/ant_ladder/parity.md holds the figures)."""
    nb = RUNGS[name][1][0]
    env = _make(name, **CASES[nb]["kw"])
    try:
        control = _control_rows(torch, oracle, nb)
        rows = _run(torch, oracle, env, nb, name)
        for a, b in zip(rows, control):
            both = a["ok"] & b["ok"]
            print(f"LADDER {name} NB={nb} k={a['k']}: max |obs - control's obs| over {int(both.sum())} envs inside the tolerance on both = "
                  f"{np.abs(a['obs'][both].astype(np.float64) - b['obs'][both]).max():.3e}")
    finally:
        env.close()
