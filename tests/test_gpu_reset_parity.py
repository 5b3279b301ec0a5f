"""In-step auto-reset and masked reset of every engine against the oracle's reset.  Run with `pytest -m gpu` on an MI355X.

A step kernel that ends an env's episode resets it inside the launch: the new state is drawn from episode_seed(seed, episode)
(csrc/mz_rng.h) and the env's global slot, `obs` gets the new episode's first observation, `final_obs` the terminal one, t and the warm
start go to zero.  That code exists once per step kernel; here every copy is held to `reset_ref.expected_reset`, the oracle's
mzo_env_reset under the same seed (ant.py:84-96, point.py:71-81, swimmer.py:56-69).

Schedule of every case (`_episode_run`): auto_reset, max_episode_steps = 4, global slot offset 1000, reset(seed=S); t[e] = e % 4 is
injected, so a quarter of the envs truncate on each step and neighbours in a wavefront sit in different episodes; nine steps with seeded
actions from the control range; in the plain mazes envs 0..7 are put on goal 0 before the second step (termination instead of
truncation, and an episode count that differs from the neighbours'); after the fifth step a masked reset with another seed.

Tolerances:
  * a reset state and its observation against the float64 oracle: 2e-6, the bound test_reset_distribution_and_oracle_rng has for fp32
    draws (a draw is q0 + (-0.1 + 0.2 u) in fp32: a few ulp of 0.1 .. 1, well below 2e-6; the Ant's Gaussian velocities go through
    logf / cosf and stay within 1e-7);
  * the terminal step of a finished env (final_observation, reward) and the step of every other env against the oracle's step from the
    fp32 state `get_state` returned before it: the tolerances of the family's single-step test in tests/test_gpu_parity.py /
    tests/test_gpu_general_engine.py, through the same `_assert_step_parity` with the same arguments (CASES below);
  * flags, goal indices, t, warm start, noise-free coordinates, the record, rows the call must leave alone: exact / bit for bit.

Swimmer / Reacher with a movable block: the reference's reset puts velocity noise on the block and the medium's explicit drag on a 0.2 g
box diverges within one step, in MuJoCo, in the oracle (every entry NaN) and on the device (status bit 1;
test_swimmer_world_with_a_movable_block, test_every_registered_id_runs_or_refuses).  An env whose oracle step is not finite is
therefore required to carry status
bit 1 on the device and its step's numbers are not compared; its flags, its reset state and everything exact are checked like any other
env's.  That is every step of SwimmerPush-v0 / ReacherPush-v1 here: those two cases pin the resets (noise on the block's slides
included), not the steps between them."""
import numpy as np
import pytest

import mujoco_maze_amd as mm
from tests import user_robots
from tests.reset_ref import expected_reset
from tests.test_gpu_parity import _assert_step_parity, _close

pytestmark = pytest.mark.gpu

S, S2, ENV0, NSTEPS, HORIZON = 90210, 4711, 1000, 9, 4
GOAL_STEP, MASK_AFTER = 2, 5  # 1-based: envs 0..7 go onto goal 0 before step 2; the masked reset follows step 5
RESET_ATOL = 2e-6

# per family: atol / max_outlier_frac of _assert_step_parity and the observation and reward tolerances (atol, rtol) of the family's
# existing single-step test; reward None = equal as fp32 (test_point_step_parity_and_bounce)
ANT = dict(atol=1e-5, obs=(1e-5, 1e-5), rew=(1e-6, 1e-5))
POINT_BARE = dict(atol=2e-6, frac=0.004, obs=(1e-6, 2e-7), rew=None)
POINT = dict(atol=2e-6, frac=0.004, obs=(2e-6, 1e-5), rew=(1e-6, 1e-5))
CHAIN = dict(atol=1e-6, frac=0.0, obs=(1e-6, 2e-7), rew=(1e-7, 1e-5))
GENERAL = dict(atol=1e-6, frac=0.006, obs=(1e-6, 1e-5), rew=(1e-6, 1e-5))
PLAIN = ("AntUMaze-v0", "PointUMaze-v0", "SwimmerUMaze-v0")

CASES = {}


def _case(name, family, tol, env_id=None, n=70, options=(), plain=None, **make_kw):
    CASES[name] = dict(family=family, tol=tol, env_id=env_id or name, n=n, options=dict(options), make_kw=make_kw,
                       plain=(env_id or name) in PLAIN if plain is None else plain)


for lanes in (8, 16, 32, 64):
    _case(f"AntUMaze-v0/lanes{lanes}", "ant", dict(ANT, frac=0.002), "AntUMaze-v0", options={"lanes_per_env": lanes})
_case("AntUMaze-v0/lanes16-wps2", "ant", dict(ANT, frac=0.002), "AntUMaze-v0", options={"lanes_per_env": 16, "waves_per_simd": 2})
for lanes in (16, 32):
    _case(f"AntPush-v0/lanes{lanes}", "ant", dict(ANT, frac=0.005), "AntPush-v0", options={"lanes_per_env": lanes})
_case("AntMultiPush-v0", "ant", dict(ANT, frac=0.006), n=38)
_case("AntSmallBilliard-v0", "ant", dict(ANT, frac=0.01, rew=(1e-5, 1e-5)), n=38)
_case("AntFall-v0", "ant", dict(ANT, frac=0.01), n=38)
# the in-step reset of step instantiations that no default reaches (every step kernel carries its own copy: DESIGN.md section 3.8; the
# table of rungs is DESIGN.md section 3.1): n and the family tolerances of the default-width cases above
_case("AntPush-v0/lanes64", "ant", dict(ANT, frac=0.005), "AntPush-v0", n=38, options={"lanes_per_env": 64})
for lanes in (16, 32):
    _case(f"AntMultiPush-v0/lanes{lanes}", "ant", dict(ANT, frac=0.006), "AntMultiPush-v0", n=38, options={"lanes_per_env": lanes})
_case("AntSmallBilliard-v0/lanes16", "ant", dict(ANT, frac=0.01, rew=(1e-5, 1e-5)), "AntSmallBilliard-v0", n=38, options={"lanes_per_env": 16})
_case("AntMultiFall-v0", "ant", dict(ANT, frac=0.01), n=38)  # the block on three slides (x, y, z): the 64-lane default
_case("AntMultiFall-v0/lanes16", "ant", dict(ANT, frac=0.01), "AntMultiFall-v0", n=38, options={"lanes_per_env": 16})
_case("PointUMaze-v0", "point", POINT_BARE)
_case("PointUMaze-v0/lanes32", "point", POINT_BARE, "PointUMaze-v0", options={"lanes_per_env": 32})
for _id in ("PointPush-v0", "PointPushMaze-v0", "PointBilliard-v0", "PointFall-v0"):
    _case(_id, "point", POINT)
for _id in ("SwimmerUMaze-v0", "SwimmerPush-v0", "ReacherUMaze-v0", "ReacherPush-v1"):
    _case(_id, "chain", CHAIN)
_case("PointUMaze-v0/general", "general", GENERAL, "PointUMaze-v0", n=10, engine="general")
_case("AntUMaze-v0/general", "general", GENERAL, "AntUMaze-v0", n=10, engine="general")
_case("YSwimmer/general", "general", dict(GENERAL, frac=0.0), "YSwimmer", n=10, plain=False)
# beyond the issue's table: a general-engine maze whose block moves (it is expelled from its platform in the first steps), so that the
# masked reset's rows for the envs it leaves alone are compared where a slide is not zero (frac: movable bodies, test_gpu_general_engine)
_case("PointFall-v0/general", "general", dict(GENERAL, frac=0.02), "PointFall-v0", n=10, engine="general")


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def _make(case):
    kw = dict(num_envs=case["n"], auto_reset=True, max_episode_steps=HORIZON, **case["make_kw"])
    if case["env_id"] == "YSwimmer":  # tests/user_robots.py: a branching swimmer, RESET_QVEL = "uniform_sym", on the general engine
        from mujoco_maze_amd import maze_task as T
        from mujoco_maze_amd.maze_env import VecMazeEnv

        cls = user_robots.robot_classes()[1]
        assert cls.RESET_QVEL == "uniform_sym"
        env = VecMazeEnv(cls, T.DistRewardUMaze, maze_size_scaling=4.0, **kw)
    else:
        env = mm.make(case["env_id"], force_vec=True, **kw)
    for key, v in case["options"].items():
        env.set_option(key, v)
    env.set_option("env_index_offset", ENV0)
    info = env.launch_info()
    for key, v in case["options"].items():
        assert info[key] == v, (key, info)
    assert info["engine"] == (1 if case["family"] == "general" else 0)
    return env


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int32) if x.dtype == np.float32 else x


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _np_state(env):
    qpos, qvel, warm, t = [x.cpu().numpy() for x in env.get_state()]
    return dict(qpos=qpos, qvel=qvel, warm=warm, t=t)


def _f64(st):
    return {k: (v.astype(np.float64) if k != "t" else v.copy()) for k, v in st.items()}


def _actions(env):
    """[NSTEPS, n, nu] float32, uniform in the control range, the same for every run of a case"""
    rng = np.random.default_rng(7)
    return rng.uniform(env.action_space.low, env.action_space.high, (NSTEPS, env.num_envs, env.nu)).astype(np.float32)


def _put_on_goal(env):
    """envs 0..7: qpos xy within 0.3 x threshold of goal 0 (test_full_size_properties does the same with a wider spread)"""
    goal = env._task.goals[0]
    rng = np.random.default_rng(3)
    r, phi = 0.3 * goal.threshold * np.sqrt(rng.uniform(0, 1, 8)), rng.uniform(0, 2 * np.pi, 8)
    qpos = env.get_state()[0]
    xy = np.asarray(goal.pos[:2])[None, :] + np.stack([r * np.cos(phi), r * np.sin(phi)], 1)
    qpos[:8, :2] = env._torch.as_tensor(xy, dtype=qpos.dtype, device=qpos.device)
    env.set_state(qpos=qpos)


def _check_reset_rows(case, cm, rows, st, obs, exp_st, exp_obs, stats):
    """State and observation of the envs `rows`, which have just been reset, against the oracle's rows for them."""
    m = cm.c
    nr, nvr = m.nq_robot, m.nv_robot
    dq = np.abs(st["qpos"][rows].astype(np.float64) - exp_st["qpos"][rows])
    dv = np.abs(st["qvel"][rows].astype(np.float64) - exp_st["qvel"][rows])
    do = np.abs(obs[rows].astype(np.float64) - exp_obs[rows])
    stats["reset_state"] = max(stats["reset_state"], dq.max(), dv.max())
    stats["reset_obs"] = max(stats["reset_obs"], do.max())
    assert dq.max() <= RESET_ATOL and dv.max() <= RESET_ATOL, f"reset state off the oracle's: qpos {dq.max():.2e}, qvel {dv.max():.2e}"
    assert np.all(st["warm"][rows] == 0.0), "a warm start survived the reset"
    assert np.all(st["t"][rows] == 0), "t not zeroed by the reset"
    # coordinates without noise (blocks of the Ant / the Point, a ball, whatever the general engine's model has beside the robot):
    # exactly the fp32 value of qpos0, at rest
    q0 = np.array(m.qpos0[:m.nq], np.float64).astype(np.float32)
    assert _same(st["qpos"][rows][:, nr:], np.tile(q0[nr:], (len(rows), 1))), "a noise-free coordinate is not at qpos0 after the reset"
    assert np.all(st["qvel"][rows][:, nvr:] == 0.0), "a noise-free coordinate moves after the reset"
    if m.njnt > 0 and m.jnt_type[0] == 0:  # free root (mz_model: MZ_JNT_FREE = 0): unit quaternion in the STATE
        a = m.jnt_qposadr[0] + 3
        qn = np.linalg.norm(st["qpos"][rows][:, a:a + 4].astype(np.float64), axis=1)
        assert np.all(np.abs(qn - 1.0) < 1e-6), f"root quaternion of the reset state not normalised: {np.abs(qn - 1.0).max():.2e}"
    assert do.max() <= RESET_ATOL, f"reset observation off the oracle's: {do.max():.2e}"
    assert np.all(obs[rows][:, -1] == 0.0), "time entry of a reset observation is not 0"


def _episode_run(torch, oracle, case, fused=False):
    """The schedule of the module docstring.  Stepping (fused False): every assertion of the module after every step; returns the
    final state, the [NSTEPS, n] done flags and the figures of the run.  fused: the same schedule through rollout() — steps 1 .. 5, the
    masked reset, steps 6 .. 9 — with nothing checked in between; returns the final state, the flags and the observation rows."""
    env = _make(case)
    try:
        n, cm, m, tol = env.num_envs, env.model, env.model.c, case["tol"]
        assert m.max_episode_steps == HORIZON
        rec = torch.full((n, env.obs_dim + 2), -7.0, device=env.device)
        env.bind_record(rec)
        obs0 = env.reset(seed=S).cpu().numpy()
        stats = dict(reset_state=0.0, reset_obs=0.0, branch=0, resets=0, diverged=0, terminated=0)
        exp_st, exp_obs = expected_reset(oracle, cm, n, S, np.zeros(n, np.int64), ENV0)
        _check_reset_rows(case, cm, np.arange(n), _np_state(env), obs0, exp_st, exp_obs, stats)
        env.set_state(t=(np.arange(n) % HORIZON).astype(np.int32))
        acts = _actions(env)
        mask = (np.arange(n) % 3 == 0).astype(np.uint8)
        if fused:
            assert not case["plain"] and env.launch_info()["rollout_fused"] == 1
            a = torch.as_tensor(acts, device=env.device)
            _, _, d1, i1 = env.rollout(a[:MASK_AFTER].contiguous(), return_obs=True)
            d1, o1 = d1.cpu().numpy().copy(), i1["observations"].cpu().numpy().copy()
            env.reset(mask=mask, seed=S2)
            _, _, d2, i2 = env.rollout(a[MASK_AFTER:].contiguous(), return_obs=True)
            return _np_state(env), np.concatenate([d1, d2.cpu().numpy()]), np.concatenate([o1, i2["observations"].cpu().numpy()])
        seed, k = S, np.zeros(n, np.int64)  # the handle's seed; done != 0 seen per env since its last mz_reset
        dones = np.zeros((NSTEPS, n), np.uint8)
        for step in range(1, NSTEPS + 1):
            if case["plain"] and step == GOAL_STEP:
                _put_on_goal(env)
            pre = _np_state(env)
            final_before = env._final_obs.cpu().numpy().copy()
            act = acts[step - 1]
            obs, rew, done, info = env.step(torch.as_tensor(act, device=env.device))
            obs, rew, done = obs.cpu().numpy().copy(), rew.cpu().numpy().copy(), done.cpu().numpy().copy()
            goal, final = info["goal_index"].cpu().numpy().copy(), info["final_observation"].cpu().numpy().copy()
            post, status = _np_state(env), env.status().cpu().numpy()
            start = _f64(pre)
            ref_state = _f64(pre)
            ref = oracle.step(cm, ref_state, act.astype(np.float64), nthreads=8)  # advances ref_state in place
            assert np.array_equal(done, ref["done"]), (step, done, ref["done"])
            dones[step - 1] = done
            rst = done != 0
            if case["plain"] and step == GOAL_STEP:
                # reached goals end these episodes, not only the time limit.  (The Point's action moves it by up to 1 m before the task looks:
                # some of the eight leave the goal again within the step — on the device exactly those that do in the oracle, see above.)
                hit = (done[:8] & 1) != 0
                assert (hit.sum() >= 4 if m.manual_collision else hit.all()) and np.any(done[:8] == 1), done[:8]
                stats["terminated"] += int((done & 1).sum())
            finite = np.isfinite(ref["obs"]).all(1) & np.isfinite(ref_state["qpos"]).all(1) & np.isfinite(ref_state["qvel"]).all(1)
            if case["env_id"] not in ("SwimmerPush-v0", "ReacherPush-v1"):
                assert finite.all(), "the oracle diverged in a maze where nothing should"
            assert np.all(status[~finite] & 1), "the oracle's step diverged and the device did not flag the env"
            stats["diverged"] += int((~finite).sum())
            # ---- envs whose episode the step ended
            k[rst] += 1
            stats["resets"] += int(rst.sum())
            rows = np.where(rst)[0]
            if len(rows):
                exp_st, exp_obs = expected_reset(oracle, cm, n, seed, k, ENV0)
                _check_reset_rows(case, cm, rows, post, obs, exp_st, exp_obs, stats)
                cmp = rows[finite[rows]]
                assert np.all(_close(final[cmp], ref["obs"][cmp], *tol["obs"])), f"step {step}: terminal observation off the oracle's step"
                if tol["rew"] is None:
                    assert _same(rew[cmp], ref["reward"][cmp].astype(np.float32))
                else:
                    assert np.all(_close(rew[cmp], ref["reward"][cmp], *tol["rew"])), f"step {step}: terminal reward off the oracle's"
                assert np.array_equal(goal[rows], ref["goal_idx"][rows])
            # ---- envs that go on: the step's own observation, an untouched final_observation row, and the step itself against the
            # oracle (for an env reset by the step before, this is the step that would show a hidden state the reset left behind)
            live = np.where(~rst)[0]
            assert _same(final[live], final_before[live]), f"step {step}: final_observation row of a running env was written"
            assert np.array_equal(post["t"][live], pre["t"][live] + 1)
            cmp = live[finite[live]]
            if len(cmp):
                sub = lambda d: {key: v[cmp] for key, v in d.items()}
                ok = _assert_step_parity(oracle, cm, sub(start), act[cmp], post["qpos"][cmp], post["qvel"][cmp], sub(ref_state), atol=tol["atol"],
                                         max_outlier_frac=tol["frac"], dev_out=(obs[cmp], rew[cmp], done[cmp]), ref_done=ref["done"][cmp])
                stats["branch"] += int((~ok).sum())
                good = cmp[ok]
                assert np.all(_close(obs[good], ref["obs"][good], *tol["obs"])), f"step {step}: observation of a running env off the oracle's step"
                if tol["rew"] is None:
                    assert _same(rew[good], ref["reward"][good].astype(np.float32))
                else:
                    assert np.all(_close(rew[good], ref["reward"][good], *tol["rew"]))
                assert np.array_equal(goal[good], ref["goal_idx"][good])
            # ---- the bound record: [new-episode obs | terminal reward | done] for the envs that were reset, the step's own for the rest
            assert _same(rec.cpu().numpy(), np.concatenate([obs, rew[:, None], done.astype(np.float32)[:, None]], 1)), f"step {step}: record"
            if step == MASK_AFTER:
                # mz_reset stores its seed in the handle for ALL envs (include/mazestep.h): masked envs restart their episode count, the
                # others keep theirs and draw their next in-step reset from episode_seed(S2, k + 1)
                obs_m = env.reset(mask=mask, seed=S2).cpu().numpy().copy()
                after = _np_state(env)
                mk = np.where(mask != 0)[0]
                exp_st, exp_obs = oracle.reset(cm, n, S2, mask, env0=ENV0)
                _check_reset_rows(case, cm, mk, after, obs_m, exp_st, exp_obs, stats)
                rest = np.where(mask == 0)[0]
                for key in ("qpos", "qvel", "warm", "t"):
                    assert _same(after[key][rest], post[key][rest]), f"masked reset touched {key} of an env outside the mask"
                assert _same(obs_m[rest], obs[rest]), "masked reset: observation rows outside the mask differ from what step 5 returned"
                seed = S2
                k[mk] = 0
        assert stats["resets"] >= 2 * n and k.max() >= 1
        return _np_state(env), dones, stats
    finally:
        env.close()


_runs = {}  # stepping runs, shared between the case test and the fused test of the same id


def _stepping(torch, oracle, name):
    if name not in _runs:
        _runs[name] = _episode_run(torch, oracle, CASES[name])
    return _runs[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_in_step_and_masked_reset_against_oracle(torch, oracle, name):
    state, dones, stats = _stepping(torch, oracle, name)
    print(f"{name}: reset state max |dev - oracle| {stats['reset_state']:.2e}, reset obs {stats['reset_obs']:.2e} (bound {RESET_ATOL:.0e}); "
          f"{stats['resets']} in-step resets, {stats['terminated']} goal terminations, {stats['branch']} envs on the discontinuity route, "
          f"{stats['diverged']} diverged env-steps")
    # every quarter of the batch truncates once in four steps, whatever else ends an episode
    assert np.all((dones != 0).sum(0) >= 2)


@pytest.mark.parametrize("name", ["PointPush-v0", "SwimmerPush-v0"])
def test_fused_rollout_resets_like_the_step_kernel(torch, oracle, name):
    """rollout() on the fused kernels under the same schedule ends in the stepping run's state, bit for bit, and the rows of obs_seq at
    reset steps are first observations (time entry 0); the rest of the fused kernels' outputs is pinned to the step kernel's by
    tests/test_gpu_rollout.py and the policy-rollout twins."""
    state, dones, _ = _stepping(torch, oracle, name)
    fstate, fdones, fobs = _episode_run(torch, oracle, CASES[name], fused=True)
    assert np.array_equal(fdones, dones)
    for key in ("qpos", "qvel", "warm", "t"):
        assert _same(fstate[key], state[key]), key
    rst = fdones != 0
    assert rst.sum() >= 2 * CASES[name]["n"]
    assert np.all(fobs[rst][:, -1] == 0.0) and np.all(fobs[~rst][:, -1] > 0.0)
