"""GPU parity tests: the HIP path (through the C-ABI) against the CPU oracle on the same
seeded inputs.  Run with `pytest -m gpu` on an MI355X.

Tolerances (north_star: "within 1e-5 fp32 per DoF, bit-exact for termination flags and
goal indices"): |dev - oracle| <= 1e-5 + 1e-5 * |oracle| on qpos / qvel / obs after ONE
MazeEnv.step (= 20 forward-dynamics evaluations for the Ant) from an identical fp32
state; flags exact.  Trajectories are chaotic, so parity is asserted per step from
injected states (SURVEY §8d "Parity inputs")."""
import os

import numpy as np
import pytest

import mujoco_maze_amd as mm

pytestmark = pytest.mark.gpu
ATOL, RTOL = 1e-5, 1e-5
# Positions are asserted in ABSOLUTE terms since round 6 (1e-5 + 1e-5 |x| admitted 2.1e-4 for an ant 20 m from the
# origin): |dev - oracle| <= 1e-5 on every qpos entry, no relative part.  Measured need (profiles/r06/parity_long.md, 254 k env-steps
# per config, ants up to 19.4 m out): 99.9 % quantile 9.6e-7, largest error outside branch flips 9.7e-7 — one fp32 ulp of a coordinate
# near 16 m is 1.9e-6; the kernels carry hi + lo position pairs inside the step.  Velocities keep the mixed
# bound (hinge rates of tens of rad/s: an fp32 ulp there is 2e-6).
POS_RTOL = 0.0


def _close(a, b, atol=ATOL, rtol=RTOL):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b) <= atol + rtol * np.abs(b)


def _f32(st):
    out = {k: v.copy() for k, v in st.items()}
    for k in ("qpos", "qvel", "warm"):
        out[k] = out[k].astype(np.float32).astype(np.float64)
    return out


# device vs the oracle's one-sided limit at a discontinuity of the step map (see _assert_step_parity): the same 1e-5 as everywhere
# else.  (Round 4 needed 5e-5 here; it was not the discontinuities — MZ_PARITY_LOG showed "branch" envs 1.4e-5 .. 3.7e-5 off on BOTH
# sides: stiff-maze envs whose accepted Newton unit step carried the fp32 elimination's error.  With the refinement step of round 5
# every env that takes this route is a real branch flip, 1e-2 .. 1e-1 off the other branch and <= 1.3e-6 off its own.)
BRANCH_ATOL = 1e-5


def _tie_mixture(dev, a, seen, branch_atol):
    """An EXACT tie, re-decided at every RK4 stage: a Point teleported onto the diagonal of a block sees two faces at the same depth,
    and so it does at each of the four stages of the step (the configuration stays symmetric) — which face wins a stage is decided
    by the last bit of two equal numbers.  The oracle, perturbed at 1e-6, lands on one side for ALL stages (outcome A or B); the
    device, like the unperturbed oracle, may pick per stage, and its step is then the RK4-weighted blend of the two: a point ON
    THE SEGMENT between A and B.  That is what is demanded here: some perturbed outcome B (clearly distinct from A) with dev within
    branch_atol + 2 % |B - A| of A + lambda (B - A), 0 <= lambda <= 1."""
    for b in seen:
        ab = b - a
        nab = np.abs(ab).max()
        if nab < 100 * branch_atol:
            continue
        lam = float(np.dot(dev - a, ab) / np.dot(ab, ab))
        if -0.02 <= lam <= 1.02 and np.abs(dev - (a + lam * ab)).max() <= branch_atol + 0.02 * nab:
            return True
    return False


def _log_branch(kind, cm, err, one_sided):
    """MZ_PARITY_LOG=<file>: one line per env that took the discontinuity route (tools: what BRANCH_ATOL really needs)."""
    path = os.environ.get("MZ_PARITY_LOG")
    if path:
        with open(path, "a") as f:
            f.write(f"{kind} robot {cm.c.robot} nblock {cm.c.nblock} elevated {cm.c.elevated} err {err:.3e} one_sided {one_sided:.3e} test {os.environ.get('PYTEST_CURRENT_TEST', '')}\n")


def _assert_step_parity(oracle, cm, start, act, dev_qpos, dev_qvel, ref_state, atol=ATOL, max_outlier_frac=0.002, dev_out=None,
                        branch_atol=BRANCH_ATOL, ref_done=None):
    """Per-DoF parity after one env.step: EVERY env is inside |dev - oracle| <= atol + 1e-5 |oracle| on qpos and qvel, or
    sits on a discontinuity of the step map AND agrees with the float64 oracle's value on the device's side of it.

    MuJoCo's soft constraints switch on at `dist < margin` / `q < limit` with a velocity-dependent (damping) term, and the
    box rules pick faces by comparisons, so the step map has jumps: an env whose contact crosses such a threshold within
    fp32 round-off legitimately lands on the other branch.  For every env outside the tolerance (round 4: no env is
    masked out any more):
      1. the oracle is re-run from the same state perturbed at the scale of the device's round-off — 2e-7 (one fp32 ulp of the
         state), 1e-6 (what absolute coordinates of ~10 m carry in fp32), 5e-6 (the error the device's intermediate states carry
         INSIDE the step: a forward evaluation is good to 2e-4 in qacc, i.e. 4e-6 in the velocity of the next RK4 stage).  Some
         perturbed run must land nearer to the device's answer than to the unperturbed oracle's: the oracle itself is
         discontinuous there, and that run is on the device's branch;
      2. bisection between the unperturbed start (oracle's branch) and that perturbed start (device's branch) walks up to the
         discontinuity: the last state on the device's side differs from the given start by < 1e-8 — nothing at the resolution of
         an fp32 state — and the oracle's step from THERE is what the device is compared with: qpos / qvel (and, with
         `dev_out` = (obs, reward, done) of the device, observation, reward and flags) within `branch_atol`.  Several
         discontinuities within round-off of each other (a block on four corners) are crossed one at a time, up to five;
      3. the one case without a branch of the oracle to compare with is an exact tie that every RK4 stage decides anew
         (_tie_mixture): the device must then lie on the segment between two outcomes of the oracle.
    `max_outlier_frac` caps how many envs may take that route (<= 2x what was measured: profiles/r02/parity.md).
    There is no looser bound without the proof (the `hard_atol` of rounds 2-4 is gone).  Returns the mask of the envs inside the
    plain tolerance."""
    ok = np.all(_close(dev_qpos, ref_state["qpos"], atol=atol, rtol=POS_RTOL), axis=1) & np.all(_close(dev_qvel, ref_state["qvel"], atol=atol), axis=1)
    bad = np.where(~ok)[0]
    n_mixed = 0
    assert len(bad) <= max(1, int(max_outlier_frac * len(ok))), (len(bad), len(ok), np.abs(dev_qvel - ref_state["qvel"]).max())
    rng = np.random.default_rng(123)

    def run(p, e):
        out = oracle.step(cm, p, act[e:e + 1].astype(np.float64))
        return p, out

    def dist_to(p, qpos, qvel):
        return max(np.abs(p["qpos"][0] - qpos).max(), np.abs(p["qvel"][0] - qvel).max())

    for e in bad:
        err = max(np.abs(dev_qvel[e] - ref_state["qvel"][e]).max(), np.abs(dev_qpos[e] - ref_state["qpos"][e]).max())
        base = {k: v[e:e + 1].copy() for k, v in start.items()}
        # walk from the given start towards the device's side, one discontinuity at a time (a block resting on four corners, a foot
        # in a wall corner: several activation thresholds within round-off of each other)
        cur, cur_res, cur_out, mixed = base, (ref_state["qpos"][e], ref_state["qvel"][e]), None, False
        for _round in range(5):
            d_cur = max(np.abs(cur_res[0] - dev_qpos[e]).max(), np.abs(cur_res[1] - dev_qvel[e]).max())
            if cur_out is not None and np.all(_close(dev_qpos[e], cur_res[0], atol=branch_atol, rtol=POS_RTOL)) and np.all(_close(dev_qvel[e], cur_res[1], atol=branch_atol)):
                break
            best, best_d, best_res = None, d_cur, None
            seen = []
            for scale in (2e-7, 1e-6, 5e-6):
                for _ in range(12):
                    p0 = {k: v.copy() for k, v in cur.items()}
                    p0["qpos"] = p0["qpos"] + rng.uniform(-scale, scale, p0["qpos"].shape) * np.maximum(1.0, np.abs(p0["qpos"]))
                    p0["qvel"] = p0["qvel"] + rng.uniform(-scale, scale, p0["qvel"].shape) * np.maximum(1.0, np.abs(p0["qvel"]))
                    p, _ = run({k: v.copy() for k, v in p0.items()}, e)
                    seen.append(np.concatenate([p["qpos"][0], p["qvel"][0]]))
                    d_dev = dist_to(p, dev_qpos[e], dev_qvel[e])
                    if d_dev < 0.5 * best_d or (best is None and d_dev < 0.9 * d_cur and d_dev < best_d):
                        best, best_d, best_res = p0, d_dev, (p["qpos"][0].copy(), p["qvel"][0].copy())
            if best is None and _tie_mixture(np.concatenate([dev_qpos[e], dev_qvel[e]]), np.concatenate(cur_res), seen, branch_atol):
                mixed = True
                break
            assert best is not None, f"env {e}: device differs from the oracle by {err:.2e} ({d_cur:.2e} after {_round} discontinuities) and no perturbation of the " \
                                     f"start state at round-off scale brings the oracle nearer: the oracle is smooth there"
            # bisection: lo = a start whose outcome is cur's, hi = one whose outcome is the nearer one; keep the nearer side
            lo, hi, hi_pack = cur, best, None
            for _ in range(14):
                mid = {k: (0.5 * (lo[k] + hi[k]) if k in ("qpos", "qvel", "warm") else hi[k].copy()) for k in hi}
                p, out = run({k: v.copy() for k, v in mid.items()}, e)
                if dist_to(p, best_res[0], best_res[1]) < dist_to(p, cur_res[0], cur_res[1]):
                    hi, hi_pack = mid, (p, out)
                else:
                    lo = mid
            if hi_pack is None:
                hi_pack = run({k: v.copy() for k, v in hi.items()}, e)
            cur, cur_out = hi, hi_pack[1]
            cur_res = (hi_pack[0]["qpos"][0].copy(), hi_pack[0]["qvel"][0].copy())
        moved = max(np.abs(cur["qpos"] - base["qpos"]).max(), np.abs(cur["qvel"] - base["qvel"]).max())
        assert moved < 2e-5, (e, moved)
        if mixed:
            # between two outcomes of the oracle (an exact tie re-decided at every RK4 stage): no single branch to compare with.
            # Rare by construction — counted, capped, and the flags must still be the oracle's
            n_mixed += 1
            assert n_mixed <= max(1, int(0.002 * len(ok))), f"{n_mixed} envs excused as tie mixtures"
            if dev_out is not None and ref_done is not None:
                assert int(dev_out[2][e]) == int(ref_done[e]), f"env {e}: done flag of a tie-mixture env differs from the oracle's"
            _log_branch("mixture", cm, err, 0.0)
            continue
        _log_branch("branch", cm, err, max(np.abs(cur_res[0] - dev_qpos[e]).max(), np.abs(cur_res[1] - dev_qvel[e]).max()))
        assert np.all(_close(dev_qpos[e], cur_res[0], atol=branch_atol, rtol=POS_RTOL)) and np.all(_close(dev_qvel[e], cur_res[1], atol=branch_atol)), \
            f"env {e}: {err:.2e} off the oracle; on the device's side of the discontinuities (start moved by {moved:.1e}) the oracle is still " \
            f"{max(np.abs(cur_res[0] - dev_qpos[e]).max(), np.abs(cur_res[1] - dev_qvel[e]).max()):.2e} away"
        if dev_out is not None:
            d_obs, d_rew, d_done = dev_out
            out = cur_out
            assert np.all(_close(d_obs[e], out["obs"][0], atol=branch_atol)), f"env {e}: observation off the oracle's on the device's branch"
            assert abs(float(d_rew[e]) - float(out["reward"][0])) <= branch_atol + 1e-4 * abs(float(out["reward"][0])), f"env {e}: reward off on the device's branch"
            assert int(d_done[e]) == int(out["done"][0]), f"env {e}: done flag differs from the oracle's on the device's branch"
    return ok


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def test_native_library_is_the_in_tree_one(torch):
    from mujoco_maze_amd import _capi

    lib = _capi.load()
    assert os.path.samefile(lib._name, os.path.join(os.path.dirname(mm.__file__), "csrc", "libmazestep.so"))
    from mujoco_maze_amd.model import MZ_ABI_VERSION

    assert lib.mz_abi_version() == MZ_ABI_VERSION == 8


@pytest.mark.parametrize("env_id", ["Ant4Rooms-v0", "AntPush-v0", "PointUMaze-v0", "SwimmerUMaze-v0", "PointSquareRoom-v0"])
def test_step_kernel_writes_the_packed_record(torch, env_id):
    """mz_bind_record: the packed [obs | reward | done] row of the sharded run's all-gather is written by the step itself (the
    Ant kernel's epilogue; one pack launch for the other robots) — equal, bit for bit, to the three outputs, also for envs
    that auto-reset inside the step (then `obs` is the new episode's first observation) and after unbinding nothing is written."""
    n = 200  # not a multiple of the envs per wavefront
    env = mm.make(env_id, num_envs=n, auto_reset=True, force_vec=True)
    rec = torch.full((n, env.obs_dim + 2), -7.0, device=env.device)
    env.bind_record(rec)
    env.reset(seed=2)
    t = env.get_state()[3]
    t[::3] = 998  # a third of the envs truncate (and auto-reset) on the second step
    env.set_state(t=t)
    g = torch.Generator(device=env.device).manual_seed(0)
    lo, hi = torch.as_tensor(env.action_space.low, device=env.device), torch.as_tensor(env.action_space.high, device=env.device)
    resets = 0
    for k in range(4):
        obs, rew, done, info = env.step(lo + (hi - lo) * torch.rand((n, env.nu), device=env.device, generator=g))
        assert torch.equal(rec, torch.cat([obs, rew[:, None], done.float()[:, None]], dim=1)), k
        resets += int((done != 0).sum())
    assert resets >= n // 3
    with pytest.raises(ValueError):
        env.bind_record(torch.zeros((n, env.obs_dim + 1), device=env.device))
    env.bind_record(None)
    rec.fill_(-7.0)
    env.step(torch.zeros((n, env.nu), device=env.device))
    assert torch.all(rec == -7.0)
    env.close()


def _rollout_states(oracle, cm, n, seed, checkpoints, robot="ant"):
    rng = np.random.default_rng(seed)
    st, _ = oracle.reset(cm, n, seed)
    snaps = {}
    for k in range(max(checkpoints) + 1):
        if k in checkpoints:
            snaps[k] = _f32(st)
        act = rng.uniform(-30, 30, (n, 8)) if robot == "ant" else np.stack([rng.uniform(-1, 1, n), rng.uniform(-0.25, 0.25, n)], 1)
        oracle.step(cm, st, act, nthreads=8)
    return snaps


@pytest.mark.parametrize("env_id", ["AntUMaze-v0", "Ant4Rooms-v0"])
def test_ant_single_step_parity(torch, oracle, env_id):
    n = 1024
    env = mm.make(env_id, num_envs=n)
    cm = env.model
    snaps = _rollout_states(oracle, cm, n, 11, {0, 1, 10, 100})
    rng = np.random.default_rng(5)
    worst = 0.0
    for k, st in sorted(snaps.items()):
        act = rng.uniform(-30, 30, (n, 8)).astype(np.float32)
        start = {kk: v.copy() for kk, v in st.items()}
        env.set_state(st["qpos"], st["qvel"], st["warm"], st["t"])
        obs, rew, done, info = env.step(torch.as_tensor(act, device=env.device))
        qpos, qvel, warm, t = [x.cpu().numpy() for x in env.get_state()]
        ref = oracle.step(cm, st, act.astype(np.float64), nthreads=8)  # advances st in place
        ok = _assert_step_parity(oracle, cm, start, act, qpos, qvel, st, dev_out=(obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy()))
        assert np.all(_close(obs.cpu().numpy()[ok], ref["obs"][ok]))
        assert np.all(_close(rew.cpu().numpy()[ok], ref["reward"][ok], atol=1e-6))
        assert np.array_equal(done.cpu().numpy(), ref["done"])
        assert np.array_equal(info["goal_index"].cpu().numpy(), ref["goal_idx"])
        assert np.all(_close(info["position"].cpu().numpy()[ok], ref["info"][ok, :2]))
        assert np.all(_close(info["reward_forward"].cpu().numpy()[ok], ref["info"][ok, 2], atol=1e-4))
        assert np.array_equal(t, st["t"])
        worst = max(worst, np.abs(qvel - st["qvel"])[ok].max())
        bad = env.status().cpu().numpy()
        assert np.all((bad & 3) == 0)  # no NaN, no contact overflow
    print(f"{env_id}: worst |qvel - oracle| over checkpoints = {worst:.2e}")
    env.close()


def test_ant_forward_dynamics_and_contact_counts(torch, oracle):
    n = 256
    env = mm.make("AntUMaze-v0", num_envs=n)
    cm = env.model
    st = _rollout_states(oracle, cm, n, 3, {30})[30]
    act = np.random.default_rng(1).uniform(-30, 30, (n, 8)).astype(np.float32)
    env.set_state(st["qpos"], st["qvel"], st["warm"], st["t"])
    qacc, counts = env.debug_forward(act)
    ref = oracle.forward(cm, st["qpos"], st["qvel"], act.astype(np.float64), st["warm"])
    assert np.array_equal(counts.cpu().numpy()[:, 0], ref["counts"][:, 0])  # identical contact sets
    assert ref["counts"][:, 0].sum() > n  # the fixture really has contacts
    err = np.abs(qacc.cpu().numpy() - ref["qacc"])
    assert np.all(err <= 2e-4 + 1e-6 * np.abs(ref["qacc"])), err.max()  # measured 1.1e-4 at |qacc| up to 245 (h * 2e-4 = 4e-6 on qvel)
    env.close()


def test_ant_lane_group_widths_agree(torch, oracle):
    """Every lane-group width (8 / 16 / 32 / 64 lanes per env: different item-to-lane schedules and reduction trees) meets the
    same per-env bar against the oracle, and the widths agree with each other to round-off."""
    n = 128
    cmref, outs = None, {}
    for g in (8, 16, 32, 64):
        env = mm.make("AntUMaze-v0", num_envs=n)
        env.set_option("lanes_per_env", g)
        cm = env.model
        if cmref is None:
            cmref = _rollout_states(oracle, cm, n, 21, {20})[20]
            act = np.random.default_rng(2).uniform(-30, 30, (n, 8)).astype(np.float32)
            ref_state = {k: v.copy() for k, v in cmref.items()}
            oracle.step(cm, ref_state, act.astype(np.float64), nthreads=8)
        env.set_state(cmref["qpos"], cmref["qvel"], cmref["warm"], cmref["t"])
        obs, *_ = env.step(torch.as_tensor(act, device=env.device))
        qpos, qvel, _, _ = [x.cpu().numpy() for x in env.get_state()]
        _assert_step_parity(oracle, cm, cmref, act, qpos, qvel, ref_state, max_outlier_frac=0.0)
        outs[g] = obs.cpu().numpy().copy()
        env.close()
    for g in (8, 32, 64):
        assert np.all(_close(outs[g], outs[16], atol=4e-6)), g


@pytest.mark.parametrize("env_id,n", [("AntUMaze-v0", 256), ("AntPush-v0", 128), ("AntMultiPush-v0", 64)])
def test_ant_unit_steps_then_exact_search_changes_nothing(torch, env_id, n):
    """Option "ls_fast_iterations" (default 5: the first five Newton iterations of a solve take the unit step, the exact line search
    of MuJoCo's Newton solver — engine_solver.c mj_solNewton / PrimalSearch — only behind them): a converged solve does not depend on
    the way there.  The same states stepped with the search in every iteration (0) and with the default agree to fp32 round-off, and
    no env runs into the iteration cap; row solver (plain ant, one block) and lane-group solver (two blocks)."""
    envs = []
    for fast in (0, 5):
        env = mm.make(env_id, num_envs=n)
        env.set_option("ls_fast_iterations", fast)
        env.reset(seed=5)
        envs.append(env)
    g = torch.Generator(device=envs[0].device).manual_seed(3)
    acts = [(torch.rand((n, envs[0].nu), device=envs[0].device, generator=g) * 2 - 1) * 30 for _ in range(18)]
    for a in acts[:12]:
        envs[0].step(a)
    sizes = []
    for a in acts[12:]:  # single steps from IDENTICAL states (a rollout would compare two chaotic trajectories, not two solvers)
        st = [x.cpu().numpy() for x in envs[0].get_state()]
        envs[1].set_state(*st)
        envs[0].step(a); envs[1].step(a)
        for x, y in zip(envs[0].get_state()[:2], envs[1].get_state()[:2]):
            d = ((x - y).abs() / (1 + x.abs())).max(1).values
            # (an env on a discontinuity of the step map may land on either side under ANY change of round-off: at most a few)
            sizes.append(int((d > 1e-5).sum().item()))
    assert sum(sizes) <= max(2, int(0.004 * n * 6)), sizes
    assert int((envs[1].status() & 4).sum().item()) == 0  # MZ_STATUS_SOLVER_MAXITER
    for env in envs:
        env.close()


@pytest.mark.parametrize("env_id,n", [("PointUMaze-v0", 512), ("PointPush-v0", 256)])
def test_point_unit_steps_are_a_run_time_option_and_custom_tasks_search_every_iteration(torch, env_id, n):
    """the Point's unit-step count is a run-time option now ("ls_fast_iterations", as for the Ant), and a CUSTOM
    task — a maze nobody has soaked — runs without unit steps by default: MuJoCo's line search in every iteration, monotone on any
    maze (a guarded unit step was built and measured: it costs what the search costs, profiles/r06/unit_guard_ab.txt).  The optimum
    does not depend on the way there: the same states stepped with 0 and with 5 unit-step iterations agree to round-off."""
    envs = []
    for fast in (0, 5):
        env = mm.make(env_id, num_envs=n)
        assert env.custom_task is False and env.launch_info()["ls_fast_iterations"] == 5  # a registered maze: unit steps
        env.set_option("ls_fast_iterations", fast)
        assert env.launch_info()["ls_fast_iterations"] == fast
        env.reset(seed=5)
        envs.append(env)
    g = torch.Generator(device=envs[0].device).manual_seed(3)
    lo, hi = torch.as_tensor(envs[0].action_space.low, device=envs[0].device), torch.as_tensor(envs[0].action_space.high, device=envs[0].device)
    acts = [lo + (hi - lo) * torch.rand((n, envs[0].nu), device=envs[0].device, generator=g) for _ in range(30)]
    for a in acts[:24]:
        envs[0].step(a)
    sizes = []
    for a in acts[24:]:  # single steps from IDENTICAL states
        st = [x.cpu().numpy() for x in envs[0].get_state()]
        envs[1].set_state(*st)
        envs[0].step(a); envs[1].step(a)
        for x, y in zip(envs[0].get_state()[:2], envs[1].get_state()[:2]):
            d = ((x - y).abs() / (1 + x.abs())).max(1).values
            sizes.append(int((d > 1e-6).sum().item()))
    assert sum(sizes) <= max(2, int(0.004 * n * 6)), sizes
    for env in envs:
        assert int((env.status() & 4).sum().item()) == 0  # MZ_STATUS_SOLVER_MAXITER
        env.close()
    from mujoco_maze_amd import maze_task as T
    from mujoco_maze_amd.agent_model import AntEnv, PointEnv
    from mujoco_maze_amd.maze_env import VecMazeEnv

    class MyMaze(T.DistRewardUMaze):  # a user's task (README.md:91-126 of the reference): not one of the registered classes
        pass

    for cls, scale in ((AntEnv, 8.0), (PointEnv, 4.0)):
        env = VecMazeEnv(cls, MyMaze, num_envs=8, maze_size_scaling=scale)
        assert env.custom_task is True and env.launch_info()["ls_fast_iterations"] == 0
        env.close()


@pytest.mark.parametrize("env_id", ["AntPush-v0", "AntFall-v0"])
def test_one_block_ant_beyond_2048_envs_takes_16_lanes(torch, oracle, env_id):
    """A batch of the one-block ant with more waves at 32 lanes per env than the device has SIMDs runs at 16 lanes (ant_kernels.hip
    ant_lanes; four such waves fit a CU's LDS with the 32 contact slots of AntDims<1>): the default of a 2048 + 64-env handle against
    the oracle on rollout states, and the same states through an explicit 16- and 32-lane handle — the default must be bit for bit the
    16-lane one (the instantiation it selects), and that within round-off of the 32-lane one."""
    n = 2048 + 64
    outs = {}
    for lanes in (0, 16, 32):
        env = mm.make(env_id, num_envs=n, auto_reset=True)
        if lanes:
            env.set_option("lanes_per_env", lanes)
        cm = env.model
        st = _rollout_states(oracle, cm, n, 21, {20})[20]
        act = np.random.default_rng(9).uniform(-30, 30, (n, 8)).astype(np.float32)
        ref_state = {k: v.copy() for k, v in st.items()}
        oracle.step(cm, ref_state, act.astype(np.float64), nthreads=8)
        env.set_state(st["qpos"], st["qvel"], st["warm"], st["t"])
        obs, rew, done, info = env.step(torch.as_tensor(act, device=env.device))
        qpos, qvel, _, _ = [x.cpu().numpy() for x in env.get_state()]
        ok = _assert_step_parity(oracle, cm, st, act, qpos, qvel, ref_state, max_outlier_frac=0.006)
        outs[lanes] = (qpos.copy(), qvel.copy(), done.cpu().numpy().copy(), ok)
        g = torch.Generator(device=env.device).manual_seed(3)
        for _ in range(40):
            env.step(torch.rand((n, 8), device=env.device, generator=g) * 60 - 30)
        assert np.all((env.status().cpu().numpy() & 7) == 0)
        env.close()
    assert np.array_equal(outs[0][0], outs[16][0]) and np.array_equal(outs[0][1], outs[16][1])
    both = outs[16][3] & outs[32][3]
    assert np.all(_close(outs[16][1][both], outs[32][1][both], atol=1e-5)) and np.array_equal(outs[16][2][both], outs[32][2][both])


def test_ant_two_waves_per_simd_kernel(torch, oracle):
    """The plain ant's second instantiation (ant_kernels.hip: WPS = 2, held to 256 registers so that two waves share a SIMD, its Hessian
    fold on the matrix cores: v_mfma_f32_16x16x1_4b_f32; taken beyond 4096 envs, or by option "waves_per_simd") against the oracle and
    against the one-wave kernel — the same step to round-off (the MFMA accumulates in another order) — then a rollout with wall
    contacts and auto-resets without a flag; and a batch large enough to select it by itself."""
    n = 512
    outs = {}
    for wps in (1, 2):
        env = mm.make("AntUMaze-v0", num_envs=n, auto_reset=True)
        env.set_option("waves_per_simd", wps)
        cm = env.model
        st = _rollout_states(oracle, cm, n, 31, {30})[30]
        act = np.random.default_rng(7).uniform(-30, 30, (n, 8)).astype(np.float32)
        ref_state = {k: v.copy() for k, v in st.items()}
        oracle.step(cm, ref_state, act.astype(np.float64), nthreads=8)
        env.set_state(st["qpos"], st["qvel"], st["warm"], st["t"])
        obs, rew, done, info = env.step(torch.as_tensor(act, device=env.device))
        qpos, qvel, _, _ = [x.cpu().numpy() for x in env.get_state()]
        ok = _assert_step_parity(oracle, cm, st, act, qpos, qvel, ref_state, max_outlier_frac=0.004)
        outs[wps] = (obs.cpu().numpy().copy(), rew.cpu().numpy().copy(), done.cpu().numpy().copy(), ok)
        g = torch.Generator(device=env.device).manual_seed(3)
        for _ in range(60):
            env.step(torch.rand((n, 8), device=env.device, generator=g) * 60 - 30)
        assert np.all((env.status().cpu().numpy() & 7) == 0)
        env.close()
    both = outs[1][3] & outs[2][3]  # (envs on a discontinuity of the step map may land on either side)
    assert np.all(_close(outs[1][0][both], outs[2][0][both], atol=3e-6)) and np.array_equal(outs[1][2][both], outs[2][2][both])
    with pytest.raises(Exception):
        env = mm.make("AntUMaze-v0", num_envs=4)
        env.set_option("waves_per_simd", 3)
    n = 4096 + 64  # more waves than the device has SIMDs: the two-wave kernel by default
    env = mm.make("AntUMaze-v0", num_envs=n)
    cm = env.model
    st, _ = oracle.reset(cm, n, 4)
    s64 = _f32(st)
    act = np.random.default_rng(8).uniform(-30, 30, (n, 8)).astype(np.float32)
    env.set_state(s64["qpos"], s64["qvel"], s64["warm"], s64["t"])
    env.step(torch.as_tensor(act, device=env.device))
    qpos, qvel, _, _ = [x.cpu().numpy() for x in env.get_state()]
    start = _f32(st)
    oracle.step(cm, s64, act.astype(np.float64), nthreads=8)
    _assert_step_parity(oracle, cm, start, act, qpos, qvel, s64, max_outlier_frac=0.002)
    env.close()


def _place_ant(st, xy, yaw=0.0):
    st["qpos"][:, 0], st["qpos"][:, 1] = xy[0], xy[1]
    st["qpos"][:, 3] = np.cos(yaw / 2) * np.ones(len(st["qpos"]))
    st["qpos"][:, 4:6] = 0
    st["qpos"][:, 6] = np.sin(yaw / 2)
    return st


def test_ant_wall_contacts_and_goal(torch, oracle):
    """Capsule-box / sphere-box wall contacts (rare under random actions) and the goal flag."""
    n = 64
    env = mm.make("AntUMaze-v0", num_envs=n)
    cm = env.model
    st = _rollout_states(oracle, cm, n, 8, {40})[40]
    rng = np.random.default_rng(4)
    # push half of the ants against the wall east of the start cell (x = 4 is the wall face of the corridor end)
    st["qpos"][: n // 2, 0] = 18.9 + rng.uniform(0.0, 0.5, n // 2)   # east wall face at x = 20: leg tips touch / dig in <= 0.3
    st["qpos"][: n // 2, 1] = rng.uniform(-1, 1, n // 2)
    st["qvel"][: n // 2, 0] = 2.0
    st["qpos"][n // 2:, 0] = rng.uniform(-0.5, 0.5, n - n // 2)       # goal region (0, 16)
    st["qpos"][n // 2:, 1] = 16.0 + rng.uniform(-0.7, 0.7, n - n // 2)
    st = _f32(st)
    act = rng.uniform(-30, 30, (n, 8)).astype(np.float32)
    env.set_state(st["qpos"], st["qvel"], st["warm"], st["t"])
    _, counts = env.debug_forward(act)
    fref = oracle.forward(cm, st["qpos"], st["qvel"], act.astype(np.float64), st["warm"])
    assert np.array_equal(counts.cpu().numpy()[:, 0], fref["counts"][:, 0])
    start = {k: v.copy() for k, v in st.items()}
    obs, rew, done, info = env.step(torch.as_tensor(act, device=env.device))
    qpos, qvel, _, _ = [x.cpu().numpy() for x in env.get_state()]
    ref = oracle.step(cm, st, act.astype(np.float64), nthreads=8)
    # stiff, partly artificial wall penetrations: measured 1 env of 64 on an activation flip (oracle-sensitive), the rest inside 1e-5
    good = _assert_step_parity(oracle, cm, start, act, qpos, qvel, st, max_outlier_frac=2 / 64, dev_out=(obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy()))
    assert np.all(_close(obs.cpu().numpy()[good], ref["obs"][good]))
    assert np.array_equal(done.cpu().numpy(), ref["done"]) and ref["done"][n // 2:].sum() > 5
    assert np.array_equal(info["goal_index"].cpu().numpy(), ref["goal_idx"])
    assert np.all(_close(rew.cpu().numpy()[good], ref["reward"][good], atol=1e-6))
    env.close()


def test_ant_corner_contacts_overflow_the_staging(torch, oracle):
    """Single-pass contact enumeration (csrc/ant_dyn.h con_enum_item): a geom keeps its first three contacts in a staging
    entry; a geom that finds more (a foot in a wall corner: floor + two walls, two contacts each) sends the env through the
    two-pass fill.  Ants are dropped into the south-east corner of the UMaze's first corridor so that both paths occur:
    contact counts of the forward evaluation equal the oracle's env by env, and a step agrees with it."""
    n = 256
    env = mm.make("AntUMaze-v0", num_envs=n)
    cm = env.model
    st = _rollout_states(oracle, cm, n, 8, {40})[40]
    rng = np.random.default_rng(9)
    # the corridor east of the start ends at the wall faces x = 20 (east) and y = -4 (south): leg tips reach 1.1 from the torso
    st["qpos"][:, 0] = 19.0 + rng.uniform(0.0, 0.7, n)
    st["qpos"][:, 1] = -3.0 - rng.uniform(0.0, 0.7, n)
    st["qvel"][:, 0] = 1.0
    st["qvel"][:, 1] = -1.0
    st = _f32(st)
    act = rng.uniform(-30, 30, (n, 8)).astype(np.float32)
    env.set_state(st["qpos"], st["qvel"], st["warm"], st["t"])
    _, counts = env.debug_forward(act)
    fref = oracle.forward(cm, st["qpos"], st["qvel"], act.astype(np.float64), st["warm"])
    nc = fref["counts"][:, 0]
    dc = counts.cpu().numpy()[:, 0]
    # equal env by env (up to the cap of 16 contact slots: flagged, not fatal) — or the env sits on a tie at the activation distance
    # that the float64 oracle shows itself: its own count changes under a perturbation of the state at fp32 round-off scale
    diff = np.where(dc != np.minimum(nc, 16))[0]
    assert len(diff) <= 3, (diff, dc[diff], nc[diff])
    prng = np.random.default_rng(77)
    for e in diff:
        counts_seen = set()
        for _ in range(24):
            q = st["qpos"][e:e + 1] + prng.uniform(-1e-6, 1e-6, (1, 15)) * np.maximum(1.0, np.abs(st["qpos"][e:e + 1]))
            counts_seen.add(int(oracle.forward(cm, q, st["qvel"][e:e + 1], act[e:e + 1].astype(np.float64), st["warm"][e:e + 1])["counts"][0, 0]))
        assert len(counts_seen) > 1, f"env {e}: device {dc[e]} contacts, oracle {nc[e]}, and the oracle's count is stable under perturbation"
    assert nc.max() >= 8 and (nc >= 6).sum() >= 20 and nc.min() <= 4  # crowded corners and ordinary stances in one batch
    start = {k: v.copy() for k, v in st.items()}
    obs, rew, done, info = env.step(torch.as_tensor(act, device=env.device))
    qpos, qvel, _, _ = [x.cpu().numpy() for x in env.get_state()]
    ref = oracle.step(cm, st, act.astype(np.float64), nthreads=8)
    status = env.status().cpu().numpy()
    # An env with more simultaneous contacts than the kernel's 16 slots loses the surplus ones and SAYS so (MZ_STATUS_CONTACT_OVERFLOW,
    # per env): it is not a parity case — the oracle keeps all of them — and it is not silent.  Every env that starts beyond the
    # slots must carry the flag; parity is demanded of every env without it.
    flagged = (status & 2) != 0
    assert flagged[nc > 16].all() and flagged.sum() <= 12, (np.where(nc > 16)[0], np.where(flagged)[0])
    keep = np.where(~flagged)[0]
    sub = lambda d: {k: v[keep] for k, v in d.items()}
    # ants dropped INTO a wall corner (leg segments through the boxes): far more activation flips than any rollout state has — every
    # outlier must still be matched with the oracle's value on its side of the discontinuity
    good = _assert_step_parity(oracle, cm, sub(start), act[keep], qpos[keep], qvel[keep], sub(st), max_outlier_frac=0.08,
                               dev_out=(obs.cpu().numpy()[keep], rew.cpu().numpy()[keep], done.cpu().numpy()[keep]))
    assert np.all(_close(obs.cpu().numpy()[keep][good], ref["obs"][keep][good]))
    assert np.array_equal(done.cpu().numpy(), ref["done"])
    assert np.all((status & 1) == 0)
    env.close()


def test_ant_push_movable_block(torch, oracle):
    """BASELINE config 5: AntPush-v0, 2048 envs — movable-block contacts, obs (33,) with block xyz at [3:6]."""
    n = 2048
    env = mm.make("AntPush-v0", num_envs=n)
    cm = env.model
    assert env.obs_dim == 33 and env.nq == 17 and env.nv == 16
    st, _ = oracle.reset(cm, n, 5)
    rng = np.random.default_rng(0)
    st["qpos"][: n // 3, 1] = 3.0 + rng.uniform(0.2, 0.6, n // 3)
    st["qvel"][: n // 3, 1] = 1.5
    for k in range(12):
        act = rng.uniform(-30, 30, (n, 8)).astype(np.float32)
        if k in (2, 11):
            s64 = _f32(st)
            env.set_state(s64["qpos"], s64["qvel"], s64["warm"], s64["t"])
            obs, rew, done, info = env.step(torch.as_tensor(act, device=env.device))
            qpos, qvel, warm, t = [x.cpu().numpy() for x in env.get_state()]
            ref = oracle.step(cm, s64, act.astype(np.float64), nthreads=8)
            # Movable-block mazes switch every default geom to solimp .995 (maze_env.py:108-112): contact rows are ~50x stiffer
            # than in AntUMaze and the block weighs 0.2 g.  Round 4: the regulariser's (1 - d) is no longer formed in fp32 from
            # d = 0.995 (impedance_pair, ant_dyn.h) and the absolute positions are carried as hi + lo pairs inside the step
            # (AntScratchT::qlo): the 99.9 % quantile is 8e-6 (profiles/r04/parity.md) and the looser `hard_atol` bound of rounds
            # 2-3 is gone — every env inside 1e-5 (+1e-5 rel), or matched with the oracle on its side of a discontinuity.
            ok = _assert_step_parity(oracle, cm, _f32(st), act, qpos, qvel, s64, max_outlier_frac=0.005, dev_out=(obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy()))
            per_env = (np.abs(qvel - s64["qvel"]) / (1.0 + np.abs(s64["qvel"]))).max(1)
            assert np.median(per_env) < 2e-6
            assert np.all(_close(obs.cpu().numpy()[ok], ref["obs"][ok]))
            assert np.all(_close(rew.cpu().numpy()[ok], ref["reward"][ok], atol=1e-6))
            assert np.array_equal(done.cpu().numpy(), ref["done"])
            assert np.array_equal(obs.cpu().numpy()[:, 5], np.full(n, 2.0, np.float32))  # block z in the obs slot
            assert np.all((env.status().cpu().numpy() & 7) == 0)
            assert np.abs(s64["qpos"][:, 15:]).max() > 0.05  # blocks are being pushed
        oracle.step(cm, st, act.astype(np.float64), nthreads=8)
    env.close()


@pytest.mark.parametrize("env_id,nblock", [("AntMultiPush-v0", 2), ("AntPushMaze-v0", 3)])
def test_ant_multi_block_mazes(torch, oracle, env_id, nblock):
    """Two / three movable blocks at maze scale 2 (ant within reach of walls and blocks at spawn): block-block
    contacts, 10 / 12-dof hub, up to 72 contact slots."""
    n = 512
    env = mm.make(env_id, num_envs=n, maze_size_scaling=2.0)
    cm = env.model
    assert cm.c.nblock == nblock and env.obs_dim == 30 + 3 * nblock
    st, _ = oracle.reset(cm, n, 5)
    rng = np.random.default_rng(0)
    st["qvel"][:, 14:] = rng.uniform(-3, 3, (n, 2 * nblock))
    worst = []
    for k in range(21):
        act = rng.uniform(-30, 30, (n, 8)).astype(np.float32)
        if k in (0, 5, 20):
            s64 = _f32(st)
            env.set_state(s64["qpos"], s64["qvel"], s64["warm"], s64["t"])
            obs, rew, done, info = env.step(torch.as_tensor(act, device=env.device))
            qpos, qvel, warm, t = [x.cpu().numpy() for x in env.get_state()]
            ref = oracle.step(cm, s64, act.astype(np.float64), nthreads=8)
            # measured: <= 0.6 % of the envs outside 1e-5, each of them inside 2e-5 or on an oracle-visible discontinuity
            ok = _assert_step_parity(oracle, cm, _f32(st), act, qpos, qvel, s64, max_outlier_frac=0.006, dev_out=(obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy()))
            per_env = (np.abs(qvel - s64["qvel"]) / (1.0 + np.abs(s64["qvel"]))).max(1)
            worst.append(per_env[ok])
            assert np.all(_close(obs.cpu().numpy()[ok], ref["obs"][ok]))
            assert np.array_equal(done.cpu().numpy(), ref["done"])
            assert np.all((env.status().cpu().numpy() & 7) == 0)
        oracle.step(cm, st, act.astype(np.float64), nthreads=8)
    worst = np.concatenate(worst)
    assert np.median(worst) < 2e-6 and worst.max() <= 1e-5, (np.median(worst), worst.max())
    env.close()


def _point_step_parity_and_bounce(torch, oracle, lanes):
    """`lanes`: None (the handle's default: 16 lanes per env at this batch size on a 256-CU device) or the option "lanes_per_env" (8 / 16 / 32: the three
    instantiations of the bare Point, csrc/point_bare.h — at 8 lanes a lane holds SW = 8 contact slots per round and the 24
    clipping candidates take three passes).  Returns the step's observations."""
    n = 4096
    env = mm.make("PointUMaze-v0", num_envs=n)
    if lanes:
        env.set_option("lanes_per_env", lanes)
    li = env.launch_info()
    assert li["lanes_per_env"] == (lanes or (16 if (n + 3) // 4 <= li["device_simds"] else 32)) and li["engine"] == 0, li
    cm = env.model
    assert cm.c.nblock == 0 and cm.c.nball == 0
    rng = np.random.default_rng(9)
    xmin, xmax, ymin, ymax = cm.world.xy_limits()
    st = dict(qpos=np.stack([rng.uniform(xmin, xmax, n), rng.uniform(ymin, ymax, n), rng.uniform(-3.2, 3.2, n)], 1),
              qvel=np.stack([rng.uniform(0, 0.1, n), rng.uniform(0, 0.1, n), rng.uniform(-12, 12, n)], 1),
              warm=np.zeros((n, 3)), t=rng.integers(0, 1000, n).astype(np.int32))
    st["t"][:8] = 999
    st = _f32(st)
    act = np.stack([rng.uniform(-1, 1, n), rng.uniform(-0.25, 0.25, n)], 1).astype(np.float32)
    act[: n // 4, 0] *= 4.0  # the reference does not clip actions (point.py:44-55): long teleports -> bounces / give-ups
    env.set_state(st["qpos"], st["qvel"], None, st["t"])
    obs, rew, done, info = env.step(torch.as_tensor(act, device=env.device))
    status = env.status().cpu().numpy()
    g = oracle.forward(cm, st["qpos"], st["qvel"])
    assert (g["counts"][:, 1] > 0).sum() > n // 4  # MuJoCo sphere-box / arrow box-box rows active in the fixture
    ref = oracle.step(cm, st, act.astype(np.float64), nthreads=8)
    # status bit 8 = collinear move (the reference raises ZeroDivisionError there, maze_env_utils.py:119-123): the SAME envs on
    # both sides, a handful at most; no other status bit anywhere
    coll = (ref["status"] & 8) != 0
    assert np.array_equal((status & 8) != 0, coll) and coll.sum() <= 4
    assert np.all((status & ~8) == 0) and np.all((ref["status"] & ~8) == 0)
    free = ~coll
    o = obs.cpu().numpy()
    assert np.all(_close(o[free], ref["obs"][free], atol=1e-6, rtol=2e-7))
    assert np.array_equal(done.cpu().numpy()[free], ref["done"][free])
    assert np.array_equal(info["goal_index"].cpu().numpy()[free], ref["goal_idx"][free])
    assert np.array_equal(rew.cpu().numpy()[free], ref["reward"][free].astype(np.float32))
    assert np.all(done.cpu().numpy()[:8] & 2)
    env.close()
    return o


@pytest.mark.parametrize("lanes", [None, 8, 16, 32], ids=["default", "8", "16", "32"])
def test_point_step_parity_and_bounce(torch, oracle, lanes):
    _point_step_parity_and_bounce(torch, oracle, lanes)


def test_point_arrow_deep_inside_a_wall(torch, oracle):
    """The deep overlap of the bare Point's arrow with a wall cell — least-penetration axis vertical: mjc_BoxBox's general face case,
    the intersection polygon of two rectangles — is clipped with one candidate per lane (csrc/point_bare.h: pb_cand, the deep jobs of
    point_forward_bare).  Here most envs are such a case (arrow centre well inside a wall box, several cells at once for some), next
    to ordinary ones: all of them must agree with the oracle's literal mjc_BoxBox restatement, for two steps in a row."""
    n = 512
    env = mm.make("PointUMaze-v0", num_envs=n)
    cm = env.model
    boxes = np.array(cm.world.wall_boxes())  # x, y, z, hx, hy, hz
    rng = np.random.default_rng(31)
    xmin, xmax, ymin, ymax = cm.world.xy_limits()

    def inside(xy, shrink):
        return ((np.abs(xy[:, None, 0] - boxes[None, :, 0]) < boxes[None, :, 3] - shrink) & (np.abs(xy[:, None, 1] - boxes[None, :, 1]) < boxes[None, :, 4] - shrink)).any(1)

    qpos = np.zeros((0, 3))
    for _ in range(200):
        c = np.stack([rng.uniform(xmin, xmax, 4096), rng.uniform(ymin, ymax, 4096), rng.uniform(-3.1, 3.1, 4096)], 1)
        arrow = c[:, :2] + 0.6 * np.stack([np.cos(c[:, 2]), np.sin(c[:, 2])], 1)  # point.xml: the arrow box sits 0.6 ahead of the centre
        # the arrow (a 0.2 cube) overlaps the wall by 0.2 vertically: the vertical axis is the least-penetration one once its centre is
        # more than 0.1 + 0.2 inside, horizontally, on every side
        keep = inside(arrow, 0.35)
        qpos = np.concatenate([qpos, c[keep]])
        if len(qpos) >= n - 64:
            break
    assert len(qpos) >= n - 64
    qpos = qpos[: n - 64]
    free = np.stack([rng.uniform(xmin, xmax, 64), rng.uniform(ymin, ymax, 64), rng.uniform(-3.1, 3.1, 64)], 1)
    st = _f32(dict(qpos=np.concatenate([qpos, free]), qvel=np.stack([rng.uniform(-0.1, 0.1, n), rng.uniform(-0.1, 0.1, n), rng.uniform(-3, 3, n)], 1),
                   warm=np.zeros((n, 3)), t=np.zeros(n, np.int32)))
    g = oracle.forward(cm, st["qpos"], st["qvel"])
    assert (g["counts"][: n - 64, 1] >= 4).mean() > 0.9, (g["counts"][: n - 64, 1] >= 4).mean()  # the face contacts of the oracle's general routine
    act = np.zeros((n, 2), np.float32)  # no teleport: the step is MuJoCo's alone (a zero-length move: no manual bounce either)
    for k in range(2):
        env.set_state(st["qpos"], st["qvel"], None, st["t"])
        obs, rew, done, info = env.step(torch.as_tensor(act, device=env.device))
        ref = oracle.step(cm, st, act.astype(np.float64), nthreads=8)
        assert np.all(env.status().cpu().numpy() == 0) and np.all(ref["status"] == 0)
        assert np.all(_close(obs.cpu().numpy(), ref["obs"], atol=1e-6, rtol=2e-7)), np.abs(obs.cpu().numpy() - ref["obs"]).max()
        assert np.array_equal(done.cpu().numpy(), ref["done"])
        st = _f32(st)  # (oracle.step advanced it in place) the second step: both sides from the same fp32 state again
    env.close()


@pytest.mark.parametrize("env_id,nblock", [("PointPush-v0", 1), ("PointMultiPush-v0", 2), ("PointPushMaze-v0", 3), ("PointBilliard-v0", 0), ("PointSmallBilliard-v1", 0)])
def test_point_with_movable_blocks(torch, oracle, env_id, nblock):
    """Point + movable XY blocks (or the Billiard's object ball) on the lane-group planar kernel (32 / 64 lanes per env)."""
    n = 1024
    env = mm.make(env_id, num_envs=n)
    cm = env.model
    nball = cm.c.nball
    assert cm.c.nblock == nblock and env.obs_dim == 7 + 3 * nblock + 3 * nball and env.nv == 3 + 2 * nblock + 3 * nball
    st, _ = oracle.reset(cm, n, 1)
    rng = np.random.default_rng(0)
    errs, moved = [], 0.0
    for k in range(81):
        act = np.stack([rng.uniform(-1, 1, n), rng.uniform(-0.25, 0.25, n)], 1).astype(np.float32)
        if k % 20 == 0:
            s64 = _f32(st)
            env.set_state(s64["qpos"], s64["qvel"], None, s64["t"])
            obs, rew, done, info = env.step(torch.as_tensor(act, device=env.device))
            qpos, qvel, _, t = [x.cpu().numpy() for x in env.get_state()]
            ref = oracle.step(cm, s64, act.astype(np.float64), nthreads=8)
            assert np.array_equal(done.cpu().numpy(), ref["done"])
            assert np.array_equal(info["goal_index"].cpu().numpy(), ref["goal_idx"])
            # every env inside 2e-6 (the kernel computes in float64; what separates it from the oracle is the fp32 state it stores), or —
            # a robot teleported onto a block's diagonal sits on a tie between two faces — on a discontinuity the oracle shows itself
            ok = _assert_step_parity(oracle, cm, _f32(st), act, qpos, qvel, s64, atol=2e-6, max_outlier_frac=0.004, dev_out=(obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy()))
            errs.append(np.abs(obs.cpu().numpy() - ref["obs"]).max(1)[ok])
            assert np.array_equal(t, s64["t"])
            assert np.all((env.status().cpu().numpy() & ~8) == 0)
            moved = max(moved, np.abs(s64["qpos"][:, 3:]).max())
        oracle.step(cm, st, act.astype(np.float64), nthreads=8)
    errs = np.concatenate(errs)
    assert np.median(errs) < 3e-7 and errs.max() <= 2e-6 + 1e-5 * 20.0, (np.median(errs), errs.max())
    assert moved > 0.5
    env.close()


@pytest.mark.parametrize("robot,nq", [("Swimmer", 5), ("Reacher", 4)])
def test_swimmer_step_parity(torch, oracle, robot, nq):
    """Swimmer and its 2-link variant, the Reacher (reacher.py / reacher.xml), on the planar-chain kernels."""
    n = 4096
    env = mm.make(f"{robot}UMaze-v0", num_envs=n)
    cm = env.model
    nu = nq - 3
    assert env.obs_dim == 2 * nq + 1 and env.nu == nu
    st, _ = oracle.reset(cm, n, 3)
    rng = np.random.default_rng(0)
    st["qpos"][:, 3:] = rng.uniform(-1.9, 1.9, (n, nu))
    st["qvel"] = rng.normal(size=(n, nq)) * 2
    for k in range(6):
        act = rng.uniform(-1.5, 1.5, (n, nu)).astype(np.float32)
        if k in (0, 5):
            s64 = _f32(st)
            env.set_state(s64["qpos"], s64["qvel"], None, s64["t"])
            obs, rew, done, info = env.step(torch.as_tensor(act, device=env.device))
            ref = oracle.step(cm, s64, act.astype(np.float64), nthreads=8)
            assert np.all(_close(obs.cpu().numpy(), ref["obs"], atol=1e-6, rtol=2e-7))
            assert np.all(_close(rew.cpu().numpy(), ref["reward"], atol=1e-7))
            assert np.array_equal(done.cpu().numpy(), ref["done"])
            assert np.all(_close(info["reward_forward"].cpu().numpy(), ref["info"][:, 2], atol=1e-6))
            assert np.all(env.status().cpu().numpy() == 0)
        oracle.step(cm, st, act.astype(np.float64), nthreads=8)
    env.close()
    single = mm.make(f"{robot}SquareRoom-v1")
    bare = single.reset(return_info=False)  # the old-gym convention of the reference's own tests (tests/test_envs.py:13: env.reset().shape)
    assert isinstance(bare, np.ndarray) and bare.shape == (2 * nq + 1,)
    s0, _ = single.reset()
    s, r, d, inf = single.step(single.action_space.sample(np.random.default_rng(1)))
    assert s0.shape == (2 * nq + 1,) and s.shape == (2 * nq + 1,)  # reference tests/test_envs.py:77-78 (swimmer: 11)
    single.close()


@pytest.mark.parametrize("env_id", ["SwimmerPush-v0", "ReacherPush-v1"])
def test_swimmer_world_with_a_movable_block(torch, oracle, env_id):
    """The swimmer family observes and re-randomises the WHOLE qpos / qvel, block slides included (swimmer.py:50-69; layout
    pinned by tests/golden/obs_layout.json: SwimmerPush 18 numbers).  No contact pairs in the swimmer's world
    (swimmer.xml:3): a block at rest is inert; a block with the reset's velocity noise blows up in the medium exactly as in
    the reference (explicit drag on a 0.2 g box) and is flagged."""
    n = 512
    env = mm.make(env_id, num_envs=n)
    cm = env.model
    nr = env.nv - 2
    assert env.obs_dim == env.nq + env.nv + 4 and cm.c.nv_robot == env.nv
    obs0 = env.reset(seed=3).cpu().numpy()
    ref_st, ref_obs0 = oracle.reset(cm, n, 3)
    assert np.abs(obs0 - ref_obs0).max() < 2e-6 and np.ptp(obs0[:, 6 + nr - 3]) > 0.1  # block slide carries reset noise
    env.step(torch.zeros((n, env.nu), device=env.device))
    assert np.all(env.status().cpu().numpy() & 1)  # every env: block velocity noise -> unstable drag, as in MuJoCo
    st = ref_st
    st["qvel"][:, nr:] = 0.0
    rng = np.random.default_rng(0)
    for k in range(6):
        act = rng.uniform(-1.5, 1.5, (n, env.nu)).astype(np.float32)
        if k in (0, 5):
            s64 = _f32(st)
            env.set_state(s64["qpos"], s64["qvel"], None, s64["t"])
            qb = s64["qpos"][:, nr:].copy()
            obs, rew, done, info = env.step(torch.as_tensor(act, device=env.device))
            ref = oracle.step(cm, s64, act.astype(np.float64), nthreads=8)
            assert np.all(_close(obs.cpu().numpy(), ref["obs"], atol=1e-6, rtol=2e-7))
            assert np.all(_close(rew.cpu().numpy(), ref["reward"], atol=1e-7))
            assert np.array_equal(done.cpu().numpy(), ref["done"]) and np.all(env.status().cpu().numpy() == 0)
            qpos, qvel, _, _ = [x.cpu().numpy() for x in env.get_state()]
            assert np.array_equal(qpos[:, nr:], qb.astype(np.float32)) and np.all(qvel[:, nr:] == 0)
        oracle.step(cm, st, act.astype(np.float64), nthreads=8)
    env.close()


def test_point_fall_maze(torch, oracle):
    """PointFall-v0 (and PointMultiFall-v2, the same maze): elevated platforms, walls on top, a falling block with limited
    y / z slides that the reference spawns INSIDE its platform (maze_env.py:563-593 ignores height_offset) — the box rule
    [ASSUME-12] expels it upwards within a few steps and it ends as an obstacle at the robot's height.  The robot has no z
    dof: lifted with the torso it hovers above the platforms (and over the chasm).  Single-step parity along a rollout
    that covers the expulsion, the settled block and robot-block pushes."""
    n = 1024
    env = mm.make("PointFall-v0", num_envs=n)
    cm = env.model
    assert cm.c.elevated == 1 and env.obs_dim == 10 and env.nv == 5 and list(cm.c.body_pos[1]) == [0.0, 0.0, 2.75]
    st, _ = oracle.reset(cm, n, 1)
    rng = np.random.default_rng(0)
    errs, moved = [], 0.0
    for k in range(101):
        act = np.stack([rng.uniform(-1, 1, n), rng.uniform(-0.25, 0.25, n)], 1).astype(np.float32)
        if k in (0, 1, 5, 20, 60, 100):
            s64 = _f32(st)
            env.set_state(s64["qpos"], s64["qvel"], None, s64["t"])
            obs, rew, done, info = env.step(torch.as_tensor(act, device=env.device))
            qpos, qvel, _, t = [x.cpu().numpy() for x in env.get_state()]
            ref = oracle.step(cm, s64, act.astype(np.float64), nthreads=8)
            assert np.array_equal(done.cpu().numpy(), ref["done"]) and np.array_equal(info["goal_index"].cpu().numpy(), ref["goal_idx"])
            ok = _assert_step_parity(oracle, cm, _f32(st), act, qpos, qvel, s64, atol=2e-6, max_outlier_frac=0.004, dev_out=(obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy()))
            errs.append(np.abs(obs.cpu().numpy() - ref["obs"]).max(1)[ok])
            assert np.array_equal(t, s64["t"])
            assert np.all((env.status().cpu().numpy() & ~8) == 0)
            moved = max(moved, np.abs(s64["qpos"][:, 3]).max())
        oracle.step(cm, st, act.astype(np.float64), nthreads=8)
    errs = np.concatenate(errs)
    assert np.median(errs) < 3e-7 and errs.max() <= 2e-6 + 1e-5 * 20.0, (np.median(errs), errs.max())
    assert (st["qpos"][:, 4] > 1.5).mean() > 0.9  # the blocks have been expelled onto their platforms (z slide ~ +1.97 for a range of [-2, 0])
    assert moved > 0.05                    # and some robots have pushed theirs along y
    env.close()
    env = mm.make("PointMultiFall-v2", num_envs=8, force_vec=True)
    assert env.model.c.elevated == 1 and env.obs_dim == 10
    env.close()


@pytest.mark.parametrize("env_id", ["AntFall-v0", "AntMultiFall-v2", "AntMultiFall-v0"])
def test_ant_fall_maze(torch, oracle, env_id):
    """AntFall (and AntMultiFall-v2, which subclasses the Fall maze, maze_task.py:342): the ant stands on the platforms of an
    elevated maze (capsule-box contacts instead of the floor plane), walls on top of them, chasms to fall into, and a falling
    block with limited y / z slides which the reference spawns inside its platform: the box rule expels
    it upwards within three steps (the single-step error is largest there: the block moves 4 m in 0.3 s against a stiff
    limit row), after which it rests on its platform as an obstacle.  3-D goal (0, 3.375, 4.5) x scale."""
    n = 1024
    env = mm.make(env_id, num_envs=n)
    cm = env.model
    multi = env_id == "AntMultiFall-v0"  # MultiFall proper: maze scale 2, a block with THREE limited slides (x, y, z)
    assert cm.c.elevated == 1 and env.obs_dim == 33 and (env.nq, env.nv) == ((18, 17) if multi else (17, 16)) and cm.c.goal_dim[0] == 3
    st, _ = oracle.reset(cm, n, 1)
    rng = np.random.default_rng(0)
    worst = []
    for k in range(41):
        act = rng.uniform(-30, 30, (n, 8)).astype(np.float32)
        if k in (0, 1, 3, 10, 40):
            s64 = _f32(st)
            env.set_state(s64["qpos"], s64["qvel"], s64["warm"], s64["t"])
            obs, rew, done, info = env.step(torch.as_tensor(act, device=env.device))
            qpos, qvel, warm, t = [x.cpu().numpy() for x in env.get_state()]
            ref = oracle.step(cm, s64, act.astype(np.float64), nthreads=8)
            # at maze scale 2 the ant straddles the seams between platform boxes and walls all the time (as in the scale-2
            # multi-block mazes): more envs sit on a contact-activation discontinuity, each of them proven on the oracle
            # cap: envs on a contact-activation discontinuity, each proven on the oracle (measured: at most 5 of 1024 per checkpoint)
            # 1e-5 like everywhere else, the step that expels the block (k = 1) included; no looser bound without the discontinuity proof
            # (rounds 3-4 held this family to 2e-5 .. 4.5e-5: the same unrefined Newton steps as AntPush's tail, see BRANCH_ATOL)
            ok = _assert_step_parity(oracle, cm, _f32(st), act, qpos, qvel, s64, max_outlier_frac=0.01,
                                     dev_out=(obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy()), ref_done=ref["done"])
            worst.append((np.abs(qvel - s64["qvel"]) / (1.0 + np.abs(s64["qvel"]))).max(1)[ok])
            assert np.all(_close(obs.cpu().numpy()[ok], ref["obs"][ok]))
            assert np.array_equal(done.cpu().numpy(), ref["done"]) and np.array_equal(info["goal_index"].cpu().numpy(), ref["goal_idx"])
            assert np.all((env.status().cpu().numpy() & 7) == 0)
        oracle.step(cm, st, act.astype(np.float64), nthreads=8)
    worst = np.concatenate(worst)
    assert np.median(worst) < 3e-6, np.median(worst)
    top = cm.c.height_offset  # ants on the platforms, blocks expelled onto theirs (z slide ~ the platform height, range [-top, 0])
    assert (st["qpos"][:, 2] > top + 0.2).mean() > 0.95 and np.all(st["qpos"][:, env.nq - 1] > 0.85 * top)
    env.close()


def test_swimmer_family_fall_maze(torch, oracle):
    """SwimmerFall / ReacherFall / *MultiFall-v2: no contacts in the swimmer's world; the falling block's drag diverges as soon
    as it moves (gravity makes it move): flagged at once on the device as in the oracle (tests/test_capi_and_emu.py has the
    reasoning); layout 2 nv + 4."""
    for env_id in ("SwimmerFall-v0", "ReacherFall-v1", "SwimmerMultiFall-v2"):
        n = 64
        env = mm.make(env_id, num_envs=n)
        cm = env.model
        assert env.obs_dim == env.nq + env.nv + 4 and cm.c.elevated == 1
        obs0 = env.reset(seed=3).cpu().numpy()
        _, ref0 = oracle.reset(cm, n, 3)
        assert np.abs(obs0 - ref0).max() < 2e-6
        env.step(torch.zeros((n, env.nu), device=env.device))
        assert np.all(env.status().cpu().numpy() & 1)
        env.close()


def test_reset_distribution_and_oracle_rng(torch, oracle):
    n = 2048
    for env_id, nq, nv in (("AntUMaze-v0", 15, 14), ("PointUMaze-v0", 3, 3), ("SwimmerUMaze-v0", 5, 5)):
        env = mm.make(env_id, num_envs=n)
        obs = env.reset(seed=1234).cpu().numpy()
        ref_st, ref_obs = oracle.reset(env.model, n, 1234)
        assert np.abs(obs - ref_obs).max() < 2e-6
        q0 = np.array(env.model.c.qpos0[:nq])
        dev = np.abs(obs[:, :nq] - q0)
        if env_id.startswith("Ant"):  # the root quaternion is observed normalised (mj_kinematics, [ASSUME-8])
            assert np.all(np.abs(np.linalg.norm(obs[:, 3:7], axis=1) - 1.0) < 1e-6) and np.all(dev[:, 3:7] <= 0.12)
            dev = np.delete(dev, [3, 4, 5, 6], axis=1)
        assert np.all(dev <= 0.1 + 1e-6)  # ant.py:85-89 / point.py:72-74
        assert np.all(obs[:, -1] == 0.0)
        v = obs[:, nq:nq + nv]
        if nq == 3:
            assert v.min() >= 0.0 and v.max() < 0.1 + 1e-6  # point.py:75: U[0,1) * 0.1
        elif nq == 5:
            assert v.min() >= -0.1 - 1e-6 and v.max() <= 0.1 + 1e-6 and abs(v.mean()) < 0.01  # swimmer.py:61-65
        else:
            assert abs(v.std() - 0.1) < 0.01 and abs(v.mean()) < 0.01  # ant.py:90: randn * 0.1
        # masked reset leaves the others untouched
        a = np.zeros((n, env.nu), np.float32)
        env.step(a)
        before = env.get_state()[0].cpu().numpy()
        mask = np.zeros(n, np.uint8); mask[::2] = 1
        env.reset(mask=mask, seed=99)
        after = env.get_state()[0].cpu().numpy()
        assert np.array_equal(after[1::2], before[1::2]) and not np.array_equal(after[::2], before[::2])
        env.close()


def _goal_predicate_f64(task, slot):
    """The reference's float64 predicate (maze_task.py:43-44,77-81) on rows of float64 slot coordinates: any goal neighbour."""
    hit = np.zeros(len(slot), bool)
    for g in task.goals:
        hit |= np.sqrt(np.sum(np.square(slot[:, : g.dim] - g.pos), axis=1)) <= g.threshold
    return hit


@pytest.mark.parametrize("env_id,n", [("AntUMaze-v0", 4096), ("Ant4Rooms-v0", 4096), ("AntPush-v0", 2048)])
def test_full_size_properties(torch, env_id, n):
    """BASELINE sizes (configs[2], [3] per GPU, [4]): size-independent properties over a 60-step rollout with auto-reset."""
    env = mm.make(env_id, num_envs=n, auto_reset=True)
    task = env._task
    env.reset(seed=5)
    g = torch.Generator(device=env.device).manual_seed(0)
    nb3 = env.obs_dim - 30
    # start a slice of the envs around the goal so that terminations do happen inside the 60 steps
    qpos, qvel, warm, t = env.get_state()
    gp = torch.as_tensor(task.goals[0].pos[:2], device=env.device, dtype=torch.float32)
    qpos[: n // 8, :2] = gp + (torch.rand((n // 8, 2), device=env.device, generator=g) - 0.5) * 2.5
    env.set_state(qpos=qpos)
    nterm = 0
    ever = torch.zeros(n, dtype=torch.bool, device=env.device)
    for k in range(60):
        act = (torch.rand((n, 8), device=env.device, generator=g) * 60 - 30)
        obs, rew, done, info = env.step(act)
        assert torch.isfinite(obs).all() and torch.isfinite(rew).all()
        # termination flag is exactly the reference's FLOAT64 predicate (maze_task.py:43-44,77-81) on the observation the
        # step produced: `obs` for running envs, info["final_observation"] for the ones that just auto-reset
        last = torch.where((done != 0)[:, None], info["final_observation"], obs).double().cpu().numpy()
        pred = _goal_predicate_f64(task, last[:, :3])
        d = done.cpu().numpy()
        assert np.array_equal((d & 1).astype(bool), pred)
        nterm += int(pred.sum())
        ever |= done != 0
        fresh = ~ever  # envs that have not auto-reset yet carry the global step count
        if k < 5:
            assert torch.allclose(obs[:, -1][fresh], torch.tensor((k + 1) * 0.001, device=env.device))
        qn = obs[:, 3 + nb3:7 + nb3].norm(dim=1)
        assert torch.all((qn - 1).abs() < 1e-5)  # integrated quaternions stay unit
        if nb3:
            assert torch.all(obs[:, 5] == 2.0)  # block z slot
    assert nterm > n // 100
    st = env.status().cpu().numpy()
    assert np.all((st & 1) == 0), "NaN / diverged envs"
    assert (st & 2).mean() < 0.01, "contact buffer overflow"
    # TimeLimit: envs at t = 999 truncate on the next step and auto-reset to t = 0
    qpos, qvel, warm, t = env.get_state()
    t[:] = 999
    env.set_state(t=t)
    obs, rew, done, info = env.step(torch.zeros((n, 8), device=env.device))
    assert torch.all(done & 2)
    assert torch.all(env.get_state()[3] == 0)
    # vector-env convention: `obs` is the FIRST observation of the new episode (t = 0, reset distribution around qpos0),
    # the terminal one (t = 1000) is in final_observation
    assert torch.all(obs[:, -1] == 0.0) and torch.allclose(info["final_observation"][:, -1], torch.tensor(1.0, device=env.device))
    qpos = env.get_state()[0]
    assert torch.equal(obs[:, :3], qpos[:, :3]) and torch.all((obs[:, 2] - 0.75).abs() <= 0.1 + 1e-6)
    env.close()


@pytest.mark.parametrize("env_id", ["Ant4Rooms-v2", "Point4Rooms-v2", "AntTRoom-v2", "PointBilliard-v2"])
def test_subgoal_first_match_parity(torch, oracle, env_id):
    """`-v2` sub-goal tasks (maze_task.py:403-407: the FIRST goal in list order that is a neighbour pays its reward_scale —
    1.0 for the main goal, 0.5 for sub-goals — else PENALTY; termination at any goal): envs placed around every goal, one
    step on the device against the oracle: reward, done and goal index."""
    n = 256
    env = mm.make(env_id, num_envs=n)
    cm, task = env.model, env._task
    assert len(task.goals) > 1
    st, _ = oracle.reset(cm, n, 4)
    rng = np.random.default_rng(1)
    object_slot = cm.c.term_slot == 1
    for gi, g in enumerate(task.goals):
        sel = slice(gi * 48, gi * 48 + 48)
        xy = g.pos[:2] + rng.normal(0.0, g.threshold * 0.7, (48, 2))
        if object_slot:  # Billiard: the ball's slide coordinates (body spawn position + q)
            b = cm.c.ball_bodyid[0]
            st["qpos"][sel, 3:5] = xy - np.array(cm.c.body_pos[b][:2])
            st["qpos"][sel, :2] = xy + np.array([3.0, 0.0])  # robot out of the way
        else:
            st["qpos"][sel, :2] = xy
    s64 = _f32(st)
    start = {k: v.copy() for k, v in s64.items()}
    lo, hi = env.action_space.low, env.action_space.high
    act = (0.05 * rng.uniform(lo, hi, (n, env.nu))).astype(np.float32)
    env.set_state(s64["qpos"], s64["qvel"], s64["warm"] if env_id.startswith("Ant") else None, s64["t"])
    obs, rew, done, info = env.step(torch.as_tensor(act, device=env.device))
    qpos, qvel, _, _ = [x.cpu().numpy() for x in env.get_state()]
    ref = oracle.step(cm, s64, act.astype(np.float64), nthreads=8)
    gidx = info["goal_index"].cpu().numpy()
    assert np.array_equal(done.cpu().numpy(), ref["done"]) and np.array_equal(gidx, ref["goal_idx"])
    for gi in range(len(task.goals)):
        assert (gidx == gi).sum() >= 8, (gi, (gidx == gi).sum())  # every goal is matched by some envs
    o = obs.double().cpu().numpy()
    slot = o[:, 3:6] if object_slot else o[:, :3]
    assert np.array_equal((done.cpu().numpy() & 1).astype(bool), _goal_predicate_f64(task, slot))
    # placed by hand around the goals, ants land on / in walls: every env inside the tolerance or on a discontinuity of the oracle
    near = _assert_step_parity(oracle, cm, start, act, qpos, qvel, s64, atol=1e-5 if env_id.startswith("Ant") else 2e-6, max_outlier_frac=0.03)
    assert np.all(_close(obs.cpu().numpy()[near], ref["obs"][near], atol=1e-5))
    inner = rew.cpu().numpy() - np.where(gidx >= 0, np.array([g.reward_scale for g in task.goals] + [0.0])[gidx], task.PENALTY)
    ref_inner = ref["reward"] - np.where(ref["goal_idx"] >= 0, np.array([g.reward_scale for g in task.goals] + [0.0])[ref["goal_idx"]], task.PENALTY)
    assert np.all(np.abs(inner - ref_inner)[near] <= 1e-5)
    env.close()


def test_rollout_tracks_oracle_and_long_run_is_clean(torch, oracle):
    """(1) every step of a 10-step rollout meets the single-step bar from the oracle's state; (2) 1500 auto-reset steps at the
    BASELINE size produce no NaN / overflow status and episode bookkeeping stays consistent."""
    n = 512
    env = mm.make("AntUMaze-v0", num_envs=n)
    cm = env.model
    st, _ = oracle.reset(cm, n, 31)
    st = _f32(st)
    env.set_state(st["qpos"], st["qvel"], st["warm"], st["t"])
    rng = np.random.default_rng(6)
    # ten consecutive steps of one rollout, the device re-synchronised to the oracle's state before each (trajectories are chaotic:
    # what can be asserted env by env is every single step of the way)
    for k in range(10):
        act = rng.uniform(-30, 30, (n, 8)).astype(np.float32)
        s64 = _f32(st)
        env.set_state(s64["qpos"], s64["qvel"], s64["warm"], s64["t"])
        env.step(torch.as_tensor(act, device=env.device))
        qpos, qvel, _, _ = [x.cpu().numpy() for x in env.get_state()]
        start = {kk: v.copy() for kk, v in s64.items()}
        oracle.step(cm, s64, act.astype(np.float64), nthreads=8)
        _assert_step_parity(oracle, cm, start, act, qpos, qvel, s64)
        oracle.step(cm, st, act.astype(np.float64), nthreads=8)
    env.close()
    n = 4096
    env = mm.make("AntUMaze-v0", num_envs=n, auto_reset=True)
    env.reset(seed=77)
    g = torch.Generator(device=env.device).manual_seed(3)
    acts = [(torch.rand((n, 8), device=env.device, generator=g) * 60 - 30) for _ in range(8)]
    ndone = 0
    for k in range(1500):
        obs, rew, done, info = env.step(acts[k % 8])
        if k % 100 == 99:
            ndone += int((done != 0).sum().item())
            assert torch.isfinite(obs).all()
    stt = env.status().cpu().numpy()
    assert np.all((stt & 3) == 0), (int((stt & 1).sum()), int((stt & 2).sum()))
    t = env.get_state()[3].cpu().numpy()
    assert t.min() >= 0 and t.max() <= 1000 and (t == 500).sum() > n // 2  # 1500 steps = one truncation + 500
    env.close()


def test_single_env_facade_shapes(torch):
    """What the reference's tests/test_envs.py pins: obs shapes and reward sign."""
    rng = np.random.default_rng(0)
    for maze_id in ("UMaze", "4Rooms", "SimpleRoom", "Corridor"):
        for i in range(2):
            env = mm.make(f"Ant{maze_id}-v{i}")
            s0, info = env.reset()
            s, r, d, inf = env.step(env.action_space.sample(rng))
            assert s0.shape == (30,) and s.shape == (30,) and s.dtype == np.float64
            assert set(inf) >= {"position", "reward_forward", "reward_ctrl"}
            env.close()
            env = mm.make(f"Point{maze_id}-v{i}")
            s0, _ = env.reset()
            s, r, d, _ = env.step(env.action_space.sample(rng))
            assert s0.shape == (7,) and s.shape == (7,)
            # reference test expects r != 0 for -v0 and r == PENALTY for -v1; both resolve to the goal
            # reward, so away from the goal both give PENALTY
            assert r == pytest.approx(env._task.PENALTY) and r < 0.0
            env.close()
    env = mm.make("PointTRoom-v0", task_kwargs={"goal": (-2.0, -3.0)})  # tests/test_envs.py:81-86
    assert env.reset()[0].shape == (7,)
    env.close()
    env = mm.make("Point4Rooms-v2")
    assert len(env._task.goals) > 1
    env.close()


@pytest.mark.parametrize("env_id", ["AntUMaze-v0", "AntPush-v0", "PointUMaze-v0", "PointPush-v0", "SwimmerUMaze-v0", "ReacherUMaze-v0"])
def test_ragged_batch_sizes_and_argument_errors(torch, oracle, env_id):
    """Batches that do not fill the last workgroup (2 or 4 envs per wavefront) and a batch of one; bad arguments raise."""
    rng = np.random.default_rng(4)
    for n in (1, 3, 37):
        env = mm.make(env_id, num_envs=n, force_vec=True)
        cm = env.model
        st, _ = oracle.reset(cm, n, 8)
        s64 = _f32(st)
        lo, hi = env.action_space.low, env.action_space.high
        act = rng.uniform(lo, hi, (n, env.nu)).astype(np.float32)
        env.set_state(s64["qpos"], s64["qvel"], s64["warm"] if env_id.startswith("Ant") else None, s64["t"])
        obs, rew, done, info = env.step(torch.as_tensor(act, device=env.device))
        ref = oracle.step(cm, s64, act.astype(np.float64), nthreads=2)
        assert obs.shape == (n, env.obs_dim) and rew.shape == (n,) and done.shape == (n,)
        assert np.all(_close(obs.cpu().numpy(), ref["obs"]))
        assert np.array_equal(done.cpu().numpy(), ref["done"])
        assert np.all(env.status().cpu().numpy() == 0)
        with pytest.raises(ValueError):
            env.step(torch.zeros((n + 1, env.nu), device=env.device))
        obs64, *_ = env.step(torch.zeros((n, env.nu), device=env.device, dtype=torch.float64))  # converted, not rejected
        assert obs64.dtype == torch.float32
        env.close()
    with pytest.raises(KeyError):
        mm.make("AntNoSuchMaze-v0")
    with pytest.raises(ValueError):  # the reference: "OBJBALL_TYPE is not registered" for robots without an object-ball flavour
        from mujoco_maze_amd import maze_task as T2
        from mujoco_maze_amd.maze_env import VecMazeEnv

        VecMazeEnv(mm.SwimmerEnv, T2.GoalRewardSmallBilliard, num_envs=2, maze_size_scaling=2.0)


def test_user_robot_xml_on_the_device(torch, oracle):
    """A parameter variant of the ant given as MJCF (mujoco_maze_amd/mjcf.py) runs on the ant kernel."""
    from tests.test_mjcf import _heavy_ant_xml

    n = 512
    env = mm.make("AntUMaze-v0", num_envs=n, robot_xml=_heavy_ant_xml())
    cm = env.model
    assert cm.c.act_gear[0] == 1.5 and env.action_space.high[0] == 40.0
    st, _ = oracle.reset(cm, n, 2)
    rng = np.random.default_rng(0)
    for k in range(21):
        act = rng.uniform(-40, 40, (n, 8)).astype(np.float32)
        if k in (0, 20):
            s64 = _f32(st)
            env.set_state(s64["qpos"], s64["qvel"], s64["warm"], s64["t"])
            obs, rew, done, info = env.step(torch.as_tensor(act, device=env.device))
            qpos, qvel, warm, t = [x.cpu().numpy() for x in env.get_state()]
            ref = oracle.step(cm, s64, act.astype(np.float64), nthreads=8)
            _assert_step_parity(oracle, cm, _f32(st), act, qpos, qvel, s64, max_outlier_frac=0.01, dev_out=(obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy()))
            assert np.array_equal(done.cpu().numpy(), ref["done"])
        oracle.step(cm, st, act.astype(np.float64), nthreads=8)
    env.close()


def test_every_registered_id_runs_or_refuses(torch):
    """All 145 ids of the reference's registry (mujoco_maze/__init__.py:17-78) build and step on the device."""
    rng = np.random.default_rng(0)
    ran, refused = 0, []
    for env_id in mm.REGISTRY:
        try:
            env = mm.make(env_id, num_envs=8, force_vec=True)
        except NotImplementedError:
            refused.append(env_id)
            continue
        env.reset(seed=1)
        lo, hi = env.action_space.low, env.action_space.high
        for _ in range(3):
            obs, rew, done, info = env.step(torch.as_tensor(rng.uniform(lo, hi, (8, env.nu)).astype(np.float32), device=env.device))
        assert obs.shape == (8, env.obs_dim), env_id
        if env.model.c.robot == 2 and env.model.c.nblock:
            # Swimmer / Reacher + movable block: the reference's reset puts velocity noise on the block (swimmer.py:56-69) and the
            # medium's explicit drag on a 0.2 g box diverges at once — MuJoCo warns (mujoco-py raises); here every env is flagged
            assert np.all(env.status().cpu().numpy() & 1), env_id
        else:
            assert torch.isfinite(obs).all() and torch.isfinite(rew).all(), env_id
            assert np.all((env.status().cpu().numpy() & 3) == 0), env_id
        env.close()
        ran += 1
    assert ran == 145 and refused == []


def test_ant_small_billiard_free_joint_ball(torch, oracle):
    """AntSmallBilliard-v0/-v1 (maze_task.py:732-762; AntEnv.OBJBALL_TYPE = "freejoint", maze_env.py:539-560): a 1.34 kg ball on
    a free joint — six more dofs, quaternion, contacts with floor, walls, torso and leg capsules.  Single-step parity from
    rollout states in which half of the ants were sent into the ball; flags / goal index (judged on the BALL's position)
    exact; the ball really rolls."""
    n = 768
    env = mm.make("AntSmallBilliard-v1", num_envs=n)
    cm = env.model
    assert (env.nq, env.nv, env.obs_dim) == (22, 20, 33)
    st, _ = oracle.reset(cm, n, 17)
    rng = np.random.default_rng(3)
    st["qpos"][: n // 2, 1] = -0.9 + rng.uniform(-0.1, 0.1, n // 2)
    st["qvel"][: n // 2, 1] = -2.0
    # a few balls start on the goal so that the termination flag and the goal index fire (goal of -v1: (-1, -2) * scale)
    goal = np.array(cm.task.goals[0].pos[:2])
    st["qpos"][-16:, 15:17] = goal + rng.uniform(-0.3, 0.3, (16, 2))
    rolled, kicked, dones = 0.0, 0, 0
    for k in range(81):
        act = rng.uniform(-30, 30, (n, 8)).astype(np.float32)
        if k in (0, 2, 10, 40, 80):
            s64 = _f32(st)
            env.set_state(s64["qpos"], s64["qvel"], s64["warm"], s64["t"])
            obs, rew, done, info = env.step(torch.as_tensor(act, device=env.device))
            qpos, qvel, warm, t = [x.cpu().numpy() for x in env.get_state()]
            ref = oracle.step(cm, s64, act.astype(np.float64), nthreads=8)
            ok = _assert_step_parity(oracle, cm, _f32(st), act, qpos, qvel, s64, max_outlier_frac=0.01, dev_out=(obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy()))
            assert np.all(_close(obs.cpu().numpy()[ok], ref["obs"][ok]))
            assert np.array_equal(done.cpu().numpy()[ok], ref["done"][ok])
            assert np.all(_close(rew.cpu().numpy()[ok], ref["reward"][ok], atol=1e-5))
            assert np.array_equal(obs.cpu().numpy()[:, 3:6], qpos[:, 15:18])  # the ball's body origin is what is observed
            dones += int((ref["done"] != 0).sum())
            rolled = max(rolled, float(np.abs(s64["qpos"][:, 18] - 1.0).max()))
            kicked = max(kicked, int((np.abs(s64["qvel"][:, 14:17]).max(1) > 0.05).sum()))
            assert np.all((env.status().cpu().numpy() & 3) == 0)
        oracle.step(cm, st, act.astype(np.float64), nthreads=8)
    assert rolled > 0.05 and kicked >= 20 and dones >= 8
    env.close()


def test_captured_state_where_the_two_enumeration_passes_diverged(torch, oracle):
    """Regression fixture of round 3's soak (tests/golden/antpushmaze_count_fill_case.npz, captured on the device by
    tools/catch_nan.py): an AntPushMaze state in which the count pass and the fill pass of the kernel's contact enumeration —
    two instantiations of one template under relaxed floating-point flags — disagreed about the second support point of an
    ankle capsule against a box.  The counted slot stayed unwritten and the step went NaN.  The fill pass now owns exactly the
    counted slots (an uncounted contact is dropped, a missing one is inert, ant_dyn.h con_fill_item) and the device kernels
    enumerate once (con_enum_item); the step must be finite and agree with the oracle."""
    c = np.load(os.path.join(os.path.dirname(__file__), "golden", "antpushmaze_count_fill_case.npz"))
    env = mm.make("AntPushMaze-v0", num_envs=1, force_vec=True)
    cm = env.model
    st = dict(qpos=c["qpos"][None].astype(np.float64), qvel=c["qvel"][None].astype(np.float64), warm=c["warm"][None].astype(np.float64),
              t=np.array([int(c["t"])], np.int32))
    env.set_state(st["qpos"], st["qvel"], st["warm"], st["t"])
    obs, rew, done, info = env.step(torch.as_tensor(c["act"][None], device=env.device))
    qpos, qvel, _, _ = [x.cpu().numpy() for x in env.get_state()]
    assert np.isfinite(qpos).all() and np.isfinite(qvel).all() and np.isfinite(obs.cpu().numpy()).all()
    assert (int(env.status().cpu().numpy()[0]) & 1) == 0
    # The state sits ON the discontinuity that made the passes differ — whether mjc_CapsuleBox's second support point exists:
    # the float64 oracle lands 1.6e-3 away from itself when the state moves by one fp32 ulp.  The device must land on one of
    # the oracle's two branches.
    rng = np.random.default_rng(0)
    branches = []
    for k in range(25):
        p = {kk: v.copy() for kk, v in st.items()}
        if k:
            p["qpos"] += rng.uniform(-2e-7, 2e-7, p["qpos"].shape) * np.maximum(1.0, np.abs(p["qpos"]))
            p["qvel"] += rng.uniform(-2e-7, 2e-7, p["qvel"].shape) * np.maximum(1.0, np.abs(p["qvel"]))
        oracle.step(cm, p, c["act"][None].astype(np.float64))
        branches.append(p["qpos"][0])
    branches = np.array(branches)
    gap = np.abs(branches - qpos[0]).max(1)
    assert np.abs(branches - branches[0]).max() > 1e-3, "fixture no longer on the discontinuity"
    assert gap.min() < 2e-5, gap.min()
    env.close()


def test_captured_state_where_the_lanes_of_a_row_parted_ways(torch, oracle):
    """Regression fixture of round 3's 60 000-step soak (tests/golden/antumaze_lane_divergence_case.npz, captured on the device
    by tools/catch_soak.py; one env in 2.5e8 env-steps): an AntUMaze state whose Newton line search starts with phi'(1) = +1e-5.
    The lanes of a 16-lane row compute alpha redundantly from group sums; with FMA contraction reaching into the butterfly
    (`rsum(p * q)` -> fma(p, q, partner's rounded product)) the sums differed in the last bit between lanes, one lane's Newton
    step on phi' rounded onto its bracket, that lane bisected to alpha = 3e-7 and declared itself done, and the row iterated
    to the cap on an inconsistent qacc: MAXITER, 2e-3 off the oracle.  The group sums are now bitwise identical on every lane
    (contract(off) in rsum / DevCtx::dpp_add / gsum); the step must converge and agree with the oracle."""
    c = np.load(os.path.join(os.path.dirname(__file__), "golden", "antumaze_lane_divergence_case.npz"))
    env = mm.make("AntUMaze-v0", num_envs=1, force_vec=True)
    st = dict(qpos=c["qpos"][None].astype(np.float64), qvel=c["qvel"][None].astype(np.float64), warm=c["warm"][None].astype(np.float64),
              t=np.array([int(c["t"])], np.int32))
    env.set_state(st["qpos"], st["qvel"], st["warm"], st["t"])
    env.step(torch.as_tensor(c["act"][None], device=env.device))
    qpos, qvel, _, _ = [x.cpu().numpy() for x in env.get_state()]
    assert int(env.status().cpu().numpy()[0]) == 0
    oracle.step(env.model, st, c["act"][None].astype(np.float64))
    assert np.abs(qpos - st["qpos"]).max() < 1e-5 and np.abs(qvel - st["qvel"]).max() < 1e-4, (np.abs(qpos - st["qpos"]).max(), np.abs(qvel - st["qvel"]).max())
    env.close()


@pytest.mark.parametrize("which", ["biped_ant", "y_swimmer"])
def test_user_robot_of_another_topology_on_the_device(torch, oracle, which):
    """SURVEY 8f rank 4 / VERDICT r02 #8: a user's AgentModel whose MJCF is NOT one of the built-in shapes — a two-legged ant with a
    tail (7 bodies, free root, 5 motors, floor and wall contacts), a Y-shaped swimmer (branching tree in the medium) — steps on the
    device through the same plugin surface (`MazeEnv(model_cls=MyRobot, maze_task=...)`, agent_model.py:12-41, README.md:127), on the
    generic tree kernel (csrc/generic_dyn.h).  Float64 on both sides: parity at 1e-6 on the fp32 state that is stored."""
    from mujoco_maze_amd import maze_task as T
    from mujoco_maze_amd.maze_env import MazeEnv, VecMazeEnv
    from tests import user_robots

    BipedAnt, YSwimmer = user_robots.robot_classes()
    cls, amp = (BipedAnt, 20.0) if which == "biped_ant" else (YSwimmer, 1.0)
    n = 300
    env = VecMazeEnv(cls, T.DistRewardUMaze, num_envs=n, maze_size_scaling=4.0)
    cm = env.model
    assert cm.c.robot == 3 and env.obs_dim == cm.c.nq + cm.c.nv + 1
    obs0 = env.reset(seed=5).cpu().numpy()
    ref_st, ref_obs0 = oracle.reset(cm, n, 5)
    assert np.abs(obs0 - ref_obs0).max() < 2e-6
    st = ref_st
    rng = np.random.default_rng(1)
    if which == "biped_ant":
        st["qpos"][: n // 3, 0] = 1.2 + rng.uniform(0.0, 0.4, n // 3)  # next to the wall east of the start cell
    contacts = 0
    for k in range(41):
        act = rng.uniform(-amp, amp, (n, env.nu)).astype(np.float32)
        if k in (0, 2, 10, 40):
            s64 = _f32(st)
            contacts += int(oracle.forward(cm, s64["qpos"], s64["qvel"], act.astype(np.float64), s64["warm"])["counts"][:, 0].sum())
            env.set_state(s64["qpos"], s64["qvel"], s64["warm"], s64["t"])
            obs, rew, done, info = env.step(torch.as_tensor(act, device=env.device))
            qpos, qvel, warm, t = [x.cpu().numpy() for x in env.get_state()]
            ref = oracle.step(cm, s64, act.astype(np.float64), nthreads=8)
            ok = _assert_step_parity(oracle, cm, _f32(st), act, qpos, qvel, s64, atol=1e-6, max_outlier_frac=0.0, dev_out=(obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy()))
            assert ok.all()
            assert np.all(_close(obs.cpu().numpy(), ref["obs"], atol=1e-6)) and np.all(_close(rew.cpu().numpy(), ref["reward"], atol=1e-6))
            assert np.array_equal(done.cpu().numpy(), ref["done"]) and np.array_equal(info["goal_index"].cpu().numpy(), ref["goal_idx"])
            assert np.all(_close(warm, s64["warm"], atol=1e-4, rtol=1e-5)) and np.array_equal(t, s64["t"])
            assert np.all((env.status().cpu().numpy() & 7) == 0)
        oracle.step(cm, st, act.astype(np.float64), nthreads=8)
    if which == "biped_ant":
        assert contacts > 500
    # auto-reset + TimeLimit + packed record work as for the built-in robots
    env.set_auto_reset(True)
    rec = torch.zeros((n, env.obs_dim + 2), device=env.device)
    env.bind_record(rec)
    tt = env.get_state()[3]; tt[:] = 999
    env.set_state(t=tt)
    obs, rew, done, info = env.step(torch.zeros((n, env.nu), device=env.device))
    assert torch.all(done & 2) and torch.all(obs[:, -1] == 0.0) and torch.equal(rec, torch.cat([obs, rew[:, None], done.float()[:, None]], 1))
    env.close()
    single = MazeEnv(cls, T.GoalRewardUMaze, maze_size_scaling=4.0)
    o, _ = single.reset()
    o2, r, d, inf = single.step(single.action_space.sample(np.random.default_rng(0)))
    assert o.shape == (cm.c.obs_dim,) and o2.shape == o.shape and isinstance(r, float)
    single.close()


@pytest.mark.parametrize("env_id", ["PointUMaze-v0", "AntUMaze-v0", "AntPush-v0", "SwimmerUMaze-v0"])
def test_wrapped_env_get_xy_set_xy_get_ori(env_id):
    """`env.wrapped_env.get_xy() / set_xy(xy) / get_ori()` (agent_model.py:35-41, ant.py:98-111, point.py:83-92, maze_env.py:218,232)
    over mz_get_state / mz_set_state: set_xy moves qpos[:2] and nothing else; get_ori is the Point's angle / the heading of
    the Ant's torso x axis."""
    import torch

    n = 16
    env = mm.make(env_id, num_envs=n)
    env.reset(seed=5)
    rng = np.random.default_rng(1)
    for _ in range(3):
        env.step(torch.as_tensor(rng.uniform(env.action_space.low, env.action_space.high, (n, env.nu)).astype(np.float32), device=env.device))
    qpos0, qvel0, warm0, t0 = [x.clone() for x in env.get_state()]
    w = env.wrapped_env
    assert w.ORI_IND == env.wrapped_cls.ORI_IND and w.FILE == env.wrapped_cls.FILE  # class knobs read through
    xy = w.get_xy()
    assert torch.equal(xy, qpos0[:, :2]) and xy.data_ptr() != qpos0.data_ptr()
    new = xy + torch.as_tensor(rng.uniform(-0.3, 0.3, (n, 2)).astype(np.float32), device=env.device)
    w.set_xy(new)
    qpos1, qvel1, warm1, t1 = env.get_state()
    assert torch.equal(qpos1[:, :2], new) and torch.equal(qpos1[:, 2:], qpos0[:, 2:])
    assert torch.equal(qvel1, qvel0) and torch.equal(warm1, warm0) and torch.equal(t1, t0)
    assert torch.equal(w.get_xy(), new)
    w.set_xy(new.cpu().numpy())  # numpy in, like the reference
    assert torch.equal(w.get_xy(), new)
    if env_id.startswith("Swimmer"):
        with pytest.raises(AttributeError):
            w.get_ori()
    else:
        ori = env.get_ori().cpu().numpy()
        q = qpos1.double().cpu().numpy()
        if env_id.startswith("Point"):
            want = q[:, 2]
        else:  # ant.py:26-35,98-103 written with explicit quaternion products
            def qmul(a, b):
                return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                                 a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3], a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]])
            want = []
            for r in q[:, 3:7]:
                o = qmul(qmul(r, [0, 1, 0, 0]), [r[0], -r[1], -r[2], -r[3]])[1:3]
                want.append(np.arctan2(o[1], o[0]))
            want = np.array(want)
        assert np.allclose(ori, want, atol=1e-12)
    env.close()


def test_single_env_facade_wrapped_env():
    env = mm.make("PointUMaze-v0")
    env.reset(seed=0)
    xy = env.wrapped_env.get_xy()
    assert isinstance(xy, np.ndarray) and xy.shape == (2,) and xy.dtype == np.float64
    env.wrapped_env.set_xy(np.array([1.5, -0.25]))
    assert np.array_equal(env.wrapped_env.get_xy(), [1.5, -0.25])
    assert isinstance(env.get_ori(), float)
    obs, r, d, info = env.step(np.zeros(2))
    assert abs(obs[0] - 1.5) < 0.2
    env.close()


def test_ant_only_options_are_refused_for_other_robots():
    """solver / diagnostic keys that only the Ant kernels read must not be accepted silently elsewhere."""
    from mujoco_maze_amd import _capi

    env = mm.make("PointUMaze-v0", num_envs=4)
    for key in ("solver_iterations", "solver_tolerance", "ls_iterations", "debug_frame_skip", "waves_per_block"):
        with pytest.raises(_capi.MazeStepError, match="Ant"):
            env.set_option(key, 1)
    env.set_option("lanes_per_env", 32)
    env.close()


@pytest.mark.parametrize("env_id,n,lanes", [("AntUMaze-v0", 256, 16), ("AntPush-v0", 128, 32)])
def test_instrumented_kernel_steps_like_the_product_kernel(torch, env_id, n, lanes):
    """The phase timers behind profiles/ come from separate instantiations of the Ant step kernel (option `profile_phases`): they must
    step like the un-instrumented kernel, and their counters must add up — per-wave totals = sum of the per-wave phases,
    totals over the waves = the global accumulators, a Newton iteration count per wave that a step can have."""
    rng = np.random.default_rng(12)
    acts = [torch.as_tensor(rng.uniform(-30, 30, (n, 8)).astype(np.float32), device="cuda") for _ in range(6)]
    outs = []
    for prof in (0, 1):
        env = mm.make(env_id, num_envs=n, force_vec=True)
        env.reset(seed=4)
        for a in acts[:3]:
            env.step(a)
        if prof:
            env.set_option("profile_phases", 1)
            env.step(acts[3])  # (the first instrumented launch zeroes nothing yet: read and drop)
            env.phase_cycles(); env.wave_cycles(n * lanes // 64); env.wave_phase_cycles(n * lanes // 64)
        else:
            env.step(acts[3])
        res = [env.step(a) for a in acts[4:]]
        outs.append([torch.cat([o, r[:, None], d[:, None].float()], 1).cpu().numpy() for o, r, d, _ in res])
        if prof:
            nw = n * lanes // 64
            glob = np.array(env.phase_cycles(), dtype=np.float64)
            tot = env.wave_cycles(nw).astype(np.float64)
            iters = env.last_wave_newton_iters.astype(np.int64)
            ph = env.wave_phase_cycles(nw).astype(np.float64)
            assert np.all(tot > 1e5) and np.all(tot < 1e8)                     # two env.steps of 20 evaluations each, per wave
            assert np.allclose(ph[:, :13].sum(1), tot)                         # per wave: phases add up to its total
            assert np.allclose(ph[:, :13].sum(0), glob[:13])                   # over the waves: the global accumulators
            assert np.all(iters >= 2 * 20) and np.all(iters <= 2 * 20 * 50)     # >= one Newton iteration per evaluation, <= the cap
            assert glob[15] == ph[:, 15].sum()
        env.close()
    for a, b in zip(*outs):  # (two instantiations: the compiler contracts their arithmetic differently — the same step to round-off, not to the bit)
        assert np.allclose(a[:, :-1], b[:, :-1], atol=1e-4, rtol=1e-5) and np.array_equal(a[:, -1], b[:, -1])

def test_kernel_timing_ring_and_its_stride(torch):
    """Options "time_kernels" / "time_kernels_stride" (bench.py's roofline.kernel_ms): HIP event pairs around the step kernel on its own
    stream, around every k-th launch only when asked — a pair around EVERY launch costs the queue ~5 us, a tenth of a Point step
    (profiles/r06/event_overhead.txt).  The sampled mean agrees with the all-launches mean; no ring -> -1."""
    env = mm.make("PointUMaze-v0", num_envs=2048, auto_reset=True)
    env.reset(seed=1)
    a = torch.zeros((2048, 2), device=env.device)
    assert env.kernel_ms() == -1.0
    for _ in range(50):
        env.step(a)
    env.set_option("time_kernels", 64)
    for _ in range(64):
        env.step(a)
    every = env.kernel_ms()
    env.set_option("time_kernels", 16)
    env.set_option("time_kernels_stride", 4)
    for _ in range(64):
        env.step(a)
    sampled = env.kernel_ms()
    assert 0.005 < every < 1.0 and 0.005 < sampled < 1.0 and abs(sampled - every) < 0.25 * every, (every, sampled)
    with pytest.raises(Exception):
        env.set_option("time_kernels_stride", 0)
    env.close()
