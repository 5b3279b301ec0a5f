"""The planar ladder, rung by rung: point_ladder / swimmer_ladder of csrc/planar_kernels.hip turn a handle into one instantiation
(NB, NS, G) of the Point kernels or (NL, NB, G) of the chain kernels, and the step kernel, the open-loop fused kernel, the policy
kernels and the reset all launch what it picks.  The other GPU modules run the rungs of the registered UMaze / Push / Billiard ids;
this one runs the fused and policy kernels on the rest (DESIGN.md section 3.6 holds the table of rungs and tests):

    Point   (0, 0, 8)   PointUMaze-v0 + lanes_per_env = 8        chains  (2, 2, 4)  ReacherPush-v1
            (2, 0, 64)  PointMultiPush-v0                                (4, 0, 4)  user MJCF chain of 4 links
            (3, 0, 64)  PointPushMaze-v0                                 (5, 0, 8)  ... of 5 links
                                                                         (6, 0, 8)  ... of 6 links

Every test first asserts, from the model constants and launch_info(), that it is on the rung it names (`_on_rung`).
launch_info()["lanes_per_env"] is the G of the instantiation the ladder picks (mzk_planar_lanes runs the ladder), not the value of
the rule the ladder reads: the rungs of one family return the same fp32 bits on all but a vanishing share of states (float64
arithmetic, fp32 state), so a ladder that sent 8 lanes to the 16-lane kernel would show nowhere else.

The comparisons are those of the neighbouring modules and nothing is looser: bit equality with the stepping twin (_twin_check of
tests/test_gpu_rollout.py, _transitions_check of tests/test_gpu_transitions.py) and with mujoco_maze_amd.policy's numpy model where
that model is exact (ReLU networks without squash, critics, the normaliser); the suite's 1e-5 where the device's libm enters (a
sampled, squashed action: policy.py, "differs from the device by libm ulps only").

Two rungs of swimmer_ladder — (3, 3, 4) and (2, 3, 4), a chain beside a block on three slides — are not run here because no handle
reaches them: such a model (Swimmer / Reacher with a custom MultiFall task; no registered id has one) is stepped by the general
engine (gen_model_needs_general_engine, csrc/generic_dyn.h).  test_three_slide_block_chains_run_on_the_general_engine holds that."""
import numpy as np
import pytest

import mujoco_maze_amd as mm
from mujoco_maze_amd import policy
from tests.test_gpu_deep_policy import _actor as _deep_actor
from tests.test_gpu_deep_policy import _critic as _deep_critic
from tests.test_gpu_env_isolation import CORNER_POINTS
from tests.test_gpu_parity import _f32
from tests.test_gpu_policy_rollout import ACTION_SCALE, _current_obs
from tests.test_gpu_policy_sample import SEED, STEP0
from tests.test_gpu_rollout import _actions, _near_goal, _same, _twin_check
from tests.test_gpu_transitions import _setup, _transitions_check, _value
from tests.test_mjcf import chain_swimmer_xml

pytestmark = pytest.mark.gpu
N = 130     # no multiple of the envs per wave (8, 2, 1 for the Point at 8, 32, 64 lanes) or per workgroup (64, 32 for the chains)
RESET_SEED = 11  # the default of _twin_check and _transitions_check


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


# ---------------------------------------------------------------------------------------------- 0. the rungs
def _point_rung(env_id, lanes=None):
    def make(n, **kw):
        env = mm.make(env_id, num_envs=n, **kw)
        if lanes:
            env.set_option("lanes_per_env", lanes)
        return env
    return make


def _user_chain(nlink):
    return lambda n, **kw: mm.make("SwimmerUMaze-v0", num_envs=n, robot_xml=chain_swimmer_xml(nlink), **kw)


# name -> (make(n, **kw), family, (a, b, G)): Point (NB blocks, NS balls, G lanes per env), chain (NL links, NB block slides, G)
RUNGS = {
    "point-0-0-8": (_point_rung("PointUMaze-v0", 8), "point", (0, 0, 8)),
    "point-0-0-16": (_point_rung("PointUMaze-v0", 16), "point", (0, 0, 16)),
    "point-0-0-32": (_point_rung("PointUMaze-v0", 32), "point", (0, 0, 32)),
    "point-1-0-32": (_point_rung("PointPush-v0"), "point", (1, 0, 32)),
    "point-2-0-64": (_point_rung("PointMultiPush-v0"), "point", (2, 0, 64)),
    "point-3-0-64": (_point_rung("PointPushMaze-v0"), "point", (3, 0, 64)),
    "point-0-1-32": (_point_rung("PointBilliard-v0"), "point", (0, 1, 32)),
    "chain-3-0-4": (lambda n, **kw: mm.make("SwimmerUMaze-v0", num_envs=n, **kw), "chain", (3, 0, 4)),
    "chain-2-0-4": (lambda n, **kw: mm.make("ReacherUMaze-v0", num_envs=n, **kw), "chain", (2, 0, 4)),
    "chain-3-2-4": (lambda n, **kw: mm.make("SwimmerPush-v0", num_envs=n, **kw), "chain", (3, 2, 4)),
    "chain-2-2-4": (lambda n, **kw: mm.make("ReacherPush-v1", num_envs=n, **kw), "chain", (2, 2, 4)),
    "chain-3-2-4-fall": (lambda n, **kw: mm.make("SwimmerFall-v0", num_envs=n, **kw), "chain", (3, 2, 4)),
    "chain-2-2-4-fall": (lambda n, **kw: mm.make("ReacherFall-v0", num_envs=n, **kw), "chain", (2, 2, 4)),
    "chain-4-0-4": (_user_chain(4), "chain", (4, 0, 4)),
    "chain-5-0-8": (_user_chain(5), "chain", (5, 0, 8)),
    "chain-6-0-8": (_user_chain(6), "chain", (6, 0, 8)),
}
POINT_NEW = ["point-0-0-8", "point-2-0-64", "point-3-0-64"]       # no fused or policy kernel of these ran in a test
CHAIN_NEW = ["chain-4-0-4", "chain-5-0-8", "chain-6-0-8"]


def _on_rung(env, name):
    """the env is on the rung `name`: model constants, lane count, the family's specialised engine, fused rollouts"""
    _, family, want = RUNGS[name]
    m, li = env.model.c, env.launch_info()
    assert li["engine"] == 0 and li["rollout_fused"] == 1, (name, li)
    if family == "point":
        assert m.nv == 3 + 2 * m.nblock + 3 * m.nball, (name, m.nv)
        got = (m.nblock, m.nball, li["lanes_per_env"])
    else:
        slides = m.body_jntnum[m.block_bodyid[0]] if m.nblock else 0
        links = m.nbody - 1 - m.nblock
        assert m.nblock <= 1 and m.nv == links + 2 + slides, (name, m.nv)
        got = (links, slides, li["lanes_per_env"])
    assert got == want, (name, got, want)


def _make(name, **kw):
    def make():
        env = RUNGS[name][0](N, **kw)
        _on_rung(env, name)
        return env
    return make


@pytest.mark.parametrize("name", list(RUNGS))
def test_every_rung_has_a_constructor(torch, name):
    env = RUNGS[name][0](N)
    try:
        _on_rung(env, name)
        if name.endswith("fall"):  # the z slide, pulled by gravity, is what sets these apart from the Push rung of the same arguments
            m = env.model.c
            j0 = m.body_jntadr[m.block_bodyid[0]]
            assert [int(np.argmax(np.abs(m.jnt_axis[j0 + a]))) for a in range(2)] == [1, 2]
    finally:
        env.close()


@pytest.mark.parametrize("cls,nv", [(mm.SwimmerEnv, 8), (mm.ReacherEnv, 7)], ids=["swimmer", "reacher"])
def test_three_slide_block_chains_run_on_the_general_engine(torch, cls, nv):
    """swimmer_ladder has rungs (3, 3, 4) and (2, 3, 4) for a block on three slides.  The only mazes with one are MultiFall's (a custom
    task for these robots: the registered Swimmer / ReacherMultiFall-v2 is built on the Fall maze), and mz_create sends such a model
    to the general engine: no handle launches those two rungs, so there is nothing of them to pin — this test fails the day one does."""
    from mujoco_maze_amd.maze_env import VecMazeEnv
    from mujoco_maze_amd.maze_task import GoalRewardMultiFall
    from mujoco_maze_amd.model import needs_general_engine

    env = VecMazeEnv(cls, GoalRewardMultiFall, num_envs=N, maze_size_scaling=4.0)
    try:
        m, li = env.model.c, env.launch_info()
        assert m.nv == nv and m.nblock == 1 and m.body_jntnum[m.block_bodyid[0]] == 3
        assert needs_general_engine(env.model) and li["engine"] == 1 and li["rollout_fused"] == 0, li
    finally:
        env.close()


def test_bare_point_crowded_corners_at_every_lane_count(torch, oracle):
    """More contacts than a row of lanes holds, at the three lane counts of the bare Point: a lane of the 8-lane rung owns contacts
    l, l + 8, l + 16 (SW = 8 in csrc/point_bare.h: its later slots are read from LDS as soon as one env of the wave has more than 8), a
    lane of the 16- and 32-lane rungs l and l + 16.  Envs deep inside an inner corner of the U (17 contacts by the oracle's count) sit
    in one batch with free ones: the default handle returns the 16-lane rung's bits (it is that instantiation), and the three rungs —
    the same float64 arithmetic on the same fp32 state, summed in another order — agree within the bare Point's parity bar
    (1e-6 + 2e-7 |x|, test_point_step_parity_and_bounce)."""
    n = 256
    envs = {g: RUNGS[f"point-0-0-{g}"][0](n) for g in (8, 16, 32)}
    envs[0] = mm.make("PointUMaze-v0", num_envs=n)
    try:
        for g in (8, 16, 32):
            _on_rung(envs[g], f"point-0-0-{g}")
        assert envs[0].launch_info()["lanes_per_env"] == 16
        cm = envs[0].model
        rng = np.random.default_rng(41)
        xmin, xmax, ymin, ymax = cm.world.xy_limits()
        qpos = np.stack([rng.uniform(xmin, xmax, n), rng.uniform(ymin, ymax, n), rng.uniform(-3.2, 3.2, n)], 1)
        for k in range(n // 2):  # half of the batch: the 17-contact corner states, jittered at 1e-3 (the count may drop by a few)
            qpos[k] = np.array(CORNER_POINTS[k % len(CORNER_POINTS)]) + (rng.uniform(-1e-3, 1e-3, 3) if k >= len(CORNER_POINTS) else 0.0)
        st = _f32(dict(qpos=qpos, qvel=np.zeros((n, 3)), warm=np.zeros((n, 3)), t=np.zeros(n, np.int32)))
        act = np.zeros((n, 2), np.float32)  # no teleport: the step is the contact solve alone
        nc = oracle.forward(cm, st["qpos"], st["qvel"])["counts"][:, 0].astype(int)
        assert (nc > 8).sum() >= n // 4 and (nc > 16).sum() >= len(CORNER_POINTS) and (nc == 0).sum() > 0, np.bincount(nc)
        out, status = {}, {}
        for g, env in envs.items():
            env.set_state(st["qpos"], st["qvel"], None, st["t"])
            env.status()
            obs, *_ = env.step(torch.as_tensor(act, device=env.device))
            status[g] = env.status().cpu().numpy().copy()
            out[g] = obs.cpu().numpy().copy()
        ref = oracle.step(cm, st, act.astype(np.float64), nthreads=8)
        bits = lambda a: a.view(np.int32)
        assert np.array_equal(bits(out[0]), bits(out[16])) and np.array_equal(status[0], status[16])
        for g in (8, 32):
            print(f"{g} lanes: {int((bits(out[g]) != bits(out[16])).any(1).sum())} of {n} envs differ from the 16-lane bits; "
                  f"max |obs - oracle| = {np.abs(out[g] - ref['obs']).max():.3e}, status words {np.unique(status[g])}, oracle's {np.unique(ref['status'])}")
            assert np.all(np.abs(out[g].astype(np.float64) - out[16]) <= 1e-6 + 2e-7 * np.abs(out[16])), g
            assert np.array_equal(status[g], status[16]), g
    finally:
        for env in envs.values():
            env.close()


# ---------------------------------------------------------------------------------------------- 2. open-loop fused rollout = stepping
@pytest.mark.parametrize("name", POINT_NEW)
def test_point_fused_rollout_equals_stepping(torch, name):
    """130 envs (idle groups in the last wave), auto-reset, K = 260 across the 256-step launch split, a 40-step time limit (six per env);
    every fourth env starts in front of the goal and all drive ahead, into walls and — on the two block mazes — into the blocks"""
    la, lb, want = _twin_check(_make(name, auto_reset=True, seed=5, max_episode_steps=40), 260, point=True, expect_done=True)
    assert int((want["done"] & 2).sum()) > 0 and int((want["done"] & 1).sum()) > 0  # time limits and goals
    assert torch.isfinite(want["obs"]).all()
    nb = RUNGS[name][2][0]
    if nb:  # the block solver was busy: some block left its spawn position by more than 5 cm (obs = robot 0:3, block k xyz at 3 + 3k)
        xy = torch.cat([want["obs"][:, :, 3 + 3 * k: 5 + 3 * k] for k in range(nb)], dim=2)
        assert int(((xy - xy[0, :1]).abs().amax(dim=(0, 2)) > 0.05).sum()) > N // 4


@pytest.mark.parametrize("name", CHAIN_NEW + ["chain-2-2-4"])
def test_chain_fused_rollout_equals_stepping(torch, name):
    """as above for the chains; ReacherPush-v1's rows are non-finite from the first step (below) — its finite comparison is
    test_chain_with_a_block_at_rest"""
    la, lb, want = _twin_check(_make(name, auto_reset=True, seed=5, max_episode_steps=40), 260, expect_done=True)
    assert int((want["done"] != 0).sum(dim=0).min()) >= 6
    if RUNGS[name][2][1] == 0:
        assert torch.isfinite(want["obs"]).all()


@pytest.mark.parametrize("name", ["chain-3-2-4-fall", "chain-2-2-4-fall"])
def test_chain_beside_a_falling_block_patterns_only(torch, oracle, name):
    """SwimmerFall-v0 / ReacherFall-v0: the (NL, 2, 4) rungs with a (y, z) block, limit rows on the slides and gravity on z.  The
    reset's velocity noise on a block of this medium blows up within the first step (by design, the reference
    does the same), and a block on a z slide moves under gravity whatever its velocity is set to, so no injected state keeps the rows
    finite: the float64 oracle is asked here, and every env's row is non-finite after the first step of an episode.  What the bit
    comparison with the stepping twin then carries: the NaN patterns of every row (`_same` compares bits), t and the flags (time
    limits, six per env), the rewards' bits, and each episode's finite FIRST row — the reset's draw by seed, episode and slot, written
    by the fused kernel's in-step reset.  The finite arithmetic of the (NL, 2, 4) rungs is compared in test_chain_with_a_block_at_rest."""
    env = RUNGS[name][0](N)
    try:
        _on_rung(env, name)
        cm = env.model
    finally:
        env.close()
    st, _ = oracle.reset(cm, N, RESET_SEED)
    ref = oracle.step(cm, st, np.zeros((N, cm.c.nu)), nthreads=8)
    assert not np.isfinite(ref["obs"]).all(axis=1).any()  # the oracle: no env has a finite row after one step
    la, lb, want = _twin_check(_make(name, auto_reset=True, seed=5, max_episode_steps=40), 260, expect_done=True)
    obs, done = want["obs"], want["done"]
    assert int((done != 0).sum(dim=0).min()) >= 6
    first = done != 0  # under auto-reset the row of a terminal step is the next episode's first observation
    assert int(first.sum()) > 0 and torch.isfinite(obs[first]).all()
    assert not torch.isfinite(obs[~first]).all(dim=-1).any()


# ---------------------------------------------------------------------------------------------- 3. chains with a block at rest
def _block_at_rest(env):
    """zero the block's velocity columns (behind the chain's links + 2) on every env"""
    m = env.model.c
    links = m.nbody - 1 - m.nblock
    qpos, qvel, warm, t = env.get_state()
    qvel[:, links + 2:] = 0.0
    env.set_state(qvel=qvel)


@pytest.mark.parametrize("name", ["chain-3-2-4", "chain-2-2-4"])
def test_chain_with_a_block_at_rest(torch, name):
    """SwimmerPush-v0 / ReacherPush-v1 with the block's reset velocity zeroed (a force-free block then stays where it is), no
    auto-reset and no time limit inside the window: by the float64 oracle every row stays finite and no status bit is set for 64
    random steps.  That is asserted first, on a stepping env's own rows — the twin's state, the twin's actions — before anything is
    compared; then the open-loop kernel, the legacy deterministic policy kernel and the SMP + CRT one go against their defining
    loops by bits, on finite numbers (asserted again on each loop's rows)."""
    K = 45
    make = _make(name, auto_reset=False, seed=5, max_episode_steps=1000)
    env = make()
    try:
        env.reset(seed=RESET_SEED)
        _block_at_rest(env)
        env.status()  # (cleared on read)
        acts = _actions(env, K, RESET_SEED + 1)  # what _twin_check steps its first env with
        rows = torch.stack([env.step(acts[k])[0].clone() for k in range(K)])
        assert torch.isfinite(rows).all(), "the stepping env's rows are not finite: the comparisons below would pass on NaN patterns"
        status = env.status()
        assert int((status != 0).sum()) == 0, status.unique()
    finally:
        env.close()
    la, lb, want = _twin_check(make, K, after_reset=_block_at_rest)
    assert _same(want["obs"], rows)  # the rows asserted finite above are the twin's
    for mode in ("deterministic", "sampled-critic"):
        loop, out, li, _ = _transitions_check(make, K, mode, after_reset=_block_at_rest, expect_done=False)
        assert torch.isfinite(loop["obs"]).all() and torch.isfinite(loop["act"]).all() and torch.isfinite(out[3]["next_observations"]).all(), mode


# ---------------------------------------------------------------------------------------------- 4. closed-loop kernels at G = 8, 64, 4
def _bind(torch, norm):
    """the `prepare` of tests/test_gpu_transitions.py test_the_critic_values_the_rows_returned; norm[id(env)] = (mean, inv_std)"""
    def prepare(env):
        rng = np.random.default_rng(3)
        m = torch.as_tensor(rng.normal(0.0, 0.3, env.obs_dim).astype(np.float32), device=env.device)
        s = torch.as_tensor(rng.uniform(0.5, 2.0, env.obs_dim).astype(np.float32), device=env.device)
        env.bind_obs_norm(m, s, 1.5)
        norm[id(env)] = (m, s)
    return prepare


CLIP = 1.5
KW = dict(auto_reset=True, seed=5, max_episode_steps=20)
K4 = 45


def _start(env, point, prepare):
    """the rows a check of this section starts from, on a fresh env: _transitions_check's preparation"""
    if prepare:
        prepare(env)
    o = env.reset(seed=RESET_SEED)
    if point:
        _near_goal(env, o)
        _current_obs(env)
    return env._obs.clone()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _rows_before(obs0, seq):
    """the row each step's networks read: the start, then the row the step before left (under auto-reset the new episode's first)"""
    return np.concatenate([obs0[None], seq[:-1]], axis=0)


@pytest.mark.parametrize("name", POINT_NEW + CHAIN_NEW)
def test_legacy_policy_kernel_equals_the_defining_loop(torch, name):
    """no flag set: one tanh layer of 5 units per env — a partial pass of the hidden loop at G = 4 and 8, idle lanes at 64"""
    point = RUNGS[name][1] == "point"
    rows, out, li, _ = _transitions_check(_make(name, **KW), K4, "deterministic", point=point, net="tanh5")
    assert torch.isfinite(rows["act"]).all() and torch.isfinite(rows["obs"]).all()
    assert int((rows["done"] & 2).sum()) > 0 and (not point or int((rows["done"] & 1).sum()) > 0)


@pytest.mark.parametrize("bound", [False, True], ids=["raw", "obs-norm"])
@pytest.mark.parametrize("name", POINT_NEW + CHAIN_NEW)
def test_relu64_actor_critic_kernel_equals_the_loop_and_the_numpy_model(torch, name, bound):
    """SMP + CRT + DEEP (+ NRM with a normaliser bound, + EXT on the return_next_obs leg), 64-64 ReLU per env: 16 / 8 / 1 passes of
    every `j += G` loop of csrc/mz_policy.h at G = 4 / 8 / 64, and obs_dim 15 / 17 > G on the long chains.

    1. the call against its defining loop and against the same call without next_observations, by bits (_transitions_check);
    2. value(next_observations[k]) is next_values[k] on a fresh env (the closing check of test_the_critic_values_the_rows_returned);
    3. a twin that runs the same device function cannot see an error both share, so the call also goes against
       mujoco_maze_amd.policy on the rows the call itself returned — with a normaliser bound on normalize_reference of the raw row:
       values and next_values by bits (a ReLU critic has no libm in it: policy.py), the sampled, squashed actions within the
       suite's 1e-5 of sample_reference (its eps, exp and tanh are float64 libm rounded to float32, the device's are its own:
       "differs from the device by libm ulps only" — the bar of tests/test_gpu_transitions.py test_action_noise_against_the_model for
       squashed networks).  The bit comparison of a whole actor is the next test's.

    chain-6-0-8: a six-link chain's closed-loop plans run the driver's defining loop (rollout_run, csrc/mazestep.hip): two fused
    instantiations of swimmer_policy_rollout_kernel<6, 0, 8, ...> — this test's [obs-norm] case and the next test's [raw] case — left
    the loop behind the first step (env 0: first actuated hinge 1.1414 against 0.1066; 5460 of 45 x 130 action rows differed) while
    the step kernel agreed with the oracle.  The cases stay: they hold whatever path those plans take to the loop and to numpy."""
    point = RUNGS[name][1] == "point"
    norm = {}
    prepare = _bind(torch, norm) if bound else None
    make = _make(name, **KW)
    rows, out, li, crt = _transitions_check(make, K4, "sampled-critic", point=point, net="relu64", critic="relu64", prepare=prepare)
    assert li["obs_norm"] == int(bound)
    assert int((rows["done"] & 2).sum()) > 0 and (not point or int((rows["done"] & 1).sum()) > 0)
    info = out[3]
    env = make()
    try:
        obs0 = _start(env, point, prepare).cpu().numpy()
        nxt, nv = info["next_observations"], info["next_values"]
        for k in range(K4):
            assert _same(_value(env, crt, nxt[k].contiguous()), nv[k].contiguous()), k
        pol, crt2, _ = _setup("sampled-critic", env, point, RESET_SEED + 1, "relu64", "relu64")  # the networks of the check: same seeds
        assert _same(crt2["value_params"], crt["value_params"])
        mean, inv_std = (t.cpu().numpy() for t in norm[id(env)]) if bound else (None, None)
    finally:
        env.close()
    seen = lambda x: policy.normalize_reference(x, mean, inv_std, CLIP) if bound else x
    par, vpar = pol["params"].cpu().numpy(), crt["value_params"].cpu().numpy()
    before = _rows_before(obs0, info["observations"].cpu().numpy())
    assert np.isfinite(before).all()
    act, val = info["actions"].cpu().numpy(), info["values"].cpu().numpy()
    nxt, nv = nxt.cpu().numpy(), nv.cpu().numpy()
    worst = 0.0
    for k in range(K4):
        x = seen(before[k])
        assert np.array_equal(_bits(val[k]), _bits(policy.value_reference(vpar, x, (64, 64), activation="relu"))), k
        assert np.array_equal(_bits(nv[k]), _bits(policy.value_reference(vpar, seen(nxt[k]), (64, 64), activation="relu"))), k
        ra, rl = policy.sample_reference(par, x, env.nu, (64, 64), squash=True, action_scale=ACTION_SCALE, noise_seed=SEED, noise_step=STEP0 + k,
                                         slots=np.arange(N), activation="relu")
        err = np.abs(act[k].astype(np.float64) - ra).max()
        worst = max(worst, err)
        assert err <= 1e-5, (k, err)
    print(f"{name} obs-norm {bound}: max |device action - sample_reference| over {K4} steps = {worst:.3e}")


@pytest.mark.parametrize("bound", [False, True], ids=["raw", "obs-norm"])
@pytest.mark.parametrize("name", POINT_NEW + CHAIN_NEW)
def test_relu64_policy_kernel_against_the_numpy_model_by_bits(torch, name, bound):
    """CRT + DEEP (+ NRM): a deterministic 64-64 ReLU actor WITHOUT squash and a 64-64 ReLU critic, one network per env.  ReLU is a
    select and the output is the plain sum, so policy.reference / value_reference equal the device bit for bit (policy.py): row k of
    info["actions"] is the model's action for the row the step read, info["values"] / ["next_values"] the model's values — an
    independent evaluation of every unit, in index order, of what the strided lane loops of mz_policy.h computed."""
    point = RUNGS[name][1] == "point"
    norm = {}
    prepare = _bind(torch, norm) if bound else None
    env = _make(name, **KW)()
    try:
        obs0 = _start(env, point, prepare).cpu().numpy()
        pol = _deep_actor(env, True, (64, 64), "relu", False, 31, False, drive=point)
        crt = _deep_critic(env, True, (64, 64), "relu", 32)
        obs, rew, done, info = env.rollout_policy(steps=K4, return_obs=True, return_actions=True, return_next_obs=True, **pol, **crt)
        torch.cuda.synchronize()
        assert env.launch_info()["obs_norm"] == int(bound)
        mean, inv_std = (t.cpu().numpy() for t in norm[id(env)]) if bound else (None, None)
        nu = env.nu
        assert int((done & 2).sum()) > 0
    finally:
        env.close()
    seen = lambda x: policy.normalize_reference(x, mean, inv_std, CLIP) if bound else x
    par, vpar = pol["params"].cpu().numpy(), crt["value_params"].cpu().numpy()
    before = _rows_before(obs0, info["observations"].cpu().numpy())
    assert np.isfinite(before).all()
    act, val, nv, nxt = (info[k].cpu().numpy() for k in ("actions", "values", "next_values", "next_observations"))
    assert np.abs(act).max() > 0.1
    for k in range(K4):
        x = seen(before[k])
        assert np.array_equal(_bits(act[k]), _bits(policy.reference(par, x, nu, (64, 64), activation="relu"))), k
        assert np.array_equal(_bits(val[k]), _bits(policy.value_reference(vpar, x, (64, 64), activation="relu"))), k
        assert np.array_equal(_bits(nv[k]), _bits(policy.value_reference(vpar, seen(nxt[k]), (64, 64), activation="relu"))), k


@pytest.mark.parametrize("name", ["point-0-0-8", "point-2-0-64"])
def test_action_noise_at_8_and_64_lanes(torch, name):
    """noise="action" (honoured by the EXT instantiations), as ACTION_CASES' last row of tests/test_gpu_transitions.py: 64-64 ReLU actor
    and critic, a normaliser bound; one rung per new group width"""
    norm = {}
    rows, out, li, _ = _transitions_check(_make(name, **KW), K4, "sampled-critic", point=True, net="relu64", critic="relu64", prepare=_bind(torch, norm),
                                          noise="action", third=False)
    assert li["rollout_fused"] == 1 and li["obs_norm"] == 1
    assert torch.isfinite(rows["act"][0]).all() and float(rows["act"].abs().max()) <= 0.9  # ACTION_SCALE of the helpers: the clip
