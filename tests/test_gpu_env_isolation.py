"""Env isolation: what an env computes depends on its own state, action, seed and global slot — never on its batch-mates.

Every kernel packs several envs into one wavefront (8, 4 or 2 for the bare Point, 8, 4 or 2 for the Ant, 16 for the Swimmer and Reacher; the chains
also 64 into one workgroup, the Ant 2 or 4 waves) and takes wave-uniform shortcuts: `cx.any(ncon > SW)` in point_bare.h, the
contact-slot guards and the wave-uniform Newton count of ant_newton_rows.h, `gballot` in planar_dyn.h, the in-kernel auto-reset of
only some lanes.  tests/test_gpu_ant_slot_guards.py holds the contract for the Ant row solver at 16 lanes; this module holds it for
every engine.  Every assertion is a bit-equality or a precondition derived from the float64 oracle: there is no tolerance.

(a) wave-mate independence, one step: arrangement B = A permuted by i -> (i % W) * e + i // W (e envs per wave, W >= e waves: the e
    envs of a wave of A land in e different waves of B), states and actions permuted alike — every output and the read-back state
    of each env bit-equal; and the same step twice from the same state.  Asserted from the oracle's counts alone: a wave of A mixes
    a least-loaded env with one at the batch's maximum, another holds least-loaded envs only.  The count is the oracle's contact
    count — for the chains, which have no contacts, its constraint-row count (joint limits; some hinges are put beyond theirs) —,
    and "least loaded" is zero wherever an env can have no contact at all; in a maze with a movable body every env carries that
    body's resting contacts (four corners of a block, one of a ball) and the least load is that.  The bare Point also holds envs
    with more contacts than a lane has register slots (> 16: deep inside an inner corner, the arrow across the walls).
    For the chains' workgroups (64 envs, 4 of them at N = 256) "no two envs share one in both arrangements" cannot hold — 64 envs
    fall into 4 workgroups — so the assertion is the most that can: every workgroup of A is spread evenly over all of B's.
(b) slot independence across auto-reset: two envs of the same N and options, the same reset seed, `env_index_offset` 0 (A) and 3 (B,
    no multiple of any envs-per-wave): after the reset and at every step of step() / rollout() / rollout_policy() — across time
    limits, goal terminations and the 256-step launch split — B[j] is bit-equal to A[j + 3].
(c) a NaN wave-mate: arrangement P = A of (a) with one robot velocity of the first env of every second wave set to NaN (the only
    poison that goes to a device here; Inf and huge values belong to tests/test_diverged_states.py on the CPU).  Every unpoisoned
    env is bit-equal to its result in A and gains no status bit, every poisoned env carries MZ_STATUS_BAD_STATE; in a fused
    auto-reset rollout the poisoned envs are finite again after their first time-limit reset and from then on bit-equal to A's.
    Reading the device-only paths for state-derived loop bounds and indices (ant_forward_rows.h, ant_newton_rows.h, the
    __HIP_DEVICE_COMPILE__ branches of point_bare.h, planar_kernels.hip, ant_kernels.hip, generic_kernels.hip): every Newton loop is
    capped by an iteration count (max_iter; 50 in point_bare.h / planar_dyn.h) next to its wave-uniform `any(!done)`, so a NaN that
    never converges costs its wave the cap, not more; contact loops run to staged counts clamped to the buffers (CAP, NC, <= 4 deep
    jobs); cell indices go through mz_cell, or — ant_forward_rows.h, the plain ant's geom_contacts — through the device's
    saturating conversion into loops bounded by themselves and reads that check their index (comments there); the kernels' own
    indices come from threadIdx / blockIdx and the env count.  NaN converts to cell 0, a cell of the grid: no loop bound there.
    The lane-group path of csrc/ant_dyn.h (rows ant8 and antmultipush16: ant_forward's last block and ant_solve; 8-lane groups and
    ants with two or more movable bodies), read the same way: the Newton loop is `while (cx.any(!done) && it < K.max_iter)`, the
    line search `for (ls < ls_max)` with ls_max one of two options; every loop over contacts runs to s.ncon or between s.cbeg[]
    entries, and every writer of those clamps to NC (con_map_item, con_fill_item: `tot > NC`, `off < NC ? off : NC`); con_map_item's
    loop over a geom's count writes only `slot < NC`, con_enum_item's staging only `n < MZ_STAGE`, con_fill_item only
    `slot < NC && slot < end` — and a geom's count is its number of emits, which the enumerators bound by themselves: constant
    trip counts (four corners, two capsule ends, two layers, bb.nu / bb.nv of 1 or 2, the blocks below e) around cell ranges that
    come from mz_cell (a block's own cell part, the ball's and a robot geom's bounding square for NB > 0: NaN gives -2, a range is
    at most MZ_MAX_GRID + 4 long, cells off the grid are skipped before a row is read) — the plain ant's robot geoms take the
    saturating conversion described above at every width.  The torso's broad phase (kin_item) is a fixed 3 x 3 ring around an
    mz_cell.  The kind / block / partner codes a contact row decodes are integers the enumerator wrote, never state.  No site
    needed a fix."""
import numpy as np
import pytest

import mujoco_maze_amd as mm
from mujoco_maze_amd import policy
from tests.test_gpu_ant_slot_guards import NAMES
from tests.test_gpu_parity import _f32, _rollout_states
from tests.test_gpu_rollout import FUSED_IDS, _actions, _same

pytestmark = pytest.mark.gpu

ALL_NAMES = NAMES + ("goal_index", "info")
BAD_STATE = 1

# (a): id, options, N, lanes per env, keywords of mm.make
ROWS = {
    # eight envs per wave, SW = 8 register slots per lane (point_bare.h); 128 envs: the oracle counts 24 envs without a contact there (arrangement
    # A needs 15), W = 16 waves >= e = 8
    "point8": ("PointUMaze-v0", {"lanes_per_env": 8}, 128, 8, {}),
    "point16": ("PointUMaze-v0", {"lanes_per_env": 16}, 64, 16, {}),
    "point32": ("PointUMaze-v0", {"lanes_per_env": 32}, 64, 32, {}),
    "pointpush": ("PointPush-v0", {}, 32, 32, {}),
    "pointbilliard": ("PointBilliard-v0", {}, 32, 32, {}),
    "antpush": ("AntPush-v0", {}, 32, 32, {}),
    "ant16wpb2": ("AntUMaze-v0", {"lanes_per_env": 16, "waves_per_block": 2}, 64, 16, {}),
    "ant16wpb4": ("AntUMaze-v0", {"lanes_per_env": 16, "waves_per_block": 4}, 64, 16, {}),
    "swimmer": ("SwimmerUMaze-v0", {}, 256, 4, {}),
    "reacher": ("ReacherUMaze-v0", {}, 256, 4, {}),
    "swimmerpush": ("SwimmerPush-v0", {}, 256, 4, {}),
    # the plain ant with eight envs per wave (the lane-group solver of csrc/ant_dyn.h: 8-lane groups run no row solver), and with two
    "ant8": ("AntUMaze-v0", {"lanes_per_env": 8}, 128, 8, {}),
    "ant32": ("AntUMaze-v0", {"lanes_per_env": 32}, 64, 32, {}),
    # ants with movable bodies that SHARE a wave: four / two envs of the lane-group solver (ant_solve: `while (cx.any(!done) ...)`
    # keeps a converged env beside its mates' iterations; the re-enumeration on s.con_over runs for some lanes of a wave only).  At
    # their default of 64 lanes these kernels have a wave per env.  Oracle counts of the recipe below (N = 64, by maze and scale):
    # MultiPush at 2: least 8 (two blocks at rest) on 36 envs, maximum 21; MultiFall: 4 on 34, 17; SmallBilliard: 1 on 35, 4.
    # (PushMaze at scale 2 has 3 least-loaded envs, 7 needed: it would be a row at scale 8 only — 48 on 38 envs, maximum 52.)
    "antmultipush16": ("AntMultiPush-v0", {"lanes_per_env": 16}, 64, 16, {"maze_size_scaling": 2.0}),
    "antmultipush32": ("AntMultiPush-v0", {"lanes_per_env": 32}, 64, 32, {"maze_size_scaling": 2.0}),
    "antbilliard16": ("AntSmallBilliard-v0", {"lanes_per_env": 16}, 64, 16, {}),
    "antmultifall16": ("AntMultiFall-v0", {"lanes_per_env": 16}, 64, 16, {}),
    # four waves per workgroup: launch_ant_step halves the workgroup until its LDS fits (test_waves_per_block_changes_no_bit)
    "antmultipush16wpb4": ("AntMultiPush-v0", {"lanes_per_env": 16, "waves_per_block": 4}, 64, 16, {"maze_size_scaling": 2.0}),
}
# Points deep inside an inner corner of the U (x = -2 / 10, y = -2 / 10 are wall faces), arrow across the walls: the oracle counts
# 17 contacts for each (fp32-exact values, found by a random search around the corners on the CPU)
CORNER_POINTS = [(-1.9416821002960205, 10.233589172363281, 4.067603588104248), (-2.178309202194214, 1.9360370635986328, 0.5767877697944641),
                 (-2.158874750137329, -1.9991836547851562, 5.6541314125061035), (-2.2772014141082764, 6.082178115844727, 5.6927289962768555),
                 (10.168045043945312, -1.8621466159820557, 3.792480945587158), (-1.9346132278442383, 2.2694833278656006, 4.1465349197387695)]


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def _regroup(w, e):
    """arrangement A -> B for e w envs in w waves of e: the env at index i of A sits at index (i % w) * e + i // w of B"""
    assert w >= e
    i = np.arange(e * w)
    return (i % w) * e + i // w


def _ctrl_range(m):
    return np.array([m.act_ctrlrange[a][0] for a in range(m.nu)]), np.array([m.act_ctrlrange[a][1] for a in range(m.nu)])


def _chain_states(oracle, cm, n, seed, steps):
    """the oracle's reset plus `steps` random-action steps of a Swimmer / Reacher batch, as fp32-representable float64"""
    rng = np.random.default_rng(seed)
    st, _ = oracle.reset(cm, n, seed)
    lo, hi = _ctrl_range(cm.c)
    for _ in range(steps):
        oracle.step(cm, st, rng.uniform(lo, hi, (n, cm.c.nu)), nthreads=8)
    return _f32(st)


def build_case(oracle, cm, key):
    """CPU only: (start state of arrangement A, actions, oracle counts, least load) of row `key` — preconditions asserted here"""
    env_id, _, n, lanes, _ = ROWS[key]
    e = 64 // lanes
    m = cm.c
    rng = np.random.default_rng(17)
    lo, hi = _ctrl_range(m)
    chain = env_id.startswith(("Swimmer", "Reacher"))
    if chain:
        st = _chain_states(oracle, cm, n, 3, 30)
        # hinges beyond their limits: every eighth env its first hinge past the upper bound, every sixteenth the last one below the lower
        nh = m.nu
        for j, sel in ((0, np.arange(n) % 8 == 5), (nh - 1, np.arange(n) % 16 == 9)):
            jid = 3 + j  # joints: slide x, slide y, the root's hinge, then the actuated hinges
            assert m.jnt_type[jid] == 3 and m.jnt_limited[jid]
            st["qpos"][sel, m.jnt_qposadr[jid]] = (m.jnt_range[jid][1] + 0.05) if j == 0 else (m.jnt_range[jid][0] - 0.08)
        st["qpos"] = st["qpos"].astype(np.float32).astype(np.float64)
        beyond = np.zeros(n, bool)
        for jid in range(3, 3 + nh):
            q = st["qpos"][:, m.jnt_qposadr[jid]]
            beyond |= (q > m.jnt_range[jid][1]) | (q < m.jnt_range[jid][0])
        assert beyond.sum() >= n // 8, beyond.sum()
    elif env_id.startswith("Ant"):
        snaps = _rollout_states(oracle, cm, n, 21, {1, 30})  # one step after the reset every ant is still in the air
        st = {k: np.concatenate([snaps[1][k][: n // 2], snaps[30][k][n // 2:]]) for k in snaps[1]}
    else:
        snaps = _rollout_states(oracle, cm, n, 21, {0, 40}, robot="point")
        st = {k: np.concatenate([snaps[0][k][: n // 2], snaps[40][k][n // 2:]]) for k in snaps[0]}
        if m.nblock == 0 and m.nball == 0:
            for k, (x, y, th) in enumerate(CORNER_POINTS):
                st["qpos"][n - 1 - k, :3] = (x, y, th)
                st["qvel"][n - 1 - k] = 0.0
            st["qpos"] = st["qpos"].astype(np.float32).astype(np.float64)
    act = rng.uniform(lo, hi, (n, m.nu)).astype(np.float32)
    counts = oracle.forward(cm, st["qpos"], st["qvel"], act.astype(np.float64), st["warm"])["counts"]
    nc = counts[:, 1 if chain else 0].astype(int)
    least = int(nc.min())
    if chain or (m.nblock == 0 and m.nball == 0):
        assert least == 0, np.bincount(nc)  # (an env of these mazes can have no contact / no limit row at all)
    else:
        assert least >= 1, np.bincount(nc)  # the movable body rests on the floor
    # arrangement A: wave 0 = least-loaded envs only, wave 1 = the most loaded env among least-loaded ones, the rest as they come
    idle = list(np.flatnonzero(nc == least))
    assert len(idle) >= 2 * e - 1, (len(idle), np.bincount(nc))
    top = int(np.argmax(nc))
    assert nc[top] > least
    order = idle[:e] + [top] + idle[e: 2 * e - 1]
    order += [i for i in range(n) if i not in set(order)]
    order = np.array(order)
    st = {k: v[order] for k, v in st.items()}
    act, nc = act[order], nc[order]
    waves = nc.reshape(-1, e)
    assert (waves[0] == least).all() and waves[1].max() == nc.max() and (waves[1] == least).any()
    if key in ("point8", "point16", "point32"):
        assert (nc > 16).sum() >= 3, np.bincount(nc)  # more contacts than the 16 register slots of a row of lanes
    return st, act, nc, least


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _step_all(torch, env, start, act):
    """one step from `start`: obs, reward, done, qpos, qvel, warm, t, goal index, info rows — and the status words"""
    env.set_state(start["qpos"], start["qvel"], start["warm"], start["t"])
    env.status()  # (cleared on read: what follows is this step's)
    obs, rew, done, info = env.step(torch.as_tensor(act, device=env.device))
    inf4 = torch.cat([info["position"], info["reward_forward"].unsqueeze(1), info["reward_ctrl"].unsqueeze(1)], 1)
    out = [x.cpu().numpy().copy() for x in (obs, rew, done, *env.get_state(), info["goal_index"], inf4)]
    return out, env.status().cpu().numpy().copy()


def _make_row(key):
    env_id, opts, n, lanes, kw = ROWS[key]
    env = mm.make(env_id, num_envs=n, **kw)
    for k, v in opts.items():
        env.set_option(k, v)
    assert env.launch_info()["lanes_per_env"] == lanes, env.launch_info()
    return env


@pytest.fixture(scope="module")
def cases(oracle):
    """start states per row of (a), built once and shared with (c)"""
    cache = {}

    def get(key, cm):
        same = ROWS[key][0], ROWS[key][2], ROWS[key][3], tuple(sorted(ROWS[key][4].items()))  # (rows that differ in a launch option only share a case)
        if same not in cache:
            cache[same] = build_case(oracle, cm, key)
        return cache[same]

    return get


def _shares(group_a, group_b):
    return len(set(zip(group_a.tolist(), group_b.tolist())))


@pytest.mark.parametrize("key", list(ROWS))
def test_wave_mate_independence(torch, cases, key):
    env_id, opts, n, lanes, _ = ROWS[key]
    e, w = 64 // lanes, n // (64 // lanes)
    env = _make_row(key)
    try:
        start, act, nc, least = cases(key, env.model)
        print(f"{key}: oracle counts of arrangement A, by wave: {nc.reshape(-1, e).tolist()}")
        first, status = _step_all(torch, env, start, act)
        second, status2 = _step_all(torch, env, start, act)
        for name, a, b in zip(ALL_NAMES, first, second):
            assert np.array_equal(_bits(a), _bits(b)), f"{name}: the same step from the same state gave different bits"
        assert np.array_equal(status, status2)
        to_b = _regroup(w, e)
        idx = np.arange(n)
        assert _shares(idx // e, to_b // e) == n  # no two envs share a wave in both arrangements
        if env_id.startswith(("Swimmer", "Reacher")):
            # workgroups of 64 envs: every workgroup of A spread evenly over all of B's (module docstring)
            pairs = np.stack([idx // 64, to_b // 64], 1)
            _, cnt = np.unique(pairs, axis=0, return_counts=True)
            assert len(cnt) == (n // 64) ** 2 and (cnt == 64 // (n // 64)).all(), cnt
        from_a = np.argsort(to_b)  # B[j] = A[from_a[j]]
        third, status3 = _step_all(torch, env, {k: v[from_a] for k, v in start.items()}, act[from_a])
        for name, a, b in zip(ALL_NAMES, first, third):
            diff = _bits(a) != _bits(b[to_b])
            assert not diff.any(), f"{name}: {int(diff.reshape(n, -1).any(1).sum())} envs step differently with other wave-mates"
        assert np.array_equal(status, status3[to_b])
    finally:
        env.close()


def test_waves_per_block_changes_no_bit(torch, cases):
    """Two-block ants at 16 lanes, one wave and four waves per workgroup (sixteen envs in one workgroup, or as many as its LDS holds:
    launch_ant_step halves the workgroup until it fits): every output, the state and the status words of one step, bit for bit."""
    outs = {}
    for key in ("antmultipush16", "antmultipush16wpb4"):
        env = _make_row(key)
        try:
            start, act, nc, least = cases(key, env.model)
            outs[key] = _step_all(torch, env, start, act)
        finally:
            env.close()
    (one, status1), (four, status4) = outs["antmultipush16"], outs["antmultipush16wpb4"]
    for name, a, b in zip(ALL_NAMES, one, four):
        diff = _bits(a) != _bits(b)
        assert not diff.any(), f"{name}: {int(diff.reshape(len(a), -1).any(1).sum())} envs step differently in a workgroup of four waves"
    assert np.array_equal(status1, status4)


# ------------------------------------------------------------------ (b) slot independence across auto-reset
OFFSET = 3


def _near_goal_by_slot(env, obs0, offset):
    """tests/test_gpu_rollout.py _near_goal, keyed by the GLOBAL slot: every env whose slot is a multiple of four"""
    import torch

    qpos, qvel, warm, t = env.get_state()
    gp = env.model.c.goal_pos[0]
    sel = (torch.arange(env.num_envs, device=env.device) + offset) % 4 == 0
    if env.model.c.nball:
        qpos[sel, 3], qpos[sel, 4] = float(gp[0]) + 0.2 - obs0[sel, 3], float(gp[1]) - obs0[sel, 4]
    else:
        qpos[sel, 0], qpos[sel, 1], qpos[sel, 2] = float(gp[0]) + 0.9, float(gp[1]), float(np.pi)
    env.set_state(qpos=qpos)
    return env.reset(mask=torch.zeros(env.num_envs, dtype=torch.uint8, device=env.device))  # the observation of the moved state, no reset


def _shift(x, dim=0):
    """A's rows of the slots B holds: A[j + 3] for j < N - 3"""
    return x.narrow(dim, OFFSET, x.shape[dim] - OFFSET)


def _head(x, dim=0):
    return x.narrow(dim, 0, x.shape[dim] - OFFSET)


def _assert_rows(a, b, dim, what):
    assert _same(_shift(a, dim).contiguous(), _head(b, dim).contiguous()), f"{what}: env B[j] differs from A[j + {OFFSET}]"


def _slot_pair(torch, make, k_step, k_fused, point):
    ea, eb = make(), make()
    try:
        eb.set_option("env_index_offset", OFFSET)
        n = ea.num_envs
        assert ea.env_goals is None and ea.launch_info() == eb.launch_info()
        npar = policy.param_count(ea.obs_dim, ea.nu, 5)
        g = torch.Generator(device=ea.device).manual_seed(99)
        par_a = (0.4 * torch.randn((n, npar), device=ea.device, generator=g)).contiguous()
        par_b = torch.cat([_shift(par_a), par_a[:OFFSET]]).contiguous()
        scale = float(ea.action_space.high[0])
        seen = np.zeros(2, dtype=np.int64)
        for path, K in (("step", k_step), ("rollout", k_fused), ("rollout_policy", k_fused)):
            oa, ob = ea.reset(seed=31), eb.reset(seed=31)
            _assert_rows(oa, ob, 0, f"{path}: observation after reset")
            for x, y, nm in zip(ea.get_state(), eb.get_state(), ("qpos", "qvel", "warm", "t")):
                _assert_rows(x, y, 0, f"{path}: {nm} after reset")
            if point:
                oa, ob = _near_goal_by_slot(ea, oa, 0), _near_goal_by_slot(eb, ob, OFFSET)
                _assert_rows(oa, ob, 0, f"{path}: observation after the goal placement")
            ea.status(); eb.status()
            acts_a = _actions(ea, K, 7, drive=point)
            acts_b = torch.cat([_shift(acts_a, 1), acts_a[:, :OFFSET]], 1).contiguous()
            if path == "step":
                for k in range(K):
                    o1, r1, d1, i1 = ea.step(acts_a[k])
                    o2, r2, d2, i2 = eb.step(acts_b[k])
                    for nm, x, y in (("obs", o1, o2), ("reward", r1, r2), ("done", d1, d2), ("goal index", i1["goal_index"], i2["goal_index"]),
                                     ("position", i1["position"], i2["position"]), ("reward_forward", i1["reward_forward"], i2["reward_forward"]),
                                     ("reward_ctrl", i1["reward_ctrl"], i2["reward_ctrl"])):
                        _assert_rows(x, y, 0, f"step {k}: {nm}")
                    fin = _shift(d1) != 0
                    assert _same(_shift(i1["final_observation"])[fin].contiguous(), _head(i2["final_observation"])[fin].contiguous()), f"step {k}: final_observation"
                    seen += np.array([int((d1 & 1).sum()), int((d1 & 2).sum())])
            else:
                if path == "rollout":
                    ra, rb = ea.rollout(acts_a, return_obs=True), eb.rollout(acts_b, return_obs=True)
                else:
                    ra = ea.rollout_policy(par_a, K, hidden=5, squash=True, action_scale=scale, return_obs=True, return_actions=True)
                    rb = eb.rollout_policy(par_b, K, hidden=5, squash=True, action_scale=scale, return_obs=True, return_actions=True)
                    _assert_rows(ra[3]["actions"], rb[3]["actions"], 1, f"{path}: actions")
                _assert_rows(ra[0], rb[0], 0, f"{path}: last observation")
                _assert_rows(ra[1], rb[1], 1, f"{path}: rewards")
                _assert_rows(ra[2], rb[2], 1, f"{path}: dones")
                for nm in ("goal_index", "position", "reward_forward", "reward_ctrl", "observations"):
                    _assert_rows(ra[3][nm], rb[3][nm], 1, f"{path}: {nm}")
                fin = (_shift(ra[2], 1) != 0).any(0)
                assert _same(_shift(ra[3]["final_observation"])[fin].contiguous(), _head(rb[3]["final_observation"])[fin].contiguous()), f"{path}: final_observation"
                seen += np.array([int((ra[2] & 1).sum()), int((ra[2] & 2).sum())])
            for x, y, nm in zip(ea.get_state(), eb.get_state(), ("qpos", "qvel", "warm", "t")):
                _assert_rows(x, y, 0, f"{path}: final {nm}")
            _assert_rows(ea.status(), eb.status(), 0, f"{path}: status words")
        return ea.launch_info(), seen
    finally:
        ea.close(); eb.close()


@pytest.mark.parametrize("env_id", FUSED_IDS)
def test_slot_independence_planar(torch, env_id):
    point = env_id.startswith("Point")
    info, seen = _slot_pair(torch, lambda: mm.make(env_id, num_envs=130, auto_reset=True, seed=5, max_episode_steps=40), 50, 260, point)
    assert info["rollout_fused"] == 1 and info["engine"] == 0
    assert seen[1] > 0  # time limits ended episodes
    if point:
        assert seen[0] > 0  # and goals were reached


def test_slot_independence_ant(torch):
    info, seen = _slot_pair(torch, lambda: mm.make("AntUMaze-v0", num_envs=66, auto_reset=True, seed=5, max_episode_steps=5), 12, 12, False)
    assert info["rollout_fused"] == 0 and seen[1] > 0


def test_slot_independence_general_engine(torch):
    info, seen = _slot_pair(torch, lambda: mm.make("PointUMaze-v0", num_envs=34, engine="general", auto_reset=True, seed=5, max_episode_steps=7),
                            16, 16, True)
    assert info["rollout_fused"] == 0 and info["engine"] == 1 and seen[1] > 0


# ------------------------------------------------------------------ (c) a NaN wave-mate
POISON_ROWS = {
    "point8": ("point8", {}), "point16": ("point16", {}), "point32": ("point32", {}), "pointpush": ("pointpush", {}), "antpush": ("antpush", {}), "swimmer": ("swimmer", {}),
    "ant16wps1": ("ant16wpb2", {"waves_per_simd": 1}), "ant16wps2": ("ant16wpb2", {"waves_per_simd": 2}),
    "ant8": ("ant8", {}), "antmultipush16": ("antmultipush16", {}),  # the lane-group path (module docstring: its loop bounds)
}


@pytest.mark.parametrize("name", list(POISON_ROWS))
def test_nan_wave_mate_one_step(torch, cases, name):
    key, extra = POISON_ROWS[name]
    env_id, opts, n, lanes, _ = ROWS[key]
    e = 64 // lanes
    env = _make_row(key)
    try:
        for k, v in extra.items():
            env.set_option(k, v)
            assert env.launch_info()[k] == v
        start, act, nc, least = cases(key, env.model)
        clean, status = _step_all(torch, env, start, act)
        poisoned = np.zeros(n, bool)
        poisoned[np.arange(0, n, 2 * e)] = True  # the first env of every second wave
        bad = {k: v.copy() for k, v in start.items()}
        bad["qvel"][poisoned, 0] = np.nan  # one velocity entry of the robot
        out, status_p = _step_all(torch, env, bad, act)
        ok = ~poisoned
        for nm, a, b in zip(ALL_NAMES, clean, out):
            diff = _bits(a)[ok] != _bits(b)[ok]
            assert not diff.any(), f"{nm}: {int(diff.reshape(ok.sum(), -1).any(1).sum())} healthy envs step differently beside a NaN env"
        assert np.array_equal(status[ok], status_p[ok]), (status[ok], status_p[ok])
        assert (status_p[poisoned] & BAD_STATE).all(), status_p[poisoned]
        assert not (status[ok] & BAD_STATE).any()
    finally:
        env.close()


@pytest.mark.parametrize("env_id", ["PointUMaze-v0", "SwimmerUMaze-v0"])
def test_nan_wave_mate_fused_rollout(torch, env_id):
    n, K, limit = 64 if env_id.startswith("Point") else 256, 25, 10
    ea, ep = (mm.make(env_id, num_envs=n, auto_reset=True, seed=5, max_episode_steps=limit) for _ in range(2))
    try:
        assert ea.launch_info()["rollout_fused"] == 1
        e = 64 // ea.launch_info()["lanes_per_env"]
        ea.reset(seed=13); ep.reset(seed=13)
        poisoned = torch.zeros(n, dtype=torch.bool, device=ea.device)
        poisoned[:: 2 * e] = True
        qpos, qvel, warm, t = ep.get_state()
        qvel[poisoned, 0] = float("nan")
        ep.set_state(qvel=qvel)
        acts = _actions(ea, K, 4)
        oa, ra, da, ia = ea.rollout(acts, return_obs=True)
        op, rp, dp, ip = ep.rollout(acts, return_obs=True)
        ok = ~poisoned
        for nm, x, y in (("reward", ra, rp), ("done", da, dp), ("goal_index", ia["goal_index"], ip["goal_index"]), ("observations", ia["observations"], ip["observations"]),
                         ("position", ia["position"], ip["position"])):
            assert _same(x[:, ok].contiguous(), y[:, ok].contiguous()), f"{nm}: healthy envs differ beside NaN envs"
        for x, y in zip(ea.get_state(), ep.get_state()):
            assert _same(x[ok].contiguous(), y[ok].contiguous())
        # a NaN env reaches no goal: its first episode ends at the time limit, at step index limit - 1, where the row already holds the
        # new episode's first observation.  A's env of the same slot is compared where it also ran to the limit (same episode number:
        # a reset draw depends on seed, episode and slot only)
        first = limit - 1
        assert ((dp[first, poisoned] & 2) != 0).all() and (dp[:first, poisoned] == 0).all()
        same_episode = poisoned & (da[:first] == 0).all(0)
        assert int(same_episode.sum()) >= int(poisoned.sum()) // 2
        assert torch.isfinite(ip["observations"][first:, poisoned]).all()
        # (row `first` of reward / done still belongs to the NaN episode's last step)
        for nm, x, y, k0 in (("observations", ia["observations"], ip["observations"], first), ("reward", ra, rp, first + 1), ("done", da, dp, first + 1)):
            assert _same(x[k0:, same_episode].contiguous(), y[k0:, same_episode].contiguous()), f"{nm}: poisoned envs after their reset"
        assert (ep.status()[poisoned] & BAD_STATE).all()
    finally:
        ea.close(); ep.close()
