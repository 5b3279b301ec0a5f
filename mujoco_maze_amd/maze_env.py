"""Batched maze environment on the MI355X and the reference-shaped single env.

`VecMazeEnv` is the drop-in for the reference's hot path (`MazeEnv.step/reset`,
mujoco_maze/maze_env.py:371-382,448-481) over `num_envs` environments in
lock-step: Python -> ctypes -> C-ABI (include/mazestep.h) -> HIP kernels.  Tensors
stay on the GPU (torch is only the owner of device memory and streams).

`MazeEnv` keeps the reference constructor signature (maze_env.py:28-44) and the
`reset() -> (obs, info)` / `step(a) -> (obs, reward, done, info)` shapes for one
environment (numpy in / numpy out, float64 like the reference), implemented as a
`VecMazeEnv` of size 1.
"""
import ctypes as C
from typing import Optional, Tuple, Type

import numpy as np

from mujoco_maze_amd import _capi
from mujoco_maze_amd.agent_model import AgentModel
from mujoco_maze_amd.maze_task import MazeTask
from mujoco_maze_amd.model import ROBOT_ID, CompiledModel, compile_model


class Box:
    """Minimal stand-in for gym.spaces.Box (gym is not a dependency)."""

    def __init__(self, low, high):
        self.low = np.asarray(low, dtype=np.float32)
        self.high = np.asarray(high, dtype=np.float32)
        self.shape = self.low.shape
        self.dtype = np.float32

    def sample(self, rng: Optional[np.random.Generator] = None):
        rng = rng or np.random.default_rng()
        return rng.uniform(self.low, self.high).astype(np.float32)


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class WrappedRobot:
    """`MazeEnv.wrapped_env` of the reference (maze_env.py:218): the robot object user code reaches into for
    `get_xy()` / `set_xy(xy)` / `get_ori()` (agent_model.py:35-41, ant.py:98-111, point.py:83-92, swimmer.py:70-76).  The
    simulators themselves live in the HIP kernels, so this object is a view on the device batch through
    mz_get_state / mz_set_state; class-level knobs of the robot class (FILE, ORI_IND, RADIUS, ...) read through.

    On a `VecMazeEnv` the methods are batched (device tensors [N, 2] / [N]); on the single-env `MazeEnv` they take and return
    float64 numpy values like the reference."""

    def __init__(self, vec: "VecMazeEnv", model_cls, single: bool = False) -> None:
        self._vec, self._cls, self._single = vec, model_cls, single

    def __getattr__(self, name):  # class attributes of the robot class (ORI_IND, RADIUS, MANUAL_COLLISION, ...)
        # (only reached for names the instance does not have: private names and a half-built instance — copy / pickle probe
        # __setstate__ & co. before __init__ has run — must not recurse through the missing `_cls`)
        if name.startswith("_") or "_cls" not in self.__dict__:
            raise AttributeError(name)
        return getattr(self._cls, name)

    def get_xy(self):
        """qpos[:2] (ant.py:110-111, point.py:83-84, swimmer.py:75-76): a fresh copy."""
        xy = self._vec.get_state()[0][:, :2].clone()
        return xy[0].double().cpu().numpy() if self._single else xy

    def set_xy(self, xy) -> None:
        """qpos[:2] = xy, everything else (qvel, qacc_warmstart, t) untouched: ant.py:105-108, point.py:86-89 call
        `set_state(qpos, qvel)` with the current qvel; the warm start is not part of mujoco-py's state and survives."""
        torch, vec = self._vec._torch, self._vec
        qpos = vec.get_state()[0]
        new = torch.as_tensor(np.asarray(xy, dtype=np.float32) if not torch.is_tensor(xy) else xy, device=vec.device).to(torch.float32)
        if self._single:
            new = new.reshape(1, 2)
        if tuple(new.shape) != (vec.num_envs, 2):
            raise ValueError(f"xy must have shape {(vec.num_envs, 2)}, got {tuple(new.shape)}")
        qpos[:, :2] = new
        vec.set_state(qpos=qpos)

    def get_ori(self):
        """Heading: the Point's qpos[ORI_IND] (point.py:91-92); the Ant's torso x axis rotated by its quaternion
        qpos[ORI_IND:ORI_IND+4] and projected on the plane, arctan2(y, x) (ant.py:98-103, q_mult / q_inv :26-35)."""
        ind = getattr(self._cls, "ORI_IND", None)
        if ind is None:
            raise AttributeError(f"{self._cls.__name__} has no ORI_IND: the reference defines get_ori for the Point and the Ant only")
        qpos = self._vec.get_state()[0].double()
        torch = self._vec._torch
        if getattr(self._cls, "ROBOT", None) == "ant":
            w, x, y, z = (qpos[:, ind + k] for k in range(4))
            # rot * (0, 1, 0, 0) * conj(rot), components 1..2, written out (ant.py:26-35 multiply without normalising)
            ox = w * w + x * x - y * y - z * z
            oy = 2.0 * (x * y + w * z)
            ori = torch.atan2(oy, ox)
        elif getattr(self._cls, "ROBOT", None) == "point":
            ori = qpos[:, ind].clone()
        else:
            # a user robot: qpos[ORI_IND] is a yaw angle only if its class says so (a free-joint robot's entry there is a
            # quaternion component) — it supplies the rule as a static `ori_from_qpos(qpos [N, nq]) -> [N]`
            fn = getattr(self._cls, "ori_from_qpos", None)
            if fn is None:
                raise AttributeError(f"{self._cls.__name__}: get_ori is defined for the Point (qpos[ORI_IND]) and the Ant (torso quaternion); "
                                     "a user robot provides `ori_from_qpos(qpos)`")
            ori = fn(qpos)
        return float(ori[0].item()) if self._single else ori


def _is_registered(model_cls, task_cls, scale) -> bool:
    """Is (robot class, task class, maze scale) one of the 145 registered combinations (mujoco_maze/__init__.py:22-78)?"""
    import mujoco_maze_amd as mm

    for spec in mm.REGISTRY.values():
        kw = spec.kwargs
        if kw["model_cls"] is model_cls and kw["maze_task"] is task_cls and float(kw["maze_size_scaling"]) == float(scale):
            return True
    return False


class VecMazeEnv:
    def __init__(self, model_cls: Type[AgentModel], maze_task: Type[MazeTask] = MazeTask, num_envs: int = 1,
                 maze_height: float = 0.5, maze_size_scaling: float = 4.0, inner_reward_scaling: float = 1.0,
                 restitution_coef: float = 0.8, task_kwargs: Optional[dict] = None, device=None,
                 max_episode_steps: int = 1000, auto_reset: bool = False, seed: int = 0, include_position: bool = True,
                 **kwargs) -> None:
        import torch  # device memory + streams only

        self._torch = torch
        self.num_envs = int(num_envs)
        self._task = maze_task(maze_size_scaling, **(task_kwargs or {}))
        robot = getattr(model_cls, "ROBOT", None)
        if robot not in ("ant", "point", "swimmer", "reacher", "generic"):
            raise NotImplementedError(f"robot {model_cls.__name__}: set ROBOT to one of the built-in families or to \"generic\" (any tree "
                                      "topology, stepped from its MJCF: AgentModel.FILE)")
        if robot == "generic":  # the user's own robot (agent_model.py:12-41, README.md:127): its MJCF, frame_skip, reset distribution
            kwargs.setdefault("robot_xml", getattr(model_cls, "FILE", None))
            # round 6: STEP = "motors" (ant.py:61-73, the default) or "point" (point.py:44-61: the action moves heading and position,
            # velocities clipped to VELOCITY_LIMITS); MANUAL_COLLISION / RADIUS as for the built-in Point
            gen_kw = dict(frame_skip=int(getattr(model_cls, "FRAME_SKIP", 1)), reset_qvel=getattr(model_cls, "RESET_QVEL", "normal"),
                          step=getattr(model_cls, "STEP", "motors"), velocity_limit=getattr(model_cls, "VELOCITY_LIMITS", None))
        else:
            gen_kw = {}
        # engine="general": step this env on the general engine (csrc/generic_dyn.h) whatever the robot — the second, independent
        # device implementation the specialised kernels are cross-checked with; "auto" (default): only where they cannot step it
        gen_kw["engine"] = kwargs.pop("engine", "auto")
        has_xml = kwargs.get("robot_xml") is not None
        self.model: CompiledModel = compile_model(
            robot, self._task, maze_size_scaling, inner_reward_scaling=inner_reward_scaling,
            restitution_coef=restitution_coef, maze_height=maze_height, max_episode_steps=max_episode_steps,
            forward_reward_weight=kwargs.pop("forward_reward_weight", 1.0), ctrl_cost_weight=kwargs.pop("ctrl_cost_weight", 1e-4),
            manual_collision=getattr(model_cls, "MANUAL_COLLISION", False), radius=getattr(model_cls, "RADIUS", None),
            robot_xml=kwargs.pop("robot_xml", None), **gen_kw)
        self.wrapped_cls = model_cls
        self.wrapped_env = WrappedRobot(self, model_cls)
        from mujoco_maze_amd.model import device_unsupported_reason

        why = device_unsupported_reason(self.model)
        if why:
            raise NotImplementedError(why)
        if not torch.cuda.is_available():
            raise _capi.MazeStepError("no GPU visible: mujoco_maze_amd steps environments on an MI355X only (no CPU fallback)")
        self._lib = _capi.load()
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        err = C.create_string_buffer(256)
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self._h = self._lib.mz_create(C.byref(self.model.c), self.num_envs, idx, err, 256)
        if not self._h:
            raise _capi.MazeStepError(f"mz_create failed: {err.value.decode()}")
        m = self.model.c
        self.nq, self.nv, self.nu, self.obs_dim = m.nq, m.nv, m.nu, m.obs_dim
        # The Ant's and the Point's Newton solvers take unit steps in the first iterations of a solve (ant_newton_rows.h).  The registered
        # mazes are soaked with them (1e8 env-steps, no solve at the iteration cap); a CUSTOM task, maze or robot variant is not, so
        # there every iteration searches the line exactly (ls_fast_iterations = 0: MuJoCo's monotone iteration on any maze, ~7 % of the
        # Ant kernel's time; a guarded unit step was measured and costs the same: profiles/r06/unit_guard_ab.txt).
        # set_option("ls_fast_iterations", 5) brings the unit steps back.  The general engine and the chain kernels search the line in
        # every iteration / solve in closed form.
        from mujoco_maze_amd.model import needs_general_engine

        self.custom_task = not _is_registered(model_cls, maze_task, maze_size_scaling) or has_xml
        if self.custom_task and robot in ("ant", "point") and not needs_general_engine(self.model):
            _capi.check(self._lib, self._h, self._lib.mz_set_option(self._h, b"ls_fast_iterations", 0.0), "mz_set_option(ls_fast_iterations)")
        n, dev = self.num_envs, self.device
        self._obs = torch.empty((n, self.obs_dim), dtype=torch.float32, device=dev)
        self._reward = torch.empty(n, dtype=torch.float32, device=dev)
        self._done = torch.empty(n, dtype=torch.uint8, device=dev)
        self._goal = torch.empty(n, dtype=torch.int32, device=dev)
        self._info = torch.empty((n, 4), dtype=torch.float32, device=dev)
        self._seed = int(seed)
        self._noise_seed = int(seed)  # default noise_seed of policy_sample / rollout_policy_sample: the last reset(seed=...), else this
        self._noise_step = 0          # their counter: +1 per policy_sample, +K per rollout_policy_sample (explicit arguments leave it alone)
        self._host_rewards = not self.model.device_rewards
        self._final_obs = None
        self._host_mask = None
        self._record = None
        self._obs_norm = None    # (mean, inv_std) of bind_obs_norm: the env holds a reference while the handle holds the pointers
        self._resampled_goals = False
        self._warned_goal_resampling = False
        self._env_goals = None   # float64 [N, MZ_MAX_GOAL, 3] once the task's sample_goals() said the goals move (per-env goal positions)
        self._goal_pool = None
        self._goal_gen = None
        self.set_auto_reset(auto_reset)
        lo = np.array([m.act_ctrlrange[a][0] for a in range(m.nu)], dtype=np.float32)
        hi = np.array([m.act_ctrlrange[a][1] for a in range(m.nu)], dtype=np.float32)
        self.action_space = Box(lo, hi)
        high = np.full(self.obs_dim, np.inf, dtype=np.float32)
        low = -high
        low[0], high[0], low[1], high[1] = self.model.world.xy_limits()
        self.observation_space = Box(low, high)

    # -- plumbing ----------------------------------------------------------
    def _stream(self):
        return C.c_void_p(self._torch.cuda.current_stream(self.device).cuda_stream)

    def set_option(self, key: str, value: float) -> None:
        if key == "auto_reset":
            return self.set_auto_reset(value != 0)
        _capi.check(self._lib, self._h, self._lib.mz_set_option(self._h, key.encode(), float(value)), f"mz_set_option({key})")
        if key == "wide_nets":  # 0 / 1 / 2 (mz_set_option has refused anything else): what `hidden=` may hold from here on
            self._wide_nets = int(value)

    def _max_width(self) -> int:
        """The widest hidden layer this env's networks may have: policy.MAX_WIDTH (256) after `set_option("wide_nets", 1 or 2)`,
        else policy.MAX_HIDDEN (64)."""
        from mujoco_maze_amd import policy

        return policy.MAX_WIDTH if getattr(self, "_wide_nets", 0) else policy.MAX_HIDDEN

    def launch_info(self) -> dict:
        """What the next step launches (mz_get_info): the engine (0 = the robot family's specialised kernel, 1 = the general engine),
        lanes per env, waves per SIMD, the device's SIMD count, whether rollout() runs this env on fused kernels ("rollout_fused":
        1) or on the step's launches in a loop (0), whether an observation normaliser is bound ("obs_norm": `bind_obs_norm`), and the
        mode of option "wide_nets" (0: hidden layers of up to 64 units; 1: up to 256, a network wider than 64 on the tiled kernel; 2:
        every network given as a sequence of widths or with ReLU units on the tiled kernel).  The
        instantiation depends on the batch size and the device; its
        results agree across instantiations to fp32 round-off, not bit for bit (include/mazestep.h)."""
        out = {}
        for key in ("engine", "lanes_per_env", "waves_per_simd", "device_simds", "ls_fast_iterations", "rollout_fused", "obs_norm", "wide_nets"):
            v = C.c_double(0.0)
            _capi.check(self._lib, self._h, self._lib.mz_get_info(self._h, key.encode(), C.byref(v)), f"mz_get_info({key})")
            out[key] = int(v.value)
        return out

    def set_auto_reset(self, on: bool) -> None:
        """Auto-reset follows the vector-env convention: an env whose step ended its episode returns the reward / done of
        that terminal step, the FIRST observation of the next episode in `obs`, and its terminal observation in
        `info["final_observation"]` (rows where done != 0).  Tasks whose reward()/termination() are Python overrides are
        judged on the host, so for them the device's own verdict must not reset anything: the kernel's auto-reset stays
        off and the host issues the masked reset after it has evaluated the task."""
        self._auto_reset = bool(on)
        if self._auto_reset and self._final_obs is None:
            self._final_obs = self._torch.zeros((self.num_envs, self.obs_dim), dtype=self._torch.float32, device=self.device)
        device_side = self._auto_reset and not self._host_rewards
        _capi.check(self._lib, self._h, self._lib.mz_bind_final_obs(self._h, _ptr(self._final_obs) if device_side else None), "mz_bind_final_obs")
        _capi.check(self._lib, self._h, self._lib.mz_set_option(self._h, b"auto_reset", 1.0 if device_side else 0.0), "mz_set_option(auto_reset)")

    def bind_record(self, record) -> None:
        """Bind (or, with None, unbind) a float32 [N, obs_dim + 2] device tensor that every step fills with the packed record
        obs | reward | done — the send buffer of the sharded run's all-gather (mz_bind_record); the caller keeps it alive."""
        if record is not None:
            if self._host_rewards:
                raise ValueError("this task's reward()/termination() are Python overrides judged on the host after the kernel: the "
                                 "kernel-written record would carry the device's built-in verdict.  Pack obs / reward / done after "
                                 "step() instead (sharding.RecordGatherer.start(obs, reward, done))")
            if tuple(record.shape) != (self.num_envs, self.obs_dim + 2) or record.dtype != self._torch.float32 or not record.is_contiguous() \
                    or record.device != self.device:
                raise ValueError(f"record must be a contiguous float32 tensor of shape {(self.num_envs, self.obs_dim + 2)} on {self.device}")
        self._record = record
        _capi.check(self._lib, self._h, self._lib.mz_bind_record(self._h, _ptr(record)), "mz_bind_record")

    def bind_obs_norm(self, mean, inv_std, clip: float = 10.0) -> None:
        """Bind an observation normaliser to the device-side networks (mz_bind_obs_norm): while bound, `policy_act`, `policy_sample`,
        `value` and every closed-loop rollout evaluate their networks on clip((obs - mean) * inv_std, -clip, clip) — float32,
        elementwise, `policy.normalize_reference` bit for bit — in place of the raw row, the critic's terminal rows included.
        Everything the env itself returns stays raw: observations, `info["observations"]`, `info["final_observation"]`, rewards, dones;
        `step` and the open-loop `rollout` do not look at the binding.  mean, inv_std: contiguous float32 [obs_dim] tensors on the
        env's device, one normaliser for all envs.  The env keeps a reference and the kernels read them at every call, so rewriting
        them IN PLACE (`normalize.RunningMeanStd.update`) takes effect at the next call without binding again.
        `bind_obs_norm(None, None)` unbinds.  A refused call leaves the previous binding in place."""
        torch = self._torch
        if mean is None and inv_std is None:
            _capi.check(self._lib, self._h, self._lib.mz_bind_obs_norm(self._h, None, None, float(clip), self._stream()), "mz_bind_obs_norm")
            self._obs_norm = None
            return
        for name, t in (("mean", mean), ("inv_std", inv_std)):
            if not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != (self.obs_dim,) or t.device != self.device \
                    or not t.is_contiguous():
                got = f"{tuple(t.shape)} {t.dtype} on {t.device}" if torch.is_tensor(t) else type(t).__name__
                raise ValueError(f"{name} must be a contiguous float32 tensor of shape {(self.obs_dim,)} on {self.device} (the kernels read "
                                 f"it in place at every call), got {got}")
        _capi.check(self._lib, self._h, self._lib.mz_bind_obs_norm(self._h, _ptr(mean), _ptr(inv_std), float(clip), self._stream()),
                    "mz_bind_obs_norm")
        self._obs_norm = (mean, inv_std)

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._torch.cuda.synchronize(self.device)
            self._lib.mz_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- API ---------------------------------------------------------------
    def get_ori(self):
        return self.wrapped_env.get_ori()  # maze_env.py:231-232

    def set_goals(self, goals=None) -> None:
        """Upload the task's goal list (default: `self._task.goals`) to the device: position, threshold, reward scale and
        dimension of every MazeGoal replace the table the step kernel's predicate reads (mz_set_goals).  The counterpart of
        the reference's `set_marker()` after `sample_goals()` (maze_env.py:374-376, 384-387)."""
        goals = self._task.goals if goals is None else goals
        n = len(goals)
        if n > 8:
            raise ValueError("too many goals (MZ_MAX_GOAL = 8)")
        pos = np.zeros((max(n, 1), 3), np.float64)
        for i, g in enumerate(goals):
            pos[i, : g.dim] = np.asarray(g.pos, np.float64)[: g.dim]
        thr = np.array([g.threshold for g in goals] or [0.0], np.float64)
        rs = np.array([g.reward_scale for g in goals] or [0.0], np.float64)
        dim = np.array([g.dim for g in goals] or [2], np.int32)
        rc = self._lib.mz_set_goals(self._h, n, pos.ctypes.data_as(C.c_void_p), thr.ctypes.data_as(C.c_void_p),
                                    rs.ctypes.data_as(C.c_void_p), dim.ctypes.data_as(C.c_void_p), self._stream())
        _capi.check(self._lib, self._h, rc, "mz_set_goals")
        # the host copy of the model follows (tools that judge with `env.model` must see the new goals; model.py fills the same fields)
        m = self.model.c
        m.ngoal = n
        for i in range(n):
            for k in range(3):
                m.goal_pos[i][k] = float(pos[i, k])
            m.goal_threshold[i], m.goal_reward_scale[i], m.goal_dim[i] = float(thr[i]), float(rs[i]), int(dim[i])

    @property
    def env_goals(self):
        """float64 [N, MZ_MAX_GOAL, 3] device tensor of per-env goal positions (None while the batch shares one goal table): the
        tensor the step kernel's goal predicate reads (mz_bind_env_goals).  Writing into it moves the goals of single envs."""
        return self._env_goals

    def _draw_goal_pool(self) -> None:
        """Per-env goals (maze_env.py:374-376: the reference calls `sample_goals()` at every episode reset of every env, each env its own
        task object).  Here one task object serves the batch, so a full reset() draws N goal tables from it — env i starts with draw i —
        and keeps the N draws as the pool from which the episodes that end later (device auto-reset, masked reset) take their next
        goals, picked by a device-side RNG: no host round trip in the step loop.  Positions only; number, thresholds, reward scales
        and dimensions of the goals are those of the shared table."""
        torch, n = self._torch, self.num_envs
        first = [np.asarray(g.pos, np.float64).copy() for g in self._task.goals]
        rows = np.zeros((n, 8, 3), np.float64)
        for r in range(n):
            if r and not self._task.sample_goals():
                raise ValueError(f"{type(self._task).__name__}.sample_goals() returned True, then False: it must keep resampling")
            if len(self._task.goals) != len(first) or len(first) > 8:
                raise ValueError("sample_goals() must keep the number of goals (and at most MZ_MAX_GOAL = 8 of them)")
            for i, g in enumerate(self._task.goals):
                rows[r, i, : g.dim] = np.asarray(g.pos, np.float64)[: g.dim]
        for g, p0 in zip(self._task.goals, first):  # the task object (and the uploaded shared table) keep the FIRST draw
            g.pos = p0
        self._goal_pool = torch.as_tensor(rows, device=self.device)
        if self._env_goals is None:
            self._env_goals = self._goal_pool.clone()
            self._goal_gen = torch.Generator(device=self.device)
            rc = self._lib.mz_bind_env_goals(self._h, _ptr(self._env_goals), self._stream())
            _capi.check(self._lib, self._h, rc, "mz_bind_env_goals")
        else:
            self._env_goals.copy_(self._goal_pool)
        self._goal_gen.manual_seed(self._seed)

    def _resample_env_goals(self, which) -> None:
        """Envs in `which` (bool [N], device) take a random member of the pool as their goals; the others keep theirs."""
        torch = self._torch
        idx = torch.randint(0, self.num_envs, (self.num_envs,), device=self.device, generator=self._goal_gen)
        torch.where(which[:, None, None], self._goal_pool[idx], self._env_goals, out=self._env_goals)

    def _sync_goals_across_ranks(self) -> None:
        """Sharded runs (sharding.py): every rank called sample_goals() on its own unsynchronised RNG — rank 0's goals win, so that
        the batch really has ONE goal table (positions only: thresholds / reward scales are class constants of the task)."""
        # Only where the caller SAID the env is one shard of a node-wide batch (sharding.ShardedVecMazeEnv sets goal_sync_group):
        # a collective hidden behind dist.is_initialized() would deadlock a trainer whose ranks reset at different times
        group = getattr(self, "goal_sync_group", None)
        if group is None:
            return
        import torch.distributed as dist

        grp = None if group == "world" else group
        if not (dist.is_available() and dist.is_initialized() and dist.get_world_size(grp) > 1):
            return
        torch = self._torch
        buf = torch.zeros((8, 3), dtype=torch.float64, device=self.device if dist.get_backend(grp) == "nccl" else "cpu")
        for i, g in enumerate(self._task.goals[:8]):
            buf[i, : g.dim] = torch.as_tensor(np.asarray(g.pos, np.float64)[: g.dim])
        dist.broadcast(buf, src=dist.get_global_rank(grp, 0) if grp is not None else 0, group=grp)
        host = buf.cpu().numpy()
        for i, g in enumerate(self._task.goals[:8]):
            g.pos = host[i, : g.dim].copy()

    def reset(self, mask=None, seed: Optional[int] = None):
        """Reset all (or the masked) envs; returns the observation tensor [N, obs_dim] on the GPU.

        A full reset (mask None) first asks the task for new goals — `MazeTask.sample_goals()`, maze_env.py:374-376 — and when it
        says they changed the batch moves to PER-ENV goal positions (`env_goals`, _draw_goal_pool): every env its own draw, and
        every later episode start (masked reset, device auto-reset) a new one for that env, as the reference's one-task-per-env
        does.  Tasks whose goals never move keep the one shared table."""
        if seed is not None:
            self._seed = int(seed)
            self._noise_seed, self._noise_step = int(seed), 0  # a reseeded env draws the same policy noise again
        if mask is None and self._task.sample_goals():
            self._resampled_goals = True
            self._sync_goals_across_ranks()
            self.set_goals()  # the shared table follows the draw (thresholds, reward scales, dims; the host copy of the model)
            if not self._host_rewards:
                self._draw_goal_pool()  # every env its own draw of sample_goals(); the step kernel reads the per-env table from here on
            elif self._auto_reset and not self._warned_goal_resampling:
                import warnings

                self._warned_goal_resampling = True
                warnings.warn(f"{type(self._task).__name__}.sample_goals() returned True, auto_reset is on and the task's reward()/termination() are "
                              "Python overrides judged on the host from ONE task object: the reference resamples goals at EVERY episode reset "
                              "(maze_env.py:374-376), here they change at full reset() calls only")
        elif mask is not None and self._env_goals is not None:
            mkb = self._torch.as_tensor(mask, device=self.device).to(self._torch.bool)
            self._resample_env_goals(mkb)  # the masked envs start a new episode: new goals for them (maze_env.py:374-376), the others keep theirs
        mk = None
        if mask is not None:
            mk = self._torch.as_tensor(mask, device=self.device).to(self._torch.uint8).contiguous()
        rc = self._lib.mz_reset(self._h, _ptr(mk), C.c_uint64(self._seed), _ptr(self._obs), self._stream())
        _capi.check(self._lib, self._h, rc, "mz_reset")
        self._seed += 1
        return self._obs

    def step(self, actions):
        """actions: float32 tensor [N, nu] on the same GPU.  Returns (obs, reward, done, info) tensors;
        `done` is uint8 with bit0 = task termination, bit1 = TimeLimit truncation."""
        torch = self._torch
        a = actions if torch.is_tensor(actions) else torch.as_tensor(np.asarray(actions, dtype=np.float32), device=self.device)
        if a.dtype != torch.float32 or not a.is_contiguous() or a.device != self.device:
            a = a.to(device=self.device, dtype=torch.float32).contiguous()
        if tuple(a.shape) != (self.num_envs, self.nu):
            raise ValueError(f"actions must have shape {(self.num_envs, self.nu)}, got {tuple(a.shape)}")
        rc = self._lib.mz_step(self._h, _ptr(a), _ptr(self._obs), _ptr(self._reward), _ptr(self._done), _ptr(self._goal),
                               _ptr(self._info), self._stream())
        _capi.check(self._lib, self._h, rc, "mz_step")
        if self._host_rewards:
            self._apply_host_task()
        elif self._env_goals is not None and self._auto_reset:
            self._resample_env_goals(self._done != 0)  # the kernel judged this step with the old goals and restarted these envs
        info = {"position": self._info[:, :2], "reward_forward": self._info[:, 2], "reward_ctrl": self._info[:, 3],
                "goal_index": self._goal}
        if self._auto_reset:
            info["final_observation"] = self._final_obs  # valid in the rows where done != 0
        return self._obs, self._reward, self._done, info

    def _next_obs_row(self, obs, done, info):
        """The row a step produced before any auto-reset, from what `step()` returned: the terminal row where the env finished."""
        if not self._auto_reset:
            return obs
        return self._torch.where((done != 0).unsqueeze(1), info["final_observation"], obs)

    def rollout(self, actions, repeat: Optional[int] = None, return_obs: bool = False, return_next_obs: bool = False):
        """K steps in one call, for callers that need nothing from the host between steps (sampling planners on pre-drawn action
        sequences, action repeat, random walks): the results and the env's state afterwards are exactly those of K `step()` calls.

        actions: float32 [K, N, nu] on the same GPU — or [N, nu] with `repeat=K`, the same actions held for K steps.
        Returns (obs, rewards [K, N], dones [K, N] uint8, info): `obs` [N, obs_dim] is what the last step returned; info holds
        "goal_index" [K, N], "position" [K, N, 2], "reward_forward" / "reward_ctrl" [K, N], "observations" [K, N, obs_dim] with
        `return_obs`, and under auto-reset "final_observation" (row i: the last terminal observation of env i).  The output tensors
        are reused by the next rollout of the same K.

        With `return_next_obs`, info["next_observations"] [K, N, obs_dim]: the row step k produced BEFORE any auto-reset — equal to
        "observations"[k] wherever dones[k] == 0, the step's terminal row where the env finished (every one of them, where
        "final_observation" keeps only the env's last).  It is the s' of the transition (s, a, r, s', d); s is the row before:
        the entry observation, then "observations"[k - 1].  One mz_rollout_ex call.

        One mz_rollout call (fused kernels for the Point, Swimmer and Reacher: `launch_info()["rollout_fused"]`) — except where the
        host has work between steps (Python reward()/termination() overrides; per-env goals under auto-reset, which are resampled
        after every step): there this method calls `step()` K times itself and stacks the results."""
        torch, n = self._torch, self.num_envs
        a = actions if torch.is_tensor(actions) else torch.as_tensor(np.asarray(actions, dtype=np.float32), device=self.device)
        if a.dtype != torch.float32 or not a.is_contiguous() or a.device != self.device:
            a = a.to(device=self.device, dtype=torch.float32).contiguous()
        if repeat is not None:
            K = int(repeat)
            if tuple(a.shape) != (n, self.nu):
                raise ValueError(f"with repeat, actions must have shape {(n, self.nu)}, got {tuple(a.shape)}")
        else:
            if a.dim() != 3 or tuple(a.shape[1:]) != (n, self.nu):
                raise ValueError(f"actions must have shape (K, {n}, {self.nu}) — or {(n, self.nu)} with repeat=K —, got {tuple(a.shape)}")
            K = int(a.shape[0])
        if not 1 <= K <= 65536:
            raise ValueError(f"a rollout takes 1 .. 65536 steps, got {K}")
        buf = self._rollout_buffers(K, return_obs, return_next_obs)
        if self._host_rewards or (self._env_goals is not None and self._auto_reset):
            for k in range(K):
                obs, rew, done, inf = self.step(a if repeat is not None else a[k])
                buf["reward"][k], buf["done"][k], buf["goal"][k], buf["info"][k] = rew, done, inf["goal_index"], self._info
                if return_obs:
                    buf["obs_seq"][k] = obs
                if return_next_obs:
                    buf["next_obs_seq"][k] = self._next_obs_row(obs, done, inf)
        elif return_next_obs:
            io = _capi.make_rollout_io(K, actions_dev=_ptr(a), action_step_stride=0 if repeat is not None else n * self.nu, obs_dev=_ptr(self._obs),
                                       reward_dev=_ptr(buf["reward"]), done_dev=_ptr(buf["done"]), goal_idx_dev=_ptr(buf["goal"]),
                                       info_dev=_ptr(buf["info"]), obs_seq_dev=_ptr(buf["obs_seq"]) if return_obs else None,
                                       next_obs_seq_dev=_ptr(buf["next_obs_seq"]))
            rc = self._lib.mz_rollout_ex(self._h, C.byref(io), self._stream())
            _capi.check(self._lib, self._h, rc, "mz_rollout_ex")
        else:
            rc = self._lib.mz_rollout(self._h, K, _ptr(a), 0 if repeat is not None else n * self.nu, _ptr(self._obs), _ptr(buf["reward"]),
                                      _ptr(buf["done"]), _ptr(buf["goal"]), _ptr(buf["info"]), _ptr(buf["obs_seq"]) if return_obs else None,
                                      self._stream())
            _capi.check(self._lib, self._h, rc, "mz_rollout")
        return self._obs, buf["reward"], buf["done"], self._rollout_info(buf, return_obs, return_next_obs)

    def _rollout_info(self, buf, return_obs: bool, return_next_obs: bool, return_actions: bool = False, **per_step) -> dict:
        """The info dict of a rollout from its buffers; per_step: what a closed-loop call adds ([K, N] each)."""
        info = {"position": buf["info"][:, :, :2], "reward_forward": buf["info"][:, :, 2], "reward_ctrl": buf["info"][:, :, 3],
                "goal_index": buf["goal"], **per_step}
        if return_obs:
            info["observations"] = buf["obs_seq"]
        if return_next_obs:
            info["next_observations"] = buf["next_obs_seq"]
        if return_actions:
            info["actions"] = buf["actions"]
        if self._auto_reset:
            info["final_observation"] = self._final_obs
        return info

    def _net_kind(self, hidden, activation: str, what: str = "hidden"):
        """(widths, activation index, legacy) of a network given as `hidden` / `activation` (policy.net_shape); legacy: an int
        `hidden` with tanh, which the entries without mz_net take.  With option "wide_nets" on, widths go up to 256 and a network
        wider than 64 is never legacy (the entries with an int `hidden` stay at 64); in mode 2 no network is: the mode puts every
        network of the env on the tiled kernel, which only the mz_net entries launch."""
        from mujoco_maze_amd import policy

        widths, act = policy.net_shape(hidden, activation, what, max_width=self._max_width())
        legacy = bool(np.ndim(hidden) == 0 and act == 0)
        if getattr(self, "_wide_nets", 0) == 2 or any(w > policy.MAX_HIDDEN for w in widths):
            legacy = False
        return widths, act, legacy

    def _policy_params(self, params, hidden, stochastic: bool = False, log_std: str = "param", cdim: int = 0):
        """params as a contiguous float32 device tensor [npar] or [N, npar] (stochastic: npar_s = npar + nu, log_std behind the
        network; log_std="state": the head count, an output layer of 2 nu units); returns (tensor, param_env_stride)."""
        from mujoco_maze_amd import policy

        torch = self._torch
        npar = policy.param_count(self.obs_dim + cdim, self.nu, hidden, stochastic, log_std, max_width=self._max_width())
        p = params if torch.is_tensor(params) else torch.as_tensor(np.asarray(params, dtype=np.float32), device=self.device)
        if p.dtype != torch.float32 or not p.is_contiguous() or p.device != self.device:
            p = p.to(device=self.device, dtype=torch.float32).contiguous()
        if tuple(p.shape) not in ((npar,), (self.num_envs, npar)):
            raise ValueError(f"params must have shape {(npar,)} (one policy) or {(self.num_envs, npar)} (one per env) for obs_dim {self.obs_dim}"
                             f"{f' + context {cdim}' if cdim else ''}, nu {self.nu}, hidden {hidden}, got {tuple(p.shape)}")
        return p, (npar if p.dim() == 2 else 0)

    def _context(self, context, in_place: bool = False):
        """context as a contiguous float32 device tensor [N, C], 1 <= C <= MZ_MAX_CONTEXT; in_place (rollouts, which update it): the
        caller's own tensor or a ValueError."""
        torch = self._torch
        if in_place:
            c = context
            if not torch.is_tensor(c) or c.dtype != torch.float32 or c.device != self.device or not c.is_contiguous():
                raise ValueError(f"context must be a contiguous float32 tensor on {self.device}: a rollout updates it in place")
        else:
            c = context if torch.is_tensor(context) else torch.as_tensor(np.asarray(context, dtype=np.float32), device=self.device)
            if c.dtype != torch.float32 or not c.is_contiguous() or c.device != self.device:
                c = c.to(device=self.device, dtype=torch.float32).contiguous()
        if c.dim() != 2 or c.shape[0] != self.num_envs or not 1 <= c.shape[1] <= _capi.MAX_CONTEXT:
            raise ValueError(f"context must have shape ({self.num_envs}, C) with 1 <= C <= {_capi.MAX_CONTEXT} (MZ_MAX_CONTEXT), got {tuple(c.shape)}")
        return c

    def _policy_obs(self, obs):
        torch = self._torch
        o = obs if torch.is_tensor(obs) else torch.as_tensor(np.asarray(obs, dtype=np.float32), device=self.device)
        if tuple(o.shape) != (self.num_envs, self.obs_dim):
            raise ValueError(f"obs must have shape {(self.num_envs, self.obs_dim)}, got {tuple(o.shape)}")
        if o.dtype != torch.float32 or not o.is_contiguous() or o.device != self.device:
            o = o.to(device=self.device, dtype=torch.float32).contiguous()
        return o

    def policy_act(self, params, obs=None, hidden=0, squash: bool = False, action_scale: float = 1.0, activation: str = "tanh", context=None):
        """Actions [N, nu] of a small policy evaluated on the device (mz_policy_act): affine (`hidden=0`) or one tanh hidden layer of
        up to 64 units; `squash` makes the output action_scale * tanh(.).  params: float32 [npar] (one policy for all envs) or
        [N, npar] (one per env), packed by `mujoco_maze_amd.policy.pack` / `pack_linear`; obs: [N, obs_dim], default the env's last
        returned observation.  The actions are not clamped (step() clamps where the reference does).  A new tensor per call.

        `hidden` may also be a sequence of one or two widths, e.g. `(64, 64)` (params packed by `policy.pack_mlp`), and
        `activation="relu"` makes the hidden units ReLU instead of tanh, one choice for both layers (mz_net_act).

        After `set_option("wide_nets", 1)` a hidden layer may have up to 256 units (SB3's and CleanRL's 256-256 off-policy networks),
        here and in `policy_sample`, `value`, `rollout_policy` and `rollout_policy_sample`: a network wider than 64 runs the tiled
        kernel (csrc/mz_net_tile.h), with the same arithmetic and the same numpy model (`policy.reference(.., max_width=256)`), and a
        rollout with such an actor or critic loops its launches inside the call on every env.  Without the option a width above 64
        stays a ValueError.

        context: float32 [N, C], 1 <= C <= 32 — a per-env row (a goal, a subgoal, a skill) the network reads BEHIND the observation:
        its input row is [obs | context], obs normalised as usual while a normaliser is bound, the context never; params are packed
        for obs_dim + C inputs (`policy.param_count(obs_dim + C, ...)`).  `policy.reference(params, policy.context_row(obs, context), ..)`
        is the numpy model.  One mz_net_eval_ctx call."""
        widths, act, legacy = self._net_kind(hidden, activation)
        cx = None if context is None else self._context(context)
        p, stride = self._policy_params(params, hidden, cdim=0 if cx is None else int(cx.shape[1]))
        o = self._obs if obs is None else self._policy_obs(obs)
        out = self._torch.empty((self.num_envs, self.nu), dtype=self._torch.float32, device=self.device)
        if cx is not None:
            net = _capi.make_net(_ptr(p), stride, widths, act, squash, action_scale)
            ctx = _capi.make_context(_ptr(cx), cx.shape[1])
            rc = self._lib.mz_net_eval_ctx(self._h, C.byref(net), None, None, C.byref(ctx), _ptr(o), _ptr(out), None, self._stream())
            _capi.check(self._lib, self._h, rc, "mz_net_eval_ctx")
        elif legacy:
            rc = self._lib.mz_policy_act(self._h, _ptr(p), stride, int(hidden), 1 if squash else 0, float(action_scale), _ptr(o), _ptr(out), self._stream())
            _capi.check(self._lib, self._h, rc, "mz_policy_act")
        else:
            net = _capi.make_net(_ptr(p), stride, widths, act, squash, action_scale)
            rc = self._lib.mz_net_act(self._h, C.byref(net), 0, 0, 0, _ptr(o), _ptr(out), None, self._stream())
            _capi.check(self._lib, self._h, rc, "mz_net_act")
        return out

    def rollout_policy(self, params, steps: int, hidden=0, squash: bool = False, action_scale: float = 1.0, obs=None,
                       return_obs: bool = False, return_actions: bool = False, value_params=None, value_hidden=0, gae=None,
                       activation: str = "tanh", value_activation: str = "tanh", return_next_obs: bool = False, context=None,
                       context_update=None, context_dims=None, return_contexts: bool = False):
        """K = `steps` closed-loop steps in one call: a = policy(obs); obs, reward, done = step(a) — exactly what K times
        (`policy_act`, `step`) give, state and outputs bit for bit.  params / hidden / squash / action_scale as in `policy_act`.
        The policy acts first on the env's last returned observation (what reset / step / rollout left in the observation buffer),
        or on `obs` [N, obs_dim] when given (copied into that buffer first).  set_state() does not refresh the buffer:
        `reset(mask=zeros)` returns every env's current observation without resetting any.

        Returns (obs, rewards [K, N], dones [K, N] uint8, info) like `rollout`; info["actions"] [K, N, nu] with `return_actions` (the
        policy's outputs, before the env's control clamp), info["observations"] [K, N, obs_dim] with `return_obs`.

        One mz_rollout_policy call — the Point, Swimmer and Reacher evaluate the policy inside their fused rollout kernels
        (`launch_info()["rollout_fused"]`), the other handles loop policy kernel + step launches inside the call — except where the
        host has work between steps (Python reward()/termination() overrides; per-env goals under auto-reset): there this method
        loops `policy_act` + `step` itself.

        value_params / value_hidden / gae: a critic evaluated along the way and the advantages from it, see `rollout_policy_sample`.
        hidden / activation as in `policy_act`, value_hidden / value_activation as in `value`: a network with two hidden layers or
        ReLU units, actor or critic, makes the call one mz_rollout_net.

        return_next_obs: info["next_observations"] [K, N, obs_dim] as in `rollout` (raw rows, whether or not a normaliser is bound);
        the call is then one mz_rollout_ex.

        context / context_update / context_dims / return_contexts: see `rollout_policy_sample`."""
        return self._rollout_closed_loop(False, params, steps, hidden, squash, action_scale, obs, None, None, return_obs, return_actions,
                                         value_params, value_hidden, gae, activation, value_activation, return_next_obs, context=context,
                                         context_update=context_update, context_dims=context_dims, return_contexts=return_contexts)

    def _noise_args(self, noise_seed, noise_step, advance: int):
        """(noise_seed, noise_step) of a draw as uint64: the env's own seed and counter where the caller gives none; the counter
        advances by `advance` only when it was used."""
        seed = self._noise_seed if noise_seed is None else int(noise_seed)
        if noise_step is None:
            step = self._noise_step
            self._noise_step += advance
        else:
            step = int(noise_step)
        return C.c_uint64(seed & 0xFFFFFFFFFFFFFFFF), C.c_uint64(step & 0xFFFFFFFFFFFFFFFF)

    def _head(self, log_std, log_std_bounds, squashed_logp, squash, mode):
        """The MzHead of `log_std="state"` (None for "param", where squashed_logp is refused)."""
        from mujoco_maze_amd import policy

        if not policy._log_std_kind(log_std):
            if squashed_logp:
                raise ValueError("squashed_logp needs log_std='state'")
            return None
        if mode != _capi.NOISE_PRE_SQUASH:
            raise ValueError("log_std='state' needs noise='pre_squash'")
        if squashed_logp and not squash:
            raise ValueError("squashed_logp needs squash=True: it is the density of action_scale * tanh(z)")
        lo, hi = policy.head_bounds(log_std_bounds)
        return _capi.make_head(float(lo), float(hi), bool(squashed_logp))

    def policy_sample(self, params, obs=None, hidden=0, squash: bool = False, action_scale: float = 1.0, noise_seed: Optional[int] = None,
                      noise_step: Optional[int] = None, activation: str = "tanh", noise: str = "pre_squash", log_std: str = "param",
                      log_std_bounds=(-20.0, 2.0), squashed_logp: bool = False, context=None):
        """One draw from a diagonal-Gaussian policy on the device (mz_policy_sample): (actions [N, nu], logp [N]).  params: float32
        [npar_s] or [N, npar_s], the vector of `policy_act` followed by log_std [nu] (`policy.pack(..., log_std=)`).  With m the
        network's pre-squash output, a = m + exp(log_std) * eps, or action_scale * tanh(.) of that with `squash`; logp is the density
        of the PRE-tanh sample, sum_u (-0.5 eps_u^2 - log_std_u - 0.9189385): apply the tanh correction from the actions yourself.

        eps is a pure function of (noise_seed, noise_step, global env slot, action index) — `policy.noise` —, so a draw does not
        depend on the batch size or on how a batch is sharded.  noise_seed defaults to the seed of the last `reset(seed=...)`, else the
        constructor's; noise_step to an env-held counter that starts at 0 (again after `reset(seed=...)`) and advances by 1 per call
        and by K per `rollout_policy_sample`.  Explicit values are used as given and leave the counter alone.

        hidden / activation as in `policy_act`; the noise and logp do not depend on the network's shape.

        noise="action" (TD3 / DDPG exploration, mz_net_sample): the noise goes on the action instead of through the squash —
        a = clip(action_scale * tanh(m) + exp(log_std) * eps, +-action_scale) with `squash`; without it the two modes are the same.
        eps and logp are those of the default "pre_squash" (logp: the density of the unclipped sum around the deterministic action).

        log_std="state" (SAC; mz_net_sample_head): the standard deviation is an output of the network.  params: float32 [count_h] or
        [N, count_h], a network whose output layer has 2 nu units — the means, then the raw log-stds — and no log_std vector
        (`policy.pack_mlp(.., log_std_head=)`, `policy.param_count(.., log_std="state")`); the raw log-std is clamped to
        `log_std_bounds` (lo, hi; -inf / inf switch a side off).  squashed_logp (needs `squash`): logp is the density of the squashed
        action action_scale * tanh(z) — the tanh correction applied on the device in a form that stays finite wherever z is — which
        is the sample SAC's entropy term takes.  `policy.sample_reference(.., log_std="state")` is the numpy model.

        context as in `policy_act`: the network reads [obs | context]; noise, logp and the head are unchanged (mz_net_eval_ctx)."""
        mode = _capi.noise_mode(noise)
        head = self._head(log_std, log_std_bounds, squashed_logp, squash, mode)
        widths, act, legacy = self._net_kind(hidden, activation)
        cx = None if context is None else self._context(context)
        p, stride = self._policy_params(params, hidden, stochastic=True, log_std=log_std, cdim=0 if cx is None else int(cx.shape[1]))
        o = self._obs if obs is None else self._policy_obs(obs)
        torch = self._torch
        out = torch.empty((self.num_envs, self.nu), dtype=torch.float32, device=self.device)
        logp = torch.empty(self.num_envs, dtype=torch.float32, device=self.device)
        seed, step = self._noise_args(noise_seed, noise_step, 1)
        if cx is not None:
            net = _capi.make_net(_ptr(p), stride, widths, act, squash, action_scale)
            nz = _capi.make_noise(mode, seed.value, step.value)
            ctx = _capi.make_context(_ptr(cx), cx.shape[1])
            rc = self._lib.mz_net_eval_ctx(self._h, C.byref(net), C.byref(head) if head is not None else None, C.byref(nz), C.byref(ctx), _ptr(o),
                                           _ptr(out), _ptr(logp), self._stream())
            _capi.check(self._lib, self._h, rc, "mz_net_eval_ctx")
        elif head is not None:
            net = _capi.make_net(_ptr(p), stride, widths, act, squash, action_scale)
            nz = _capi.make_noise(mode, seed.value, step.value)
            rc = self._lib.mz_net_sample_head(self._h, C.byref(net), C.byref(head), C.byref(nz), _ptr(o), _ptr(out), _ptr(logp), self._stream())
            _capi.check(self._lib, self._h, rc, "mz_net_sample_head")
        elif mode != _capi.NOISE_PRE_SQUASH:
            net = _capi.make_net(_ptr(p), stride, widths, act, squash, action_scale)
            nz = _capi.make_noise(mode, seed.value, step.value)
            rc = self._lib.mz_net_sample(self._h, C.byref(net), C.byref(nz), _ptr(o), _ptr(out), _ptr(logp), self._stream())
            _capi.check(self._lib, self._h, rc, "mz_net_sample")
        elif legacy:
            rc = self._lib.mz_policy_sample(self._h, _ptr(p), stride, int(hidden), 1 if squash else 0, float(action_scale), seed, step, _ptr(o), _ptr(out),
                                            _ptr(logp), self._stream())
            _capi.check(self._lib, self._h, rc, "mz_policy_sample")
        else:
            net = _capi.make_net(_ptr(p), stride, widths, act, squash, action_scale)
            rc = self._lib.mz_net_act(self._h, C.byref(net), 1, seed, step, _ptr(o), _ptr(out), _ptr(logp), self._stream())
            _capi.check(self._lib, self._h, rc, "mz_net_act")
        return out, logp

    def rollout_policy_sample(self, params, steps: int, hidden=0, squash: bool = False, action_scale: float = 1.0, obs=None,
                              noise_seed: Optional[int] = None, noise_step: Optional[int] = None, return_obs: bool = False,
                              return_actions: bool = False, value_params=None, value_hidden=0, gae=None, activation: str = "tanh",
                              value_activation: str = "tanh", noise: str = "pre_squash", return_next_obs: bool = False,
                              log_std: str = "param", log_std_bounds=(-20.0, 2.0), squashed_logp: bool = False, context=None,
                              context_update=None, context_dims=None, return_contexts: bool = False):
        """K = `steps` closed-loop steps with a sampled action each, in one call: exactly what K times (`policy_sample` with
        noise_step + k, `step`) give, state and outputs bit for bit.  Everything as in `rollout_policy`, plus info["logp"] [K, N], the
        log-probabilities of the draws (see `policy_sample`); info["actions"] [K, N, nu] with `return_actions` holds the sampled
        actions.  noise_seed / noise_step as in `policy_sample`; the env's counter advances by K.

        One mz_rollout_policy_sample call — sampled inside the fused rollout kernels of the Point, Swimmer and Reacher — except
        where the host has work between steps (as in `rollout_policy`): there this method loops `policy_sample` + `step` itself.

        With `value_params` (a critic as in `value`, `value_hidden` its hidden width) the call also returns info["values"] [K, N], the
        critic's value of the row the policy acted on at step k, and info["next_values"] [K, N], its value of the row step k produced
        BEFORE any auto-reset — for an env that finished, of its terminal observation, which is what a time-limit truncation
        (done & 2) bootstraps from; next_values[k] equals values[k + 1] wherever done[k] == 0.  With `gae=(gamma, lam)` as well,
        info["advantages"] and info["returns"] [K, N] (`gae`).  One mz_rollout_actor_critic call (the critic runs inside the fused
        kernels, on the row that is on chip anyway) plus one mz_gae call; the critic changes nothing else the call returns.  Where
        this method loops itself it loops `value` + `policy_sample` + `step` + `value`, with the terminal rows taken from
        info["final_observation"].

        hidden / activation as in `policy_act`, value_hidden / value_activation as in `value`: `hidden=(64, 64)`,
        `value_hidden=(64, 64)` is the default network of PPO / A2C code.  A network with two hidden layers or ReLU units, actor or
        critic, makes the call one mz_rollout_net — the same loop, the same fused kernels on the Point, Swimmer and Reacher.

        noise as in `policy_sample` ("action": TD3 / DDPG exploration), return_next_obs as in `rollout`: either makes the call one
        mz_rollout_ex, which runs the same kernels.  Together they collect an off-policy batch in one call: s = the entry observation
        followed by "observations"[:-1], a = "actions", r, s' = "next_observations", terminated = dones & 1.

        log_std="state" / log_std_bounds / squashed_logp as in `policy_sample` (a SAC actor): one mz_rollout_head call — sampled
        inside the fused rollout kernels of the Point, Swimmer and Reacher (chains of five or six links excepted), a loop of the head
        kernel and the step's launches inside the call on every other handle —, bit for bit what K times
        (`policy_sample(log_std="state")`, `step`) give; info["logp"] is then the entropy term's sample.  Critic, return_next_obs, a
        bound normaliser compose as above.

        context: a contiguous float32 device tensor [N, C], 1 <= C <= 32, that actor and critic read behind the observation (see
        `policy_act`; both networks packed for obs_dim + C inputs).  It is IN/OUT: on return it holds what step K would read, so two
        calls in a row equal one call over the joined steps.  context_update=None holds it for the whole call;
        context_update="relative" with context_dims=D (1 <= D <= min(C, obs_dim)) applies HIRO's goal transition after every step k, in
        float32, where dones[k] == 0:  tmp = c[:D] + s[:D];  c[:D] = tmp - s'[:D]  with s the raw row the actor acted on and s' the
        raw row the step produced ("next_observations"[k]); an env that finished keeps its context, entries d >= D hold.
        info["values"][k] reads the context of step k, info["next_values"][k] the context after the transition.  return_contexts:
        info["contexts"] [K, N, C], the context the networks read at step k.  `policy.context_transition_reference` is the numpy
        model.  One mz_rollout_ctx call, bit for bit what K times (`value`, `policy_sample(context=c, noise_step + k)`, `step`,
        `value`, the transition in torch) give; where the host has work between steps this method runs that loop itself."""
        return self._rollout_closed_loop(True, params, steps, hidden, squash, action_scale, obs, noise_seed, noise_step, return_obs,
                                         return_actions, value_params, value_hidden, gae, activation, value_activation, return_next_obs, noise,
                                         log_std, log_std_bounds, squashed_logp, context, context_update, context_dims, return_contexts)

    def _value_params(self, value_params, hidden, cdim: int = 0):
        """A critic's parameters as a contiguous float32 device tensor [nvpar] or [N, nvpar]; returns (tensor, env_stride)."""
        from mujoco_maze_amd import policy

        torch = self._torch
        policy.net_shape(hidden, what="the critic's hidden", max_width=self._max_width())
        npar = policy.param_count(self.obs_dim + cdim, 1, hidden, max_width=self._max_width())
        p = value_params if torch.is_tensor(value_params) else torch.as_tensor(np.asarray(value_params, dtype=np.float32), device=self.device)
        if p.dtype != torch.float32 or not p.is_contiguous() or p.device != self.device:
            p = p.to(device=self.device, dtype=torch.float32).contiguous()
        if tuple(p.shape) not in ((npar,), (self.num_envs, npar)):
            raise ValueError(f"value_params must have shape {(npar,)} (one critic) or {(self.num_envs, npar)} (one per env) for obs_dim "
                             f"{self.obs_dim}{f' + context {cdim}' if cdim else ''}, hidden {hidden}, got {tuple(p.shape)}")
        return p, (npar if p.dim() == 2 else 0)

    def value(self, value_params, obs=None, hidden=0, activation: str = "tanh", context=None):
        """Values [N] of a small critic evaluated on the device (mz_value): a policy of `policy_act` with one output, never squashed —
        affine (`hidden=0`) or one tanh hidden layer of up to 64 units.  value_params: float32 [nvpar] (one critic for all envs) or
        [N, nvpar] (one per env), nvpar = policy.param_count(obs_dim, 1, hidden), packed by `policy.pack` / `pack_linear` with
        nu = 1; obs: [N, obs_dim], default the env's last returned observation.  A new tensor per call.  `hidden` may also be a
        sequence of one or two widths (`policy.pack_mlp`), `activation="relu"` makes the hidden units ReLU (mz_net_value).

        context as in `policy_act`: the critic reads [obs | context], value_params packed for obs_dim + C inputs (mz_net_value_ctx).
        `value(vp, obs=rows, context=actions)` is Q(s, a) on the device."""
        widths, act, legacy = self._net_kind(hidden, activation, "the critic's hidden")
        cx = None if context is None else self._context(context)
        p, stride = self._value_params(value_params, hidden, 0 if cx is None else int(cx.shape[1]))
        o = self._obs if obs is None else self._policy_obs(obs)
        out = self._torch.empty(self.num_envs, dtype=self._torch.float32, device=self.device)
        if cx is not None:
            net = _capi.make_net(_ptr(p), stride, widths, act)
            ctx = _capi.make_context(_ptr(cx), cx.shape[1])
            rc = self._lib.mz_net_value_ctx(self._h, C.byref(net), C.byref(ctx), _ptr(o), _ptr(out), self._stream())
            _capi.check(self._lib, self._h, rc, "mz_net_value_ctx")
        elif legacy:
            rc = self._lib.mz_value(self._h, _ptr(p), stride, int(hidden), _ptr(o), _ptr(out), self._stream())
            _capi.check(self._lib, self._h, rc, "mz_value")
        else:
            net = _capi.make_net(_ptr(p), stride, widths, act)
            rc = self._lib.mz_net_value(self._h, C.byref(net), _ptr(o), _ptr(out), self._stream())
            _capi.check(self._lib, self._h, rc, "mz_net_value")
        return out

    def gae(self, rewards, dones, values, next_values, gamma: float = 0.99, lam: float = 0.95, out=None):
        """Generalised advantage estimates of a rollout in one kernel (mz_gae): rewards, values, next_values float32 [K, N], dones
        uint8 [K, N] as `rollout_policy_sample(..., value_params=)` returns them.  Per env, from the last step back, in float32:
        delta = reward + (0 if done & 1 else gamma * next_value) - value; adv = delta + (0 if done else gamma * lam * adv of the
        step after).  A true termination does not bootstrap, a time limit alone bootstraps from the terminal observation's value,
        any episode end cuts the recursion (`policy.gae_reference` is the numpy model).  Returns (advantages, returns = advantages +
        values), new [K, N] tensors — or the pair `out`."""
        torch, n = self._torch, self.num_envs

        def arr(t, dtype, what):
            t = t if torch.is_tensor(t) else torch.as_tensor(np.asarray(t), device=self.device)
            if t.dtype != dtype or not t.is_contiguous() or t.device != self.device:
                t = t.to(device=self.device, dtype=dtype).contiguous()
            if t.dim() != 2 or t.shape[1] != n:
                raise ValueError(f"{what} must have shape (K, {n}), got {tuple(t.shape)}")
            return t

        r, d = arr(rewards, torch.float32, "rewards"), arr(dones, torch.uint8, "dones")
        v, nv = arr(values, torch.float32, "values"), arr(next_values, torch.float32, "next_values")
        K = int(r.shape[0])
        if not (d.shape == v.shape == nv.shape == r.shape) or not 1 <= K <= 65536:
            raise ValueError(f"rewards, dones, values and next_values must share one (K, {n}) shape with 1 <= K <= 65536, got "
                             f"{tuple(r.shape)}, {tuple(d.shape)}, {tuple(v.shape)}, {tuple(nv.shape)}")
        adv, ret = out if out is not None else (torch.empty_like(r), torch.empty_like(r))
        rc = self._lib.mz_gae(self._h, K, _ptr(r), _ptr(d), _ptr(v), _ptr(nv), float(gamma), float(lam), _ptr(adv), _ptr(ret), self._stream())
        _capi.check(self._lib, self._h, rc, "mz_gae")
        return adv, ret

    def return_scan(self, rewards, dones, gamma: float = 1.0, carry=None, length_carry=None):
        """Running discounted returns and episode step counts of a rollout in one kernel (mz_return_scan): rewards float32 [K, N],
        dones uint8 [K, N].  Per env, from the first step on, in float32: ret = gamma * carry + reward; length += 1; an episode end
        (done != 0) then clears both.  carry: float32 [N], length_carry: int32 [N] — contiguous tensors on the env's device, UPDATED IN
        PLACE, so that the next rollout's scan continues where this one stopped; None: fresh zeros for this call.  With gamma = 1
        `ret_seq[dones != 0]` are the returns of the episodes that ended and `len_seq[dones != 0]` their lengths; with gamma < 1
        ret_seq is the series whose running variance reward scaling divides by (`normalize.RunningMeanStd`).
        `policy.return_scan_reference` is the numpy model, bit-equal.  Returns (ret_seq float32 [K, N], len_seq int32 [K, N])."""
        torch, n = self._torch, self.num_envs

        def arr(t, dtype, what):
            t = t if torch.is_tensor(t) else torch.as_tensor(np.asarray(t), device=self.device)
            if t.dtype != dtype or not t.is_contiguous() or t.device != self.device:
                t = t.to(device=self.device, dtype=dtype).contiguous()
            if t.dim() != 2 or t.shape[1] != n:
                raise ValueError(f"{what} must have shape (K, {n}), got {tuple(t.shape)}")
            return t

        def carried(t, dtype, what):
            if t is None:
                return torch.zeros(n, dtype=dtype, device=self.device)
            if not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != (n,) or t.device != self.device or not t.is_contiguous():
                raise ValueError(f"{what} must be a contiguous {dtype} tensor of shape {(n,)} on {self.device} (it is updated in place)")
            return t

        r, d = arr(rewards, torch.float32, "rewards"), arr(dones, torch.uint8, "dones")
        K = int(r.shape[0])
        if d.shape != r.shape or not 1 <= K <= 65536:
            raise ValueError(f"rewards and dones must share one (K, {n}) shape with 1 <= K <= 65536, got {tuple(r.shape)}, {tuple(d.shape)}")
        c, lc = carried(carry, torch.float32, "carry"), carried(length_carry, torch.int32, "length_carry")
        ret, ln = torch.empty_like(r), torch.empty((K, n), dtype=torch.int32, device=self.device)
        rc = self._lib.mz_return_scan(self._h, K, _ptr(r), _ptr(d), float(gamma), _ptr(c), _ptr(lc), _ptr(ret), _ptr(ln), self._stream())
        _capi.check(self._lib, self._h, rc, "mz_return_scan")
        return ret, ln

    def _rollout_closed_loop(self, sample: bool, params, steps, hidden, squash, action_scale, obs, noise_seed, noise_step, return_obs,
                             return_actions, value_params, value_hidden, gae, activation="tanh", value_activation="tanh",
                             return_next_obs=False, noise="pre_squash", log_std="param", log_std_bounds=(-20.0, 2.0), squashed_logp=False,
                             context=None, context_update=None, context_dims=None, return_contexts=False):
        """rollout_policy (sample False) / rollout_policy_sample (sample True): the defining loop where the host has work between
        steps, else one C call — mz_rollout_head with log_std="state"; mz_rollout_ex with return_next_obs or noise="action";
        mz_rollout_net where a network, actor or critic, needs mz_net; mz_rollout_actor_critic with a critic; mz_rollout_policy_sample /
        mz_rollout_policy without one.  With a context: mz_rollout_ctx, whatever else the call asks for."""
        torch, n = self._torch, self.num_envs
        if context is None:
            if context_update is not None or context_dims is not None or return_contexts:
                raise ValueError("context_update, context_dims and return_contexts need context=")
            cx, cdim, cupd, D = None, 0, _capi.CTX_HOLD, 0
        else:
            cx = self._context(context, in_place=True)
            cdim = int(cx.shape[1])
            cupd, D = _capi.context_args(cdim, self.obs_dim, context_update, context_dims)
        mode = _capi.noise_mode(noise)
        head = self._head(log_std, log_std_bounds, squashed_logp, squash, mode) if sample else None
        extended = return_next_obs or mode != _capi.NOISE_PRE_SQUASH or head is not None
        with_critic = value_params is not None
        if gae is not None and not with_critic:
            raise ValueError("gae=(gamma, lam) needs a critic: pass value_params")
        if gae is not None:
            gamma, lam = (float(x) for x in gae)
        widths, act, legacy = self._net_kind(hidden, activation)
        p, stride = self._policy_params(params, hidden, stochastic=sample, log_std=log_std if sample else "param", cdim=cdim)
        if with_critic:
            vwidths, vact, vlegacy = self._net_kind(value_hidden, value_activation, "the critic's hidden")
            vp, vstride = self._value_params(value_params, value_hidden, cdim)
            legacy = legacy and vlegacy
        K = int(steps)
        if not 1 <= K <= 65536:
            raise ValueError(f"a rollout takes 1 .. 65536 steps, got {K}")
        if obs is not None:
            o = self._policy_obs(obs)
            if o.data_ptr() != self._obs.data_ptr():
                self._obs.copy_(o)
        buf = self._rollout_buffers(K, return_obs, return_next_obs)
        if return_actions and "actions" not in buf:
            buf["actions"] = torch.empty((K, n, self.nu), dtype=torch.float32, device=self.device)
        for key in (("logp",) if sample else ()) + (("values", "next_values") if with_critic else ()) + (("advantages", "returns") if gae is not None else ()):
            if key not in buf:
                buf[key] = torch.empty((K, n), dtype=torch.float32, device=self.device)
        if return_contexts and ("contexts" not in buf or buf["contexts"].shape[2] != cdim):
            buf["contexts"] = torch.empty((K, n, cdim), dtype=torch.float32, device=self.device)
        seed, step = self._noise_args(noise_seed, noise_step, K) if sample else (C.c_uint64(0), C.c_uint64(0))
        if self._host_rewards or (self._env_goals is not None and self._auto_reset):
            for k in range(K):
                if return_contexts:
                    buf["contexts"][k] = cx
                if D:
                    s_old = self._obs[:, :D].clone()
                if with_critic:
                    buf["values"][k] = self.value(vp, None, value_hidden, value_activation, cx)
                if sample:
                    a, buf["logp"][k] = self.policy_sample(p, None, hidden, squash, action_scale, seed.value, step.value + k, activation, noise,
                                                           log_std, log_std_bounds, squashed_logp, cx)
                else:
                    a = self.policy_act(p, None, hidden, squash, action_scale, activation, cx)
                o, rew, done, inf = self.step(a)
                buf["reward"][k], buf["done"][k], buf["goal"][k], buf["info"][k] = rew, done, inf["goal_index"], self._info
                if D:  # the relative transition where the episode goes on: there `o` is the row the step produced
                    nxt = cx[:, :D] + s_old
                    nxt = nxt - o[:, :D]
                    cx[:, :D] = torch.where((done == 0).unsqueeze(1), nxt, cx[:, :D])
                if with_critic:
                    nv = self.value(vp, None, value_hidden, value_activation, cx)
                    if self._auto_reset:  # an env that finished: the value of its terminal row, which `o` no longer holds
                        nv = torch.where(done != 0, self.value(vp, inf["final_observation"], value_hidden, value_activation, cx), nv)
                    buf["next_values"][k] = nv
                if return_obs:
                    buf["obs_seq"][k] = o
                if return_next_obs:
                    buf["next_obs_seq"][k] = self._next_obs_row(o, done, inf)
                if return_actions:
                    buf["actions"][k] = a
        elif extended or cx is not None:
            io = _capi.make_rollout_io(K, actor=_capi.make_net(_ptr(p), stride, widths, act, squash, action_scale),
                                       noise=_capi.make_noise(mode, seed.value, step.value) if sample else None,
                                       critic=_capi.make_net(_ptr(vp), vstride, vwidths, vact) if with_critic else None,
                                       obs_dev=_ptr(self._obs), reward_dev=_ptr(buf["reward"]), done_dev=_ptr(buf["done"]),
                                       goal_idx_dev=_ptr(buf["goal"]), info_dev=_ptr(buf["info"]),
                                       obs_seq_dev=_ptr(buf["obs_seq"]) if return_obs else None,
                                       actions_seq_dev=_ptr(buf["actions"]) if return_actions else None,
                                       logp_seq_dev=_ptr(buf["logp"]) if sample else None,
                                       value_seq_dev=_ptr(buf["values"]) if with_critic else None,
                                       next_value_seq_dev=_ptr(buf["next_values"]) if with_critic else None,
                                       next_obs_seq_dev=_ptr(buf["next_obs_seq"]) if return_next_obs else None)
            if cx is not None:
                ctx = _capi.make_context(_ptr(cx), cdim, cupd, D, _ptr(buf["contexts"]) if return_contexts else None)
                rc = self._lib.mz_rollout_ctx(self._h, C.byref(io), C.byref(head) if head is not None else None, C.byref(ctx), self._stream())
                _capi.check(self._lib, self._h, rc, "mz_rollout_ctx")
            elif head is not None:
                rc = self._lib.mz_rollout_head(self._h, C.byref(io), C.byref(head), self._stream())
                _capi.check(self._lib, self._h, rc, "mz_rollout_head")
            else:
                rc = self._lib.mz_rollout_ex(self._h, C.byref(io), self._stream())
                _capi.check(self._lib, self._h, rc, "mz_rollout_ex")
        elif not legacy:
            actor = _capi.make_net(_ptr(p), stride, widths, act, squash, action_scale)
            critic = _capi.make_net(_ptr(vp), vstride, vwidths, vact) if with_critic else None
            rc = self._lib.mz_rollout_net(self._h, K, C.byref(actor), 1 if sample else 0, seed, step, C.byref(critic) if with_critic else None,
                                          _ptr(buf["values"]) if with_critic else None, _ptr(buf["next_values"]) if with_critic else None,
                                          _ptr(self._obs), _ptr(buf["reward"]), _ptr(buf["done"]), _ptr(buf["goal"]), _ptr(buf["info"]),
                                          _ptr(buf["obs_seq"]) if return_obs else None, _ptr(buf["actions"]) if return_actions else None,
                                          _ptr(buf["logp"]) if sample else None, self._stream())
            _capi.check(self._lib, self._h, rc, "mz_rollout_net")
        else:
            legacy_args = (self._h, K, _ptr(p), stride, int(hidden), 1 if squash else 0, float(action_scale))
            outputs = (_ptr(self._obs), _ptr(buf["reward"]), _ptr(buf["done"]), _ptr(buf["goal"]), _ptr(buf["info"]),
                       _ptr(buf["obs_seq"]) if return_obs else None, _ptr(buf["actions"]) if return_actions else None)
            if with_critic:
                critic = _capi.MzCritic(_ptr(vp), vstride, int(value_hidden), 0, _ptr(buf["values"]), _ptr(buf["next_values"]))
                rc = self._lib.mz_rollout_actor_critic(*legacy_args, 1 if sample else 0, seed, step, C.byref(critic), *outputs,
                                                       _ptr(buf["logp"]) if sample else None, self._stream())
                _capi.check(self._lib, self._h, rc, "mz_rollout_actor_critic")
            elif sample:
                rc = self._lib.mz_rollout_policy_sample(*legacy_args, seed, step, *outputs, _ptr(buf["logp"]), self._stream())
                _capi.check(self._lib, self._h, rc, "mz_rollout_policy_sample")
            else:
                rc = self._lib.mz_rollout_policy(*legacy_args, *outputs, self._stream())
                _capi.check(self._lib, self._h, rc, "mz_rollout_policy")
        per_step = {}
        if with_critic:
            per_step["values"], per_step["next_values"] = buf["values"], buf["next_values"]
        if sample:
            per_step["logp"] = buf["logp"]
        if return_contexts:
            per_step["contexts"] = buf["contexts"]
        if gae is not None:
            per_step["advantages"], per_step["returns"] = self.gae(buf["reward"], buf["done"], buf["values"], buf["next_values"], gamma, lam,
                                                                   out=(buf["advantages"], buf["returns"]))
        return self._obs, buf["reward"], buf["done"], self._rollout_info(buf, return_obs, return_next_obs, return_actions, **per_step)

    def _rollout_buffers(self, K: int, with_obs: bool, with_next_obs: bool = False) -> dict:
        """Output tensors of rollout(), allocated per K and kept."""
        torch, n, dev = self._torch, self.num_envs, self.device
        cache = self.__dict__.setdefault("_rollout_cache", {})
        buf = cache.get(K)
        if buf is None:
            buf = cache[K] = {"reward": torch.empty((K, n), dtype=torch.float32, device=dev), "done": torch.empty((K, n), dtype=torch.uint8, device=dev),
                              "goal": torch.empty((K, n), dtype=torch.int32, device=dev), "info": torch.empty((K, n, 4), dtype=torch.float32, device=dev)}
        if with_obs and "obs_seq" not in buf:
            buf["obs_seq"] = torch.empty((K, n, self.obs_dim), dtype=torch.float32, device=dev)
        if with_next_obs and "next_obs_seq" not in buf:
            buf["next_obs_seq"] = torch.empty((K, n, self.obs_dim), dtype=torch.float32, device=dev)
        return buf

    def _apply_host_task(self):
        """User-defined Python reward()/termination(): evaluated on the host from the obs batch (one device-to-host copy
        per step; the kernel supplied the inner reward terms, the task part is computed here).  With
        auto-reset the host then resets exactly the envs ITS verdict finished (the kernel's auto-reset is off for these
        tasks, see set_auto_reset)."""
        torch = self._torch
        m = self.model.c
        # one device-to-host copy: obs | info | done packed into one tensor
        packed = torch.cat([self._obs, self._info, self._done.to(torch.float32).unsqueeze(1)], dim=1).double().cpu().numpy()
        obs, inf, dev_done = packed[:, : self.obs_dim], packed[:, self.obs_dim: self.obs_dim + 4], packed[:, -1].astype(np.uint8)
        inner = (m.forward_reward_weight * inf[:, 2] + inf[:, 3]) * m.inner_reward_scaling  # ant.py:68, swimmer.py:43
        if m.robot == 0:
            inner[:] = 0.0  # point.py:61
        rew = np.array([self._task.reward(o) for o in obs]) + inner
        term = np.array([bool(self._task.termination(o)) for o in obs])
        done = (term.astype(np.uint8) | (dev_done & 2)).astype(np.uint8)
        self._reward.copy_(torch.as_tensor(rew, dtype=torch.float32))
        self._done.copy_(torch.as_tensor(done))
        # the device's first-match goal index belongs to the built-in task descriptor, not to the Python override that just
        # judged the step: it is not defined for host-judged tasks
        self._goal.fill_(-1)
        if self._auto_reset and done.any():
            if self._host_mask is None:  # persistent: the reset kernel may still read it after this call returns
                self._host_mask = torch.empty(self.num_envs, dtype=torch.uint8, device=self.device)
            torch.ne(self._done, 0, out=self._host_mask.view(torch.bool))
            self._final_obs[self._host_mask.view(torch.bool)] = self._obs[self._host_mask.view(torch.bool)]
            rc = self._lib.mz_reset(self._h, _ptr(self._host_mask), C.c_uint64(self._seed), _ptr(self._obs), self._stream())
            _capi.check(self._lib, self._h, rc, "mz_reset (host-judged auto-reset)")
            self._seed += 1

    def get_state(self):
        torch, n = self._torch, self.num_envs
        qpos = torch.empty((n, self.nq), dtype=torch.float32, device=self.device)
        qvel = torch.empty((n, self.nv), dtype=torch.float32, device=self.device)
        warm = torch.empty((n, self.nv), dtype=torch.float32, device=self.device)
        t = torch.empty(n, dtype=torch.int32, device=self.device)
        _capi.check(self._lib, self._h, self._lib.mz_get_state(self._h, _ptr(qpos), _ptr(qvel), _ptr(warm), _ptr(t), self._stream()), "mz_get_state")
        return qpos, qvel, warm, t

    def set_state(self, qpos=None, qvel=None, warmstart=None, t=None):
        torch = self._torch

        def prep(x, dt, shape):
            if x is None:
                return None
            x = torch.as_tensor(x, device=self.device).to(dt).contiguous()
            if tuple(x.shape) != shape:
                raise ValueError(f"expected shape {shape}, got {tuple(x.shape)}")
            return x

        n = self.num_envs
        qpos = prep(qpos, torch.float32, (n, self.nq)); qvel = prep(qvel, torch.float32, (n, self.nv))
        warmstart = prep(warmstart, torch.float32, (n, self.nv)); t = prep(t, torch.int32, (n,))
        rc = self._lib.mz_set_state(self._h, _ptr(qpos), _ptr(qvel), _ptr(warmstart), _ptr(t), self._stream())
        _capi.check(self._lib, self._h, rc, "mz_set_state")
        torch.cuda.current_stream(self.device).synchronize()  # inputs may be temporaries

    def status(self):
        out = self._torch.empty(self.num_envs, dtype=self._torch.int32, device=self.device)
        _capi.check(self._lib, self._h, self._lib.mz_get_status(self._h, _ptr(out), self._stream()), "mz_get_status")
        return out

    def debug_forward(self, actions=None):
        torch, n = self._torch, self.num_envs
        qacc = torch.empty((n, self.nv), dtype=torch.float32, device=self.device)
        counts = torch.empty((n, 2), dtype=torch.int32, device=self.device)
        a = None if actions is None else torch.as_tensor(actions, device=self.device).to(torch.float32).contiguous()
        _capi.check(self._lib, self._h, self._lib.mz_debug_forward(self._h, _ptr(a), _ptr(qacc), _ptr(counts), self._stream()), "mz_debug_forward")
        return qacc, counts

    def debug_task_eval(self, obs):
        """Task reward / termination / first matching goal for rows of observations [n, obs_dim] (parity tests)."""
        torch = self._torch
        o = torch.as_tensor(obs, device=self.device).to(torch.float32).contiguous()
        n = o.shape[0]
        rew = torch.empty(n, dtype=torch.float32, device=self.device)
        done = torch.empty(n, dtype=torch.uint8, device=self.device)
        gi = torch.empty(n, dtype=torch.int32, device=self.device)
        _capi.check(self._lib, self._h, self._lib.mz_debug_task_eval(self._h, n, _ptr(o), _ptr(rew), _ptr(done), _ptr(gi), self._stream()), "mz_debug_task_eval")
        torch.cuda.current_stream(self.device).synchronize()
        return rew, done, gi

    def debug_detect(self, old_xy, new_xy):
        """The Point's manual wall rule on float64 moves [n, 2]: (hit, point, final_xy); hit 0 none, 1 bounce, 2 give-up, -1 collinear."""
        torch = self._torch
        o = torch.as_tensor(np.asarray(old_xy, np.float64), device=self.device).contiguous()
        w = torch.as_tensor(np.asarray(new_xy, np.float64), device=self.device).contiguous()
        n = o.shape[0]
        hit = torch.empty(n, dtype=torch.int32, device=self.device)
        pt = torch.zeros((n, 2), dtype=torch.float64, device=self.device)
        fin = torch.empty((n, 2), dtype=torch.float64, device=self.device)
        _capi.check(self._lib, self._h, self._lib.mz_debug_detect(self._h, n, _ptr(o), _ptr(w), _ptr(hit), _ptr(pt), _ptr(fin), self._stream()), "mz_debug_detect")
        torch.cuda.current_stream(self.device).synchronize()
        return hit, pt, fin

    def phase_cycles(self):
        """Phase timers of the instrumented kernel (set_option('profile_phases', 1) first)."""
        out = (C.c_uint64 * 16)()
        _capi.check(self._lib, self._h, self._lib.mz_read_phase_cycles(self._h, out), "mz_read_phase_cycles")
        return list(out)

    def wave_cycles(self, n: int):
        """Per-workgroup cycle totals of the instrumented kernel since the last call (numpy uint64 [n])."""
        out = np.zeros(n, np.uint64)
        _capi.check(self._lib, self._h, self._lib.mz_read_wave_cycles(self._h, out.ctypes.data_as(C.c_void_p), n), "mz_read_wave_cycles")
        self.last_wave_newton_iters = out >> np.uint64(40)  # Newton iterations the wave ran (packed above the cycle count)
        return out & np.uint64((1 << 40) - 1)

    def wave_phase_cycles(self, n: int):
        """Per-workgroup phase cycles of the instrumented kernel since the last call (numpy uint64 [n, 16])."""
        out = np.zeros((n, 16), np.uint64)
        _capi.check(self._lib, self._h, self._lib.mz_read_wave_phase_cycles(self._h, out.ctypes.data_as(C.c_void_p), n), "mz_read_wave_phase_cycles")
        return out

    def kernel_ms(self) -> float:
        return float(self._lib.mz_last_kernel_ms(self._h))

    # -- render / export bridge (render.py; reference: MazeEnv.render, maze_env.py:389-420) ----------------------------
    def render(self, mode: str = "rgb_array", env_index: int = 0, image_shape: Tuple[int, int] = (600, 480)):
        """Top view of env `env_index` as an uint8 [H, W, 3] array: its state is pulled from the device and rasterised on the
        host (render.render_top_down).  There is no GL context or websocket server next to a device batch: every mode
        returns the array."""
        from mujoco_maze_amd import render as R

        qpos = self.get_state()[0][env_index].double().cpu().numpy()
        return R.render_top_down(self.model, qpos, image_shape)

    def render_batch(self, env_indices=None, image_shape: Tuple[int, int] = (600, 480), qpos=None, out=None):
        """Top views of many envs at once, drawn on the device (mz_render): uint8 [k, H, W, 3] on `self.device` with, for every
        env, the pixels render.render_top_down draws for its state (image_shape = (width, height), row 0 at the top).

        env_indices: the envs to draw (a sequence of ints or an int tensor; any order, repeats allowed), default all.  qpos:
        float32 [k, nq] states to draw instead of the envs' current ones (the envs then only pick the per-env goals).  out: a
        contiguous uint8 [k, H, W, 3] tensor on the device to draw into.  Enqueued on the current stream without a host
        synchronisation: called right after step() it draws the post-step state — under auto-reset the new episode's first
        state, like the observation.  Indices in a device tensor are not checked on the host: an index outside the batch gives an
        all-zero image."""
        from mujoco_maze_amd import render as R

        torch, n = self._torch, self.num_envs
        if self.model.c.robot == ROBOT_ID["generic"]:
            raise NotImplementedError("render_batch: render.py does not draw a user robot's geoms (ROBOT = \"generic\")")
        w, h = (int(v) for v in image_shape)
        if w < 2 or h < 2 or w > 16384 or h > 16384:
            raise ValueError(f"image_shape must be (width, height) with 2 <= width, height <= 16384, got {tuple(image_shape)}")
        idx = None
        if env_indices is not None:
            if torch.is_tensor(env_indices):
                if env_indices.dim() != 1 or env_indices.dtype not in (torch.int32, torch.int64):
                    raise ValueError("env_indices must be a 1-D integer tensor")
                idx = env_indices.to(device=self.device, dtype=torch.int32).contiguous()
            else:
                a = np.asarray(env_indices)
                if a.ndim != 1 or (a.size and a.dtype.kind not in "iu"):
                    raise ValueError("env_indices must be a 1-D sequence of ints")
                if a.size and (a.min() < 0 or a.max() >= n):
                    raise ValueError(f"env_indices must lie in 0 .. {n - 1}")
                idx = torch.from_numpy(a.astype(np.int32)).pin_memory().to(self.device, non_blocking=True)
            k = idx.shape[0]
        q = None
        if qpos is not None:
            q = qpos if torch.is_tensor(qpos) else torch.as_tensor(np.asarray(qpos, np.float32))
            if q.dim() != 2 or q.shape[1] != self.nq or not q.is_floating_point():
                raise ValueError(f"qpos must be a float tensor of shape [k, nq = {self.nq}], got {tuple(q.shape)} {q.dtype}")
            q = q.to(device=self.device, dtype=torch.float32).contiguous()
            if idx is not None and q.shape[0] != k:
                raise ValueError(f"qpos has {q.shape[0]} rows for {k} env_indices")
            if idx is None:
                k = q.shape[0]
                if k > n:
                    raise ValueError(f"qpos has {k} rows, more than the {n} envs: pass env_indices")
        if idx is None and q is None:
            k = n
        shape = (k, h, w, 3)
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=self.device)
        elif not torch.is_tensor(out) or tuple(out.shape) != shape or out.dtype != torch.uint8 or not out.is_contiguous() \
                or out.device != self.device:
            raise ValueError(f"out must be a contiguous uint8 tensor of shape {shape} on {self.device}")
        rgb, size = R.goal_style(self.model)
        rgb, size = np.ascontiguousarray(rgb, np.uint8), np.ascontiguousarray(size, np.float64)
        rc = self._lib.mz_render(self._h, _ptr(q), _ptr(idx), k, w, h, len(size), rgb.ctypes.data_as(C.c_void_p),
                                 size.ctypes.data_as(C.c_void_p), _ptr(out), self._stream())
        _capi.check(self._lib, self._h, rc, "mz_render")
        return out

    def state_for_viewer(self, env_index: int = 0) -> dict:
        """MJCF of the model + the env's qpos / qvel (plain lists) for replay in an external MuJoCo viewer."""
        from mujoco_maze_amd import render as R

        qpos, qvel, _, _ = self.get_state()
        return R.state_for_viewer(self.model, qpos[env_index].double().cpu().numpy(), qvel[env_index].double().cpu().numpy())

    @property
    def has_extended_obs(self) -> bool:
        return bool(self._task.TOP_DOWN_VIEW or self._task.OBSERVE_BLOCKS or self._task.OBSERVE_BALLS)


class MazeEnv:
    """Single environment with the reference's constructor and step/reset shapes."""

    def __init__(self, model_cls: Type[AgentModel], maze_task: Type[MazeTask] = MazeTask, include_position: bool = True,
                 maze_height: float = 0.5, maze_size_scaling: float = 4.0, inner_reward_scaling: float = 1.0,
                 restitution_coef: float = 0.8, task_kwargs: Optional[dict] = None, websock_port: Optional[int] = None,
                 camera_move_x=None, camera_move_y=None, camera_zoom=None, image_shape: Tuple[int, int] = (600, 480),
                 **kwargs) -> None:
        self.vec = VecMazeEnv(model_cls, maze_task, num_envs=1, maze_height=maze_height, maze_size_scaling=maze_size_scaling,
                              inner_reward_scaling=inner_reward_scaling, restitution_coef=restitution_coef,
                              task_kwargs=task_kwargs, **kwargs)
        self._task = self.vec._task
        self.wrapped_env = WrappedRobot(self.vec, model_cls, single=True)
        self.t = 0
        self.action_space = self.vec.action_space
        self.observation_space = self.vec.observation_space
        self._max_steps = self.vec.model.c.max_episode_steps
        self._image_shape = image_shape

    def render(self, mode="human", **kwargs):
        """The reference hands back MuJoCo's camera image (or pushes it to its websocket viewer); here: the host-side top
        view of the device state (render.py), as an uint8 [H, W, 3] array in every mode."""
        return self.vec.render(mode, 0, self._image_shape)

    @property
    def unwrapped(self):
        return self

    @property
    def has_extended_obs(self) -> bool:
        return self.vec.has_extended_obs

    @property
    def _observe_balls(self) -> bool:
        return self._task.OBSERVE_BALLS

    def get_ori(self) -> float:
        return self.wrapped_env.get_ori()  # maze_env.py:231-232

    def reset(self, *, return_info: bool = True, **kwargs):
        """`(obs, info)` like the reference's MazeEnv.reset (maze_env.py:371-382).  `return_info=False` hands back the bare
        observation — the old-gym convention the reference's own tests are written against (`env.reset().shape`,
        tests/test_envs.py:13,27), for callers that have not moved to the tuple."""
        self.t = 0
        obs = self.vec.reset(seed=kwargs.get("seed"))[0].double().cpu().numpy()
        return (obs, {}) if return_info else obs

    def step(self, action):
        self.t += 1
        v = self.vec
        torch = v._torch
        if getattr(self, "_act_dev", None) is None:  # pinned staging for the action: an asynchronous upload, no allocation per step
            self._act_host = torch.empty((1, v.nu), dtype=torch.float32, pin_memory=True)
            self._act_dev = torch.empty((1, v.nu), dtype=torch.float32, device=v.device)
        self._act_host.numpy()[0, :] = np.asarray(action, dtype=np.float32).reshape(-1)
        self._act_dev.copy_(self._act_host, non_blocking=True)
        obs, reward, done, info = v.step(self._act_dev)
        # ONE device-to-host copy per step (obs | reward | done | info packed on the device): six separate reads were six synchronisations
        # (round 6: 158 -> 60 us per PointUMaze step)
        host = torch.cat([obs[0], reward, done.to(torch.float32), v._info[0]]).cpu().numpy().astype(np.float64)
        k = v.obs_dim
        d = int(host[k + 1])
        out_info = {"position": host[k + 2: k + 4].copy(), "reward_forward": float(host[k + 4]), "reward_ctrl": float(host[k + 5])}
        if d & 2:
            out_info["TimeLimit.truncated"] = not (d & 1)
        return host[:k].copy(), float(host[k]), bool(d), out_info

    def close(self) -> None:
        self.vec.close()
