"""ctypes binding of the C-ABI (include/mazestep.h) — libmazestep.so.

There is no CPU path: if the HIP library is missing, or no GPU is visible when an
environment is created, the call raises.  (`load(require_gpu=False)` is only for
checking that the library loads and exports every declared symbol.)
"""
import ctypes as C
import os

from mujoco_maze_amd.model import MzModel

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB_PATH = os.path.join(_HERE, "csrc", "libmazestep.so")
# A/B timing of a developer library (`make dev` / `make dev1`) or of a library built from another commit only: the override is announced on stderr when the library is loaded and
# recorded in bench.py's JSON line (config.library), so a stale variable cannot swap the stepper silently
# — and it is honoured only together with MZ_DEBUG=1 (a developer's shell), never on its own
LIB_PATH = (os.environ.get("MZ_LIBMAZESTEP_EXPERIMENT") if os.environ.get("MZ_DEBUG") == "1" else None) or DEFAULT_LIB_PATH

# every entry point declared in include/mazestep.h
SYMBOLS = [
    "mz_abi_version", "mz_model_sizeof", "mz_create", "mz_destroy", "mz_last_error", "mz_num_envs", "mz_obs_dim", "mz_nq",
    "mz_nv", "mz_nu", "mz_set_option", "mz_reset", "mz_set_state", "mz_get_state", "mz_step", "mz_get_status",
    "mz_debug_forward", "mz_last_kernel_ms", "mz_read_phase_cycles", "mz_bind_final_obs", "mz_debug_task_eval", "mz_debug_detect", "mz_read_wave_cycles", "mz_bind_record",
    "mz_set_goals", "mz_read_wave_phase_cycles", "mz_get_info", "mz_bind_env_goals", "mz_render", "mz_rollout",
    "mz_policy_act", "mz_rollout_policy", "mz_policy_sample", "mz_rollout_policy_sample",
    "mz_value", "mz_rollout_actor_critic", "mz_gae",
    "mz_net_act", "mz_net_value", "mz_rollout_net",
    "mz_bind_obs_norm", "mz_return_scan",
    "mz_net_sample", "mz_rollout_ex",
    "mz_net_sample_head", "mz_rollout_head",
    "mz_net_eval_ctx", "mz_net_value_ctx", "mz_rollout_ctx",
]


class MzCritic(C.Structure):
    """`mz_critic` of include/mazestep.h: the critic of one mz_rollout_actor_critic call."""
    _fields_ = [("params_dev", C.c_void_p), ("env_stride", C.c_int64), ("hidden", C.c_int32), ("reserved", C.c_int32),
                ("value_seq_dev", C.c_void_p), ("next_value_seq_dev", C.c_void_p)]


ACT_TANH, ACT_RELU = 0, 1  # MZ_ACT_* (include/mazestep.h)


class MzNet(C.Structure):
    """`mz_net` of include/mazestep.h: a network of up to two hidden layers, actor or critic, of one mz_net_* call."""
    _fields_ = [("struct_size", C.c_uint32), ("n_hidden", C.c_int32), ("hidden", C.c_int32 * 2), ("activation", C.c_int32),
                ("squash", C.c_int32), ("action_scale", C.c_double), ("params_dev", C.c_void_p), ("env_stride", C.c_int64)]


def make_net(params_ptr, env_stride: int, widths, activation: int, squash: bool = False, action_scale: float = 1.0) -> MzNet:
    """An MzNet with struct_size set; widths: a sequence of 0 .. 2 hidden widths."""
    w = tuple(int(x) for x in widths)
    return MzNet(C.sizeof(MzNet), len(w), (C.c_int32 * 2)(*(w + (0, 0))[:2]), int(activation), 1 if squash else 0, float(action_scale), params_ptr,
                 int(env_stride))


NOISE_PRE_SQUASH, NOISE_ACTION = 0, 1  # MZ_NOISE_* (include/mazestep.h)
NOISE_MODES = {"pre_squash": NOISE_PRE_SQUASH, "action": NOISE_ACTION}


def noise_mode(noise: str) -> int:
    """MZ_NOISE_* of the `noise=` argument of policy_sample / rollout_policy_sample / policy.sample_reference."""
    try:
        return NOISE_MODES[noise]
    except (KeyError, TypeError):
        raise ValueError(f"noise must be one of {sorted(NOISE_MODES)}, got {noise!r}") from None


class MzNoise(C.Structure):
    """`mz_noise` of include/mazestep.h: the noise of one mz_net_sample / mz_rollout_ex call."""
    _fields_ = [("struct_size", C.c_uint32), ("mode", C.c_int32), ("seed", C.c_uint64), ("step", C.c_uint64)]


class MzRolloutIo(C.Structure):
    """`mz_rollout_io` of include/mazestep.h: the arguments of one mz_rollout_ex call."""
    _fields_ = [("struct_size", C.c_uint32), ("n_steps", C.c_int32), ("actions_dev", C.c_void_p), ("action_step_stride", C.c_int64),
                ("actor", C.POINTER(MzNet)), ("noise", C.POINTER(MzNoise)), ("critic", C.POINTER(MzNet)),
                ("obs_dev", C.c_void_p), ("reward_dev", C.c_void_p), ("done_dev", C.c_void_p), ("goal_idx_dev", C.c_void_p),
                ("info_dev", C.c_void_p), ("obs_seq_dev", C.c_void_p), ("actions_seq_dev", C.c_void_p), ("logp_seq_dev", C.c_void_p),
                ("value_seq_dev", C.c_void_p), ("next_value_seq_dev", C.c_void_p), ("next_obs_seq_dev", C.c_void_p)]


HEAD_STATE_STD = 1  # MZ_HEAD_STATE_STD (include/mazestep.h)


class MzHead(C.Structure):
    """`mz_head` of include/mazestep.h: the state-dependent log-std head of one mz_net_sample_head / mz_rollout_head call."""
    _fields_ = [("struct_size", C.c_uint32), ("kind", C.c_int32), ("log_std_min", C.c_float), ("log_std_max", C.c_float),
                ("logp_squashed", C.c_int32), ("reserved", C.c_int32)]


def make_head(log_std_min: float, log_std_max: float, logp_squashed: bool = False) -> MzHead:
    """An MzHead with struct_size and kind set."""
    return MzHead(C.sizeof(MzHead), HEAD_STATE_STD, float(log_std_min), float(log_std_max), 1 if logp_squashed else 0, 0)


MAX_CONTEXT = 32  # MZ_MAX_CONTEXT (include/mazestep.h)
CTX_HOLD, CTX_RELATIVE = 0, 1  # MZ_CTX_*
CTX_UPDATES = {None: CTX_HOLD, "hold": CTX_HOLD, "relative": CTX_RELATIVE}


class MzContext(C.Structure):
    """`mz_context` of include/mazestep.h: the per-env context rows of one mz_net_eval_ctx / mz_net_value_ctx / mz_rollout_ctx call."""
    _fields_ = [("struct_size", C.c_uint32), ("dim", C.c_int32), ("update", C.c_int32), ("rel_dims", C.c_int32), ("reserved", C.c_int64),
                ("ctx_dev", C.c_void_p), ("ctx_seq_dev", C.c_void_p)]


def context_args(dim: int, obs_dim: int, context_update=None, context_dims=None, rollout: bool = True):
    """(MZ_CTX_*, rel_dims) of the `context_update=` / `context_dims=` arguments for a context of `dim` entries, checked as
    mz_rollout_ctx checks them: ValueError names the argument.  rollout False: a single call, which takes no update."""
    dim = int(dim)
    if not 1 <= dim <= MAX_CONTEXT:
        raise ValueError(f"context must have 1 .. {MAX_CONTEXT} (MZ_MAX_CONTEXT) entries per env, got {dim}")
    try:
        update = CTX_UPDATES[context_update]
    except (KeyError, TypeError):
        raise ValueError(f"context_update must be None or 'relative', got {context_update!r}") from None
    if update == CTX_HOLD:
        if context_dims not in (None, 0):
            raise ValueError(f"context_dims needs context_update='relative', got context_dims={context_dims!r} with a context that holds")
        return update, 0
    if not rollout:
        raise ValueError("context_update='relative' needs a rollout: a transition needs a step")
    if context_dims is None:
        raise ValueError("context_update='relative' needs context_dims=D, 1 <= D <= min(C, obs_dim)")
    d = int(context_dims)
    if not 1 <= d <= min(dim, int(obs_dim)):
        raise ValueError(f"context_dims must be 1 .. min(C, obs_dim) = {min(dim, int(obs_dim))}, got {d}")
    return update, d


def make_context(ctx_ptr, dim: int, update: int = CTX_HOLD, rel_dims: int = 0, ctx_seq_ptr=None) -> MzContext:
    """An MzContext with struct_size set."""
    return MzContext(C.sizeof(MzContext), int(dim), int(update), int(rel_dims), 0, ctx_ptr, ctx_seq_ptr)


def make_noise(mode: int, seed: int, step: int) -> MzNoise:
    """An MzNoise with struct_size set; seed and step wrap to uint64."""
    return MzNoise(C.sizeof(MzNoise), int(mode), int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFFFFFFFFFF)


def make_rollout_io(n_steps: int, **fields) -> MzRolloutIo:
    """An MzRolloutIo with struct_size set; fields by name (pointers: ints or None; actor / noise / critic: the structs, kept alive by
    the returned object)."""
    io = MzRolloutIo(struct_size=C.sizeof(MzRolloutIo), n_steps=int(n_steps))
    keep = []
    for name, value in fields.items():
        if name in ("actor", "noise", "critic"):
            if value is not None:
                keep.append(value)
                setattr(io, name, C.pointer(value))
        else:
            setattr(io, name, value.value if isinstance(value, C.c_void_p) else value)
    io._keep = keep
    return io


_lib = None


class MazeStepError(RuntimeError):
    pass


def load():
    """Load libmazestep.so (built in-tree by `__graft_entry__.build()` / csrc/Makefile)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MazeStepError(
            f"{LIB_PATH} not found: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()' "
            "or make -C mujoco_maze_amd/csrc). mujoco_maze_amd has no CPU fallback.")
    # torch first: its wheel carries its own HIP runtime, and the device buffers this library works on are torch tensors — if
    # libmazestep.so were loaded before torch, the process would hold the system's libamdhip64 as well and the second runtime to
    # initialise sees no device (found on the GPU box: build() loading the library ahead of smoke()'s `import torch`)
    import torch  # noqa: F401

    if LIB_PATH != DEFAULT_LIB_PATH:
        import sys

        print(f"mujoco_maze_amd: MZ_LIBMAZESTEP_EXPERIMENT is set — loading {LIB_PATH} instead of {DEFAULT_LIB_PATH}", file=sys.stderr)
    lib = C.CDLL(LIB_PATH)
    vp, i32, u64 = C.c_void_p, C.c_int32, C.c_uint64
    lib.mz_abi_version.restype = C.c_int
    lib.mz_model_sizeof.restype = u64
    lib.mz_create.restype = vp
    lib.mz_create.argtypes = [C.POINTER(MzModel), i32, i32, C.c_char_p, i32]
    lib.mz_destroy.argtypes = [vp]
    lib.mz_last_error.restype = C.c_char_p
    lib.mz_last_error.argtypes = [vp]
    for name in ("mz_num_envs", "mz_obs_dim", "mz_nq", "mz_nv", "mz_nu"):
        getattr(lib, name).restype = i32
        getattr(lib, name).argtypes = [vp]
    lib.mz_set_option.restype = i32
    lib.mz_set_option.argtypes = [vp, C.c_char_p, C.c_double]
    lib.mz_bind_env_goals.restype = i32
    lib.mz_bind_env_goals.argtypes = [vp, vp, vp]
    lib.mz_get_info.restype = i32
    lib.mz_get_info.argtypes = [vp, C.c_char_p, C.POINTER(C.c_double)]
    lib.mz_reset.restype = i32
    lib.mz_reset.argtypes = [vp, vp, u64, vp, vp]
    lib.mz_set_state.restype = i32
    lib.mz_set_state.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.mz_get_state.restype = i32
    lib.mz_get_state.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.mz_step.restype = i32
    lib.mz_step.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
    lib.mz_rollout.restype = i32
    lib.mz_rollout.argtypes = [vp, i32, vp, C.c_int64, vp, vp, vp, vp, vp, vp, vp]
    lib.mz_policy_act.restype = i32
    lib.mz_policy_act.argtypes = [vp, vp, C.c_int64, i32, i32, C.c_double, vp, vp, vp]
    lib.mz_rollout_policy.restype = i32
    lib.mz_rollout_policy.argtypes = [vp, i32, vp, C.c_int64, i32, i32, C.c_double, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.mz_policy_sample.restype = i32
    lib.mz_policy_sample.argtypes = [vp, vp, C.c_int64, i32, i32, C.c_double, u64, u64, vp, vp, vp, vp]
    lib.mz_rollout_policy_sample.restype = i32
    lib.mz_rollout_policy_sample.argtypes = [vp, i32, vp, C.c_int64, i32, i32, C.c_double, u64, u64, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.mz_value.restype = i32
    lib.mz_value.argtypes = [vp, vp, C.c_int64, i32, vp, vp, vp]
    lib.mz_rollout_actor_critic.restype = i32
    lib.mz_rollout_actor_critic.argtypes = [vp, i32, vp, C.c_int64, i32, i32, C.c_double, i32, u64, u64, C.POINTER(MzCritic), vp, vp, vp, vp, vp, vp,
                                            vp, vp, vp]
    lib.mz_net_act.restype = i32
    lib.mz_net_act.argtypes = [vp, C.POINTER(MzNet), i32, u64, u64, vp, vp, vp, vp]
    lib.mz_net_value.restype = i32
    lib.mz_net_value.argtypes = [vp, C.POINTER(MzNet), vp, vp, vp]
    lib.mz_rollout_net.restype = i32
    lib.mz_rollout_net.argtypes = [vp, i32, C.POINTER(MzNet), i32, u64, u64, C.POINTER(MzNet), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.mz_net_sample.restype = i32
    lib.mz_net_sample.argtypes = [vp, C.POINTER(MzNet), C.POINTER(MzNoise), vp, vp, vp, vp]
    lib.mz_rollout_ex.restype = i32
    lib.mz_rollout_ex.argtypes = [vp, C.POINTER(MzRolloutIo), vp]
    lib.mz_net_sample_head.restype = i32
    lib.mz_net_sample_head.argtypes = [vp, C.POINTER(MzNet), C.POINTER(MzHead), C.POINTER(MzNoise), vp, vp, vp, vp]
    lib.mz_rollout_head.restype = i32
    lib.mz_rollout_head.argtypes = [vp, C.POINTER(MzRolloutIo), C.POINTER(MzHead), vp]
    lib.mz_net_eval_ctx.restype = i32
    lib.mz_net_eval_ctx.argtypes = [vp, C.POINTER(MzNet), C.POINTER(MzHead), C.POINTER(MzNoise), C.POINTER(MzContext), vp, vp, vp, vp]
    lib.mz_net_value_ctx.restype = i32
    lib.mz_net_value_ctx.argtypes = [vp, C.POINTER(MzNet), C.POINTER(MzContext), vp, vp, vp]
    lib.mz_rollout_ctx.restype = i32
    lib.mz_rollout_ctx.argtypes = [vp, C.POINTER(MzRolloutIo), C.POINTER(MzHead), C.POINTER(MzContext), vp]
    lib.mz_bind_obs_norm.restype = i32
    lib.mz_bind_obs_norm.argtypes = [vp, vp, vp, C.c_double, vp]
    lib.mz_return_scan.restype = i32
    lib.mz_return_scan.argtypes = [vp, i32, vp, vp, C.c_double, vp, vp, vp, vp, vp]
    lib.mz_gae.restype = i32
    lib.mz_gae.argtypes = [vp, i32, vp, vp, vp, vp, C.c_double, C.c_double, vp, vp, vp]
    lib.mz_get_status.restype = i32
    lib.mz_get_status.argtypes = [vp, vp, vp]
    lib.mz_debug_forward.restype = i32
    lib.mz_debug_forward.argtypes = [vp, vp, vp, vp, vp]
    lib.mz_bind_final_obs.restype = i32
    lib.mz_bind_final_obs.argtypes = [vp, vp]
    lib.mz_bind_record.restype = i32
    lib.mz_bind_record.argtypes = [vp, vp]
    lib.mz_set_goals.restype = i32
    lib.mz_set_goals.argtypes = [vp, i32, vp, vp, vp, vp, vp]
    lib.mz_debug_task_eval.restype = i32
    lib.mz_debug_task_eval.argtypes = [vp, i32, vp, vp, vp, vp, vp]
    lib.mz_debug_detect.restype = i32
    lib.mz_debug_detect.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp]
    lib.mz_read_phase_cycles.restype = i32
    lib.mz_read_phase_cycles.argtypes = [vp, vp]
    lib.mz_read_wave_cycles.restype = i32
    lib.mz_read_wave_cycles.argtypes = [vp, vp, i32]
    lib.mz_read_wave_phase_cycles.restype = i32
    lib.mz_read_wave_phase_cycles.argtypes = [vp, vp, i32]
    lib.mz_render.restype = i32
    lib.mz_render.argtypes = [vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp]
    lib.mz_last_kernel_ms.restype = C.c_double
    lib.mz_last_kernel_ms.argtypes = [vp]
    if lib.mz_model_sizeof() != C.sizeof(MzModel):
        raise MazeStepError("mz_model layout mismatch between include/mazestep.h and mujoco_maze_amd/model.py")
    _lib = lib
    return lib


def check(lib, handle, rc, what):
    if rc != 0:
        msg = lib.mz_last_error(handle)
        raise MazeStepError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}")
