/* mazestep.h — C-ABI of the MI355X batched maze-environment stepper.
 *
 * This is the drop-in boundary for the hot path of kngwyu/mujoco-maze:
 *
 *   reference call (Python, one env)                       replaced by (batched, device)
 *   -----------------------------------------------------  ------------------------------
 *   MazeEnv.__init__       mujoco_maze/maze_env.py:28-233   mz_create   (compiled mz_model in)
 *   MazeEnv.reset          mujoco_maze/maze_env.py:371-382  mz_reset
 *     AntEnv.reset_model   mujoco_maze/ant.py:84-96
 *     PointEnv.reset_model mujoco_maze/point.py:71-81
 *   MazeEnv.step           mujoco_maze/maze_env.py:448-481  mz_step
 *     AntEnv.step          mujoco_maze/ant.py:61-73           (ctrl write + mj_step x frame_skip,
 *     PointEnv.step        mujoco_maze/point.py:44-61          forward reward, ctrl cost)
 *     CollisionDetector.detect  maze_env_utils.py:186-206      (Point wall bounce)
 *     MazeEnv._get_obs     mujoco_maze/maze_env.py:351-369     (obs assembly)
 *     MazeTask.reward / termination  maze_task.py:77-81,110-111,403-407
 *   MujocoEnv.set_state (gym) via set_xy  ant.py:105-108    mz_set_state / mz_get_state
 *   mujoco-py exceptions / warnings                         integer status + mz_last_error,
 *                                                           per-env status words (mz_get_status)
 *
 * All array arguments named *_dev are DEVICE pointers (HBM) owned by the caller
 * (e.g. torch tensors' data_ptr()); the library never frees caller memory.  The
 * handle owns the persistent per-env state.  Calls are asynchronous and ordered
 * on the hipStream_t passed as `stream` (void* here so that this header needs
 * no HIP include; NULL = the default stream).  One host thread per handle.
 *
 * No torch / C++ types appear in any signature.
 */
#ifndef MAZESTEP_H
#define MAZESTEP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MZ_ABI_VERSION 8

#define MZ_MAX_BODY 24
#define MZ_MAX_JNT 24
#define MZ_MAX_DOF 24
#define MZ_MAX_Q 28
#define MZ_MAX_GEOM 24
#define MZ_MAX_ACT 8
#define MZ_MAX_GRID 12
#define MZ_MAX_SEG 96
#define MZ_MAX_GOAL 8
#define MZ_MAX_OBS 48        /* observation without the top-down view */
#define MZ_VIEW_DIM 75       /* MazeEnv.get_top_down_view: 5 x 5 cells x (walls, chasms, movable blocks), maze_env.py:95 */
#define MZ_POLICY_MAX_HIDDEN 64 /* widest hidden layer of a device-side policy (mz_policy_act / mz_rollout_policy, csrc/mz_policy.h) */

/* robot kinds */
#define MZ_ROBOT_POINT 0
#define MZ_ROBOT_ANT 1
#define MZ_ROBOT_SWIMMER 2 /* planar link chains: Swimmer (3 links) and Reacher (2 links; reacher.xml is <mujoco model="swimmer">) */
#define MZ_ROBOT_GENERIC 3 /* a user's AgentModel of any tree topology (agent_model.py:12-41, README.md:127): stepped by walking the compiled tree */

/* joint types (MuJoCo numbering) */
#define MZ_JNT_FREE 0
#define MZ_JNT_BALL 1
#define MZ_JNT_SLIDE 2
#define MZ_JNT_HINGE 3

/* geom types (MuJoCo numbering; pair order is by type) */
#define MZ_GEOM_PLANE 0
#define MZ_GEOM_SPHERE 2
#define MZ_GEOM_CAPSULE 3
#define MZ_GEOM_BOX 6

/* maze cell codes in mz_model.grid (MazeCell, maze_env_utils.py:19-33) */
#define MZ_CELL_EMPTY 0
#define MZ_CELL_BLOCK 1
#define MZ_CELL_CHASM 2
#define MZ_CELL_ROBOT 255

/* reward kinds (mujoco_maze_amd/maze_task.py) */
#define MZ_REWARD_ZERO 0
#define MZ_REWARD_FIRST_MATCH 1
#define MZ_REWARD_NEG_DIST 2
#define MZ_SLOT_AGENT 0
#define MZ_SLOT_OBJECT 1

/* per-env status bits (mz_get_status) */
#define MZ_STATUS_OK 0
#define MZ_STATUS_BAD_STATE 1      /* NaN / |x| > 1e10 in qpos/qvel/qacc (MuJoCo mj_check*) */
#define MZ_STATUS_CONTACT_OVERFLOW 2 /* more simultaneous contacts (or, generic robots, joint-limit rows) than the kernel's buffers */
#define MZ_STATUS_SOLVER_MAXITER 4 /* constraint solver hit its iteration cap */

/* error codes */
#define MZ_OK 0
#define MZ_ERR_ARG (-1)
#define MZ_ERR_HIP (-2)
#define MZ_ERR_UNSUPPORTED (-3)

/* The compiled model: what MazeEnv.__init__ + the MuJoCo model compiler produce
 * in the reference (maze_env.py:97-218 writes MJCF; MuJoCo compiles it).  Built
 * on the host by mujoco_maze_amd/model.py.  Plain doubles/ints; the library
 * converts to fp32 device constants. */
typedef struct mz_model {
  int32_t abi_version;
  int32_t robot; /* MZ_ROBOT_* */
  int32_t nbody, njnt, nq, nv, ngeom, nu;
  int32_t nq_robot, nv_robot; /* leading coordinates the robot's own _get_obs reports and reset_model re-randomises: ant 15/14
                               * (ant.py:75-96), point 3/3 (point.py:63-81), swimmer / reacher ALL nq / nv, movable blocks
                               * included (swimmer.py:50-69) */
  int32_t frame_skip;
  int32_t integrator_rk4; /* 1: RK4 (every reference asset); 0: MuJoCo's default Euler — semi-implicit, implicit in the joint damping
                           * (mj_EulerSkip) — for user robots, stepped by the general engine */
  int32_t collision_predefined; /* swimmer: no dynamic contact pairs */
  int32_t manual_collision;     /* Point: CollisionDetector bounce */
  int32_t max_episode_steps;    /* gym TimeLimit (mujoco_maze/__init__.py:31) */
  int32_t obs_dim;
  int32_t reset_qvel_kind; /* 0 normal*0.1, 1 U[0,1)*0.1, 2 U(-.1,.1) */
  int32_t engine; /* 0: the robot family's specialised kernels where they can step this model, the general engine (csrc/generic_dyn.h:
                   * walks the compiled tree; any joints / geoms / movable bodies this struct can describe) where they cannot — SPIN
                   * plates, user robots, more than three blocks; 1: the general engine whatever the robot (ABI 8) */
  double timestep;
  double gravity[3];
  double density, viscosity;
  double meaninertia;

  /* bodies (0 = world) */
  int32_t body_parent[MZ_MAX_BODY];
  int32_t body_jntadr[MZ_MAX_BODY];
  int32_t body_jntnum[MZ_MAX_BODY];
  int32_t body_dofadr[MZ_MAX_BODY];
  int32_t body_dofnum[MZ_MAX_BODY];
  double body_pos[MZ_MAX_BODY][3];
  double body_quat[MZ_MAX_BODY][4];
  double body_ipos[MZ_MAX_BODY][3];
  double body_inertia[MZ_MAX_BODY][6]; /* xx yy zz xy xz yz about COM, body frame */
  /* MuJoCo's own form of the same tensor: principal moments and the inertial frame's orientation in the body frame
   * (mjModel.body_inertia / body_iquat; ximat = xmat * R(iquat)).  A body with ONE geom takes that geom's frame and moments
   * (a capsule's fromto frame, axial moment third); several geoms: eigen-decomposition of the summed tensor, moments in
   * decreasing order.  The inertia-box fluid model works in this frame. */
  double body_iquat[MZ_MAX_BODY][4];
  double body_pinertia[MZ_MAX_BODY][3];
  double body_mass[MZ_MAX_BODY];
  double body_invweight0[MZ_MAX_BODY][2];

  /* joints */
  int32_t jnt_type[MZ_MAX_JNT];
  int32_t jnt_qposadr[MZ_MAX_JNT];
  int32_t jnt_dofadr[MZ_MAX_JNT];
  int32_t jnt_bodyid[MZ_MAX_JNT];
  int32_t jnt_limited[MZ_MAX_JNT];
  double jnt_pos[MZ_MAX_JNT][3];
  double jnt_axis[MZ_MAX_JNT][3];
  double jnt_range[MZ_MAX_JNT][2];
  double jnt_margin[MZ_MAX_JNT];
  double jnt_solref[MZ_MAX_JNT][2];
  double jnt_solimp[MZ_MAX_JNT][5];
  double jnt_stiffness[MZ_MAX_JNT]; /* hinge / slide spring (MJCF joint stiffness): passive force -k (q - springref); a model with any goes to the general engine */
  double jnt_springref[MZ_MAX_JNT]; /* rest position of that spring in joint coordinates (radians / metres; MJCF springref) */

  /* dofs */
  int32_t dof_bodyid[MZ_MAX_DOF];
  int32_t dof_jntid[MZ_MAX_DOF];
  double dof_armature[MZ_MAX_DOF];
  double dof_damping[MZ_MAX_DOF];
  double dof_invweight0[MZ_MAX_DOF];
  double qpos0[MZ_MAX_Q];

  /* geoms (0 = floor plane; maze wall boxes are implicit in `grid`) */
  int32_t geom_type[MZ_MAX_GEOM];
  int32_t geom_bodyid[MZ_MAX_GEOM];
  int32_t geom_contype[MZ_MAX_GEOM];
  int32_t geom_conaffinity[MZ_MAX_GEOM];
  int32_t geom_condim[MZ_MAX_GEOM];
  double geom_pos[MZ_MAX_GEOM][3];
  double geom_quat[MZ_MAX_GEOM][4];
  double geom_size[MZ_MAX_GEOM][3];
  double geom_friction[MZ_MAX_GEOM][3];
  double geom_solref[MZ_MAX_GEOM][2];
  double geom_solimp[MZ_MAX_GEOM][5];
  double geom_margin[MZ_MAX_GEOM];
  double geom_gap[MZ_MAX_GEOM];
  double geom_rbound[MZ_MAX_GEOM];

  /* actuators: motor on one dof */
  int32_t act_dofid[MZ_MAX_ACT];
  int32_t act_ctrllimited[MZ_MAX_ACT];
  double act_gear[MZ_MAX_ACT];
  double act_ctrlrange[MZ_MAX_ACT][2];
  double act_gainprm[MZ_MAX_ACT];    /* actuator force = gainprm * ctrl + biasprm[0] + biasprm[1] * length + biasprm[2] * velocity, with length =  */
  double act_biasprm[MZ_MAX_ACT][3]; /* gear * q, velocity = gear * qvel of its joint; on the dof: gear * force.  motor: 1 | 0 0 0; <position kp>:
                                      * kp | 0 -kp 0; <velocity kv>: kv | 0 0 -kv.  Anything but a motor is stepped by the general engine */

  /* maze world (maze_env.py:116-152): cell (i,j) centre = (j*s - torso_x, i*s - torso_y) */
  int32_t grid_rows, grid_cols;
  uint8_t grid[MZ_MAX_GRID][MZ_MAX_GRID];
  double maze_scale, torso_x, torso_y;
  double wall_half_xy, wall_half_z, wall_center_z; /* box half sizes / centre height */
  int32_t wall_contype, wall_conaffinity, wall_condim;
  int32_t step_kind; /* the robot's own step (AgentModel.step): 0 = the robot family's; 1 = motors (ant.py:61-73, swimmer.py:37-48: clamped
                      * motors, forward reward, control cost); 2 = the Point's (point.py:44-61: heading / position moved by the action,
                      * velocity clip, no control).  Read by the general engine; a user robot picks one (ABI 8) */
  double wall_friction[3];
  double wall_solref[2];
  double wall_solimp[5];
  double wall_margin, wall_gap;

  /* Point manual collision (maze_env_utils.py:151-184; maze_env.py:36,457-464) */
  int32_t nseg, pad2;
  double seg[MZ_MAX_SEG][4]; /* x1 y1 x2 y2 */
  double restitution;
  double velocity_limit; /* point.py:33,56 */

  /* task (maze_task.py) */
  int32_t ngoal;
  int32_t reward_kind, reward_slot, reward_binary, term_slot;
  int32_t goal_dim[MZ_MAX_GOAL];
  double goal_pos[MZ_MAX_GOAL][3];
  double goal_threshold[MZ_MAX_GOAL];
  double goal_reward_scale[MZ_MAX_GOAL];
  double penalty, task_scale, inner_reward_scaling;
  double forward_reward_weight, ctrl_cost_weight; /* ant.py:47-53 */

  /* movable XY blocks (maze_env.py:563-660: body + slide-x + slide-y + box geom appended after the
   * robot); observed as body xpos at obs[3:3+3*nblock] when observe_blocks (maze_env.py:364-368) */
  int32_t nblock, observe_blocks;
  int32_t block_bodyid[4];
  int32_t block_geomid[4];

  /* object balls (Billiard; maze_env.py:167-191, 489-536: body at z = 0 with slide-x, slide-y and a z hinge, sphere geom
   * of radius r at height r); observed as body xpos BEFORE the blocks when observe_balls (maze_env.py:360-363) */
  int32_t nball, observe_balls;
  int32_t ball_bodyid[4];
  int32_t ball_geomid[4];

  /* elevated mazes (Fall / MultiFall, maze_env.py:102-107,124-137): under every cell that is not a CHASM stands a platform
   * box of the wall's footprint from z = 0 to z = height_offset (centre wall_half_z, half height wall_half_z); the walls
   * stand on top of it (wall_center_z = wall_half_z + height_offset) and the robot's torso starts 0.75 above it.
   * Movable blocks of such mazes slide along z as well (limited joints; block_bodyid / the joint arrays describe them). */
  int32_t elevated;
  /* MazeTask.TOP_DOWN_VIEW (maze_env.py:54,351-369): the robot-centred 5 x 5 x 3 occupancy view of get_top_down_view
   * (maze_env.py:262-349), flattened row-major, sits between the robot's observation and the trailing t * 0.001; obs_dim
   * counts its MZ_VIEW_DIM entries */
  int32_t top_down_view;
  double height_offset;
} mz_model;

typedef struct mz_handle mz_handle;

int mz_abi_version(void);
uint64_t mz_model_sizeof(void); /* host-side struct layout check for FFI users */

/* Create a batch of `num_envs` environments on HIP device `device`.
 * Returns NULL on failure with a message in err (if non-NULL). */
mz_handle* mz_create(const mz_model* model, int32_t num_envs, int32_t device, char* err, int32_t errlen);
void mz_destroy(mz_handle* h);
const char* mz_last_error(const mz_handle* h);

/* accessors: the value, or MZ_ERR_ARG for a NULL handle */
int32_t mz_num_envs(const mz_handle* h);
int32_t mz_obs_dim(const mz_handle* h);
int32_t mz_nq(const mz_handle* h);
int32_t mz_nv(const mz_handle* h);
int32_t mz_nu(const mz_handle* h);

/* Tunables: "auto_reset" (0/1), "seed", "env_index_offset" (global slot of local env 0 in a
 * sharded run: keys the reset RNG), "solver_iterations", "solver_tolerance", "solver_rtol",
 * "ls_iterations" (Ant solver: evaluations of the exact line search), "ls_fast_iterations" / "ls_fast" (the first n Newton
 * iterations of a solve search the line with at most that many evaluations; defaults 5 / 0: unit steps; "ls_fast_iterations" also
 * sets the Point's float64 solvers; 0 = MuJoCo's search in every iteration, monotone on any maze at ~7 % of the Ant kernel's time:
 * what the host mirror sets for custom tasks, whose stiffness nobody has soaked — the registered mazes are), "lanes_per_env" (8/16/32/64 lanes of a wavefront per environment; 8 on an Ant
 * with movable blocks or a ball is refused with MZ_ERR_UNSUPPORTED and leaves the handle's width as it was: those kernels exist at 16, 32 and 64 lanes, and
 * mz_get_info("lanes_per_env") always names the instantiation that steps; defaults: plain Ant 16,
 * Ant with one movable block 32 — 16 for batches beyond 2048 envs, where 32 would mean more waves than the device has SIMDs —, with more blocks / a three-slide block / the ball 64; Point 16 while that leaves every wave a SIMD of its own (up to 4096 envs), else 32; with one block or the ball 32, with two or three blocks 64;
 * Swimmer / Reacher 4, fixed), "waves_per_block" (1/2/4, Ant), "waves_per_simd" (plain Ant at 16 lanes: 1 = the one-wave
 * kernel, 2 = the kernel held to 256 registers so that two waves share a SIMD, 0 = default: by the wave count of the
 * launch — more waves than SIMDs takes the second), "profile_phases" (0/1: instrumented Ant kernel, see
 * mz_read_phase_cycles), "time_kernels" (n > 0: ring of n HIP event pairs around the step kernel, see
 * mz_last_kernel_ms), "time_kernels_stride" (k >= 1, default 1: only every k-th mz_step carries the pair — a pair costs the queue
 * ~5 us per launch, a tenth of a Point or Swimmer step; bench.py samples every 8th), "wide_nets" (0/1/2: mz_net networks of up to
 * MZ_NET_MAX_WIDTH units per layer on the tiled kernel, see "Wide networks" below). Returns MZ_OK, MZ_ERR_ARG, or MZ_ERR_UNSUPPORTED for an Ant-only key on another robot. */
int32_t mz_set_option(mz_handle* h, const char* key, double value);

/* What the next mz_step launches (ABI 8).  The kernel instantiation a handle steps with is chosen from the robot, its maze's
 * movable bodies, the BATCH SIZE and the device's compute-unit count (lanes per env, one or two waves per SIMD: see
 * "lanes_per_env" / "waves_per_simd" above), and the instantiations agree to fp32 round-off, not bit for bit: the same seed and
 * states give round-off-different trajectories at different num_envs, on shards of unequal size or on devices with another
 * CU count.  Keys: "engine" (0 = the robot family's specialised kernel, 1 = the general engine of mz_model.engine),
 * "lanes_per_env", "waves_per_simd", "device_simds" (4 x compute units), "ls_fast_iterations", "rollout_fused" (1: mz_rollout runs
 * this handle on its fused kernels, 0: it runs the step's launches in a loop), "wide_nets" (the option's mode).  Returns MZ_OK or
 * MZ_ERR_ARG. */
int32_t mz_get_info(const mz_handle* h, const char* key, double* value);

/* Auto-reset observation convention.  With option "auto_reset" = 1 an env whose step ended its episode (done != 0) is
 * re-seeded inside the same kernel; mz_step then returns, for that env, the reward / done / goal index of the terminal step
 * and in obs_dev the FIRST observation of the new episode (t = 0) — what a policy must act on next.  The terminal
 * observation (the one the reference's MazeEnv.step returns, maze_env.py:474-481) is written to row i of the buffer bound
 * here ([N, obs_dim] fp32, device, caller-owned; rows of envs that did not finish are left untouched); NULL unbinds.
 * Without auto-reset obs_dev always holds the step's own observation and this buffer is never written. */
int32_t mz_bind_final_obs(mz_handle* h, float* final_obs_dev);

/* Packed per-env record for sharded runs (the one collective of the path is the all-gather of this tensor).
 * When bound ([N, obs_dim + 2] fp32, device, caller-owned; NULL unbinds), every mz_step also writes row i =
 * obs_dev row i (obs_dim floats, i.e. under auto-reset the first observation of the new episode) | reward | done as float,
 * from inside the step kernel (Ant) or with one extra pack launch (Point / Swimmer / Reacher, top-down-view tasks), so the
 * caller can hand the buffer to the collective without copy launches of its own.  No reference counterpart (the
 * reference steps one env per process: mujoco_maze/maze_env.py:448-481 returns the three values separately). */
int32_t mz_bind_record(mz_handle* h, float* record_dev);

/* Goal resampling (MazeEnv.reset calls MazeTask.sample_goals() and, when it returns True, moves the goal markers:
 * mujoco_maze/maze_env.py:374-376; MazeTask.sample_goals: maze_task.py:66-67).  Replaces the goal table the task predicate of
 * every later mz_step / mz_debug_task_eval evaluates: ngoal <= MZ_MAX_GOAL rows of HOST arrays — pos [ngoal][3] (z ignored where
 * dim = 2), threshold [ngoal], reward_scale [ngoal], dim [ngoal] (2 or 3) — float64, the reference's own values
 * (maze_task.py:26-47).  Work already queued on `stream` is finished first (the call synchronises on it), so a step launched
 * before the call is judged on the old goals and every step after it on the new ones.  Reward kind, slots, PENALTY stay
 * those of the model.  Returns MZ_OK or MZ_ERR_ARG. */
int32_t mz_set_goals(mz_handle* h, int32_t ngoal, const double* pos, const double* threshold, const double* reward_scale,
                     const int32_t* dim, void* stream);

/* Per-env goal positions (ABI 8).  The reference gives every env its own task object and resamples its goals at EVERY episode reset
 * (maze_env.py:374-376); a batch that shares one goal table can only do so at a full reset.  goal_pos_dev: DEVICE pointer,
 * [num_envs][MZ_MAX_GOAL][3] float64, caller-owned and caller-updated between steps (the host mirror rewrites the rows of the envs
 * whose episode just ended); NULL unbinds.  Thresholds, reward scales, dims and the goal count stay those of the shared table
 * (mz_set_goals / the model).  Synchronises on `stream` first.  Returns MZ_OK, MZ_ERR_ARG or MZ_ERR_HIP. */
int32_t mz_bind_env_goals(mz_handle* h, const double* goal_pos_dev, void* stream);

/* reset(): envs with mask_dev[i] != 0 (all when NULL) get t = 0 and a fresh state
 * from the reference's reset distribution (counter-based RNG keyed by seed and
 * env slot; streams differ from numpy's — distributional parity only).
 * obs_dev [N, obs_dim] may be NULL.  Rows of envs the mask leaves alone are written too, from their present state and t: with an
 * all-zero mask the call resets nothing and returns every env's current observation (e.g. after mz_set_state).
 * The call stores `seed` in the handle for ALL envs and zeroes the episode count of the masked ones only.  So from here on the k-th
 * in-step auto-reset of a masked env draws from episode_seed(seed, k) (csrc/mz_rng.h), and an env the mask left alone keeps its
 * episode count e and draws its next one from episode_seed(seed, e + 1): the new seed with the old count. */
int32_t mz_reset(mz_handle* h, const uint8_t* mask_dev, uint64_t seed, float* obs_dev, void* stream);

/* State injection / read-back (row-major [N, nq], [N, nv], [N, nv], [N]).
 * Any pointer may be NULL to skip that field.  warmstart = the constraint solver's starting guess carried between steps
 * (MuJoCo's qacc_warmstart): the Ant and the general engine keep the last evaluation's qacc; the bare Point keeps its constraint part
 * qacc - qacc_smooth (read back by mz_get_state; mz_set_state with a new qpos / qvel clears it — a guess only, results agree to the
 * solver tolerance whatever it holds); the Swimmer / Reacher and the Point with movable bodies keep none (reads 0, writes ignored). */
int32_t mz_set_state(mz_handle* h, const float* qpos_dev, const float* qvel_dev, const float* warmstart_dev,
                     const int32_t* t_dev, void* stream);
int32_t mz_get_state(mz_handle* h, float* qpos_dev, float* qvel_dev, float* warmstart_dev, int32_t* t_dev,
                     void* stream);

/* One MazeEnv.step for every env.
 *  actions_dev [N, nu] fp32 row-major
 *  obs_dev     [N, obs_dim]   the step's observation (under auto-reset: see mz_bind_final_obs)
 *  reward_dev  [N]            inner_reward_scaling * inner + task reward
 *  done_dev    [N] u8         bit0 = task termination, bit1 = TimeLimit truncation
 *  goal_idx_dev[N] i32        first matching goal (list order) or -1 (nullable): the goal whose reward_scale the reward is
 *                             (maze_task.py:403-407); for zero / distance rewards the first goal that terminates
 *  info_dev    [N, 4]         position x, y, reward_forward, reward_ctrl (nullable) */
int32_t mz_step(mz_handle* h, const float* actions_dev, float* obs_dev, float* reward_dev, uint8_t* done_dev,
                int32_t* goal_idx_dev, float* info_dev, void* stream);

/* n_steps successive steps in one call, for callers that need nothing from the host between steps: sampling planners that run
 * pre-drawn action sequences from one state, action repeat, random-walk data collection.
 * The call leaves the handle and every output exactly as n_steps successive mz_step calls on the same stream would: state, t,
 * episode counters, warm start, status words, the bound final_obs buffer (under auto-reset row i is overwritten each time env i
 * finishes) and the bound record (the last step's row).
 *  n_steps            1 .. 65536; longer windows are split inside the call: no kernel launch advances more than 256 steps
 *  actions_dev        step k reads its [N, nu] actions at actions_dev + k * action_step_stride floats
 *  action_step_stride N * nu (a [n_steps, N, nu] tensor) or 0 (one [N, nu] block repeated: action repeat); else MZ_ERR_ARG
 *  obs_dev      [N, obs_dim]           what the last step's mz_step would have written (under auto-reset the first observation
 *                                      of the new episode for envs the last step finished)
 *  reward_dev   [n_steps, N]           every step's reward
 *  done_dev     [n_steps, N] u8        every step's done bits
 *  goal_idx_dev [n_steps, N] i32       every step's goal index (nullable)
 *  info_dev     [n_steps, N, 4]        every step's info row (nullable)
 *  obs_seq_dev  [n_steps, N, obs_dim]  every step's observation row, i.e. what obs_dev held after that step (nullable)
 * The Point, Swimmer and Reacher (with or without movable bodies, no top-down view) run fused kernels that keep the env on chip
 * between steps; the Ant, the general engine and top-down-view tasks run the step's own launches n_steps times inside the call
 * (mz_get_info key "rollout_fused": 1 / 0).  The "time_kernels" event ring does not record rollouts: mz_last_kernel_ms is
 * unaffected by this call.  Returns MZ_OK, MZ_ERR_ARG (NULL handle or required array, n_steps or stride out of range) or MZ_ERR_HIP. */
int32_t mz_rollout(mz_handle* h, int32_t n_steps, const float* actions_dev, int64_t action_step_stride, float* obs_dev,
                   float* reward_dev, uint8_t* done_dev, int32_t* goal_idx_dev, float* info_dev, float* obs_seq_dev, void* stream);

/* Device-side policies (closed-loop rollouts): a small policy evaluated where the observation already sits, for population methods
 * with one policy per env and for evaluating a trained linear or one-hidden-layer policy over whole episodes.
 *
 * One policy is `npar` fp32 numbers, weights input-major (nn.Linear.weight.T: adjacent output units at adjacent addresses), with
 * obs_dim = mz_obs_dim (the top-down view included where the task has one) and nu = mz_nu:
 *   hidden == 0 (affine)                  Wt [obs_dim][nu], b [nu]                                   npar = obs_dim * nu + nu
 *   1 <= hidden <= MZ_POLICY_MAX_HIDDEN   W1t [obs_dim][H], b1 [H], W2t [H][nu], b2 [nu]            npar = obs_dim * H + H + H * nu + nu
 * Arithmetic (csrc/mz_policy.h, the one definition every kernel and the host build compile): each unit starts from its bias and
 * adds w * x over the inputs in index order, in fp32, the multiply and the add rounded separately (no fused multiply-add); hidden
 * units are tanhf of that sum; an output is the sum itself (squash == 0) or (float)action_scale * tanhf(sum) (squash == 1).  NaN
 * propagates.  The affine, unsquashed case is therefore reproduced bit for bit by fp32 arithmetic anywhere (mujoco_maze_amd/policy.py
 * reference); the tanh cases carry the tanhf of the library that runs them and are bit-equal between the device kernels only.
 *  params_dev        [npar] (param_env_stride == 0: one policy shared by all envs) or [N, npar] (param_env_stride == npar: env i
 *                    reads params_dev + i * npar); any other stride is MZ_ERR_ARG
 *
 * mz_policy_act: actions_dev[r] = policy(obs_dev[r]) for the N rows; obs_dev [N, obs_dim], actions_dev [N, nu].  The actions are
 * the policy's outputs, not clamped to the control range (the step clamps where the reference does).
 *
 * mz_rollout_policy: n_steps times a = policy(obs); obs, reward, done, ... = step(a).  The call leaves the handle and every output
 * exactly as this loop on the same stream would:
 *     for k in 0 .. n_steps - 1:
 *         mz_policy_act(obs_dev -> a_k)
 *         mz_step(a_k -> obs_dev, row k of reward_dev / done_dev / goal_idx_dev / info_dev)
 * — state, t, episode counters, warm start, status words, the bound final_obs buffer and the bound record (the last step's row).
 * Under auto-reset the policy acts on the first observation of the new episode, as it would in the loop.
 *  obs_dev [N, obs_dim] is IN/OUT: on entry the observation the policy acts on first — what the last mz_step / mz_reset /
 *          mz_rollout / mz_rollout_policy wrote there —, on return the last step's observation.  mz_set_state does NOT refresh
 *          the caller's observation buffer; after it, mz_reset with an all-zero mask writes every env's current observation
 *          without resetting any (every engine's reset kernel writes the rows of unmasked envs from their present state and t).
 *  n_steps 1 .. 65536; reward_dev, done_dev, goal_idx_dev, info_dev, obs_seq_dev as in mz_rollout
 *  actions_seq_dev [n_steps, N, nu] (nullable): the actions the policy produced, before the env's own control clamp
 * Handles with "rollout_fused" = 1 (mz_get_info) evaluate the policy inside the fused rollout kernels, between two steps, on the
 * observation row that stays on chip (launches of at most 256 steps, each of which writes obs_dev at its last step and the next
 * picks it up from there); every other handle runs the loop above inside the call, launch by launch, with a_k in row k of
 * actions_seq_dev or in a scratch buffer of the handle.  The "time_kernels" ring does not record these calls.
 * Both return MZ_OK, MZ_ERR_ARG (NULL handle or required array, hidden outside 0 .. MZ_POLICY_MAX_HIDDEN, squash outside {0, 1},
 * a stride that is neither 0 nor npar, n_steps out of range) or MZ_ERR_HIP. */
int32_t mz_policy_act(mz_handle* h, const float* params_dev, int64_t param_env_stride, int32_t hidden, int32_t squash,
                      double action_scale, const float* obs_dev, float* actions_dev, void* stream);
int32_t mz_rollout_policy(mz_handle* h, int32_t n_steps, const float* params_dev, int64_t param_env_stride, int32_t hidden,
                          int32_t squash, double action_scale, float* obs_dev, float* reward_dev, uint8_t* done_dev,
                          int32_t* goal_idx_dev, float* info_dev, float* obs_seq_dev, float* actions_seq_dev, void* stream);

/* Stochastic device-side policies (on-policy data collection, exploration with action noise): a diagonal Gaussian around the
 * policy above, sampled where the observation sits, with the log-probability of what was drawn.
 *
 * Parameters: the packed vector above followed by log_std[nu] — npar_s = npar + nu fp32 numbers; params_dev [npar_s]
 * (param_env_stride == 0) or [N, npar_s] (param_env_stride == npar_s); any other stride is MZ_ERR_ARG.
 * Noise: eps(noise_seed, noise_step, slot, u) is a pure function of four integers — slot is the GLOBAL env slot ("env_index_offset"
 * + i), u the action index — and of nothing else: not of N, nu, hidden, lanes per env, the engine or the kernel that computes it,
 * so a shard of a batch draws what the whole batch would.  In uint64 arithmetic with wrap-around (csrc/mz_rng.h, csrc/mz_policy.h):
 *     key = mix64(noise_seed ^ (0xA24BAED4963EE407 * (noise_step + 1)))
 *     x1 = rng_u32(key, slot, 2u), x2 = rng_u32(key, slot, 2u + 1)                         (the words of the reset stream's generator)
 *     u1 = ((x1 >> 8) + 1) * 2^-24, u2 = (x2 >> 8) * 2^-24, eps = sqrtf(-2 logf(u1)) * cosf(6.2831855f * u2)       |eps| <= 5.77
 * Sample: with m_u the pre-squash sum of output unit u, z_u = m_u + expf(log_std[u]) * eps_u (product and sum rounded separately);
 * the action is z_u (squash == 0) or (float)action_scale * tanhf(z_u) (squash == 1).
 * Log-prob: logp = sum_u (-0.5 * eps_u^2 - log_std[u] - 0.9189385), the density of z under the Gaussian, in fp32, u in order, every
 * operation rounded separately.  With squash it is the PRE-tanh density: the caller applies the tanh correction from the returned
 * actions.  NaN in log_std reaches that env's action and logp only.
 *
 * mz_policy_sample: one draw for the N rows of obs_dev [N, obs_dim] -> actions_dev [N, nu], logp_dev [N] (nullable).
 *
 * mz_rollout_policy_sample: n_steps times a ~ policy(obs); step(a); step k draws with noise_step + k.  The call leaves the handle
 * and every output exactly as this loop on the same stream would:
 *     for k in 0 .. n_steps - 1:
 *         mz_policy_sample(noise_seed, noise_step + k, obs_dev -> a_k, row k of logp_seq_dev)
 *         mz_step(a_k -> obs_dev, row k of reward_dev / done_dev / goal_idx_dev / info_dev)
 * Arrays as in mz_rollout_policy; actions_seq_dev [n_steps, N, nu] (nullable) gets the sampled actions, logp_seq_dev [n_steps, N]
 * (nullable) their log-probs.  Handles with "rollout_fused" = 1 sample inside the fused rollout kernels (launches of at most 256
 * steps; the next launch continues at noise_step + the steps done so far), every other handle runs the loop above inside the call.
 * Both return MZ_OK, MZ_ERR_ARG (as the two entries above, with npar_s for npar) or MZ_ERR_HIP. */
int32_t mz_policy_sample(mz_handle* h, const float* params_dev, int64_t param_env_stride, int32_t hidden, int32_t squash,
                         double action_scale, uint64_t noise_seed, uint64_t noise_step, const float* obs_dev, float* actions_dev,
                         float* logp_dev, void* stream);
int32_t mz_rollout_policy_sample(mz_handle* h, int32_t n_steps, const float* params_dev, int64_t param_env_stride, int32_t hidden,
                                 int32_t squash, double action_scale, uint64_t noise_seed, uint64_t noise_step, float* obs_dev,
                                 float* reward_dev, uint8_t* done_dev, int32_t* goal_idx_dev, float* info_dev, float* obs_seq_dev,
                                 float* actions_seq_dev, float* logp_seq_dev, void* stream);

/* A critic on the device, and generalised advantage estimation (actor-critic data collection: PPO, A2C, REINFORCE with a baseline).
 *
 * A critic is a policy as above with nu = 1, never squashed, in a parameter vector of its own: hidden == 0 affine, 1 <= hidden <=
 * MZ_POLICY_MAX_HIDDEN one tanh hidden layer, nvpar = obs_dim * Hv + Hv + Hv + 1 (or obs_dim + 1) fp32 numbers, input-major;
 * vparams_dev [nvpar] (env_stride == 0) or [N, nvpar] (env_stride == nvpar); any other stride is MZ_ERR_ARG.  The value of a row is
 * the pre-squash sum of its one output unit, in the arithmetic of the policies (one lane per unit, serially, fp32, no contraction):
 * numpy reproduces the affine case bit for bit.  NaN in one env's critic parameters reaches that env's values only.
 *
 * mz_value: values_dev [N] = V(obs_dev [N, obs_dim]).
 *
 * mz_rollout_actor_critic: mz_rollout_policy (sample == 0: noise_seed, noise_step and logp_seq_dev are ignored) or
 * mz_rollout_policy_sample (sample == 1) with the critic evaluated where the observation rows sit.  The defining loop — the call leaves
 * the handle and every output as these calls on the same stream would leave them, bit for bit:
 *     for k in 0 .. n_steps - 1:
 *         value_seq[k]      = mz_value(obs_dev)
 *         a_k               = sample ? mz_policy_sample(noise_step + k, obs_dev) : mz_policy_act(obs_dev)
 *         mz_step(a_k -> obs_dev, row k of the outputs)
 *         next_value_seq[k][i] = (auto_reset && done[k][i]) ? mz_value(row i of the bound final_obs) : mz_value(row i of obs_dev)
 * so next_value_seq[k] is the value of the row step k produced BEFORE any auto-reset — for an env that finished, of its terminal
 * observation, which a learner needs to bootstrap a time-limit truncation (done & 2) —, and equals value_seq[k + 1] wherever
 * done[k] == 0.  With critic == NULL the call IS mz_rollout_policy / mz_rollout_policy_sample.  A critic cannot influence the
 * rollout: actions, state, rewards, dones and status words are those of the call without it.  Handles with "rollout_fused" = 1
 * evaluate the critic inside the fused rollout kernels (on the terminal row before the auto-reset overwrites it, once more on the new
 * episode's first row); every other handle runs the loop above inside the call.
 * MZ_ERR_ARG, with a message that names the argument: sample outside {0, 1}; with a non-NULL critic: NULL critic->params_dev,
 * critic->hidden outside 0 .. MZ_POLICY_MAX_HIDDEN, critic->env_stride neither 0 nor nvpar, critic->reserved != 0, and
 * critic->next_value_seq_dev requested with auto-reset on and no final_obs buffer bound (mz_bind_final_obs) — on every handle, so
 * that the contract does not depend on the engine; and everything mz_rollout_policy / mz_rollout_policy_sample refuse.
 *
 * mz_gae: advantages and returns from the [n_steps, N] rows of a rollout, one backward scan per env, k from n_steps - 1 down to 0,
 * carry = 0 at the start; fp32 throughout, every operation rounded separately; selects, not multiplications by a mask, so a NaN
 * bootstrap value behind a true termination cannot leak (csrc/mz_gae.h):
 *     g = (float)gamma;  gl = g * (float)lam
 *     b     = (done & 1) ? 0.0f : g * next_value       true termination: no bootstrap; a time limit alone (done == 2) bootstraps from
 *     delta = (reward + b) - value                     the terminal observation's value
 *     c     = done ? 0.0f : gl * carry                 any episode end cuts the recursion
 *     adv   = delta + c;  carry = adv;  ret = adv + value
 * adv_dev [n_steps, N]; ret_dev [n_steps, N] (nullable).  n_steps 1 .. 65536.  Returns MZ_OK, MZ_ERR_ARG or MZ_ERR_HIP. */
typedef struct mz_critic {
  const float* params_dev;
  int64_t env_stride;
  int32_t hidden;
  int32_t reserved;          /* 0 */
  float* value_seq_dev;      /* [n_steps, N]  V(the row the policy acted on at step k)            (nullable) */
  float* next_value_seq_dev; /* [n_steps, N]  V(the row step k produced, BEFORE any auto-reset)   (nullable) */
} mz_critic;
int32_t mz_value(mz_handle* h, const float* vparams_dev, int64_t env_stride, int32_t hidden, const float* obs_dev, float* values_dev,
                 void* stream);
int32_t mz_rollout_actor_critic(mz_handle* h, int32_t n_steps, const float* params_dev, int64_t param_env_stride, int32_t hidden,
                                int32_t squash, double action_scale, int32_t sample, uint64_t noise_seed, uint64_t noise_step,
                                const mz_critic* critic, float* obs_dev, float* reward_dev, uint8_t* done_dev, int32_t* goal_idx_dev,
                                float* info_dev, float* obs_seq_dev, float* actions_seq_dev, float* logp_seq_dev, void* stream);
int32_t mz_gae(mz_handle* h, int32_t n_steps, const float* reward_dev, const uint8_t* done_dev, const float* value_dev,
               const float* next_value_dev, double gamma, double lam, float* adv_dev, float* ret_dev, void* stream);

/* Networks of up to two hidden layers, with tanh or ReLU units (the obs -> 64 -> 64 -> out default of PPO / A2C / ES code): the
 * policies and critics above, described by a struct.  Additive entries: MZ_ABI_VERSION does not change for them, and the struct
 * carries its own size (struct_size = sizeof of the struct as the caller compiled it; any other value is MZ_ERR_ARG).
 *
 * A network has n_hidden = 0, 1 or 2 hidden layers of hidden[0], hidden[1] = 1 .. MZ_POLICY_MAX_HIDDEN units (entries of layers not
 * in use: 0) and one activation for both: MZ_ACT_TANH, tanhf(acc), or MZ_ACT_RELU, acc < 0.0f ? 0.0f : acc — a select that adds no
 * rounding, keeps -0.0f and lets a NaN through.  Packed vector, input-major as above; n_hidden 0 and 1 are the two layouts above, and
 *   n_hidden == 2     W1t [obs_dim][H1], b1 [H1], W2t [H1][H2], b2 [H2], W3t [H2][nout], b3 [nout]
 * with nout = nu for an actor and 1 for a critic, then log_std [nu] where the call samples.  count: the floats of one vector, log_std
 * included where the call samples; params_dev [count] (env_stride == 0) or [N, count] (env_stride == count).  The arithmetic is that
 * of the policies above (csrc/mz_policy.h: one lane per unit, serially through one dot product, fp32, no contraction; a layer-2 unit
 * reads the complete layer-1 vector), so a ReLU network without squash is reproduced bit for bit by fp32 arithmetic anywhere, at any
 * depth (mujoco_maze_amd/policy.py reference), and with n_hidden <= 1 and MZ_ACT_TANH every entry below returns the bits of the
 * entry above it stands for.  squash and action_scale belong to an actor; a critic has squash == 0 and its action_scale is ignored.
 *
 * mz_net_act: mz_policy_act (sample == 0: noise_seed, noise_step and logp_dev are ignored) or mz_policy_sample (sample == 1).
 * mz_net_value: mz_value.
 * mz_rollout_net: the loop in the comment of mz_rollout_actor_critic with mz_net_value / mz_net_act in place of mz_value /
 * mz_policy_act / mz_policy_sample — the call leaves the handle and every output as that loop would, bit for bit; critic nullable,
 * value_seq_dev / next_value_seq_dev [n_steps, N] (nullable; ignored without a critic).  Noise, log-prob, the launch split of the
 * fused handles, the final_obs requirement for next_value_seq_dev under auto-reset and n_steps 1 .. 65536 are as above.  Handles with
 * "rollout_fused" = 1 evaluate both networks inside the fused rollout kernels; every other handle runs the loop inside the call.
 * MZ_ERR_ARG, with a message that names the argument: a NULL net or NULL params_dev, a wrong struct_size, n_hidden outside 0 .. 2, a
 * width outside 1 .. MZ_POLICY_MAX_HIDDEN in a layer in use, a non-zero width in a layer not in use, activation outside
 * {MZ_ACT_TANH, MZ_ACT_RELU}, squash outside {0, 1}, a critic with squash != 0, an env_stride that is neither 0 nor count, sample
 * outside {0, 1}, and everything mz_rollout_actor_critic refuses.
 *
 * Wide networks: mz_set_option(h, "wide_nets", v), v = 0, 1 or 2 (anything else: MZ_ERR_ARG, the mode stays), reported by
 * mz_get_info(h, "wide_nets").  Opt-in per handle; MZ_POLICY_MAX_HIDDEN, MZ_ABI_VERSION and every struct stay as they are.
 *   0 (default)  as described above: a width above MZ_POLICY_MAX_HIDDEN is refused.
 *   1            every entry that takes an mz_net — mz_net_act, mz_net_value, mz_net_sample, mz_net_sample_head, mz_net_eval_ctx,
 *                mz_net_value_ctx, mz_rollout_net, mz_rollout_ex, mz_rollout_head, mz_rollout_ctx — accepts hidden[k] = 1 ..
 *                MZ_NET_MAX_WIDTH.  A network with a layer wider than MZ_POLICY_MAX_HIDDEN runs the tiled kernel (csrc/mz_net_tile.h:
 *                a tile of 16 rows per block, each shared weight loaded once per tile); every other network runs what it ran, the
 *                fused rollout kernels included.
 *   2            as 1, and every mz_net network of the handle runs the tiled kernel whatever its widths.
 * The arithmetic does not change — one serial fp32 dot product per unit, in index order, product and sum rounded separately —, so the
 * two kernel families return the same bits for the same network and policy.py stays the model at every width.  Everything else
 * about a network is as above: the packed layout, count and both env_stride values, both activations, the squash, both noise modes,
 * log_std behind the network or a head, a bound normaliser, a context, the final_obs row of a critic under auto-reset.  A rollout
 * plan in which the actor or the critic runs tiled takes the launch-by-launch loop on every handle, as a plan with a context does,
 * and each of its networks picks its kernel by its own widths and the mode; "rollout_fused" keeps describing mz_rollout.  The entries
 * that take an int `hidden` stay at MZ_POLICY_MAX_HIDDEN and on their kernels in every mode.  MZ_ERR_UNSUPPORTED: a tiled network
 * with more than 128 output units (nu > 128, or a head with nu > 64). */
#define MZ_NET_MAX_WIDTH 256
#define MZ_NET_MAX_HIDDEN_LAYERS 2
#define MZ_ACT_TANH 0
#define MZ_ACT_RELU 1
typedef struct mz_net {
  uint32_t struct_size;      /* sizeof(mz_net); anything else: MZ_ERR_ARG */
  int32_t n_hidden;          /* 0, 1, 2 */
  int32_t hidden[2];         /* widths 1 .. MZ_POLICY_MAX_HIDDEN of the layers in use; unused entries 0 */
  int32_t activation;        /* MZ_ACT_*, of the hidden layers */
  int32_t squash;            /* actor: 0 / 1; a critic: 0 */
  double action_scale;
  const float* params_dev;   /* [count] or [N, count] */
  int64_t env_stride;        /* 0 or count (count includes log_std[nu] when the call samples) */
} mz_net;
int32_t mz_net_act(mz_handle* h, const mz_net* actor, int32_t sample, uint64_t noise_seed, uint64_t noise_step, const float* obs_dev,
                   float* actions_dev, float* logp_dev, void* stream);
int32_t mz_net_value(mz_handle* h, const mz_net* critic, const float* obs_dev, float* values_dev, void* stream);
int32_t mz_rollout_net(mz_handle* h, int32_t n_steps, const mz_net* actor, int32_t sample, uint64_t noise_seed, uint64_t noise_step,
                       const mz_net* critic, float* value_seq_dev, float* next_value_seq_dev, float* obs_dev, float* reward_dev,
                       uint8_t* done_dev, int32_t* goal_idx_dev, float* info_dev, float* obs_seq_dev, float* actions_seq_dev,
                       float* logp_seq_dev, void* stream);

/* Off-policy collection (TD3 / DDPG / SAC-style replay): every step's transition (s_k, a_k, r_k, s'_k, d_k) from one call, and
 * exploration noise on the action.  Additive entries: MZ_ABI_VERSION does not change for them; both structs carry their own size.
 *
 * next_obs_seq_dev [n_steps, N, obs_dim] fp32 (nullable): the row step k produced, BEFORE any auto-reset — raw, never normalised:
 *     after mz_step k:  next_obs_seq[k][i] = (auto_reset && done[k][i]) ? final_obs[i] : obs_dev[i]
 * Where done[k][i] == 0, and everywhere without auto-reset, it holds the bits of obs_seq[k][i]; where the env finished under
 * auto-reset it is that step's terminal row (the view entries of a top-down-view task included), which obs_seq never holds and of
 * which the bound final_obs buffer keeps only the env's latest.  s_k is the row the policy acted on: the entry observation for
 * k = 0, obs_seq[k - 1] afterwards.  Handles with "rollout_fused" = 1 store the row from inside the fused kernels, where it is on
 * chip; every other handle launches one select kernel per step (a plain copy without auto-reset).  With auto-reset on and no
 * final_obs buffer bound the request is MZ_ERR_ARG on every handle — the rule of next_value_seq_dev.
 *
 * mz_noise: how a sampled action is formed from the actor's pre-squash output m_u, s = expf(log_std[u]) and eps_u (above):
 *   MZ_NOISE_PRE_SQUASH  z = m + s * eps;  a = squash ? A * tanhf(z) : z                     (mz_policy_sample: the noise is squashed)
 *   MZ_NOISE_ACTION      p = s * eps;  b = squash ? A * tanhf(m) : m;  z = b + p;
 *                        a = squash ? (z < -A ? -A : (z > A ? A : z)) : z                    (the tanh belongs to the deterministic actor
 *                        a learner trains, the noise goes on the action, the result is clipped to the action range: TD3 / DDPG)
 * A = (float)action_scale; fp32, every operation rounded separately, selects (a NaN passes).  eps, the key schedule (step k draws
 * with step + k) and logp are the same in both modes — logp is the density of the unclipped z around b, bit-equal to the other
 * mode's for the same seed and step — and with squash == 0 the two modes return the same bits.
 *
 * mz_net_sample: mz_net_act with sample == 1 and the noise of `noise` (required); logp_dev nullable.
 *
 * mz_rollout_ex: the open-loop and the closed-loop rollouts behind one struct.  Exactly one of io->actions_dev (then it is
 * mz_rollout with action_step_stride) and io->actor (then it is mz_rollout_net: noise NULL means sample == 0, critic nullable,
 * value_seq_dev / next_value_seq_dev ignored without a critic) is non-NULL; the remaining fields are the arrays of those two
 * entries and next_obs_seq_dev.  With next_obs_seq_dev == NULL and mode MZ_NOISE_PRE_SQUASH the call runs the launches of
 * mz_rollout / mz_rollout_net and returns their bits; next_obs_seq_dev and the mode change nothing else the call returns.
 * MZ_ERR_ARG, with a message that names the argument: a NULL io; a wrong struct_size in either struct; both action sources or
 * neither; noise or critic without an actor; noise->mode outside {MZ_NOISE_PRE_SQUASH, MZ_NOISE_ACTION}; next_obs_seq_dev under
 * auto-reset without a bound final_obs buffer; and everything mz_rollout / mz_rollout_net refuse.  A refused call leaves the
 * handle as it was. */
#define MZ_NOISE_PRE_SQUASH 0
#define MZ_NOISE_ACTION 1
typedef struct mz_noise {
  uint32_t struct_size;      /* sizeof(mz_noise); anything else: MZ_ERR_ARG */
  int32_t mode;              /* MZ_NOISE_* */
  uint64_t seed, step;       /* noise_seed; noise_step of the first step */
} mz_noise;
typedef struct mz_rollout_io {
  uint32_t struct_size;      /* sizeof(mz_rollout_io); anything else: MZ_ERR_ARG */
  int32_t n_steps;           /* 1 .. 65536 */
  const float* actions_dev;  /* open loop: step k reads its [N, nu] actions at actions_dev + k * action_step_stride ... */
  int64_t action_step_stride;
  const mz_net* actor;       /* ... or closed loop: a_k = actor(obs) */
  const mz_noise* noise;     /* NULL: deterministic */
  const mz_net* critic;      /* nullable */
  float* obs_dev;            /* [N, obs_dim]; IN/OUT with an actor */
  float* reward_dev;         /* [n_steps, N] */
  uint8_t* done_dev;         /* [n_steps, N] */
  int32_t* goal_idx_dev;     /* [n_steps, N]           (nullable) */
  float* info_dev;           /* [n_steps, N, 4]        (nullable) */
  float* obs_seq_dev;        /* [n_steps, N, obs_dim]  (nullable) */
  float* actions_seq_dev;    /* [n_steps, N, nu]       (nullable; closed loop) */
  float* logp_seq_dev;       /* [n_steps, N]           (nullable; with noise) */
  float* value_seq_dev;      /* [n_steps, N]           (nullable; with a critic) */
  float* next_value_seq_dev; /* [n_steps, N]           (nullable; with a critic) */
  float* next_obs_seq_dev;   /* [n_steps, N, obs_dim]  (nullable) */
} mz_rollout_io;
int32_t mz_net_sample(mz_handle* h, const mz_net* actor, const mz_noise* noise, const float* obs_dev, float* actions_dev, float* logp_dev,
                      void* stream);
int32_t mz_rollout_ex(mz_handle* h, const mz_rollout_io* io, void* stream);

/* Stochastic actors with a state-dependent log-std head (SAC; PPO code with a second head): the standard deviation is an output of
 * the network, and the log-probability may be that of the squashed action.  Additive entries: MZ_ABI_VERSION does not change for
 * them; mz_head carries its own size.
 *
 * A head actor is an mz_net whose output layer has 2 nu units — units 0 .. nu - 1 the means m_u, units nu .. 2 nu - 1 the raw
 * log-stds r_u; packed input-major as above, ... W_out_t [nin][2 nu], b_out [2 nu] — and NO trailing log_std vector:
 * count = the floats of the network with nout = 2 nu; params_dev [count] (env_stride == 0) or [N, count] (env_stride == count).
 * Every unit is one lane through one dot product, as above.  In fp32, every operation rounded separately (csrc/mz_policy.h):
 *     ls_u = r_u < lo ? lo : (r_u > hi ? hi : r_u)         two selects: a NaN passes; lo = -inf / hi = +inf switch a side off
 *     s = expf(ls_u);  p = s * eps_u;  z_u = m_u + p;  a_u = squash ? A * tanhf(z_u) : z_u                  (MZ_NOISE_PRE_SQUASH)
 * with eps_u and the key schedule of mz_policy_sample (step k of a rollout draws with noise->step + k; slot: the global env slot).
 * logp, one lane, u = 0 .. nu - 1 in order:
 *     q = eps_u * eps_u;  h = -0.5f * q;  t = h - ls_u;  t = t - 0.9189385f;                     (mz_policy_sample's, clamped ls_u)
 *     logp_squashed:  x = -2.0f * z_u;  ax = fabsf(x);  e = expf(-ax);  l = log1pf(e);  sp = (x > 0.0f ? x : 0.0f) + l;
 *                     c = 0.6931472f - z_u;  c = c - sp;  c = 2.0f * c;  c = c + logA;  t = t - c;
 *     acc = acc + t
 * The correction is log |d(A tanh z) / dz| = log A + 2 (log 2 - z - softplus(-2 z)), finite wherever z is — never log(1 - tanh^2),
 * which is -inf in fp32 from |z| ~ 9.  logA = logf((float)action_scale) is computed once per call on the host and is exactly 0 for
 * action_scale == 1.  A NaN log-std unit reaches that unit's action and the row's logp only.  With zero weights into the log-std
 * units and a bias b inside the bounds the actions and the un-squashed logp are the bits of mz_net_sample with log_std = b; with
 * lo = -inf and a bias of -inf the actions are the bits of mz_net_act on the means' columns (wherever the mean is not -0).
 *
 * mz_net_sample_head: the head actor on the rows of obs_dev; actions_dev [N, nu], logp_dev [N] (nullable).
 * mz_rollout_head: mz_rollout_ex with a head actor.  The call leaves the handle, every output, the status words and the bound
 * buffers as this loop would, bit for bit:
 *     for k:  [mz_net_value]; mz_net_sample_head(noise step + k); mz_step; [mz_net_value of the terminal / new row, as in
 *             mz_rollout_actor_critic]
 * Critic, next_obs_seq_dev, a bound normaliser and a bound final_obs buffer compose as in mz_rollout_ex.  Handles with
 * "rollout_fused" = 1 sample inside the fused rollout kernels — chains of five or six links excepted —; every other handle runs the
 * loop inside the call.
 * head == NULL: the two calls ARE mz_net_sample and mz_rollout_ex — the same launches, the same bits.
 * MZ_ERR_ARG, with a message that names the argument: a wrong head->struct_size, kind or reserved; logp_squashed outside {0, 1}, or
 * 1 with actor->squash == 0; a NaN bound or log_std_min > log_std_max; a head without an actor or without noise (a head samples);
 * noise->mode != MZ_NOISE_PRE_SQUASH; an actor->env_stride that is neither 0 nor the head count; and everything mz_net_sample /
 * mz_rollout_ex refuse.  MZ_ERR_UNSUPPORTED: nu > MZ_POLICY_MAX_HIDDEN.  A refused call leaves the handle as it was. */
#define MZ_HEAD_STATE_STD 1
typedef struct mz_head {
  uint32_t struct_size;      /* sizeof(mz_head); anything else: MZ_ERR_ARG */
  int32_t kind;              /* MZ_HEAD_STATE_STD */
  float log_std_min, log_std_max; /* lo, hi of the clamp; -inf / +inf allowed; NaN or lo > hi: MZ_ERR_ARG */
  int32_t logp_squashed;     /* 0: density of z (as mz_policy_sample); 1: density of the action A * tanh(z); needs squash == 1 */
  int32_t reserved;          /* 0 */
} mz_head;
int32_t mz_net_sample_head(mz_handle* h, const mz_net* actor, const mz_head* head, const mz_noise* noise, const float* obs_dev,
                           float* actions_dev, float* logp_dev, void* stream);
int32_t mz_rollout_head(mz_handle* h, const mz_rollout_io* io, const mz_head* head, void* stream);

/* Context inputs (goal-conditioned actors pi(a | s, g), HIRO's low level pi(a | s, subgoal), skill policies pi(a | s, z), Q(s, a)):
 * a per-env row c of `dim` fp32 entries that every network of the call reads BEHIND the observation.  Additive entries:
 * MZ_ABI_VERSION does not change for them; mz_context carries its own size.
 *
 * With a context the input row of a network is r = [y | c], obs_dim + dim entries: y the obs_dim entries of the observation (a
 * top-down view's included), normalised exactly as above while a normaliser is bound, else raw; c the context, never normalised and
 * never clipped.  Every first-layer unit is the one dot product of above over r in index order — the context terms last — and the
 * packed vectors are the layouts above with obs_dim + dim in place of obs_dim (count likewise).  Noise, log-prob, head, squash, the
 * noise mode and the critic — which reads the same r — are unchanged.  A context whose columns carry zero weights returns the bits of
 * the network without those rows (a sum plus +-0 is the sum); a NaN in env i's context reaches env i's outputs only.
 *
 * update == MZ_CTX_HOLD: the context is constant for the whole call.
 * update == MZ_CTX_RELATIVE (rollouts; HIRO's goal transition h(s, g, s') = s + g - s'), rel_dims = D, 1 <= D <= min(dim, obs_dim):
 * after step k, for each env with done[k] == 0 and each d < D, in fp32, a sum then a difference, two roundings:
 *     tmp = c[d] + s[d];   c[d] = tmp - s'[d]
 * s: the RAW row the actor acted on at step k; s': the RAW row step k produced (next_obs_seq[k]), never normalised.  Where
 * done[k] != 0 the context is left alone, with or without auto-reset: no transition crosses an episode end.  Entries d >= D hold.
 * value_seq[k] reads the context of step k; next_value_seq[k] the context after the transition (for an env that finished: the
 * unchanged context with the terminal row), and so does the value of a new episode's first row.
 *
 * ctx_dev [N, dim] is read by the single calls and IN/OUT for a rollout: on return it holds what step n_steps would read, so two
 * calls in a row equal one call over the joined steps.  ctx_seq_dev [n_steps, N, dim] (nullable; rollouts): the context the networks
 * read at step k.
 *
 * mz_net_eval_ctx: mz_net_act with sample == 0 (noise == NULL), mz_net_sample (noise given) or mz_net_sample_head (head given) on
 * the rows [obs | ctx].  mz_net_value_ctx: mz_net_value likewise — with the actions as the context it is Q(s, a).
 * mz_rollout_ctx: mz_rollout_head (head nullable) with the context; the call leaves the handle, every output and ctx_dev as this
 * loop would, bit for bit:
 *     for k:  [ctx_seq[k] = ctx]; [mz_net_value_ctx]; mz_net_eval_ctx(noise step + k); mz_step; [the transition];
 *             [mz_net_value_ctx of the terminal / new row, as in mz_rollout_actor_critic]
 * Every handle runs that loop inside the call: one copy of the D old columns before the step and one small kernel behind it apply the
 * transition.  The networks run the kernels of the bound-normaliser path; without a normaliser the staged row holds the raw bits.
 * ctx == NULL: each entry IS the call it extends — the same launches, the same bits.
 * MZ_ERR_ARG, with a message that names the argument: a wrong ctx->struct_size; dim outside 1 .. MZ_MAX_CONTEXT; an unknown update;
 * rel_dims outside 1 .. min(dim, obs_dim) with MZ_CTX_RELATIVE, or non-zero with MZ_CTX_HOLD; MZ_CTX_RELATIVE or ctx_seq_dev in a
 * single call; reserved != 0; a NULL ctx_dev; an env_stride that is neither 0 nor the count for obs_dim + dim; an open-loop io; and
 * everything the extended entry refuses.  A refused call leaves the handle as it was. */
#define MZ_MAX_CONTEXT 32
#define MZ_CTX_HOLD 0
#define MZ_CTX_RELATIVE 1
typedef struct mz_context {
  uint32_t struct_size;      /* sizeof(mz_context); anything else: MZ_ERR_ARG */
  int32_t dim;               /* C: 1 .. MZ_MAX_CONTEXT */
  int32_t update;            /* MZ_CTX_* */
  int32_t rel_dims;          /* D with MZ_CTX_RELATIVE: 1 .. min(dim, obs_dim); 0 with MZ_CTX_HOLD */
  int64_t reserved;          /* 0 */
  float* ctx_dev;            /* [N, dim]; IN/OUT for a rollout */
  float* ctx_seq_dev;        /* [n_steps, N, dim]  (nullable; rollouts) */
} mz_context;
int32_t mz_net_eval_ctx(mz_handle* h, const mz_net* actor, const mz_head* head, const mz_noise* noise, const mz_context* ctx,
                        const float* obs_dev, float* actions_dev, float* logp_dev, void* stream);
int32_t mz_net_value_ctx(mz_handle* h, const mz_net* critic, const mz_context* ctx, const float* obs_dev, float* values_dev, void* stream);
int32_t mz_rollout_ctx(mz_handle* h, const mz_rollout_io* io, const mz_head* head, const mz_context* ctx, void* stream);

/* Normalised observations for the device-side networks (the observation half of VecNormalize; ARS-V2's state normalisation), and the
 * forward return scan that reward scaling and episode logging need.  Additive entries: MZ_ABI_VERSION does not change for them.
 *
 * mz_bind_obs_norm: binds one normaliser, shared by all envs, to the handle.  mean_dev and inv_std_dev are [obs_dim] fp32 DEVICE
 * arrays owned by the caller (obs_dim = mz_obs_dim: a top-down view's entries included).  While bound, every network evaluation reads
 * the row y in place of the raw row x — element i, fp32, every operation rounded separately (csrc/mz_policy.h mzp_norm_elem):
 *     d = x[i] - mean[i];   y = d * inv_std[i];   y = y < -c ? -c : (y > c ? c : y)             c = (float)clip
 * a product with inv_std, never a quotient; two selects, so a NaN passes through, clip = +inf switches the clip off, x = +-inf becomes
 * +-c and a constant column (d == 0) becomes 0 whatever a finite inv_std is.  numpy reproduces it bit for bit
 * (mujoco_maze_amd/policy.py normalize_reference), so an affine or ReLU network without squash on normalised rows stays
 * bit-reproducible.
 *  normalised  what the NETWORKS read in mz_policy_act, mz_policy_sample, mz_value, mz_net_act, mz_net_value and the four closed-loop
 *              rollouts mz_rollout_policy, mz_rollout_policy_sample, mz_rollout_actor_critic, mz_rollout_net — the critic's terminal row
 *              included: the final_obs row in the loop form, the on-chip terminal row in the fused form.  Each of these calls equals
 *              the unbound call on rows normalised beforehand, and the rollouts still equal their defining loops bit for bit.
 *  raw         everything the env itself reads or writes: obs_dev, obs_seq_dev, the bound final_obs buffer and the bound record; the
 *              task predicate and the info rows; mz_step and the open-loop mz_rollout, which do not look at the binding.
 * The arrays are read by every later evaluation in stream order, so the caller may rewrite them between two calls without binding
 * again.  Both pointers NULL unbinds (clip is ignored).  The call stores the two pointers and clip and does not synchronise (`stream`
 * is not used).  While a normaliser is bound the legacy entries (int `hidden`, tanh) run the kernels of the mz_net entries, which
 * return the same bits for such a network.  mz_get_info "obs_norm" is 1 while a normaliser is bound, else 0.
 * Returns MZ_OK, or MZ_ERR_ARG with a message that names the argument: exactly one pointer NULL; clip NaN or <= 0.  A refused call
 * leaves the previous binding in place.
 *
 * mz_return_scan: the running discounted return and the episode step count of every env over the [n_steps, N] rows of a rollout, one
 * forward scan per env, k from 0 up to n_steps - 1; fp32, every operation rounded separately; selects (csrc/mz_returns.h):
 *     g = (float)gamma
 *     p = g * carry;  s = p + reward[k];  ret_seq[k] = s;  len = len + 1;  len_seq[k] = len
 *     carry = done[k] ? 0.0f : s;         len = done[k] ? 0 : len
 *  carry_dev [N] fp32 and len_carry_dev [N] i32 are IN/OUT and per env: a scan over K1 steps followed by a scan over K2 steps equals
 *            one scan over K1 + K2 steps.  A new series starts from zeros.
 *  ret_seq_dev [n_steps, N] fp32; len_seq_dev [n_steps, N] i32.
 * With gamma == 1 the product is exact: ret_seq[k] where done[k] != 0 is that episode's return and len_seq[k] its length.  With
 * gamma < 1 ret_seq is the series whose running variance VecNormalize divides rewards by.  len_carry_dev and len_seq_dev are nullable;
 * a NULL len_carry_dev means the length is not tracked, and a len_seq_dev without it is MZ_ERR_ARG.  carry_dev and ret_seq_dev are
 * required.  n_steps 1 .. 65536.  Returns MZ_OK, MZ_ERR_ARG or MZ_ERR_HIP. */
int32_t mz_bind_obs_norm(mz_handle* h, const float* mean_dev, const float* inv_std_dev, double clip, void* stream);
int32_t mz_return_scan(mz_handle* h, int32_t n_steps, const float* reward_dev, const uint8_t* done_dev, double gamma,
                       float* carry_dev, int32_t* len_carry_dev, float* ret_seq_dev, int32_t* len_seq_dev, void* stream);

/* Per-env status words accumulated since the last call (then cleared). [N] i32. */
int32_t mz_get_status(mz_handle* h, int32_t* status_dev, void* stream);

/* Diagnostics for parity tests: one forward-dynamics evaluation at the current
 * state with ctrl = actions; writes qacc [N, nv] and ncon/nefc [N, 2]. */
int32_t mz_debug_forward(mz_handle* h, const float* actions_dev, float* qacc_dev, int32_t* counts_dev, void* stream);

/* Parity-test entries for the two places where the reference's float64 DECISIONS must be reproduced bit for bit.
 * mz_debug_task_eval: MazeTask.reward / termination / first matching goal (maze_task.py:43-47,77-81,110-111,403-407) on
 *   n_rows observation rows [n_rows, obs_dim] fp32 — the very task_eval_dev (csrc/mz_task.h) instance the handle's step kernel runs:
 *   reward_dev[n_rows] = task reward only (no inner reward), done_dev[n_rows] u8 = termination, goal_idx_dev (nullable).
 *   With per-env goals bound (mz_bind_env_goals) row r < num_envs is judged with env r's goals, later rows with the shared table.
 * mz_debug_detect: CollisionDetector.detect + the bounce / give-up rule of MazeEnv.step (maze_env_utils.py:96-123,186-206;
 *   maze_env.py:457-464) on n_rows float64 moves old_xy -> new_xy ([n_rows, 2] each): hit_dev[n_rows] = 0 no wall hit,
 *   1 bounced, 2 gave up (position restored), -1 collinear move (the reference raises ZeroDivisionError);
 *   point_dev[n_rows, 2] (nullable) = first collision point, final_xy_dev[n_rows, 2] = position after the rule.  Point only. */
int32_t mz_debug_task_eval(mz_handle* h, int32_t n_rows, const float* obs_dev, float* reward_dev, uint8_t* done_dev,
                           int32_t* goal_idx_dev, void* stream);
int32_t mz_debug_detect(mz_handle* h, int32_t n_rows, const double* old_xy_dev, const double* new_xy_dev, int32_t* hit_dev,
                        double* point_dev, double* final_xy_dev, void* stream);

/* Kernel-internal phase timers (option "profile_phases" = 1 selects the instrumented kernel build):
 * 16 accumulators over the window since the last mz_read_wave_phase_cycles (which clears the slots this call sums; this call clears
 * nothing) — slots 0..12 shader cycles per phase (ids: tools/phase_profile.py), 13 the most loaded workgroup's total over the window,
 * 14 the sum of squared per-workgroup window totals (units of 256 cycles), 15 Newton iterations — taken from the first env group of
 * every workgroup and reduced on the host from the per-workgroup slots (the kernels issue no same-address atomics: they disturbed
 * the waves still running); out16_host is HOST memory. */
int32_t mz_read_phase_cycles(mz_handle* h, uint64_t* out16_host);
/* Same instrumented build: total shader cycles of every workgroup (one wavefront = 64 / lanes_per_env envs) accumulated
 * since the last call, n_host <= num_envs entries into HOST memory; cleared on read.  For load-balance analysis. */
int32_t mz_read_wave_cycles(mz_handle* h, uint64_t* out_host, int32_t n_host);
/* Same build: the 16 phase slots of every workgroup ([n_host][16] into HOST memory, accumulated since the last call, cleared on
 * read) — which phase makes the slowest waves slow (Ant kernels). */
int32_t mz_read_wave_phase_cycles(mz_handle* h, uint64_t* out_host, int32_t n_host);

/* Top view of env states as images: render.render_top_down (mujoco_maze_amd/render.py; the reference's MazeEnv.render with
 * image_shape, mujoco_maze/maze_env.py:389-420, draws a 3-D camera image instead) for `count` envs in one launch, pixel for pixel
 * what the Python rasteriser draws (csrc/mz_render.h; the device's sin / cos / atan2 of state angles may differ from the host's by
 * an ulp, which can move an edge pixel).
 *  qpos_dev    [count, nq] fp32 states to draw, row i for image i; NULL: the batch's current state, row env_idx[i] of what
 *              mz_get_state returns (the handle's engine copies it into a scratch buffer on `stream` first)
 *  env_idx_dev [count] i32 env of image i (any order, repeats allowed: it picks the state row without qpos_dev and the env's row
 *              of the per-env goal table of mz_bind_env_goals); NULL: 0 .. count - 1.  An index outside 0 .. num_envs - 1
 *              gives an all-zero image
 *  ngoal_style must equal the goal table's count; goal_rgb [ngoal][3] u8 and goal_size [ngoal] float64 are HOST arrays (the
 *              task's colours after Python's round() and marker radii, render.goal_style), read before the call returns
 *  rgb_dev     [count, height, width, 3] u8, row 0 at the top; width, height 2 .. 16384
 * Asynchronous on `stream`, no synchronisation.  Returns MZ_OK, MZ_ERR_ARG, MZ_ERR_HIP, or MZ_ERR_UNSUPPORTED for a user robot
 * (mz_model.robot = MZ_ROBOT_GENERIC: render.py does not draw a user's geoms). */
int32_t mz_render(mz_handle* h, const float* qpos_dev, const int32_t* env_idx_dev, int32_t count, int32_t width, int32_t height,
                  int32_t ngoal_style, const uint8_t* goal_rgb, const double* goal_size, uint8_t* rgb_dev, void* stream);

/* Average duration (ms) of the step kernel over the launches recorded since "time_kernels" was set (HIP events on
 * the stream each mz_step was given; synchronises on them); returns < 0 if not available. */
double mz_last_kernel_ms(const mz_handle* h);

#ifdef __cplusplus
}
#endif
#endif /* MAZESTEP_H */
