/* flybody_engine.h -- C-ABI of the MI355X-native batched fly-physics engine (libflybody_hip.so).
 *
 * WHAT THIS BOUNDARY REPLACES.  The reference has no FFI of its own: its hot path is
 *   env.step(action)  ->  dm_control composer.Environment.step  ->  10 x mujoco mj_step
 * created at flybody/fly_envs.py:152 (walk_imitation) / :94 (flight_imitation) and driven by the
 * task hooks flybody/tasks/walk_imitation.py:92-203, tasks/base.py:197-268 and
 * fruitfly/fruitfly.py:390-405,532-544,594-684.  The entry points below are what a maintainer
 * would bind (ctypes) behind `fly_envs.walk_imitation()` to step thousands of flies in lock-step
 * on one GPU; see INTEGRATION.md for the binding stub.
 *
 * Conventions: every function returns 0 on success and a negative code on failure, the message
 * is available from fb_last_error() (thread local).  The caller owns all buffers it passes in;
 * the library owns the handles.  One fb_batch is bound to one device; it is not thread-safe,
 * distinct batches may be driven from distinct host threads / processes (one process per GPU).
 * Batched arrays are row-major [n_env][width]: one environment's row is contiguous, so the
 * wavefront that owns the environment reads it coalesced.
 */
#ifndef FLYBODY_ENGINE_H
#define FLYBODY_ENGINE_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fb_model fb_model;
typedef struct fb_batch fb_batch;

/* fields for fb_batch_get / fb_batch_set / fb_batch_device_ptr */
enum {
  FB_QPOS = 0,        /* [n_env][nq]   physics real   */
  FB_QVEL = 1,        /* [n_env][nv]                  */
  FB_ACT = 2,         /* [n_env][na]                  */
  FB_CTRL = 3,        /* [n_env][nu]                  */
  FB_QACC = 4,        /* [n_env][nv]                  */
  FB_XPOS = 5,        /* [n_env][nbody][3]            */
  FB_XQUAT = 6,       /* [n_env][nbody][4]            */
  FB_SENSORDATA = 7,  /* [n_env][33]                  */
  FB_OBS = 8,         /* [n_env][nobs]   float32      */
  FB_REWARD = 9,      /* [n_env]         float32      */
  FB_DISCOUNT = 10,   /* [n_env]         float32      */
  FB_STEP_TYPE = 11,  /* [n_env]         int32  0 FIRST 1 MID 2 LAST (dm_env.StepType) */
  FB_NCON = 12,       /* [n_env]         int32        */
  FB_NEFC = 13,       /* [n_env]         int32        */
  FB_SOLVER_NITER = 14, /* [n_env]       int32        */
  FB_QFRC_BIAS = 15,  /* [n_env][nv]                  */
  FB_QFRC_PASSIVE = 16,
  FB_QACC_SMOOTH = 17,
  FB_QM = 18,         /* [n_env][nM] sparse mass matrix (dof_Madr layout) */
  FB_CONTACT = 19,    /* [n_env][64][8] dist,pos3,normal3,pairid      */
  FB_EFC_FORCE = 20,  /* [n_env][FB_MAXEFC]           */
  FB_QFRC_ACTUATOR = 21,
  FB_QFRC_CONSTRAINT = 22,
  FB_STEP_COUNT = 23, /* [n_env] int32 control steps since reset */
  FB_SUBTREE_COM = 24,/* [n_env][3] centre of mass of the WHOLE model (MuJoCo's subtree_com[0]: every body of every kinematic tree,
                         in walk_on_ball the ball included); the one reference point of FB_CVEL */
  FB_GEOM_XPOS = 27,  /* [n_env][ngeom][3] */
  FB_GEOM_XMAT = 28,  /* [n_env][ngeom][9] */
  FB_CVEL = 29,       /* [n_env][nbody][6] spatial velocity [angular, linear] of every body about FB_SUBTREE_COM, in a model with
                         several kinematic trees as well.  MuJoCo's cvel refers body b to subtree_com[body_rootid[b]], its own tree's
                         CoM: with two trees (walk_on_ball) the linear parts differ from MuJoCo's, the angular parts and every point
                         velocity do not -- the velocity of a point p of body b is linear + angular x (p - FB_SUBTREE_COM)
                         (flybody_amd/fluid.py: object_velocity; tests/test_smooth_stages.py) */
  FB_STEP_TICKS = 30, /* [n_env] int32: duration of the environment's last control step on the GPU (100 MHz ticks) */
  FB_LAUNCH_ORDER = 31, /* [n_env] int32: environment ids in the order the next full-batch step launches them
                           (longest last step first; scheduling only, results do not depend on it) */
  FB_REWARD_FACTORS = 26, /* [n_env][5] training-mode reward factors (com, qvel, root2site, joint_quat, wings) */
  FB_PROF = 25,       /* [n_env][112] int32 = 56 int64 per-phase cycle counters (profiling builds) */
  FB_WARN = 32,       /* [n_env] int32: FB_WARN_* bits raised during the last launch (cleared when a control step / reset starts).
                         Mirrors MuJoCo's nconmax / njmax warnings (fruitfly.xml:6) and adds the iteration limits. */
  FB_WARN_EVER = 33,  /* [n_env] int32: the same bits accumulated since the environment's last reset */
  FB_SIZE_STATS = 34, /* [n_env][4] int32: largest contact count, largest constraint-row count, number of substeps with more than 32 rows,
                         number of substeps with more than 64 rows (= beyond one row per lane: d_newton_wide) -- over every constraint
                         set-up since the batch was created, i.e. every substep AND every forward evaluation (fb_batch_forward, the
                         forward pass of a reset); not cleared by resets; fb_batch_set(FB_SIZE_STATS, zeros) clears.  Against FB_MAXCON / FB_MAXEFC and
                         MuJoCo's nconmax 100 / njmax 300 (fruitfly.xml:6) this says how close a run came to the caps. */
  FB_SITE_XPOS = 35,  /* [n_env][nsite][3] site positions (position stage) */
  FB_IK_ERR = 36,     /* [n_env][2] FP64: err_norm, err_norm_first_term of the last fb_batch_ik (read-only; allocated by the first call) */
  FB_IK_STEPS = 37,   /* [n_env][2] int32: steps, success of the last fb_batch_ik (read-only; allocated by the first call) */
  FB_QFRC_INVERSE = 38,  /* [n_env][nv] FP64: qfrc_inverse of the last fb_batch_inverse (read-only; allocated by the first call) */
  FB_CONTACT_FORCE = 39, /* [n_env][FB_MAXCON][3] FP64: force of contact c of the last fb_batch_inverse in its contact frame (normal,
                            tangent 1, tangent 2; zero beyond the contact's condim and for c >= FB_NCON), rows as FB_CONTACT (read-only) */
  FB_QFRC_APPLIED = 40,  /* [n_env][nv] physics real: MuJoCo's qfrc_applied, a generalised force per dof (caller-owned input, see below) */
  FB_XFRC_APPLIED = 41,  /* [n_env][nbody][6] physics real: MuJoCo's xfrc_applied, a Cartesian wrench per body: force(3) then torque(3) in the
                            world frame, applied at the body's centre of mass (xipos); the world body's row is ignored */
  FB_ENV_MODEL = 42,     /* [n_env] int32: index into the models of fb_batch_create_group that the environment is stepped with (see below);
                            fails on a batch made by fb_batch_create */
  FB_QFRC_LAW = 43,      /* [n_env][nv] physics real: the generalised force u of the control law in the environment's last substep (or forward
                            evaluation); zero after a reset (read-only; allocated by fb_batch_set_control_law) */
  FB_CONTROL_LAW = 44,   /* [n_rows][5][nv] physics real: the law's coefficient block, rows bias, act_gain, pos_gain, pos_ref, vel_gain
                            (fb_batch_device_ptr only: torch rewrites gains between steps without a host copy) */
  FB_TIME = 45,          /* [n_env] FP64 at either precision: the episode clock (MuJoCo's d->time) -- 0 at a reset, + opt_timestep per substep.  It picks
                            the reference frame of the reward and ends the episode at the time limit; setting it moves an episode in front of such a
                            boundary (the step counter FB_STEP_COUNT is not moved with it) */
  FB_NFIELD
};

enum { FB_MAXCON = 64, FB_MAXEFC = 192, FB_NSENSOR = 33 };
/* FB_WARN bits: more than FB_MAXCON contacts (the rest were dropped); more than FB_MAXEFC constraint rows (contacts beyond
 * the cap were dropped); the constraint solver stopped at opt.iterations; a convex-pair penetration query (MPR) hit its
 * iteration limit */
enum { FB_WARN_CONTACT_CAP = 1, FB_WARN_EFC_CAP = 2, FB_WARN_SOLVER_MAXITER = 4, FB_WARN_CCD_MAXITER = 8,
       FB_WARN_SOLVER_FALLBACK = 32 /* (rounds 3-4: the model selects Newton but the system had more than 64 rows and block PGS ran instead.  Never raised
                                       since round 5: the engine runs Newton at every system size, like MuJoCo -- fb_newton.hpp: d_newton_wide.  The bit
                                       stays defined so that FB_WARN words keep their layout.) */,
       FB_WARN_SCHED_WAIT = 16 /* substep scheduler: the wait for an environment's previous substep hit its iteration cap (never observed).
                                  The environment's control step was ABANDONED (its row is not stepped concurrently with its holder);
                                  fb_batch_synchronize / fb_batch_get fail from then on until the batch is destroyed. */,
       FB_WARN_MODEL_ID = 64 /* grouped batch: the environment's FB_ENV_MODEL entry was outside [0, n_models) when the kernel picked the
                                environment up (only possible through the device pointer); it was clamped into range for that launch. */ };

/* model dimensions by name: "nq","nv","nu","na","nbody","nobs","nsubstep", ... ; -1 if unknown.
   Also the build's constraint-matrix placement: "lds_ar_rows_f64" / "lds_ar_rows_f32" (largest system whose Delassus matrix lives in the
   LDS matrix slot) and "lds_wide_rows_f64" / "lds_wide_rows_f32" (largest system solved from LDS at all; at most 64). */
int fb_model_dim(const fb_model* m, const char* name);

/* Load a compiled-model blob (flybody_amd/model_blob.py: "FBM1"). */
int fb_model_load(const void* blob, size_t nbytes, fb_model** out);
void fb_model_destroy(fb_model* m);

/* Create n_env environments on HIP device `device`.  precision is 64 (FP64 physics) or
 * 32 (FP32 physics).  Fails (never falls back to a CPU path) if no GPU is present. */
int fb_batch_create(const fb_model* m, int n_env, int device, int precision, fb_batch** out);
void fb_batch_destroy(fb_batch* b);

/* Reference trajectory shared by all environments (host pointers, FP64), as produced by the
 * reference's trajectory loaders (tasks/trajectory_loaders.py:267-309):
 * ref_qpos[T][7] root position+quaternion, ref_qvel[T][6].  Mirrors
 * `env.task._traj_generator.set_next_trajectory` (tests/test_walking_env.py:43-44) plus the
 * walk_imitation() kwargs future_steps / terminal_com_dist / time_limit (fly_envs.py:100-155). */
int fb_batch_set_reference(fb_batch* b, const double* ref_qpos, const double* ref_qvel, int T,
                           int future_steps, double terminal_com_dist, double time_limit);

/* walk_on_ball (fly_envs.py:158-191): no reference trajectory; only the episode time limit is configurable
 * (2 s in the reference).  Replaces fb_batch_set_reference for that task. */
int fb_batch_set_time_limit(fb_batch* b, double time_limit);

/* flight_imitation only: wing-beat pattern generator tables (flybody/tasks/pattern_generators.py:17-129 builds them;
 * flybody_amd/wbpg.py restates it).  traj[rows][6], phase[rows], offset[nfreq+1] (row range of each frequency's
 * sequence), freqs[nfreq]; rate = exp(-dt_ctrl / ctrl_filter); seed keys the per-episode initial phase. */
int fb_batch_set_wbpg(fb_batch* b, const double* traj, const double* phase, const int32_t* offset, const double* freqs,
                      int nfreq, double base_freq, double rel_range, double rate, uint32_t seed);

/* walk_imitation TRAINING mode (fly_envs.walk_imitation(ref_path=...), tasks/walk_imitation.py:57-67,92-177): the whole
 * reference dataset (tasks/trajectory_loaders.py:185-264) is uploaded once, row-concatenated; every environment picks a
 * snippet at episode start on the GPU (a pure function of seed, global env id and episode number -- the reference uses
 * RandomState.choice) and is rewarded with the DeepMimic factors of tasks/rewards.py:84-116 x (20,1,1,1) and the
 * wing-retraction tolerance.  Replaces fb_batch_set_reference for that mode.  Host pointers, FP64. */
typedef struct fb_walk_dataset {
  int32_t n_traj, n_joints, n_sites, n_select;
  const int32_t* traj_offset;     /* [n_traj + 1] first row of each trajectory */
  const double* qpos;             /* [rows][7 + n_joints]  root pose + mocap joint angles */
  const double* qvel;             /* [rows][6 + n_joints] */
  const double* root2site;        /* [rows][n_sites][3] */
  const double* joint_quat;       /* [rows][n_joints][4] */
  const int32_t* joint_ids;       /* [n_joints] model joint ids of the mocap joints */
  const int32_t* site_ids;        /* [n_sites] model site ids */
  const int32_t* select;          /* [n_select] trajectory ids to sample from (traj_indices) */
  int32_t future_steps; double terminal_com_dist, time_limit; uint32_t seed; int32_t env_id_base;
} fb_walk_dataset;
int fb_batch_set_walk_dataset(fb_batch* b, const fb_walk_dataset* ds);

/* flight_imitation with a reference dataset (fly_envs.flight_imitation(ref_path=...), tasks/trajectory_loaders.py:67-141,
 * tasks/flight_imitation.py:82-110): every trajectory of the dataset, row-concatenated and already converted from the
 * dataset's CoM track to the root joint (task_utils.com2root); per episode every environment picks a trajectory out of
 * `select` and -- with randomize_start_step -- a start row in [0, len - 50) on the GPU (pure functions of seed, global env
 * id and episode number; the reference uses RandomState.choice / randint), re-centres x / y on the first row of the slice
 * and tracks it.  Replaces fb_batch_set_reference for that mode; fb_batch_set_wbpg is still required.  Host pointers, FP64. */
typedef struct fb_flight_dataset {
  int32_t n_traj, n_select;
  const int32_t* traj_offset;     /* [n_traj + 1] first row of each trajectory */
  const double* qpos;             /* [rows][7] ROOT position + quaternion */
  const double* qvel;             /* [rows][6] */
  const int32_t* select;          /* [n_select] trajectory ids to sample from (traj_indices) */
  int32_t future_steps, randomize_start_step; double terminal_com_dist, time_limit; uint32_t seed; int32_t env_id_base;
} fb_flight_dataset;
int fb_batch_set_flight_dataset(fb_batch* b, const fb_flight_dataset* ds);

/* env.reset() for the listed environments (env_ids == NULL: all).  `stream` is a hipStream_t
 * (NULL = default stream).  Asynchronous. */
int fb_batch_reset(fb_batch* b, const int32_t* env_ids, int n, void* stream);

/* env.step(action) for every environment: `action` is a DEVICE pointer to float32
 * [n_env][nact] in the reference's action order (fruitfly.py:342-379); nact = nu + user actions
 * (59 for walk_imitation, 12 for flight_imitation; fb_model_dim(m, "nact")).  Environments whose
 * previous step returned LAST are reset instead (dm_env auto-reset convention).
 * Asynchronous on `stream`; results land in FB_OBS/FB_REWARD/FB_DISCOUNT/FB_STEP_TYPE. */
int fb_batch_step(fb_batch* b, const float* action, void* stream);

/* Debug / parity entry points: run one physics substep (mj_step2 then mj_step1 order, as
 * dm_control's legacy step does) with the current FB_CTRL, or only re-evaluate the
 * position/velocity stage at the current state. */
int fb_batch_substep(fb_batch* b, int nsub, void* stream);
int fb_batch_forward(fb_batch* b, void* stream);
/* Profiling entry point: ONE stage of a control step for every environment, so that per-dispatch hardware counters (rocprofv3
 * --pmc) can be attributed to stages.  stage_word = stage id | damp << 8 | half << 9 | part mask << 12 (fb_step.hpp: ST_*,
 * MODE_STAGE); the caller walks the stage sequence of a control step itself (tools/stage_profile.py), `action` is only read by
 * the first stage (the task's before_step hook).  Same results as fb_batch_step while no environment ends its episode. */
int fb_batch_stage(fb_batch* b, int stage_word, const float* action, void* stream);
/* Profiling entry point: the raw workspace row of ONE environment (which = 0: the physics-real arena row, 1: the int32 arena row), copied
 * to (write = 0) or from (write = 1) host memory after a device synchronisation.  bytes = 0 with a non-null `row_bytes` only reports the
 * row size.  The layout is internal (fb_types.hpp: FB_WS_REAL / FB_WS_INT); tools/footprint.py uses this to measure which cache lines of a
 * row a substep reads and writes.  Not a parity or product interface. */
int fb_batch_row(fb_batch* b, int which, int env, void* host, size_t bytes, int write, size_t* row_bytes);

/* Synchronous host copies (physics-real fields are converted to/from FP64; FB_OBS/REWARD/
 * DISCOUNT are float32, the int fields int32).  `bytes` must match exactly. */
int fb_batch_get(fb_batch* b, int field, void* dst_host, size_t bytes);
int fb_batch_set(fb_batch* b, int field, const void* src_host, size_t bytes);

/* Device pointer of a field (e.g. to wrap FB_OBS in a torch tensor without a copy): FB_OBS, FB_REWARD, FB_DISCOUNT, FB_STEP_TYPE, and the
 * applied-force arrays FB_QFRC_APPLIED / FB_XFRC_APPLIED at the batch's precision (allocating them: see fb_batch_clear_forces), and FB_ENV_MODEL of a
 * grouped batch, FB_QFRC_LAW and FB_CONTROL_LAW while a control law is set.  FB_QPOS and FB_QVEL (physics real) point into the batch's
 * arena: environment e's row starts e x row_bytes further on, row_bytes as fb_batch_row(b, 0, ...) reports it -- for rewards and
 * terminations computed on the device (fb_batch_end_episode); writing there between steps is fb_batch_set without its checks.
 * NULL otherwise. */
void* fb_batch_device_ptr(fb_batch* b, int field);
int fb_batch_synchronize(fb_batch* b, void* stream);

/* Average duration (ms) of the last `fb_batch_step` launches, measured with HIP events on the
 * launch stream between fb_batch_timing_begin / fb_batch_timing_end. */
int fb_batch_timing_begin(fb_batch* b, void* stream);
int fb_batch_timing_end(fb_batch* b, void* stream, float* total_ms, int* n_launches);
/* Duration (ms) of EVERY fb_batch_step kernel of the last timed region (HIP events around each launch, up to 2048 of them): returns
 * how many were written to ms[0 .. cap).  Call after fb_batch_timing_end.  bench.py reports their min / median / p90 / max, so that a
 * single long control step (one environment with a very large constraint system ends the launch) shows in a 20-step window. */
int fb_batch_timing_launches(fb_batch* b, float* ms, int cap);

/* How fb_batch_step schedules a control step of this batch: 1 = substep scheduler (the batch exceeds the GPU's resident wave slots:
 * waves draw (environment, substep) tickets per XCD until the step is complete), 0 = one environment per wave, longest first.
 * Scheduling only: results are identical.  `slots` (may be NULL) receives the number of resident environments of this build. */
int fb_batch_scheduler(const fb_batch* b, int* slots);
/* fb_batch_step validates every stream ONCE (a probe kernel checks that the stream reaches every XCD: a CU-masked stream would leave ticket
 * queues undrawn) and remembers the handle.  Call this before destroying a stream the batch was stepped on: a later stream that reuses the
 * handle is then probed again.  (NULL / unknown streams: no-op.) */
int fb_batch_forget_stream(fb_batch* b, void* stream);

/* Synthetic random actions for throughput rollouts (per-environment RNG = Philox(seed, stream = env id)):
 * fills the DEVICE array action[n_env][nact] (float32) for control step `step`.  One Philox4x32-10 stream per GLOBAL environment id
 * -- env_ids[e] (device pointer) or env_id_base + e when env_ids is NULL -- so an environment is fed the same actions whatever the
 * number of ranks its batch is sharded over (the reference steps one independent environment per actor process,
 * agents/ray_distributed_dmpo.py:232).  dist 0: N(0,1) clipped to [-1, 1]; dist 1: U(-1, 1).  Asynchronous on `stream`. */
int fb_random_actions(float* action, const int32_t* env_ids, int n_env, int nact, uint64_t seed, int step, int env_id_base, int dist, void* stream);

/* Multi-site inverse kinematics, the reference's qpos_from_site_xpos (flybody/inverse_kinematics.py) for every environment at once:
 * momentum gradient descent of |site_xpos - target|^2 (over the included components) + reg_strength |hinge qpos|^2 over the dofs of
 * the listed joints, up to max_steps iterations, stopping a frame when lr |update| / err < progress_threshold (checked every 100 steps).
 * Environment e fits target_xpos[e] (HOST pointer, FP64 [n_env][n_site][3]) starting from its FB_QPOS, and leaves the result there (the
 * reference's inplace=True); the position-stage outputs (FB_XPOS, FB_SITE_XPOS, ...) are left consistent with it, nothing else of the
 * environment changes.  Results per environment in FB_IK_ERR / FB_IK_STEPS.  FP64 batches only.  Validates every argument (ids in range
 * and unique, n_site >= 1, finite hyper-parameters, max_steps >= 1, no NaN target, include entries 0 / 1).  Asynchronous on `stream`
 * after the (blocking) upload of the targets. */
typedef struct fb_ik_config {
  int32_t n_site, n_joint;
  const int32_t* site_ids;        /* [n_site] model site ids */
  const int32_t* joint_ids;       /* [n_joint] model joint ids (expanded to their dofs) */
  const int32_t* include;         /* [3 n_site] 1: the component of target_xpos enters the objective (the reference's include_inds), 0: ignored */
  double reg_strength, lr, beta, progress_threshold;
  int32_t max_steps;
} fb_ik_config;
int fb_batch_ik(fb_batch* b, const fb_ik_config* cfg, const double* target_xpos, void* stream);

/* Inverse dynamics, MuJoCo's mj_inverse for every environment at once (FP64 batches only): from the environment's FB_QPOS, FB_QVEL and a
 * caller-set FB_QACC,
 *     FB_QFRC_INVERSE = M qacc + qfrc_bias - qfrc_passive - qfrc_constraint
 * with M including armature, qfrc_passive = springs, dampers and the fluid forces, and qfrc_constraint = J' f(J qacc - aref), f the
 * soft-constraint primal map (no solver runs).  Per-contact forces in FB_CONTACT_FORCE; FB_EFC_FORCE and FB_QFRC_CONSTRAINT hold the
 * inverse's values afterwards, and the position / velocity stage outputs (FB_XPOS, FB_CONTACT, FB_QM, FB_QFRC_BIAS, ...) are refreshed
 * from qpos / qvel as fb_batch_forward refreshes them.  FB_QACC is read, not written; nothing a later control step reads changes.
 * Noslip is not inverted (neither does mj_inverse): for a model with noslip_iterations > 0 (fruitfly.xml sets 3) the inverse of a
 * forward pass's qacc differs from its qfrc_actuator by what the noslip passes changed.
 * flags: FB_INV_DISCRETE (MuJoCo's mjENBL_INVDISCRETE for the engine's semi-implicit Euler with implicit joint damping): FB_QACC is
 * read as (qvel+ - qvel) / h and converted to M^-1 (M + h D) qacc first.  Fails on an FP32 batch, unknown flags and a non-finite
 * FB_QACC (checked on the host: the call synchronises the device before it launches).  Asynchronous on `stream` after that. */
enum { FB_INV_DISCRETE = 1 };
int fb_batch_inverse(fb_batch* b, int flags, void* stream);

/* Transition derivatives, MuJoCo's mjd_transitionFD for the engine's step (FP64 batches only; csrc/fb_deriv.hpp): the
 * finite-difference Jacobians of n_substeps physics substeps with ctrl held,
 *     A = dx'/dx [ndx][ndx]   B = dx'/du [ndx][nu]   C = ds'/dx [33][ndx]   D = ds'/du [33][nu]      per frame, row-major, FP64,
 * in caller-provided DEVICE buffers [n_frames][..][..].  x = (qpos, qvel, act), u = ctrl, s = FB_SENSORDATA as the last substep leaves it
 * (the engine's legacy-step timing: acceleration-stage sensors lag one substep).  The tangent is dx = (dq[nv], dv[nv], dact[na]),
 * ndx = 2 nv + na, with dq in the joints' velocity space (mj_integratePos / mj_differentiatePos: free-joint translation, free- and
 * ball-joint rotation as a local 3-vector, hinge angle).
 * Frame k is environment env_ids[k] (k when env_ids is NULL) as it stands: its FB_QPOS / FB_QVEL / FB_ACT / FB_CTRL, and its warm start
 * w = the acceleration its next solve would start from (after fb_batch_forward: that pass's FB_QACC).  The transition recomputes the
 * position and velocity stages from the (perturbed) state -- no cached stage output is trusted --, then runs the substeps in the step's
 * own order (actuation .. acceleration sensors, Euler with implicit damping, position + velocity stages of the new state; noslip
 * included).  The first substep's constraint solve warm-starts from w, the SAME w for every perturbation (as MuJoCo saves and restores
 * qacc_warmstart); later substeps from their predecessor.  No task hook runs: no action mapping, reward, termination, auto-reset or
 * pattern generator -- the transition is a function of (qpos, qvel, act, ctrl, w) only.
 * Columns: j < nv: qpos integrated by +-eps e_j; j < 2 nv: qvel[j - nv] +- eps; j < ndx: act +- eps; beyond: ctrl +- eps.  centered = 1:
 * diff(T(x-), T(x+)) / (2 eps); 0: diff(T(x), T(x+)) / eps; diff is differentiatePos on the qpos rows, subtraction elsewhere.  The
 * actuation stage clamps ctrl to ctrlrange, so a ctrl nudge that would leave the range is not taken: a centred column becomes one-sided
 * on the side that stays inside, a forward column nudges backwards, and if neither side fits the column is zero (MuJoCo's rule).
 * A NULL output is skipped: with A and C NULL no state column is run, with B and D NULL no ctrl column; with C and D NULL the position
 * and velocity stages behind the last integration are skipped too.  status (optional, DEVICE, int32 [n_frames]) receives the OR of the
 * FB_WARN_* bits any of the frame's transitions raised (contact / row caps, the solver's iteration limit, ...): a derivative through a
 * capped solve is not a derivative.
 * Nothing a later control step reads changes: the environments' rows are only read; state, caches, warm start, FB_WARN*, FB_SIZE_STATS
 * and FB_STEP_TICKS stay as they were.  The work runs on scratch rows the batch owns (allocated on the first call: one workspace row per
 * resident wave slot -- fb_batch_scheduler's `slots` -- never frames x columns; pool_rows uses fewer) and through a staging buffer of at
 * most 256 MB: more frames than fit are processed in chunks.  Results do not depend on pool_rows or on scheduling: two calls give the
 * same bits.
 * Refused, with the reason in fb_last_error(): an FP32 batch; a grouped batch of more than one model; a batch with a control law set or
 * with applied forces allocated (as fb_batch_stage refuses them); null batch or config; all four outputs NULL; eps not finite or <= 0;
 * n_substeps < 1; n_frames < 1; centered other than 0 / 1; an environment id out of range; pool_rows out of range.
 * Asynchronous on `stream` after validation, ordered like any other launch on that stream.
 * fb_batch_fd_tickets: the number of transitions (nominal + perturbed) the last call ran; synchronises the device (a debug counter). */
typedef struct fb_fd_config {
  double eps;                 /* > 0, finite; MuJoCo's default use is 1e-6 */
  int32_t centered;           /* 0 forward, 1 centred */
  int32_t n_substeps;         /* >= 1: derivative of n physics substeps with ctrl held (1 = mjd_transitionFD) */
  int32_t n_frames;           /* >= 1 */
  const int32_t* env_ids;     /* HOST [n_frames]: the environments linearised; NULL: 0 .. n_frames-1 */
  int32_t pool_rows;          /* 0: the resident slots; otherwise 1 .. resident slots */
} fb_fd_config;
int fb_batch_transition_fd(fb_batch* b, const fb_fd_config* cfg, double* A, double* B, double* C, double* D, int32_t* status, void* stream);
int fb_batch_fd_tickets(fb_batch* b, int64_t* n);

/* Open-loop rollouts (MuJoCo's rollout module for the engine's step): what happens if this input sequence is applied from here?
 * Rollout r starts from environment env_ids[r] (r when env_ids is NULL) as it stands and runs `horizon` control intervals of n_substeps
 * physics substeps each, the interval's input held over its substeps.  Exactly one kind of input is given, a DEVICE buffer:
 *     ctrl   FP64 [n_roll][horizon][nu]     copied to FB_CTRL of the rollout; the actuation stage clamps it to ctrlrange as it clamps FB_CTRL;
 *     action FP32 [n_roll][horizon][nact]   handed to the task's before_step hook, the one fb_batch_step runs: action scatter, NaN -> 0,
 *                                           and for the flight task the wing-beat pattern generator's step and the wing commands.
 * Outputs, caller-provided DEVICE buffers written directly (no staging): state [n_roll][horizon][nq + nv + na] = (qpos', qvel', act')
 * after every interval; sensordata (optional) [n_roll][horizon][33] = FB_SENSORDATA as the interval's last substep leaves it (the
 * engine's legacy-step timing: acceleration-stage sensors lag one substep); status (optional) int32 [n_roll] = the OR of the FB_WARN_*
 * bits the rollout raised (contact / row caps, the solver's iteration limit, ...).
 * What is copied: the head of the source environment's row -- FB_QPOS, FB_QVEL, FB_ACT, FB_CTRL, the warm start, the simulation time and
 * the pattern generator's filtered frequency -- and, for an action rollout, the pattern generator's table position.  What is recomputed:
 * everything else; the position and velocity stages of the copied state run first and no cached stage output is trusted (the mid-phase
 * neighbour list included).  Then the substeps run in the step's own order (actuation .. acceleration sensors, Euler with implicit
 * damping, position + velocity stages of the new state; noslip included); with sensordata NULL the position and velocity stages behind
 * the very last integration are skipped.  Warm start: the first constraint solve starts from the acceleration the environment's next
 * solve would start from, every later solve from its predecessor.  No other hook runs: no reward, termination, auto-reset, dataset or
 * ghost logic -- a rollout from an environment whose step type is LAST continues its physics, it does not reset.  A ctrl rollout equals
 * fb_batch_set(FB_CTRL) + fb_batch_substep(n_substeps) per interval on a copy of the environment, an action rollout equals
 * fb_batch_step on one (while that copy does not reach LAST), bit for bit.
 * Nothing a later control step reads changes: the environments' rows are only read; state, caches, warm start, FB_WARN*, FB_SIZE_STATS
 * and FB_STEP_TICKS stay as they were.  The work runs on the scratch rows fb_batch_transition_fd uses too (allocated on the first call of
 * either: one workspace row per resident wave slot, never one per rollout; pool_rows uses fewer); a wave takes one rollout after the
 * other.  Results do not depend on pool_rows or on which wave drew which rollout: two calls give the same bits.  The two users of the
 * rows are ordered only when they are on one stream: concurrent fb_batch_transition_fd / fb_batch_rollout calls on the same batch from
 * different streams are the caller's to order.
 * Refused, with the reason in fb_last_error(): an FP32 batch; a grouped batch of more than one model; a batch with a control law set or
 * with applied forces allocated; null batch, config or state; both or neither of ctrl and action; n_roll < 1; horizon < 1;
 * n_substeps < 0; an environment id out of range (env_ids NULL with n_roll > n_env included); pool_rows out of range; an action rollout
 * of the flight task before fb_batch_set_wbpg.
 * Asynchronous on `stream` after validation, ordered like any other launch on that stream; after the first call nothing synchronises and
 * the only upload is env_ids.
 * fb_batch_rollouts_run: the number of rollouts the last call finished; synchronises the device (a debug counter). */
typedef struct fb_rollout_config {
  int32_t n_roll;             /* >= 1 */
  int32_t horizon;            /* T >= 1 control intervals */
  int32_t n_substeps;         /* >= 1 physics substeps per interval, input held; 0: the model's own (fb_model_dim "nsubstep") */
  const int32_t* env_ids;     /* HOST [n_roll]: source environment of every rollout, repeats allowed (K samples of one state); NULL: r */
  int32_t pool_rows;          /* 0: all scratch rows; otherwise 1 .. that many */
} fb_rollout_config;
int fb_batch_rollout(fb_batch* b, const fb_rollout_config* cfg, const double* ctrl, const float* action,
                     double* state, double* sensordata, int32_t* status, void* stream);
int fb_batch_rollouts_run(fb_batch* b, int64_t* n);

/* Closed-loop rollouts: fb_batch_rollout with the input of interval t computed on the device from the state the rollout has reached,
 *     dx  = x_t (-) x_nom[nom][t]
 *     u_i = clamp( u_nom[nom][t][i] + (alpha[r]*k[nom][t][i] + sum_j K[nom][t][i][j]*dx[j]) )
 * -- LQR tracking, the forward pass and line search of iLQR, the stability test of a gain.  nom = nom_ids[r] is the rollout's nominal
 * trajectory; many rollouts may share one.  x = (qpos, qvel, act); dx lives in fb_batch_transition_fd's tangent space (dq[nv], dv[nv],
 * dact[na]; ndx = 2 nv + na): subtraction for hinge and slide joints and free-joint translation, the local rotation vector that takes
 * the nominal quaternion to the state's for free- and ball-joint rotation.  x_nom[nom][t] is the nominal state at the START of interval
 * t; x_0 is the source environment's state as it stands.  clamp: to ctrlrange where the actuator is ctrllimited, the clamp the actuation
 * stage applies, which therefore leaves u as it is.  u is held over the interval's n_substeps substeps and written to ctrl_out.
 * LAYOUT OF K: the C-ABI takes the gains TRANSPOSED, K[n_nom][horizon][ndx][nu] (entry [j][i] multiplies dx[j] into u_i), the layout
 * the kernel streams; a caller with [nu][ndx] matrices transposes them once on its stream (the Python shim does).  The sum runs over
 * j = 0 .. ndx-1 in ascending order, one accumulator per output: two calls, and any pool_rows, give the same bits.
 * Everything else is fb_batch_rollout's: fb_rollout_config unchanged, what is copied and recomputed, the records state / sensordata /
 * status, the scratch rows, the sources only read, fb_batch_rollouts_run.  With K and k NULL (or zero), or alpha = 0 and K zero, the
 * result has the bits of fb_batch_rollout(ctrl = u_nom); feeding ctrl_out back to fb_batch_rollout reproduces state and sensordata bit
 * for bit.  Feedback is on ctrl only: an action-space law (the flight task's pattern generator in the loop) is not offered.
 * Refused, with the reason in fb_last_error(): everything fb_batch_rollout refuses (an input is not asked for), and: null fbk, x_nom or
 * u_nom; n_nom < 1; a nominal id out of range; nom_ids NULL with n_nom != n_roll; a model whose ndx exceeds the kernel's 384 dx registers.
 * Asynchronous on `stream` after validation; after the first call nothing synchronises and the only upload is env_ids / nom_ids. */
typedef struct fb_feedback {
  int32_t n_nom;            /* >= 1 nominal trajectories */
  const int32_t* nom_ids;   /* HOST [n_roll], 0 .. n_nom-1: the nominal of every rollout (many rollouts may share one); NULL: r, and n_nom == n_roll */
  const double* x_nom;      /* DEVICE [n_nom][horizon][nq+nv+na]: state at the START of interval t */
  const double* u_nom;      /* DEVICE [n_nom][horizon][nu] */
  const double* K;          /* DEVICE [n_nom][horizon][ndx][nu]: TRANSPOSED (above); NULL: zero */
  const double* k;          /* DEVICE [n_nom][horizon][nu], NULL: zero */
  const double* alpha;      /* DEVICE [n_roll], NULL: 1 -- the step length of a line search */
} fb_feedback;
int fb_batch_rollout_feedback(fb_batch* b, const fb_rollout_config* cfg, const fb_feedback* fbk,
                              double* state, double* sensordata, double* ctrl_out, int32_t* status, void* stream);

/* The backward pass of LQR / iLQR for n_nom independent nominals, on the device: from the transition derivatives of
 * fb_batch_transition_fd to the gains fb_batch_rollout_feedback streams, without a trip to the host.  Conventions: no 1/2 in the cost,
 * u = u_nom + K dx, linear model dx_{t+1} = A_t dx_t + B_t du_t.  For the cost
 *     J = sum_t ( dx'Q dx + du'R du + 2 q_t'dx + 2 r_t'du ) + dx_T'Qf dx_T + 2 q_T'dx_T
 * and the value V_t = dx'P_t dx + 2 p_t'dx + const, from P_T = Qf, p_T = q_T and for t = T-1 .. 0:
 *     W   = P_{t+1} A_t                 Y   = P_{t+1} B_t
 *     Qxx = Q + A_t'W                   Qux = B_t'W               Quu = R + B_t'Y
 *     Qx  = q_t + A_t'p_{t+1}           Qu  = r_t + B_t'p_{t+1}
 *     Quu_reg = Quu + mu[m] I           (Cholesky)
 *     K_t = -Quu_reg^-1 Qux             k_t = -Quu_reg^-1 Qu
 *     P_t = sym( Qxx + K'Quu K + K'Qux + Qux'K )          -- the general form: runs when mu is given (whatever its values)
 *     P_t = sym( Qxx + Qux'K )                            -- the short form, equal to it when Quu_reg = Quu: runs when mu is NULL
 *     p_t = Qx + K'(Quu k + Qu) + Qux'k                   -- always this form
 *     dV[m] += ( 2 k'Qu , k'Quu k )     (the predicted change of J for step length alpha is alpha dV[0] + alpha^2 dV[1])
 * With mu, q and r NULL this is the time-varying LQR recursion, K = -(R + B'PB)^-1 B'PA.
 * LAYOUT (all arrays DEVICE, contiguous doubles, row-major matrices):
 *     A  [n_nom][horizon][ndx][ndx]   B  [n_nom][horizon][ndx][nu]   Q, Qf [ndx][ndx]   R [nu][nu]   (one each for the call; Qf NULL: Q)
 *     q  [n_nom][horizon+1][ndx]      r  [n_nom][horizon][nu]        mu [n_nom]         (optional: NULL is zero)
 *     Kt [n_nom][horizon][ndx][nu]    -- K_t TRANSPOSED, the layout fb_feedback.K takes: the two calls hand over without a copy
 *     k  [n_nom][horizon][nu]         P  [n_nom][horizon+1][ndx][ndx]   p [n_nom][horizon+1][ndx]   dV [n_nom][2]   status [n_nom]
 * STATIONARY MODE (stationary = 1), the batched fixed-point iteration of infinite-horizon LQR: A [n_nom][ndx][ndx] and B [n_nom][ndx][nu]
 * serve every t, the recursion runs `horizon` times and only the outputs of t = 0 are kept: Kt [n_nom][1][ndx][nu], k [n_nom][1][nu],
 * P [n_nom][2][ndx][ndx] = (P_0, P_1) -- max |P_0 - P_1| tells convergence --, p [n_nom][2][ndx] likewise; q is [n_nom][2][ndx] (the
 * running q, then q_T) and r [n_nom][1][nu].
 * FAILURE IS DATA: when a pivot of the Cholesky of Quu_reg is <= 0 or not finite, nothing faults and no NaN is written: status[m] = 1 + t
 * of the first such interval, that nominal's Kt, k, P, p are zero for all intervals <= t and dV[m] = 0; every other nominal is unaffected.
 * status[m] = 0 otherwise.
 * The batch supplies the device, the stream convention and ownership of the workspace only: the call reads no environment and works on
 * any batch (FP32, grouped, with forces or a control law).  ndx and nu are the caller's.  WORKSPACE, a block of the batch that grows on
 * demand (ordered on the device when it does) and is freed with it: 3 ndx^2 + 3 ndx nu + nu^2 + 2 ndx doubles per nominal -- three
 * ndx x ndx buffers whose roles rotate (P_{t+1}; W, then P_t; the sum under sym), Y, Qux, Quu K + Qux, Quu, p twice: 2.2 MB for the
 * walking fly (ndx 275, nu 59).  The Cholesky factor lives in LDS.
 * Refused, with the reason in fb_last_error(): null batch, cfg, A, B, Q, R, Kt or status; n_nom, horizon, ndx or nu < 1; ndx > 1024;
 * nu > 64 (the factor's rows in LDS and a lane's right-hand side in registers); stationary not 0 or 1.
 * Asynchronous on `stream` after validation; with the shapes of the call before: no allocation, no upload, no synchronisation.  Sums run
 * in a fixed order: two calls give the same bits, and a nominal's bits do not depend on the others in the call. */
typedef struct fb_lqr_config {
  int32_t n_nom, horizon, ndx, nu;   /* ndx, nu are the caller's: the call does not read the model */
  int32_t stationary;                /* 0 / 1 (above) */
} fb_lqr_config;
int fb_batch_lqr_backward(fb_batch* b, const fb_lqr_config* cfg,
                          const double* A, const double* B,
                          const double* Q, const double* R, const double* Qf,
                          const double* q, const double* r, const double* mu,
                          double* Kt, double* k, double* P, double* p,
                          double* dV, int32_t* status, void* stream);
/* The product kernel of the call above on its own, for tests of its tile map and edges: C [m][n] = op(X) op(Y) (+ D [m][n]; NULL: none),
 * X stored [m][k] (trans_x: [k][m]), Y stored [k][n] (trans_y: [n][k]); all DEVICE, row-major doubles; m, n, k in 1 .. 4096. */
int fb_riccati_gemm(fb_batch* b, int m, int n, int k, int trans_x, int trans_y,
                    const double* X, const double* Y, const double* D, double* C, void* stream);

/* Batched ray casting: MuJoCo's mj_ray / mj_multiRay and the rangefinder sensor, for n_ray rays in each of n_frames frames.  A frame is
 * a live environment (env_ids); the rays meet the model's geoms where the last control step, reset or fb_batch_forward left them
 * (FB_GEOM_XPOS / FB_GEOM_XMAT) and, optionally, a caller-supplied height field.  The environments are only read: nothing a later step
 * reads changes.
 * A RAY is (origin[3], dir[3]); dir need not be unit length.  The result is the smallest x >= 0 with origin + x dir on the boundary of a
 * visible object -- mj_ray's convention, distance in units of |dir| -- so an origin INSIDE a closed geom reports the exit point.  A miss
 * is dist = -1, geomid = -1.  A hit with x > cutoff is a miss (cutoff > 0 in the same units; +inf or 0: none).  A zero or non-finite ray
 * is a miss, and so is one whose |dir|^2 underflows or overflows at the batch's precision or whose distance does not fit float32.  With body >= 0 the rays are given in that body's frame (FB_XPOS / FB_XQUAT of the frame's environment), else in the world's.
 * GEOMS.  Plane: hit only from its front (the direction's local z < 0), and only where the hit point lies within +-size[0], +-size[1]
 * wherever that size is > 0 (the fly's floor is 8 x 8, finite).  Sphere, ellipsoid: the quadratic in the geom's frame.  Capsule: the
 * cylinder side between the cap centres plus the two half spheres.  Cylinder: the side plus the two discs.
 * VISIBILITY.  geom_mask: optional bytes [ngeom], 0 hides the geom.  bodyexclude: -1, or a body whose geoms are skipped.
 * TERRAIN, as MuJoCo's hfield asset: nrow x ncol float32 samples in [0, 1], row <-> y, column <-> x; size = (rx, ry, elevation_z, base_z)
 * and a world position pos (no rotation).  Sample (r, c) sits at x = -rx + 2 rx c / (ncol - 1), y = -ry + 2 ry r / (nrow - 1) with height
 * elevation_z * data[r][c]; every cell is split into the triangles (v00, v11, v10) and (v00, v11, v01): the diagonal joins (r, c) to
 * (r + 1, c + 1).  The terrain is the SOLID {|x| <= rx, |y| <= ry, -base_z <= z <= h(x, y)}; the ray reports the first crossing of its
 * boundary -- surface, side walls or bottom -- and from inside the exit.  A terrain hit has geomid = ngeom.  There may be n_terrain grids
 * of one shape, with a terrain index per frame (terrain_ids): per-episode terrain without a re-upload.  Between geoms and terrain the
 * nearest hit wins.  Samples outside [0, 1] are the caller's error: results are then wrong, nothing faults.
 * Both precisions: the arithmetic runs at the batch's.  Works with applied forces or a control law set (it only reads poses).
 * Refused, with the reason in fb_last_error(): a null batch, cfg, rays, dist or geomid; a grouped batch of more than one model; n_frames or
 * n_ray < 1, or more than 2^23 workgroups of 1024 rays; per_frame not 0 or 1; an environment id, body, bodyexclude or terrain id out of
 * range; a terrain with null data, nrow or ncol outside 2 .. 4096, n_terrain < 1, rx or ry not > 0, elevation_z or base_z < 0, or a
 * non-finite size or pos; a negative or NaN cutoff.
 * Asynchronous on `stream` after validation; the only uploads are the small host arrays (env_ids, terrain_ids, the visible geoms), into
 * ONE block of the batch that every call rewrites: the calls on one batch must be stream-ordered (one stream, or events between them),
 * as those of fb_batch_transition_fd and fb_batch_rollout must. */
typedef struct fb_terrain {
  int32_t nrow, ncol, n_terrain;          /* nrow, ncol in 2 .. 4096 */
  double size[4], pos[3];
  const float* data;                      /* DEVICE [n_terrain][nrow][ncol] */
  const int32_t* terrain_ids;             /* HOST [n_frames], NULL: 0 */
} fb_terrain;
typedef struct fb_ray_config {
  int32_t n_frames, n_ray;
  int32_t per_frame;                      /* 0: rays [n_ray][6], shared by the frames; 1: rays [n_frames][n_ray][6] */
  const int32_t* env_ids;                 /* HOST [n_frames], NULL: 0 .. n_frames-1; repeats allowed */
  int32_t body;                           /* -1: world frame; else the rays are given in this body's frame */
  int32_t bodyexclude;                    /* -1, or the body whose geoms are invisible */
  const uint8_t* geom_mask;               /* HOST [ngeom] or NULL */
  double cutoff;
} fb_ray_config;
int fb_batch_ray(fb_batch* b, const fb_ray_config* cfg, const double* rays /* DEVICE */,
                 const fb_terrain* terrain /* NULL: none */,
                 float* dist /* DEVICE [n_frames][n_ray] */,
                 int32_t* geomid /* DEVICE [n_frames][n_ray] */, void* stream);

/* External forces (FB_QFRC_APPLIED, FB_XFRC_APPLIED), MuJoCo's two user inputs for everything that is not an actuator, a contact or the
 * fluid model.  Every substep
 *     qfrc_smooth = qfrc_passive - qfrc_bias + qfrc_actuator + qfrc_applied + sum_b J_b(xipos_b)' xfrc_applied_b
 * with J_b at that substep's positions (mj_xfrcAccumulate); xfrc_applied also enters cfrc_ext, so the force sensors read what
 * mj_rnePostConstraint gives (qfrc_applied does not); the accelerometer reads qacc, which holds the effect.
 * Who reads them: the substeps of fb_batch_step and fb_batch_substep, and fb_batch_forward.  The forward pass of a reset does NOT
 * (fb_batch_reset, and the auto-reset of an environment whose last step was LAST): MuJoCo's reset clears the arrays, so a FIRST
 * observation is the same with and without forces.  fb_batch_inverse needs nothing: its FB_QFRC_INVERSE of a forward pass's qacc equals
 * qfrc_actuator + qfrc_applied + J' xfrc_applied.
 * Ownership, and the difference from MuJoCo: the arrays are caller-owned inputs like the actions.  They persist until the caller changes
 * them, the kernels never write them, and NOTHING clears them on a reset -- an environment that auto-resets keeps its row; clearing is the
 * caller's job (fly_envs.BatchedFlyEnv.reset() does it for the host-side reset).
 * Allocation: both arrays are allocated, zeroed, by the first fb_batch_set or fb_batch_device_ptr of either field (fb_batch_get before
 * that fails).  From then on control steps, substeps and forward evaluations run a second step kernel that carries the applied-force
 * stage (k_step_forces; with all-zero forces its results equal the plain kernel's, up to the sign of a zero); fb_batch_clear_forces frees
 * the arrays and returns the batch to the plain kernel, whose code and speed the feature does not touch.  While forces are allocated
 * fb_batch_stage (single-stage profiling) fails.  fb_batch_set rejects a wrong size and non-finite values; non-finite values written
 * through the device pointer end the environment's episode through the blow-up guard, as a NaN action does.
 * Both precisions.  fb_batch_forces_active: 1 while the arrays are allocated, 0 otherwise. */
int fb_batch_clear_forces(fb_batch* b);
int fb_batch_forces_active(const fb_batch* b);

/* Substep control laws.  A law is five rows per dof, evaluated by the step kernel in EVERY physics substep of fb_batch_step and
 * fb_batch_substep, and in fb_batch_forward:
 *     u[i] = bias[i] + act_gain[i]*qfrc_actuator[i] - pos_gain[i]*(qpos[adr(i)] - pos_ref[i]) - vel_gain[i]*qvel[i]
 *     qfrc_smooth = qfrc_passive - qfrc_bias + qfrc_actuator + u + qfrc_applied + J' xfrc_applied
 * adr(i) is the qpos address of dof i's hinge.  It is what MuJoCo's mjcb_control does when it writes qfrc_applied from the state, for the
 * laws that are diagonal in the dofs: joint springs and dampers, motor noise, assistive torques.
 * qfrc_actuator is THIS substep's actuator force.  MuJoCo runs the callback before it computes the actuator forces, so a callback that
 * reads qfrc_actuator sees the previous substep's; the current one is used here because "act_gain = g" then means exactly "every motor
 * is (1 + g) times as strong", which can be checked against a model whose gains, biases and force ranges are scaled.
 * Rows: n_rows = 1 (one law for the batch) or n_env (one per environment), each row [nv] FP64, converted to the batch's precision; a
 * null row is zeros; all values must be finite; pos_gain must be zero on every dof that is not a hinge's (free root, ball joints): the
 * call fails naming the dof.  u of the last substep is readable as FB_QFRC_LAW; the forward pass of a reset (fb_batch_reset and the
 * auto-reset) skips the law, as it skips the applied forces, and leaves FB_QFRC_LAW zero.  FB_QFRC_ACTUATOR stays the actuators' own.
 * Setting a law allocates the applied-force arrays as their first access does, and the batch is stepped by a third step kernel
 * (k_step_law: the forces kernel plus the law stage; an all-zero law gives the forces kernel's results).  fb_batch_set_control_law(b, NULL)
 * clears the law and returns the batch to the kernel it had: the forces kernel if the caller touched the force arrays, the plain one
 * otherwise.  Refused: a grouped batch (give every model a batch of its own); fb_batch_stage, fb_batch_ik and fb_batch_inverse while a law
 * is set (clear it first); fb_batch_clear_forces while a law is set.  The coefficient block on the device is FB_CONTROL_LAW
 * (fb_batch_device_ptr); values written there are not validated -- a non-finite one ends the episode through the blow-up guard.
 * fb_batch_control_law_active: 1 while a law is set. */
typedef struct { const double *bias, *act_gain, *pos_gain, *pos_ref, *vel_gain; int n_rows; } fb_control_law;
int fb_batch_set_control_law(fb_batch* b, const fb_control_law* law);
int fb_batch_control_law_active(const fb_batch* b);

/* Ends episodes from the device, for rewards and terminations computed outside the kernel (e.g. in PyTorch).  One thread per
 * environment, asynchronous on `stream`: where mask_dev[e] != 0 and the environment's last step type is MID, FB_STEP_TYPE becomes LAST,
 * FB_DISCOUNT becomes discount_dev[e] (0 when discount_dev is NULL) and the next fb_batch_step auto-resets the environment, exactly as
 * after a LAST the step kernel decided.  Environments that are FIRST or already LAST are left as the kernel left them.  mask_dev:
 * [n_env] bytes, discount_dev: [n_env] float32, both device pointers.  Every task. */
int fb_batch_end_episode(fb_batch* b, const uint8_t* mask_dev, const float* discount_dev, void* stream);

/* Per-environment physics models in one batch (domain randomisation).  fb_batch_create_group creates n_env environments that share ONE
 * tree and differ in real-valued constants: environment e is stepped with models[FB_ENV_MODEL[e]].  The models must be compatible with
 * models[0]: the same arrays with the same shapes, every integer array equal (topology, types, ids, iteration counts, solver, task and
 * action layout), opt_timestep and opt_control_timestep equal.  Every other real array may differ (masses, inertias, frames, sizes,
 * qpos0, springs, ranges, damping, armature, gains, biases, pair_*, geom_fluid, gravity, density, viscosity, solref / solimp,
 * invweights, stat_meaninertia); what the host derives from real constants (neighbour-list slack, bounding boxes, fluid geoms, total
 * mass) is derived per model.  A violation fails with fb_last_error() naming the first array that differs.  At most FB_MAX_MODELS models;
 * n_models == 1 steps like fb_batch_create (the plain kernels).  The batch keeps the model pointers: destroy the models after the batch.
 * FB_ENV_MODEL is initialised to e % n_models and is available through fb_batch_get / fb_batch_set (ids outside [0, n_models) are
 * rejected) / fb_batch_device_ptr.  The kernels read it when they pick the environment up: once per launch, or once per ticket of the
 * substep scheduler.  A change is supported AT AN EPISODE BOUNDARY ONLY: before fb_batch_reset of the environment, or while its step type
 * is LAST, so that the auto-reset of the next fb_batch_step runs under the new model (the forward pass of a reset recomputes every cached
 * stage).  Changing it mid-episode is unsupported: the first substep would use the old model's position stage.  An id written out of
 * range through the device pointer is clamped by the kernel and raises FB_WARN_MODEL_ID.
 * The setters (fb_batch_set_reference, _time_limit, _wbpg, both datasets) apply to every model of the group.  fb_batch_step, _substep,
 * _forward and _reset work at both precisions, under both schedulers and together with applied forces; fb_batch_ik, fb_batch_inverse
 * and fb_batch_stage fail on a batch of more than one model (they never silently use model 0). */
enum { FB_MAX_MODELS = 256 };
int fb_batch_create_group(const fb_model* const* models, int n_models, int n_env, int device, int precision, fb_batch** out);
int fb_batch_n_models(const fb_batch* b);

const char* fb_last_error(void);

/* Build identity of the shared object: "flybody_engine <abi> (<target>, <hash of the kernel sources it was built from>)".
 * smoke() and the GPU tests print it and compare the hash with the sources in the tree, so a log shows which binary ran. */
const char* fb_version(void);

#ifdef __cplusplus
}
#endif
#endif
