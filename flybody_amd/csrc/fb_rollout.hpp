// Batched open-loop rollouts: MuJoCo's `rollout` for the engine's step, on the device.  Rollout r starts from the state of a source
// environment as it stands and applies T control intervals of n physics substeps each; the input of interval t is either a ctrl row
// (copied to w.ctrl(), clamped by the actuation stage as FB_CTRL is) or an action row handed to the task's before_step hook s_pre --
// the hook fb_batch_step runs: action scatter, NaN -> 0, flight's pattern-generator step and wing commands.  No other hook runs: no
// s_post, reward, termination, auto-reset, dataset or ghost logic; a rollout from an environment at LAST continues its physics.
// DESIGN.md 20.
//
// Work unit: a TICKET = one rollout.  Waves draw tickets with one atomicAdd on a counter the host zeroes on the stream; no ticket waits
// for another and there is no spin loop.  A wave owns ONE scratch row of the pool fb_batch_transition_fd owns too (fb_deriv.hpp: one
// real + one int arena row per resident wave, never one per rollout); for each ticket it
//   * prepares the row as k_transition_fd does: the head of the source environment's real row (qpos .. rfac: state, ctrl, warm start,
//     simtime, the pattern generator's filtered frequency) is copied, istate is zeroed -- the mid-phase neighbour list starts invalid,
//     IS_WARN starts clear -- and, for an action rollout, the two task words s_pre reads from the int row (IS_WB_STEP, IS_WB_FREQ:
//     fb_task.hpp, d_flight_pre) follow the source's.  Everything behind the head is an output of the position / velocity stages that
//     run first.  The source rows are only read;
//   * runs the position and velocity stages of the copied state once, then per interval: the input, n substeps in d_run's order
//     (actuation .. acceleration sensors, Euler with implicit damping, position + velocity stages of the new state; noslip included),
//     and the record [r][t] = (qpos', qvel', act') -- and sensordata as the interval's last substep leaves it -- straight into the
//     caller's buffers.  The first constraint solve warm-starts from the source row's qacc_ws, every later one from its predecessor.
// status[r] = the OR of the FB_WARN_* bits the rollout raised, one plain store at its end.  Which wave drew which rollout does not
// enter: two calls give the same bits, with any number of rows.
//
// The stage sequence is the kernel's own (NOT a mode of d_run: that would move every step kernel's code).  The kernel runs on the step
// kernel's LDS layout and under its launch bounds, so the FB_NOINLINE stage functions it shares with k_fly and k_transition_fd are
// compiled for the same budget and their code does not change.  FP64 only.
#pragma once
#include "fb_step.hpp"

template <typename real>
struct RolloutArgs {
  const real* rarena; const int* iarena;        // the batch's environments: read only
  real* pool_r; int* pool_i;                    // scratch rows [nwave]
  const int* roll_env;                          // [n_roll] source environment of every rollout
  const real* ctrl;                             // [n_roll][horizon][nu], or null
  const float* action;                          // [n_roll][horizon][nact], or null (exactly one of the two is set)
  real* state;                                  // [n_roll][horizon][nq + nv + na]
  real* sens;                                   // [n_roll][horizon][FB_NSENS], or null
  int* status;                                  // [n_roll], or null
  int* counter;                                 // [0] next ticket (zeroed before the launch), [1] rollouts finished
  int* sched;                                   // [horizon*n_substeps] progress counters, zeroed before the launch (null: more rollouts than rows, no priorities)
  int n_roll, horizon, n_substeps, nwave;
};

template <typename real>
__device__ __forceinline__ void rollout_kernel(const DevModel<real>* Mp, const RolloutArgs<real>& A) {
  constexpr int EPB = LdsCfg<real>::EPB;
  __shared__ real s_pool[EPB][LdsCfg<real>::POOL];
  __shared__ LdsTab s_tab;
  const DevModel<real>& M = as_constant(*Mp);
  const int tid = threadIdx.x;
  // the workgroup's elimination-tree tables, staged as fly_kernel stages them
  for (int i = tid; i < M.nv; i += FB_WAVE*EPB) {
    s_tab.depth[i] = (uint8_t)M.dof_depth[i]; s_tab.cl[i] = (uint8_t)M.dof_cl[i]; s_tab.gen[i] = (uint8_t)M.dof_gen[i]; s_tab.madr[i] = (uint16_t)M.dof_Madr[i];
  }
  for (int i = tid; i < 2*FB_WAVE; i += FB_WAVE*EPB) s_tab.gen[FB_MAXNV + i] = (uint8_t)M.fac_dof[i];
  for (int i = tid; i < FB_LGEN*FB_MAXCH; i += FB_WAVE*EPB) { s_tab.gk[i] = (uint32_t)M.gen_k[i]; s_tab.gm[2*i] = (uint32_t)M.gen_m[2*i]; s_tab.gm[2*i + 1] = (uint32_t)M.gen_m[2*i + 1]; }
  __syncthreads();
  const int wave = uniform_int(tid / FB_WAVE), lane = tid % FB_WAVE;
  const int row = uniform_int(blockIdx.x*EPB + wave);
  if (row >= A.nwave) return;
  // the wave's scratch row: an environment row like any other, in the pool's arenas
  const WS<real> w = ws_env(M, A.pool_r, A.pool_i, row, s_pool, wave, &s_tab);
  const WS<real> wc = w;
  const int nv = M.nv, na = M.na, nq = M.nq, nu = M.nu, nx = nq + nv + na;
  const int nhead = (int)M.off.xpos;            // qpos .. rfac: everything in front of the first position-stage output
  const int total = uniform_int(A.n_roll), T = uniform_int(A.horizon), nsub = uniform_int(A.n_substeps);
  const bool by_action = uniform_int(A.action ? 1 : 0) != 0, want_sens = uniform_int(A.sens ? 1 : 0) != 0;
  for (int guard = 0; guard < (1 << 30); guard++) {
    int r = 0;
    if (lane == 0) r = atomicAdd(A.counter, 1);
    r = uniform_int(__shfl(r, 0, FB_WAVE));
    if (r >= total) return;
    const int env = uniform_int(A.roll_env[r]);
    const real* src = A.rarena + (size_t)env*M.off.nreal;
    const int* isrc = A.iarena + (size_t)env*M.off.nint + M.off.istate;
    // ---- prepare the row: nothing of the row's previous ticket survives
#ifdef FB_EMULATE
    for (int i = lane; i < LdsCfg<real>::POOL; i += FB_WAVE) w.lLD[i] = (real)NAN;      // (as on k_fly's ticket path: the LDS pool is not read before it is written)
#endif
    for (int i = lane; i < nhead; i += FB_WAVE) w.rb[i] = src[i];
    for (int i = lane; i < IS_N; i += FB_WAVE) w.istate()[i] = (by_action && (i == IS_WB_STEP || i == IS_WB_FREQ)) ? isrc[i] : 0;
    SYNC();
    // ---- mj_step1 of the copied state
    s_kinematics(M, wc, lane); s_com_pos(M, wc, lane); s_crb(M, wc, lane);
    s_collision(M, wc, lane); s_make_constraint(M, wc, lane);
    s_velocity(M, wc, false, (int*)nullptr, 0, lane);
    for (int t = 0; t < T; t++) {
      const size_t rec = (size_t)r*T + t;
      // ---- the interval's input
      if (by_action) s_pre(M, wc, A.action + rec*M.nact, lane);
      else {
        const real* u = A.ctrl + rec*nu;
        for (int i = lane; i < nu; i += FB_WAVE) w.ctrl()[i] = u[i];
        SYNC();
      }
      // ---- n x (mj_step2, Euler, mj_step1)
      for (int s = 0; s < nsub; s++) {
        s_actuation(M, wc, lane);
        d_factor(M, wc, false, lane);
        d_solve(M, wc, true, lane);
        s_project_constraint(M, wc, 3, lane);
        const bool need = uniform_int(s_constraint_a(M, wc, lane) ? 1 : 0) != 0;
        if (need) d_solve(M, wc, false, lane);
        s_constraint_b(M, wc, lane);
        s_sensor_acc(M, wc, lane);
        d_factor(M, wc, true, lane);
        d_solve(M, wc, true, lane);
        s_integrate(M, wc, lane);
        if (s == nsub - 1 && t == T - 1 && !want_sens) break;      // no sensor output wanted: x' is complete behind the Euler stage, and nothing follows
        s_kinematics(M, wc, lane); s_com_pos(M, wc, lane); s_crb(M, wc, lane);
        s_collision(M, wc, lane); s_make_constraint(M, wc, lane);
        // tail-aware issue priority, as in d_run: with a rollout per row the launch ends with its slowest rollout, and every wave is
        // resident from the start; each wave counts itself into the substep's counter, and the more were there before it, the higher its
        // priority for the next substep
        const int prio = uniform_int(s_velocity(M, wc, false, A.sched ? A.sched + (t*nsub + s) : (int*)nullptr, A.nwave, lane));
        if (prio >= 0) FB_SETPRIO(prio);
      }
      SYNC();
      // ---- the record [r][t], straight to the caller's buffers
      real* out = A.state + rec*nx;
      for (int i = lane; i < nq; i += FB_WAVE) out[i] = w.qpos()[i];
      for (int i = lane; i < nv; i += FB_WAVE) out[nq + i] = w.qvel()[i];
      for (int i = lane; i < na; i += FB_WAVE) out[nq + nv + i] = w.act()[i];
      if (want_sens && lane < FB_NSENS) A.sens[rec*FB_NSENS + lane] = w.sens()[lane];
    }
    if (lane == 0) {
      if (A.status) A.status[r] = w.istate()[IS_WARN];
      atomicAdd(A.counter + 1, 1);
    }
    SYNC();
  }
}

template <typename real>
__global__ void __launch_bounds__(FB_WAVE*LdsCfg<real>::EPB, LdsCfg<real>::WAVES_PER_SIMD) k_rollout(const DevModel<real>* Mp, RolloutArgs<real> A) {
  rollout_kernel<real>(Mp, A);
}
