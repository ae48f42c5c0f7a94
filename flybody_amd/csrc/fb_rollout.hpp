// Batched open-loop rollouts: MuJoCo's `rollout` for the engine's step, on the device.  Rollout r starts from the state of a source
// environment as it stands and applies T control intervals of n physics substeps each; the input of interval t is either a ctrl row
// (copied to w.ctrl(), clamped by the actuation stage as FB_CTRL is) or an action row handed to the task's before_step hook s_pre --
// the hook fb_batch_step runs: action scatter, NaN -> 0, flight's pattern-generator step and wing commands.  No other hook runs: no
// s_post, reward, termination, auto-reset, dataset or ghost logic; a rollout from an environment at LAST continues its physics.
// DESIGN.md 20.
//
// Work unit: a TICKET = one rollout, drawn onto the pool of scratch rows (fb_side.hpp: the pool, tickets, the row's preparation, the
// frame the kernel runs in; never one row per rollout).  For each ticket the wave
//   * prepares its row from the rollout's source environment; for an action rollout the two pattern-generator words of the int row
//     follow the source's, because s_pre reads them;
//   * runs the position and velocity stages of the copied state once, then per interval: the input, n substeps (side_substep and the
//     position + velocity stages of the new state), and the record [r][t] = (qpos', qvel', act') -- and sensordata as the interval's
//     last substep leaves it -- straight into the caller's buffers.  The first constraint solve warm-starts from the source row's
//     qacc_ws, every later one from its predecessor.
// status[r] = the OR of the FB_WARN_* bits the rollout raised, one plain store at its end.  Which wave drew which rollout does not
// enter: two calls give the same bits, with any number of rows.  FP64 only.
//
// CLOSED-LOOP rollouts (k_closedloop_rollout): a kernel of its own next to k_rollout -- not a mode of it, for fb_side.hpp's reason:
// a run-time switch would move k_rollout's code -- that differs in one thing, the interval's input.  Tickets, rows, LDS layout, launch
// bounds, stage sequence, priorities, records and status are rollout_kernel's, stated once; the template argument FEEDBACK selects the
// input at compile time.  At the start of interval t the wave evaluates a time-varying affine feedback on the row's own state:
//     dx  = x_t (-) xnom[nom][t]                     the tangent space of fb_side.hpp (dq[nv], dv[nv], dact[na]; side_qpos_diff)
//     u_i = clamp( unom[nom][t][i] + (alpha[r]*k[nom][t][i] + sum_j K[nom][t][i][j]*dx[j]) )
// clamp = clampr to act_ctrlrange where act_ctrllimited: s_actuation's own function and condition, so the stage's clamp is the identity on
// it.  u goes to w.ctrl() and to the optional record [r][t][nu].  Mapping: lane == output i (blocks of 64 for nu > 64); dx lives in
// REGISTERS, element j in slot j/64 of lane j%64 (FeedbackArgs::DXSLOTS slots; the host refuses a model with more), and is broadcast by
// v_readlane; the gains are read TRANSPOSED, Kt[nom][t][j][i], so that the lanes of one j read consecutive doubles and the j rows
// follow one another (one stream of ndx*nu doubles per interval; rollouts of one nominal share it through L2).  The sum runs over
// j = 0 .. ndx-1 in ascending order in ONE accumulator per output, from 0: fixed by the code, the same bits for any pool and any call.
// No LDS beyond the step kernel's layout.  Feedback is on ctrl only: an action-space law (the pattern generator in the loop) is not offered.
#pragma once
#include "fb_side.hpp"

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

#define FB_FBK_BLOCK 16      // gain rows a wave has in flight at once (s_feedback)

// k_closedloop_rollout's own arguments: everything else is RolloutArgs (ctrl and action null)
template <typename real>
struct FeedbackArgs {
  static constexpr int DXSLOTS = 6;             // dx registers per lane: ndx <= 64*DXSLOTS (2*FB_MAXNV + na; the fly: 275)
  const int* roll_nom;                          // [n_roll] nominal of every rollout
  const real* x_nom;                            // [n_nom][horizon][nq + nv + na]: the state at the START of interval t
  const real* u_nom;                            // [n_nom][horizon][nu]
  const real* Kt;                               // [n_nom][horizon][ndx][nu]: the gains, transposed; null: zero
  const real* k;                                // [n_nom][horizon][nu], null: zero
  const real* alpha;                            // [n_roll], null: 1
  real* ctrl_out;                               // [n_roll][horizon][nu] the inputs applied, or null
};

// The input of one interval under the feedback law (above): a stage of its own, not inlined, like the stages around it -- its registers
// (dx, the gain loads in flight) are allocated apart from the kernel's, whose frame stays k_rollout's.  xn, un, Kt (null: zero), kt (null:
// zero): the interval's rows of the rollout's nominal; out (null: none): its row of the ctrl record.  All 64 lanes call.
template <typename real> FB_STAGE_C void s_feedback(const DevModel<real>& M_, const WS<real>& w_, const real* xn_, const real* un_, const real* Kt_, const real* kt_,
                                                    real al, real* out_, int lane) {
  const DevModel<real>& M = as_constant(M_); const WS<real> w = ws_uniform(w_, M);
  const real *xn = uniform_p(xn_), *un = uniform_p(un_), *Kt = uniform_p(Kt_), *kt = uniform_p(kt_); real* out = uniform_p(out_);
  constexpr int NS = FeedbackArgs<real>::DXSLOTS;
  const int nv = M.nv, na = M.na, nq = M.nq, nu = M.nu, ndx = 2*nv + na;
  SYNC();
  real dx[NS];
#pragma unroll
  for (int m = 0; m < NS; m++) {
    const int c = lane + FB_WAVE*m;
    real v = 0;
    if (c < nv) v = side_qpos_diff(M, c, (const real*)w.qpos(), xn);
    else if (c < 2*nv) v = w.qvel()[c - nv] - xn[nq + c - nv];
    else if (c < ndx) v = w.act()[c - 2*nv] - xn[nq + nv + c - 2*nv];
    dx[m] = v;
  }
  for (int i0 = 0; i0 < nu; i0 += FB_WAVE) {
    const int i = i0 + lane;
    const bool on = i < nu;
    real s = 0;
    if (Kt) {
#pragma unroll
      for (int m = 0; m < NS; m++) {
        // blocks of FB_FBK_BLOCK rows with a constant trip count: the broadcast is a convergent operation, so the compiler does not
        // unroll a loop around it whose trip count it does not know, and one load per trip leaves the wave waiting for memory ndx
        // times per interval.  A block loads its rows together (rows behind ndx: not read, their dx is zero) and adds them in order.
        const real* Km = Kt + (size_t)FB_WAVE*m*nu + i;
        for (int q = 0; q < FB_WAVE/FB_FBK_BLOCK; q++) {
          const int j0 = uniform_int(FB_WAVE*m + FB_FBK_BLOCK*q);
          if (j0 >= ndx) break;
          real g[FB_FBK_BLOCK];
#pragma unroll
          for (int e = 0; e < FB_FBK_BLOCK; e++) g[e] = (on && j0 + e < ndx) ? Km[(size_t)(FB_FBK_BLOCK*q + e)*nu] : (real)0;
#pragma unroll
          for (int e = 0; e < FB_FBK_BLOCK; e++) s += g[e]*rdlane(dx[m], FB_FBK_BLOCK*q + e);
        }
      }
    }
    if (on) {
      real u = un[i] + (al*(kt ? kt[i] : (real)0) + s);
      if (M.act_ctrllimited[i]) u = clampr(u, M.act_ctrlrange[2*i], M.act_ctrlrange[2*i + 1]);
      w.ctrl()[i] = u;
      if (out) out[i] = u;
    }
  }
  SYNC();
}

template <typename real, bool FEEDBACK>
__device__ __forceinline__ void rollout_kernel(const DevModel<real>* Mp, const RolloutArgs<real>& A, const FeedbackArgs<real>& F) {
  constexpr int EPB = LdsCfg<real>::EPB;
  __shared__ real s_pool[EPB][LdsCfg<real>::POOL];
  __shared__ LdsTab s_tab;
  const DevModel<real>& M = as_constant(*Mp);
  const int tid = threadIdx.x;
  side_stage_tables(M, s_tab, tid);
  const int wave = uniform_int(tid / FB_WAVE), lane = tid % FB_WAVE;
  const int row = uniform_int(blockIdx.x*EPB + wave);
  if (row >= A.nwave) return;
  // the wave's scratch row: an environment row like any other, in the pool's arenas
  const WS<real> w = ws_env(M, A.pool_r, A.pool_i, row, s_pool, wave, &s_tab);
  const WS<real> wc = w;
  const int nv = M.nv, na = M.na, nq = M.nq, nu = M.nu, nx = nq + nv + na;
  const int total = uniform_int(A.n_roll), T = uniform_int(A.horizon), nsub = uniform_int(A.n_substeps);
  const bool by_action = uniform_int(A.action ? 1 : 0) != 0, want_sens = uniform_int(A.sens ? 1 : 0) != 0;
  for (int guard = 0; guard < (1 << 30); guard++) {
    const int r = side_draw_ticket(A.counter, lane);
    if (r >= total) return;
    const int env = uniform_int(A.roll_env[r]);
    int nom = 0;
    real al = 1;
    if constexpr (FEEDBACK) { nom = uniform_int(F.roll_nom[r]); if (F.alpha) al = F.alpha[r]; }
    const real* src = A.rarena + (size_t)env*M.off.nreal;
    const int* isrc = A.iarena + (size_t)env*M.off.nint + M.off.istate;
    side_prepare_row(M, w, src, isrc, by_action, lane);
    side_position_velocity(M, wc, lane);
    for (int t = 0; t < T; t++) {
      const size_t rec = (size_t)r*T + t;
      // ---- the interval's input
      if constexpr (FEEDBACK) {
        const size_t nt = (size_t)nom*T + t;
        s_feedback(M, wc, F.x_nom + nt*nx, F.u_nom + nt*nu, F.Kt ? F.Kt + nt*(2*nv + na)*nu : nullptr, F.k ? F.k + nt*nu : nullptr, al,
                   F.ctrl_out ? F.ctrl_out + rec*nu : nullptr, lane);
      }
      else if (by_action) s_pre(M, wc, A.action + rec*M.nact, lane);
      else {
        const real* u = A.ctrl + rec*nu;
        for (int i = lane; i < nu; i += FB_WAVE) w.ctrl()[i] = u[i];
        SYNC();
      }
      // ---- n x (mj_step2, Euler, mj_step1)
      for (int s = 0; s < nsub; s++) {
        side_substep(M, wc, lane);
        if (s == nsub - 1 && t == T - 1 && !want_sens) break;      // no sensor output wanted: x' is complete behind the Euler stage, and nothing follows
        side_position(M, wc, lane);
        // tail-aware issue priority, as in d_run: with a rollout per row the launch ends with its slowest rollout, and every wave is
        // resident from the start; each wave counts itself into the substep's counter, and the more were there before it, the higher its
        // priority for the next substep
        const int prio = uniform_int(s_velocity(M, wc, false, A.sched ? A.sched + (t*nsub + s) : (int*)nullptr, A.nwave, lane));
        if (prio >= 0) FB_SETPRIO(prio);
      }
      SYNC();
      // ---- the record [r][t], straight to the caller's buffers
      side_store_state(M, w, A.state + rec*nx, lane);
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
  rollout_kernel<real, false>(Mp, A, FeedbackArgs<real>());
}

template <typename real>
__global__ void __launch_bounds__(FB_WAVE*LdsCfg<real>::EPB, LdsCfg<real>::WAVES_PER_SIMD) k_closedloop_rollout(const DevModel<real>* Mp, RolloutArgs<real> A, FeedbackArgs<real> F) {
  rollout_kernel<real, true>(Mp, A, F);
}
