// What the kernels beside k_fly share: k_inverse (fb_inverse.hpp), k_transition_fd / k_fd_assemble (fb_deriv.hpp), k_rollout and
// k_closedloop_rollout (fb_rollout.hpp).  Each runs the step kernel's FB_NOINLINE stage functions (fb_step.hpp) in a sequence of its own
// -- NOT a mode of d_run: that would move every step kernel's code -- on the step kernel's LDS layout (pool + elimination-tree tables,
// EPB rows per workgroup) and under its launch bounds, so the stages are compiled for the same budget and k_fly's code does not change.
// The pieces of that frame are stated here once, all inlined into their callers (no stage function lives here).  k_ik (fb_ik.hpp) has
// a layout of its own and uses none of this.  DESIGN.md 22.
//
// THE SCRATCH POOL.  k_transition_fd and the rollout kernels only read the environments' rows; they run on a pool of scratch rows, one
// real + one int arena row per resident wave, never one per ticket.  A wave owns the row of its index and draws TICKETS (a perturbed
// transition; a rollout) with one atomicAdd on a counter the host zeroes on the stream: no ticket waits for another, there is no spin
// loop.  For each ticket it prepares the row from the ticket's source environment and runs the position and velocity stages of the copy
// first: nothing cached in the source row is trusted, nothing of the row's previous ticket survives, no result depends on who drew what.
#pragma once
#include "fb_step.hpp"

// The workgroup's elimination-tree tables into its LdsTab (declared __shared__ in the kernel's body), then the kernel's only
// workgroup-wide barrier.  This is fly_kernel's staging (fb_engine.hip, the three loops in front of its __syncthreads), which keeps a
// copy of its own: calling this helper from there changed the text of all twelve step and reset kernels, and their ISA is held fixed
// (DESIGN.md 22).  Whoever changes the tables changes both places.
template <typename real>
__device__ __forceinline__ void side_stage_tables(const DevModel<real>& M, LdsTab& s_tab, int tid) {
  constexpr int EPB = LdsCfg<real>::EPB;
  for (int i = tid; i < M.nv; i += FB_WAVE*EPB) {
    s_tab.depth[i] = (uint8_t)M.dof_depth[i]; s_tab.cl[i] = (uint8_t)M.dof_cl[i]; s_tab.gen[i] = (uint8_t)M.dof_gen[i]; s_tab.madr[i] = (uint16_t)M.dof_Madr[i];
  }
  for (int i = tid; i < 2*FB_WAVE; i += FB_WAVE*EPB) s_tab.gen[FB_MAXNV + i] = (uint8_t)M.fac_dof[i];
  for (int i = tid; i < FB_LGEN*FB_MAXCH; i += FB_WAVE*EPB) { s_tab.gk[i] = (uint32_t)M.gen_k[i]; s_tab.gm[2*i] = (uint32_t)M.gen_m[2*i]; s_tab.gm[2*i + 1] = (uint32_t)M.gen_m[2*i + 1]; }
  __syncthreads();
}

// mj_step1 of the row's state: the position stages, then the plain velocity stage (a rollout's substep ends with a counted one of its own).
template <typename real>
__device__ __forceinline__ void side_position(const DevModel<real>& M, const WS<real>& wc, int lane) {
  s_kinematics(M, wc, lane); s_com_pos(M, wc, lane); s_crb(M, wc, lane);
  s_collision(M, wc, lane); s_make_constraint(M, wc, lane);
}
template <typename real>
__device__ __forceinline__ void side_position_velocity(const DevModel<real>& M, const WS<real>& wc, int lane) {
  side_position(M, wc, lane);
  s_velocity(M, wc, false, (int*)nullptr, 0, lane);
}

// One plain physics substep up to the Euler stage (mj_step2, Euler with implicit damping; noslip included).  The order's source is d_run
// (fb_step.hpp): its states ST_ACT, ST_ACC_PRE / ST_FACTOR, ST_ACC_SOLVE / ST_SOLVE, ST_ACC_POST, ST_CONSTR_A (and ST_SOLVE where it
// asks), ST_CONSTR_B, ST_SENS, ST_EULER_PRE / ST_FACTOR, ST_EULER_SOLVE / ST_SOLVE, ST_EULER_POST, for a batch without applied forces
// or control law.  The new state's position and velocity stages (ST_KIN, ST_COLL) follow in the caller.
template <typename real>
__device__ __forceinline__ void side_substep(const DevModel<real>& M, const WS<real>& wc, int lane) {
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
}

// The next ticket of the counter, wave-uniform: lane 0 draws, the wave hears.
__device__ __forceinline__ int side_draw_ticket(int* counter, int lane) {
  int t = 0;
  if (lane == 0) t = atomicAdd(counter, 1);
  return uniform_int(__shfl(t, 0, FB_WAVE));
}

// Prepare the scratch row w for a ticket from its source environment's real row src and istate words isrc.  The head of the real row
// is copied (qpos .. rfac: state, ctrl, warm start, simtime, the pattern generator's filtered frequency -- everything in front of the
// first position-stage output); istate is zeroed -- the mid-phase neighbour list starts invalid (IS_VL_OK = 0), IS_WARN starts clear --
// except that with keep_wb the two task words s_pre reads from the int row (IS_WB_STEP, IS_WB_FREQ: fb_task.hpp, d_flight_pre) follow
// the source's.  Everything behind the head is an output of the stages that run first.
template <typename real>
__device__ __forceinline__ void side_prepare_row(const DevModel<real>& M, const WS<real>& w, const real* src, const int* isrc, bool keep_wb, int lane) {
  const int nhead = (int)M.off.xpos;
#ifdef FB_EMULATE
  for (int i = lane; i < LdsCfg<real>::POOL; i += FB_WAVE) w.lLD[i] = (real)NAN;      // (as on k_fly's ticket path: the LDS pool is not read before it is written)
#endif
  for (int i = lane; i < nhead; i += FB_WAVE) w.rb[i] = src[i];
  for (int i = lane; i < IS_N; i += FB_WAVE) w.istate()[i] = (keep_wb && (i == IS_WB_STEP || i == IS_WB_FREQ)) ? isrc[i] : 0;
  SYNC();
}

// The row's state record (qpos, qvel, act) to out[nq + nv + na]
template <typename real>
__device__ __forceinline__ void side_store_state(const DevModel<real>& M, const WS<real>& w, real* out, int lane) {
  const int nv = M.nv, na = M.na, nq = M.nq;
  for (int i = lane; i < nq; i += FB_WAVE) out[i] = w.qpos()[i];
  for (int i = lane; i < nv; i += FB_WAVE) out[nq + i] = w.qvel()[i];
  for (int i = lane; i < na; i += FB_WAVE) out[nq + nv + i] = w.act()[i];
}

// ---- the tangent space of a state, dx = (dq[nv], dv[nv], dact[na]); dq lives in the joints' velocity space (fb_deriv.hpp)
// q <- q * exp(d e_axis / 2), normalised (mju_quatIntegrate with a unit axis)
template <typename real>
__device__ __forceinline__ void fd_rotate_quat(real* q, int axis, real d) {
  real ax[3] = {0, 0, 0}, qr[4], qq[4] = {q[0], q[1], q[2], q[3]}, res[4];
  ax[axis] = d < 0 ? (real)-1 : (real)1;
  axisangle2quat(qr, ax, d < 0 ? -d : d);
  normquat(qq); mulquat(res, qq, qr); normquat(res);
  for (int k = 0; k < 4; k++) q[k] = res[k];
}

// mju_subQuat: the local 3-vector that takes quaternion qa to qb
template <typename real>
__device__ __forceinline__ void fd_sub_quat(real* res, const real* qb, const real* qa) {
  const real ca[4] = {qa[0], -qa[1], -qa[2], -qa[3]};
  real d[4];
  mulquat(d, ca, qb);
  real ax[3] = {d[1], d[2], d[3]};
  const real s = sqrt(ax[0]*ax[0] + ax[1]*ax[1] + ax[2]*ax[2]);
  real ang = 2*atan2(s, d[0]);
  if (ang > (real)3.14159265358979323846) ang -= 2*(real)3.14159265358979323846;
  const real sc = s > 0 ? ang/s : (real)0;
  for (int k = 0; k < 3; k++) res[k] = ax[k]*sc;
}

// Element c < nv of qb (-) qa: the free joint's rotation and a ball joint by fd_sub_quat, everything else by subtraction.
template <typename real>
__device__ __forceinline__ real side_qpos_diff(const DevModel<real>& M, int c, const real* qb, const real* qa) {
  const int j = M.dof_jntid[c], jt = M.jnt_type[j], adr = M.jnt_qposadr[j], kk = c - M.jnt_dofadr[j];
  if (jt == JNT_FREE && kk >= 3) { real dq[3]; fd_sub_quat(dq, qb + adr + 3, qa + adr + 3); return dq[kk - 3]; }
  if (jt == JNT_BALL) { real dq[3]; fd_sub_quat(dq, qb + adr, qa + adr); return dq[kk]; }
  return qb[adr + kk] - qa[adr + kk];
}
