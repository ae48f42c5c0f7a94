// Batched transition derivatives: MuJoCo's mjd_transitionFD for the engine's step, by finite differences on the device.
//     A = dx'/dx   B = dx'/du   C = ds'/dx   D = ds'/du        x = (qpos, qvel, act), u = ctrl, s = sensordata
// in the tangent space dx = (dq[nv], dv[nv], dact[na]): dq lives in the joints' velocity space (mj_integratePos / mj_differentiatePos:
// free-joint translation, free- and ball-joint rotation as a local 3-vector, hinge angle).  DESIGN.md 18.
//
// Transition T_n(x, u; w): the position and velocity stages of the (perturbed) state are recomputed -- nothing cached in the source row
// is trusted -- then n physics substeps run in the step's own order (fb_step.hpp: actuation .. acceleration sensors, Euler with implicit
// damping, position + velocity stages of the new state; noslip included).  The constraint solver of the first substep warm-starts from
// w = the source row's qacc_ws, the SAME w for every perturbation (MuJoCo saves and restores qacc_warmstart); later substeps warm-start
// from their predecessor.  No task hook runs.
//
// Work unit: a TICKET = (frame, column, side), plus one nominal ticket per frame (forward differences divide by it, and so does a centred
// ctrl column that a range limit made one-sided), drawn onto the pool of scratch rows (fb_side.hpp: the pool, tickets, the row's
// preparation, the frame the kernel runs in; never frames x columns rows).  For each ticket the wave prepares its row from the frame's
// environment, perturbs one coordinate (below), runs the transition and writes the raw (qpos', qvel', act', sensordata) to the ticket's
// staging slot.  k_fd_assemble, one wave per output column, then forms the quotients in the tangent space.  Which wave drew which ticket
// does not enter: two calls give the same bits.
//
// Columns: j < nv: qpos integrated by +-eps e_j; j < 2 nv: qvel; j < ndx = 2 nv + na: act; beyond: ctrl.  Centred: diff(T(x-), T(x+)) / 2 eps,
// forward: diff(T(x), T(x+)) / eps; diff = differentiatePos on the qpos rows, subtraction elsewhere.  The actuation stage clamps ctrl to
// ctrlrange, so a ctrl nudge that would leave the range is not taken (MuJoCo's rule): a centred column becomes one-sided on the side that
// fits, a forward column nudges backwards, and with neither side the column is zero.  fd_ctrl_sides() states the rule once for both kernels.
// FP64 only.
#pragma once
#include "fb_side.hpp"

// Staging memory of one fb_batch_transition_fd call: the host processes the frames in chunks whose tickets fit this budget
// (walk_imitation: 669 tickets x 309 doubles = 1.65 MB per centred frame; 4096 frames at once would be 6.8 GB).
#ifndef FB_FD_STAGING_BYTES
#define FB_FD_STAGING_BYTES (256u << 20)
#endif

template <typename real>
struct FdArgs {
  const real* rarena; const int* iarena;        // the batch's environments: read only
  real* pool_r; int* pool_i;                    // scratch rows [nwave]
  const int* frame_env;                         // [n_frames] source environment of every frame of this chunk
  real* stage;                                  // [n_frames][per_frame][nstage] raw ticket outputs
  int* counter;                                 // [0] next ticket (zeroed before the launch), [1] tickets run since the call began
  int* status;                                  // [n_frames] OR of the FB_WARN_* bits of the frame's tickets (null: not wanted)
  real *A, *B, *C, *D;                          // outputs of this chunk's frames (null: skipped)
  real eps;
  int n_frames, c0, c1, centered, n_substeps, skip_tail, nwave;
  // per frame: ticket 0 = nominal, then (centered ? 2 : 1) tickets per column c0 .. c1-1: slot 0 = the plus side, slot 1 = the minus side
  __device__ __forceinline__ int sides() const { return centered ? 2 : 1; }
  __device__ __forceinline__ int per_frame() const { return 1 + sides()*(c1 - c0); }
};

template <typename real>
__device__ __forceinline__ int fd_nstage(const DevModel<real>& M) { return M.nq + M.nv + M.na + FB_NSENS; }

// The sides of a ctrl column that are taken (MuJoCo's mjd_stepFD): a nudge must stay inside ctrlrange.  Returns bit 0: ticket slot 0 runs,
// bit 1: slot 1 runs; sgn0: the sign of slot 0's nudge (a forward difference whose plus side does not fit nudges backwards in slot 0).
template <typename real>
__device__ __forceinline__ int fd_ctrl_sides(const DevModel<real>& M, int i, real ctrl, real eps, bool centered, int& sgn0) {
  const bool limited = M.act_ctrllimited[i] != 0;
  const real lo = M.act_ctrlrange[2*i], hi = M.act_ctrlrange[2*i + 1];
  const bool in = ctrl >= lo && ctrl <= hi;
  const bool fwd = !limited || (in && ctrl + eps <= hi), back = !limited || (in && ctrl - eps >= lo);
  sgn0 = 1;
  if (centered) return (fwd ? 1 : 0) | (back ? 2 : 0);
  if (fwd) return 1;
  if (back) { sgn0 = -1; return 1; }
  return 0;
}

template <typename real>
__device__ __forceinline__ void transition_fd_kernel(const DevModel<real>* Mp, const FdArgs<real>& A) {
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
  const int nv = M.nv, na = M.na, nq = M.nq, ndx = 2*nv + na;
  const int per_frame = uniform_int(A.per_frame()), total = uniform_int(A.n_frames*per_frame), nst = fd_nstage(M);
  for (int guard = 0; guard < (1 << 30); guard++) {
    const int t = side_draw_ticket(A.counter, lane);
    if (t >= total) return;
    const int f = t / per_frame, k = t - f*per_frame;
    const int env = uniform_int(A.frame_env[f]);
    const real* src = A.rarena + (size_t)env*M.off.nreal;
    // ---- which coordinate, which way
    int col = -1; real d = 0;
    if (k > 0) {
      const int slot = (k - 1) % A.sides();
      col = A.c0 + (k - 1)/A.sides();
      int sgn = slot ? -1 : 1;
      if (col >= ndx) {
        int sgn0;
        const int run = fd_ctrl_sides(M, col - ndx, src[M.off.ctrl + col - ndx], A.eps, A.centered != 0, sgn0);
        if (!((run >> slot) & 1)) continue;               // the nudge would leave ctrlrange: not taken, k_fd_assemble does not read the slot
        if (slot == 0) sgn = sgn0;
      }
      d = sgn*A.eps;
    }
    side_prepare_row(M, w, src, (const int*)nullptr, false, lane);
    // ---- perturb
    if (lane == 0 && col >= 0) {
      if (col < nv) {
        const int j = M.dof_jntid[col], jt = M.jnt_type[j], qa = M.jnt_qposadr[j], kk = col - M.jnt_dofadr[j];
        real* q = w.qpos();
        if (jt == JNT_FREE) { if (kk < 3) q[qa + kk] += d; else fd_rotate_quat(q + qa + 3, kk - 3, d); }
        else if (jt == JNT_BALL) fd_rotate_quat(q + qa, kk, d);
        else q[qa] += d;
      }
      else if (col < 2*nv) w.qvel()[col - nv] += d;
      else if (col < ndx) w.act()[col - 2*nv] += d;
      else w.ctrl()[col - ndx] += d;
    }
    SYNC();
    // ---- the transition: mj_step1 of the state, then n x (mj_step2, Euler, mj_step1)
    side_position_velocity(M, wc, lane);
    const int nsub = uniform_int(A.n_substeps);
    for (int s = 0; s < nsub; s++) {
      side_substep(M, wc, lane);
      if (s == nsub - 1 && A.skip_tail) break;           // no sensor output wanted: x' is complete behind the Euler stage
      side_position_velocity(M, wc, lane);
    }
    SYNC();
    // ---- raw results to the ticket's staging slot
    real* out = A.stage + (size_t)t*nst;
    side_store_state(M, w, out, lane);
    if (lane < FB_NSENS) out[nq + nv + na + lane] = w.sens()[lane];
    if (lane == 0) {
      const int wbits = w.istate()[IS_WARN];
      if (wbits && A.status) atomicOr(A.status + f, wbits);
      atomicAdd(A.counter + 1, 1);
    }
    SYNC();
  }
}

template <typename real>
__global__ void __launch_bounds__(FB_WAVE*LdsCfg<real>::EPB, LdsCfg<real>::WAVES_PER_SIMD) k_transition_fd(const DevModel<real>* Mp, FdArgs<real> A) {
  transition_fd_kernel<real>(Mp, A);
}

// One wave per (frame, column): the quotient of the column's two staged states in the tangent space, lane == output row.
template <typename real>
__global__ void __launch_bounds__(FB_WAVE) k_fd_assemble(const DevModel<real>* Mp, FdArgs<real> A) {
  const DevModel<real>& M = *Mp;
  const int nv = M.nv, na = M.na, nq = M.nq, nu = M.nu, ndx = 2*nv + na, nst = fd_nstage(M);
  const int ncol = A.c1 - A.c0, f = blockIdx.x / ncol, col = A.c0 + blockIdx.x % ncol, lane = threadIdx.x;
  if (f >= A.n_frames) return;
  const int per_frame = A.per_frame();
  const size_t t0 = (size_t)f*per_frame, tp = t0 + 1 + (size_t)(col - A.c0)*A.sides();
  const real* nom = A.stage + t0*nst;
  const real* s0 = A.stage + tp*nst;                    // slot 0: the plus side (or a forward column's backward nudge)
  const real* s1 = A.stage + (tp + 1)*nst;              // slot 1: the minus side (centred only)
  const real *xa = nullptr, *xb = nullptr; real h = A.eps;
  if (col < ndx) {
    if (A.centered) { xa = s1; xb = s0; h = 2*A.eps; } else { xa = nom; xb = s0; }
  } else {
    int sgn0;
    const int env = A.frame_env[f];
    const int run = fd_ctrl_sides(M, col - ndx, A.rarena[(size_t)env*M.off.nreal + M.off.ctrl + col - ndx], A.eps, A.centered != 0, sgn0);
    if (run == 3) { xa = s1; xb = s0; h = 2*A.eps; }
    else if (run == 1) { if (sgn0 > 0) { xa = nom; xb = s0; } else { xa = s0; xb = nom; } }
    else if (run == 2) { xa = s1; xb = nom; }
  }
  real* X = col < ndx ? A.A : A.B;                      // rows 0 .. ndx-1 of the column
  real* S = col < ndx ? A.C : A.D;                      // rows 0 .. FB_NSENS-1
  const int width = col < ndx ? ndx : nu, cc = col < ndx ? col : col - ndx;
  if (X) {
    real* Xf = X + (size_t)f*ndx*width;
    for (int r = lane; r < ndx; r += FB_WAVE) {
      real v = 0;
      if (xa) {
        if (r < nv) v = side_qpos_diff(M, r, xb, xa);
        else v = xb[nq + r - nv] - xa[nq + r - nv];       // qvel and act follow qpos in a staging slot
        v /= h;
      }
      Xf[(size_t)r*width + cc] = v;
    }
  }
  if (S && lane < FB_NSENS) {
    const int o = nq + nv + na + lane;
    S[((size_t)f*FB_NSENS + lane)*width + cc] = xa ? (xb[o] - xa[o])/h : (real)0;
  }
}
