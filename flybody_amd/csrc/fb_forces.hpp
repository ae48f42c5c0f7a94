// External forces on the batched step: MuJoCo's two user inputs qfrc_applied (a generalised force per dof) and xfrc_applied (a
// Cartesian wrench per body: force(3) then torque(3), world frame, applied at the body's centre of mass xipos; the world body's row
// is ignored).  Every substep
//     qfrc_smooth = qfrc_passive - qfrc_bias + qfrc_actuator + qfrc_applied + sum_b J_b(xipos_b)' xfrc_b
// with J_b at that substep's positions (mj_xfrcAccumulate), and xfrc_b enters cfrc_ext, so the force sensors read what
// mj_rnePostConstraint would (d_sensor_acc, fb_step.hpp); qfrc_applied does not.
//
// The arrays are caller-owned inputs like the actions: [n_env][nv] and [n_env][nbody][6] at the batch's precision, in buffers of
// their own (not in the arena row), read and never written by the kernels.  They reach the device code as ONE extra kernel argument
// of a second step kernel, k_step_forces (fb_engine.hip): fly_kernel / d_run carry a compile-time flag, k_fly instantiates it false
// and is the code it was; Batch<real> has no new member.  The forward pass of a reset ignores the forces (MuJoCo's reset clears them).
//
// s_applied_forces, the stage behind ST_ACC_PRE, is the scheme of d_passive's fluid wrenches and of k_ik: one lane per body forms the
// wrench of xfrc_b about the tree CoM as [torque; force], subtree_sum_lds<6> sums them up the tree, and dof i gets
// cdof_i . wrench[dof_bodyid[i]] + qfrc_applied[i].  The factor of M is not built yet at that point, so the LDS pool is free: the
// wrenches sit at its start, the solve vector lx (= qfrc_actuator, from ST_ACT) at its end, and the result is added to lx before
// qfrc_smooth is formed from it.  DESIGN.md 14.
#pragma once
#include "fb_smooth.hpp"

// the two arrays of the batch (null: no forces); the kernel argument of k_step_forces
template <typename real>
struct ForceArgs {
  const real* qfrc_applied;     // [n_env][nv]
  const real* xfrc_applied;     // [n_env][nbody][6]
};

// wrench of xfrc_applied[b] about the tree CoM as [torque + (xipos_b - com) x force; force]; xf = the environment's [nbody][6] rows
template <typename real>
FBD void applied_wrench(const DevModel<real>& M, const WS<real>& w, const FB_GLOBAL real* xf, int b, real* out) {
  real f[6], bp[3], bq[4], t[3], xi[3], off[3], tq[3];
#pragma unroll
  for (int k = 0; k < 6; k++) f[k] = xf[6*b + k];
#pragma unroll
  for (int k = 0; k < 3; k++) bp[k] = w.xpos()[3*b + k];
#pragma unroll
  for (int k = 0; k < 4; k++) bq[k] = w.xquat()[4*b + k];
  // xipos from the body frame and the record's body_ipos (the kinematics stage stores xpos / xquat only)
  rotvecquat(t, (const real*)(M.body_rec + b*FB_BODYREC + 11), bq);
  add3(xi, bp, t);
  sub3(off, xi, (const real*)w.com());
  cross3(tq, off, f);
#pragma unroll
  for (int k = 0; k < 3; k++) { out[k] = f[3 + k] + tq[k]; out[3 + k] = f[k]; }
}

// lx[i] += qfrc_applied[i] + cdof_i . (sum of the applied wrenches over the subtree of dof i's body)
template <typename real>
__device__ FB_NOINLINE void s_applied_forces(const DevModel<real>& M_, const WS<real>& w_, const real* qfrc_, const real* xfrc_, int lane) {
  const DevModel<real>& M = as_constant(M_); const WS<real> w = ws_uniform(w_, M);
  const FB_GLOBAL real* qf = (const FB_GLOBAL real*)uniform_p(qfrc_);
  const FB_GLOBAL real* xf = (const FB_GLOBAL real*)uniform_p(xfrc_);
  FB_LDS real* X = w.lLD;                                   // [nbody][6] body wrenches (6 nbody <= FB_LDS_SCRATCH: checked at model load)
#pragma unroll
  for (int q = 0; q < 2; q++) {
    const int b = lane + q*FB_WAVE;
    if (b < M.nbody) {
      real x[6] = {0, 0, 0, 0, 0, 0};
      if (b > 0) applied_wrench(M, w, xf, b, x);
#pragma unroll
      for (int k = 0; k < 6; k++) X[6*b + k] = x[k];
    }
  }
  SYNC_LDS();
  subtree_sum_lds<6>(M, X, lane);
  for (int i = lane; i < M.nv; i += FB_WAVE) {
    const int bd = M.dof_bodyid[i];
    real c[6], x[6];
#pragma unroll
    for (int k = 0; k < 6; k++) { c[k] = w.cdof()[6*i + k]; x[k] = X[6*bd + k]; }
    w.lx()[i] += dot6(c, x) + qf[i];
  }
  SYNC_LDS();
}
