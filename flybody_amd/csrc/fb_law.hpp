// Substep control laws: a per-dof feedback law that the step kernel evaluates in EVERY physics substep, where a Python callback
// (fly_envs.BatchedFlyEnv.control_callback) runs once per control step.  A law is five rows per dof,
//     u[i] = bias[i] + act_gain[i]*qfrc_actuator[i] - pos_gain[i]*(qpos[adr(i)] - pos_ref[i]) - vel_gain[i]*qvel[i]
//     qfrc_smooth = qfrc_passive - qfrc_bias + qfrc_actuator + u + qfrc_applied + J' xfrc_applied
// with adr(i) the qpos address of dof i's hinge (pos_gain is zero on every other dof: the setter refuses anything else), either one set
// for the batch or one per environment.  u is MuJoCo's mjcb_control writing qfrc_applied from the state: reflex springs and dampers,
// motor noise (act_gain), an assistive torque (bias).
//
// Which actuator force: THIS substep's.  When the stage runs (first thing of ST_ACC_PRE) the solve vector lx holds the qfrc_actuator that
// ST_ACT assembled a moment ago, before the applied forces are added to it.  MuJoCo calls mjcb_control from mj_fwdActuation BEFORE it
// computes the actuator forces, so a callback that reads qfrc_actuator there sees the previous substep's (stated from the library's
// call order, not re-measured here).  The current one was chosen because it gives "act_gain = g" an exact meaning -- every motor's
// force is scaled by 1 + g in the substep it acts in -- and with it an identity against the oracle (gains and force ranges x (1 + g))
// that a test can hold to rounding; the stale variant has no such twin.  DESIGN.md 16.
//
// The coefficients [n_rows][5][nv] (FB_CONTROL_LAW) and the qpos addresses [nv] live in buffers of their own at the batch's precision;
// the stage's u goes to the environment's row of FB_QFRC_LAW [n_env][nv] with one store per lane (read-only for the caller).  The
// forward pass of a reset skips the law, as it skips the applied forces, and zeroes the row.  They reach the device code as one extra
// kernel argument of a third step kernel, k_step_law (fb_engine.hip: FORCES and LAW compiled in); the other kernels keep their code.
#pragma once
#include "fb_smooth.hpp"

enum { LAW_BIAS = 0, LAW_ACT_GAIN = 1, LAW_POS_GAIN = 2, LAW_POS_REF = 3, LAW_VEL_GAIN = 4, LAW_NROW = 5 };

// the kernel argument of k_step_law (null coef: no law)
template <typename real>
struct LawArgs {
  const real* coef;      // [n_rows][LAW_NROW][nv]
  const int* qadr;       // [nv] qpos address of dof i's hinge (0 where the dof is not a hinge's: pos_gain is 0 there)
  real* out;             // [n_env][nv] FB_QFRC_LAW
  int per_env;           // 1: n_rows == n_env, 0: one set for the batch
};

// lx[i] += u[i], FB_QFRC_LAW[i] = u[i]; coef_ / out_ = the environment's block and row.  One lane per dof, two passes for nv = 108; every
// row is read coalesced at clamped indices, then selected (one round of loads per pass).
// `zero` (the forward pass of a reset): no law, the row is zeroed.
template <typename real>
__device__ FB_NOINLINE void s_control_law(const DevModel<real>& M_, const WS<real>& w_, const real* coef_, const int* qadr_, real* out_, bool zero, int lane) {
  const DevModel<real>& M = as_constant(M_); const WS<real> w = ws_uniform(w_, M);
  const FB_GLOBAL real* cf = (const FB_GLOBAL real*)uniform_p(coef_);
  const FB_GLOBAL int* qa = (const FB_GLOBAL int*)uniform_p(qadr_);
  FB_GLOBAL real* out = (FB_GLOBAL real*)uniform_p(out_);
  const int nv = M.nv;
  if (uniform_int(zero ? 1 : 0) != 0) { for (int i = lane; i < nv; i += FB_WAVE) out[i] = 0; return; }
#pragma unroll
  for (int q = 0; q < (FB_MAXNV + FB_WAVE - 1)/FB_WAVE; q++) {
    const int i = lane + q*FB_WAVE; const bool ok = i < nv; const int is = ok ? i : 0;
    const real bias = cf[LAW_BIAS*nv + is], ag = cf[LAW_ACT_GAIN*nv + is], pg = cf[LAW_POS_GAIN*nv + is], pr = cf[LAW_POS_REF*nv + is], vg = cf[LAW_VEL_GAIN*nv + is];
    const int a = qa[is];
    const real fa = w.lx()[is], qv = w.qvel()[is], qp = w.qpos()[a];
    const real u = bias + ag*fa - pg*(qp - pr) - vg*qv;
    if (ok) { w.lx()[i] = fa + u; out[i] = u; }
  }
  SYNC_LDS();
}
