// Batched inverse dynamics: MuJoCo's mj_inverse for the engine's model, one frame per wavefront.  A frame is the batch environment of
// the same index; its qpos, qvel and a user-set qacc (FB_QACC) go in, the generalised force that produces that acceleration comes out:
//     qfrc_inverse = M qacc + qfrc_bias - qfrc_passive - qfrc_constraint,   qfrc_constraint = J' f(J qacc - aref)
// (M with armature; qfrc_passive = springs, dampers and both fluid models, as d_passive computes them; f = the soft-constraint primal map
// of the limit rows, frictionless contacts and elliptic cones -- no solver runs).
//
// The position and velocity stages of a forward pass run unchanged, in the frame every kernel beside k_fly runs in (fb_side.hpp: the step
// kernel's LDS layout and launch bounds, side_stage_tables, side_position_velocity).  Then, new here:
//   * FB_INV_DISCRETE (MuJoCo's mjENBL_INVDISCRETE for semi-implicit Euler with implicit joint damping): qacc is read as
//     (qvel+ - qvel) / h and converted to the continuous acceleration M^-1 (M + h D) qacc = qacc + M^-1 (h D qacc)  (d_factor / d_solve);
//   * M qacc, lane == dof over the sparse qM: dof i's row holds its ancestors (qM[dof_Madr[i] + depth difference]), its column the
//     DFS-contiguous descendants i+1 .. i+ndesc;
//   * jar = J qacc - aref, aref = -B (J qvel) - K imp (pos - margin), as d_constraint_a forms it for qacc_ws;
//   * f(jar): the PGS warm-start block of d_constraint_a, restated (the same zones as the Newton constraint update nw_update) -- it is
//     not factored out of the step kernel so that k_fly's ISA stays as it is;
//   * J' f, lane == dof, rows in order, A side before B side: the summation order of d_constraint_a's one-row-per-lane path;
//   * per-contact forces in the contact frame (normal, tangent 1, tangent 2), zero beyond the contact's condim.
// Noslip is NOT inverted (MuJoCo's mj_inverse does not either): for a model with noslip_iterations > 0 the forward pass's friction forces
// are the noslip-corrected ones and an inverse of its qacc differs from qfrc_actuator by what noslip changed.
//
// What it writes: the position / velocity stage outputs (derived from qpos / qvel, as fb_batch_forward refreshes them), efc_vel /
// efc_aref / efc_jar / efc_force, qfrc_constraint, and the two result arrays.  It reads qacc and writes neither qacc nor qacc_ws, so a
// control step after it starts from the same state.  DESIGN.md 13; tests/test_side_kernel_resources.py pins its residency.
#pragma once
#include "fb_side.hpp"

enum { FB_INV_FLAG_DISCRETE = 1 };

template <typename real>
struct InvArgs {
  real* qfrc_inverse;     // [n_env][nv]
  real* contact_force;    // [n_env][FB_MAXCON_][3]
  int n_env, flags;
};

template <typename real>
__device__ __forceinline__ void inverse_kernel(const DevModel<real>* Mp, real* rarena, int* iarena, const InvArgs<real>& A) {
  constexpr int EPB = LdsCfg<real>::EPB;
  __shared__ real s_pool[EPB][LdsCfg<real>::POOL];
  __shared__ LdsTab s_tab;
  const DevModel<real>& M = as_constant(*Mp);
  const int tid = threadIdx.x;
  side_stage_tables(M, s_tab, tid);
  const int wave = uniform_int(tid / FB_WAVE), lane = tid % FB_WAVE;
  const int env = uniform_int(blockIdx.x*EPB + wave);
  if (env >= A.n_env) return;
  const WS<real> w = ws_env(M, rarena, iarena, env, s_pool, wave, &s_tab);
  const WS<real> wc = w;
  // ---- mj_invPosition + mj_invVelocity: the forward pass's stages, unchanged
  side_position_velocity(M, wc, lane);
  const int nv = M.nv;
  // ---- the continuous acceleration, in the solve vector lx (the LDS pool is free behind the velocity stage)
  FB_LDS real* Q = w.lx();
  if (A.flags & FB_INV_FLAG_DISCRETE) {
    // mj_discreteAcc (Euler): M^-1 (M + h D) qacc = qacc + M^-1 (h D qacc); the correction term alone goes through the solve, so the
    // rounding of M qacc and its solve does not enter the result
    for (int i = lane; i < nv; i += FB_WAVE) Q[i] = M.timestep*M.dof_damping[i]*w.qacc()[i];
    SYNC();
    d_factor_plain(M, wc, lane);          // (x = the solve vector lx = Q, no damping)
    d_solve(M, wc, true, lane);
    for (int i = lane; i < nv; i += FB_WAVE) Q[i] += w.qacc()[i];
  } else {
    for (int i = lane; i < nv; i += FB_WAVE) Q[i] = w.qacc()[i];
  }
  SYNC();
  // ---- jar = J qacc - aref (and efc_vel / efc_aref, as mj_inverse leaves them), lane == row
  const int nefc = uniform_int(w.istate()[IS_NEFC]);
  for (int r = lane; r < nefc; r += FB_WAVE) {
    real vel = 0, ja = 0;
    for (int side = 0; side < 2; side++) {
      const int body = side ? w.efc_bB()[r] : w.efc_bA()[r], len = side ? w.efc_lB()[r] : w.efc_lA()[r];
      for (int s = 0; s < len; s++) {
        const int dof = M.body_chain[body*FB_MAXCH + s];
        const real j = w.efc_J()[JIDX(side, s, r)];
        vel += j*w.qvel()[dof]; ja += j*Q[dof];
      }
    }
    const real aref = -w.efc_B()[r]*vel - w.efc_K()[r]*w.efc_imp()[r]*(w.efc_pos()[r] - w.efc_margin()[r]);
    w.efc_vel()[r] = vel; w.efc_aref()[r] = aref; w.efc_jar()[r] = ja - aref;
  }
  SYNC();
  // ---- f(jar): the primal map (d_constraint_a's PGS warm-start block); the first row of a contact handles its block
  for (int r = lane; r < nefc; r += FB_WAVE) {
    const int type = w.efc_type()[r];
    if (type != CN_ELLIPTIC) { const real jar = w.efc_jar()[r]; w.efc_force()[r] = jar < 0 ? -w.efc_D()[r]*jar : (real)0; }
    else {
      const int c = w.efc_id()[r];
      if (w.con_efc()[c] != r) continue;
      const real* fr = M.pair_friction + 5*w.con_pair()[c];
      const real mu = w.efc_mu()[r];
      const real j0 = w.efc_jar()[r], j1 = w.efc_jar()[r+1], j2 = w.efc_jar()[r+2];
      const real U0 = j0*mu, U1 = j1*fr[0], U2 = j2*fr[1];
      const real N = U0, T = sqrt(U1*U1 + U2*U2);
      real f0, f1, f2;
      if (N >= mu*T || (T <= 0 && N >= 0)) { f0 = f1 = f2 = 0; }                                      // top zone: separated
      else if (mu*N + T <= 0 || (T <= 0 && N < 0)) { f0 = -w.efc_D()[r]*j0; f1 = -w.efc_D()[r+1]*j1; f2 = -w.efc_D()[r+2]*j2; }   // bottom zone
      else {                                                                                           // middle zone: the cone surface
        const real Dm = w.efc_D()[r] / fmax(FB_MINV, mu*mu*(1 + mu*mu));
        const real NT = N - mu*T;
        f0 = -Dm*NT*mu;
        f1 = -f0/T*U1*fr[0];
        f2 = -f0/T*U2*fr[1];
      }
      w.efc_force()[r] = f0; w.efc_force()[r+1] = f1; w.efc_force()[r+2] = f2;
    }
  }
  SYNC();
  // ---- per dof: qfrc_constraint = J' f and qfrc_inverse = M qacc + qfrc_bias - qfrc_passive - qfrc_constraint
  real* qinv = A.qfrc_inverse + (size_t)env*nv;
  for (int i = lane; i < nv; i += FB_WAVE) {
    const int dep = M.dof_depth[i], nd = M.dof_ndesc[i], madr = M.dof_Madr[i];
    real fc = 0;
    for (int r = 0; r < nefc; r++) {
      const real f = w.efc_force()[r];
      const int ea = w.efc_eA()[r], eb = w.efc_eB()[r];
      if (ea >= i && ea <= i + nd) fc += w.efc_J()[JIDX(0, dep, r)]*f;
      if (eb >= i && eb <= i + nd) fc += w.efc_J()[JIDX(1, dep, r)]*f;
    }
    // M qacc: the row of dof i (diagonal, then its ancestors on the chain of its body, nearest first) ...
    const int* ch = M.body_chain + M.dof_bodyid[i]*FB_MAXCH;
    real mq = w.qM()[madr]*Q[i];
    for (int t = dep - 1; t >= 0; t--) mq += w.qM()[madr + dep - t]*Q[ch[t]];
    // ... and its column: the descendants k, whose rows hold i at the depth difference
    for (int k = i + 1; k <= i + nd; k++) mq += w.qM()[M.dof_Madr[k] + M.dof_depth[k] - dep]*Q[k];
    w.qfrc_constraint()[i] = fc;
    qinv[i] = mq + w.qfrc_bias()[i] - w.qfrc_passive()[i] - fc;
  }
  // ---- contact forces in the contact frame (mj_contactForce; elliptic rows are in the contact frame already)
  real* cf = A.contact_force + (size_t)env*FB_MAXCON_*3;
  const int ncon = uniform_int(w.istate()[IS_NCON]);
  for (int k = lane; k < 3*FB_MAXCON_; k += FB_WAVE) {
    const int c = k / 3, d = k % 3;
    real f = 0;
    if (c < ncon) {
      const int adr = w.con_efc()[c], dim = w.con_dim()[c];
      if (adr >= 0 && d < dim) f = w.efc_force()[adr + d];
    }
    cf[k] = f;
  }
  SYNC();
}

template <typename real>
__global__ void __launch_bounds__(FB_WAVE*LdsCfg<real>::EPB, LdsCfg<real>::WAVES_PER_SIMD) k_inverse(const DevModel<real>* Mp, real* rarena, int* iarena, InvArgs<real> A) {
  inverse_kernel<real>(Mp, rarena, iarena, A);
}
