// Batched multi-site inverse kinematics: the reference's qpos_from_site_xpos (flybody/inverse_kinematics.py:14-165), one frame per
// wavefront.  A frame is the batch environment of the same index; it iterates in that environment's arena row with the position stages
// of the physics step (d_kinematics, d_com_pos: fb_smooth.hpp), unchanged.  Momentum gradient descent on
//     objective(q) = |mask (s(q) - s*)|^2 + reg_strength |q_hinge|^2
// per iteration, in the reference's order (inverse_kinematics.py:102-131):
//   residual r = site_xpos - target (masked components are left out); the gradient of the first term is J^T (2 r), i.e. the point forces
//   2 r at the sites as body wrenches about the tree CoM, summed over subtrees (subtree_sum_lds) and dotted with the motion axes cdof --
//   what d_passive does with the fluid wrenches; + 2 reg_strength qpos on the selected hinge dofs; update = beta update + grad (two dof
//   slots per lane, in registers); qpos <- integratePos(qpos, -lr update) as mj_integratePos; kinematics again.
// Every 100 steps, and only then, the objective is evaluated and the wave stops when lr |update| / err < progress_threshold (a
// wave-uniform, per-frame exit).
//
// Reference semantics kept on purpose (tests/ik_reference.py restates them line by line):
//  * the regularisation acts on the raw hinge qpos, not on qpos - qpos0;
//  * err_norm is the objective of the LAST CHECK, not of the final state;
//  * err_norm_first_term is the objective with reg = 0 on the site positions the reference's `site_xpos` variable holds at exit: the
//    final state when the exit iteration ran a check (convergence, or max_steps - 1 a multiple of 100), otherwise the positions BEFORE
//    the last update (the reference re-reads site_xpos at the top of every iteration and after a check only);
//  * steps = the loop index at exit, max_steps - 1 when the loop ran out; success only on the progress criterion;
//  * no joint-range clipping;
//  * err == 0 follows IEEE (lr |update| / 0 = inf, 0 / 0 = NaN: neither is below a threshold) -- written out explicitly, because the
//    device build's division is not the IEEE sequence (fb_build_flags.h: -fapprox-func); every other quotient is within 1 ulp of it.
//
// Residency: 64 threads = one frame per workgroup, FB_IK_POOL reals of LDS per frame (the kinematics staging 7 nbody + 10 njnt is the
// largest user: walk_on_ball 1513), 2 waves per SIMD = 8 frames per CU (256 VGPRs; LDS would allow 12).  Measured on MI355X at 4096
// frames x 20 000 iterations: 1.44 s at 2 waves per SIMD (208 B of spills per lane) against 2.30 s at 3 (168 VGPRs, 588 B of spills):
// the position stages are written for the step kernel's 256-register budget, and at 168 their spill traffic costs more than the extra
// wave hides.  No Delassus matrix or constraint space.  DESIGN.md 12; tests/test_ik_resources.py pins it.
#pragma once
#include "fb_smooth.hpp"

#define FB_IK_POOL 1536
#define FB_IK_WAVES_PER_SIMD 2
#define FB_IK_CHECK 100             // the reference evaluates the objective every 100 steps (inverse_kinematics.py:122)

template <typename real>
struct IKArgs {
  const int* site;          // [n_site] model site ids
  const int* bsite_off;     // [nbody + 1] the sites on body b are bsite[bsite_off[b] .. bsite_off[b + 1]) (indices into `site`, ascending)
  const int* bsite;         // [n_site]
  const int* include;       // [3 n_site] 1: the component enters the objective
  const int* dof;           // [n_dof] selected dofs (the joints' dofs, in joint order)
  const int* dof_hq;        // [n_dof] qpos address of a selected HINGE dof (regularised), -1 otherwise
  const real* target;       // [n_env][3 n_site]
  real* err;                // [n_env][2] err_norm, err_norm_first_term
  int* steps;               // [n_env][2] steps, success
  int n_site, n_dof, max_steps, n_env;
  real reg, lr, beta, thr;
};

// MuJoCo's mju_quatIntegrate (mju_normalize3 / mju_axisAngle2Quat / mju_normalize4 with their mjMINVAL branches): quat <- quat * exp(vel / 2)
template <typename real>
FBD void ik_quat_integrate(real* q, const real* vel) {
  real ax[3] = {vel[0], vel[1], vel[2]};
  const real an = sqrt(ax[0]*ax[0] + ax[1]*ax[1] + ax[2]*ax[2]);
  if (an < FB_MINV) { ax[0] = 1; ax[1] = 0; ax[2] = 0; }
  else { const real inv = (real)1/an; ax[0] *= inv; ax[1] *= inv; ax[2] *= inv; }
  real qr[4] = {1, 0, 0, 0};
  if (an != 0) { const real s = sin((real)0.5*an); qr[0] = cos((real)0.5*an); qr[1] = ax[0]*s; qr[2] = ax[1]*s; qr[3] = ax[2]*s; }
  const real qn = sqrt(q[0]*q[0] + q[1]*q[1] + q[2]*q[2] + q[3]*q[3]);
  if (qn < FB_MINV) { q[0] = 1; q[1] = q[2] = q[3] = 0; }
  else if (fabs(qn - 1) > FB_MINV) { const real inv = (real)1/qn; q[0] *= inv; q[1] *= inv; q[2] *= inv; q[3] *= inv; }
  real r[4];
  mulquat(r, q, qr);
  q[0] = r[0]; q[1] = r[1]; q[2] = r[2]; q[3] = r[3];
}

// sum over the included components of (site_xpos - target)^2, as the reference forms it: np.linalg.norm(diff)**2.  All lanes call.
template <typename real>
FBD real ik_site_err(const IKArgs<real>& A, const WS<real>& w, const real* tgt, int lane) {
  real s = 0;
  for (int c = lane; c < 3*A.n_site; c += FB_WAVE) {
    const real r = w.sxpos()[3*A.site[c/3] + c%3] - tgt[c];
    if (A.include[c]) s += r*r;
  }
  const real n = sqrt(wave_sum(s));
  return n*n;
}

template <typename real>
__device__ __forceinline__ void ik_kernel(const DevModel<real>* Mp, real* rarena, int* iarena, const IKArgs<real>& A) {
  __shared__ real s_ik[1][FB_IK_POOL];                          // (one wave per workgroup)
  const DevModel<real>& M = as_constant(*Mp);
  const int lane = threadIdx.x % FB_WAVE;
  const int env = uniform_int(blockIdx.x);
  if (env >= A.n_env) return;
  const WS<real> w = ws_env(M, rarena, iarena, env, s_ik, 0, (const LdsTab*)nullptr);      // (the position stages use the pool only, not the elimination-tree tables)
  const real* tgt = A.target + (size_t)env*3*A.n_site;
  const int nv = M.nv, nbody = M.nbody;
  // LDS after the position stages: cdof [6 nv] (d_com_pos mirrors it at the pool's start) | body wrenches [6 nbody] | qpos update [nv]
  const FB_LDS real* Lc = w.lLD;
  FB_LDS real* X = w.lLD + 6*nv;
  FB_LDS real* Lu = X + 6*nbody;
  // the lane's two dof slots: dof id, hinge qpos address, momentum
  int di[2], hq[2]; bool dok[2]; real upd[2] = {0, 0};
#pragma unroll
  for (int u = 0; u < 2; u++) {
    const int d = lane + u*FB_WAVE; dok[u] = d < A.n_dof;
    di[u] = dok[u] ? A.dof[d] : 0; hq[u] = dok[u] ? A.dof_hq[d] : -1;
  }
  // mj_fwdPosition before the loop (inverse_kinematics.py:84)
  d_kinematics(M, w, lane);
  d_com_pos(M, w, lane);
  real err = 0, first = 0;
  int step = 0, success = 0;
  for (step = 0; step < A.max_steps; step++) {
    const bool last = step == A.max_steps - 1;
    // the reference's site_xpos of this iteration, should the loop end here without a check
    if (last && step % FB_IK_CHECK != 0) first = ik_site_err(A, w, tgt, lane);
    // ---- body wrenches of the point forces 2 r about the tree CoM: [sum (p - com) x F ; sum F] over the body's sites
    const real com[3] = {w.com()[0], w.com()[1], w.com()[2]};
#pragma unroll
    for (int q = 0; q < 2; q++) {
      const int b = lane + q*FB_WAVE;
      if (b < nbody) {
        real x[6] = {0, 0, 0, 0, 0, 0};
        for (int t = A.bsite_off[b]; t < A.bsite_off[b + 1]; t++) {
          const int k = A.bsite[t], s = A.site[k];
          real p[3], F[3], off[3], tq[3];
#pragma unroll
          for (int c = 0; c < 3; c++) {
            p[c] = w.sxpos()[3*s + c];
            F[c] = A.include[3*k + c] ? (real)2*(p[c] - tgt[3*k + c]) : (real)0;
          }
          sub3(off, p, com); cross3(tq, off, F);
#pragma unroll
          for (int c = 0; c < 3; c++) { x[c] += tq[c]; x[3 + c] += F[c]; }
        }
#pragma unroll
        for (int c = 0; c < 6; c++) X[6*b + c] = x[c];
      }
    }
    for (int i = lane; i < nv; i += FB_WAVE) Lu[i] = 0;
    SYNC_LDS();
    subtree_sum_lds<6>(M, X, lane);
    // ---- gradient on the selected dofs, momentum, the update vector
#pragma unroll
    for (int u = 0; u < 2; u++) {
      if (dok[u]) {
        const int i = di[u], bd = M.dof_bodyid[i];
        real c[6], x[6];
#pragma unroll
        for (int k = 0; k < 6; k++) { c[k] = Lc[6*i + k]; x[k] = X[6*bd + k]; }
        real g = dot6(c, x);
        if (hq[u] >= 0) g += (real)2*A.reg*w.qpos()[hq[u]];
        upd[u] = A.beta*upd[u] + g;
        Lu[i] = -A.lr*upd[u];
      }
    }
    SYNC_LDS();
    // ---- qpos <- mj_integratePos(qpos, Lu, 1): every joint, lane-parallel (unselected ones with a zero update, as the reference)
    for (int j = lane; j < M.njnt; j += FB_WAVE) {
      const int jt = M.jnt_type[j], qa = M.jnt_qposadr[j], da = M.jnt_dofadr[j];
      real* qp = w.qpos() + qa;
      if (jt == JNT_FREE) {
        real v[3] = {Lu[da + 3], Lu[da + 4], Lu[da + 5]}, qt[4] = {qp[3], qp[4], qp[5], qp[6]};
        qp[0] += Lu[da]; qp[1] += Lu[da + 1]; qp[2] += Lu[da + 2];
        ik_quat_integrate(qt, v);
        qp[3] = qt[0]; qp[4] = qt[1]; qp[5] = qt[2]; qp[6] = qt[3];
      } else if (jt == JNT_BALL) {
        real v[3] = {Lu[da], Lu[da + 1], Lu[da + 2]}, qt[4] = {qp[0], qp[1], qp[2], qp[3]};
        ik_quat_integrate(qt, v);
        qp[0] = qt[0]; qp[1] = qt[1]; qp[2] = qt[2]; qp[3] = qt[3];
      } else qp[0] += Lu[da];
    }
    SYNC();                                  // the kinematics read qpos from the row
    d_kinematics(M, w, lane);
    d_com_pos(M, w, lane);
    // ---- progress check (inverse_kinematics.py:122-131)
    if (step % FB_IK_CHECK == 0) {
      const real e1 = ik_site_err(A, w, tgt, lane);
      real h2 = 0, u2 = 0;
#pragma unroll
      for (int u = 0; u < 2; u++) {
        if (hq[u] >= 0) { const real q = w.qpos()[hq[u]]; h2 += q*q; }
        if (dok[u]) u2 += upd[u]*upd[u];
      }
      const real hn = sqrt(wave_sum(h2)), un = sqrt(wave_sum(u2));
      err = e1 + A.reg*(hn*hn);
      first = e1;
      const real num = A.lr*un;
      const real crit = err != 0 ? num/err : (num != 0 ? (real)INFINITY : (real)NAN);
      if (uniform_int(crit < A.thr ? 1 : 0)) { success = 1; break; }
    }
  }
  if (step >= A.max_steps) step = A.max_steps - 1;
  if (lane == 0) {
    A.err[2*(size_t)env] = err; A.err[2*(size_t)env + 1] = first;
    A.steps[2*(size_t)env] = step; A.steps[2*(size_t)env + 1] = success;
  }
}

template <typename real>
__global__ void __launch_bounds__(FB_WAVE, FB_IK_WAVES_PER_SIMD) k_ik(const DevModel<real>* Mp, real* rarena, int* iarena, IKArgs<real> A) {
  ik_kernel<real>(Mp, rarena, iarena, A);
}
