// Sensors, integrator and the substep driver: the stage machine of a control step, with the task hooks (fb_task.hpp:
// observations, reward, termination, auto-reset) fused behind the physics.
#pragma once
#include "fb_types.hpp"
#include "fb_math.hpp"
#include "fb_smooth.hpp"
#include "fb_forces.hpp"
#include "fb_law.hpp"
#include "fb_collide.hpp"
#include "fb_constraint.hpp"
#include "fb_task.hpp"

// ------------------------------------------------------------------ sensors
template <typename real>
__device__ __forceinline__ void d_sensor_vel(const DevModel<real>& M, const WS<real>& w, int lane) {
  if (lane == 0) {
    int s = M.site_thorax;
    real lvel[6];
    object_velocity(w, M.site_bodyid[s], w.sxpos() + 3*s, w.sxmat() + 9*s, lvel);
    for (int k = 0; k < 3; k++) { w.sens()[3 + k] = lvel[k]; w.sens()[6 + k] = lvel[3 + k]; }
  }
  SYNC();
}

template <typename real>
FBD real ray_quad(real a, real b, real c, real* x) {
  real det = b*b - a*c;
  if (det < FB_MINV || a < FB_MINV) { x[0] = -1; x[1] = -1; return -1; }
  det = sqrt(det);
  x[0] = (-b - det)/a; x[1] = (-b + det)/a;
  if (x[0] >= 0) return x[0];
  if (x[1] >= 0) return x[1];
  return -1;
}
template <typename real>
FBD real ray_site(const real* pos, const real* mat, const real* size, int type, const real* pnt, const real* vec) {
  real dif[3], lp[3], lv[3], xx[2];
  sub3(dif, pnt, pos);
  mulmatT3(lp, mat, dif); mulmatT3(lv, mat, vec);
  if (type == GEOM_SPHERE) return ray_quad(dot3(lv, lv), dot3(lv, lp), dot3(lp, lp) - size[0]*size[0], xx);
  if (type == GEOM_CAPSULE) {
    real best = -1;
    real a = lv[0]*lv[0] + lv[1]*lv[1], b = lv[0]*lp[0] + lv[1]*lp[1], c = lp[0]*lp[0] + lp[1]*lp[1] - size[0]*size[0];
    ray_quad(a, b, c, xx);
    for (int k = 0; k < 2; k++) if (xx[k] >= 0 && fabs(lp[2] + xx[k]*lv[2]) <= size[1] && (best < 0 || xx[k] < best)) best = xx[k];
    for (int sgn = -1; sgn <= 1; sgn += 2) {
      real lq[3] = {lp[0], lp[1], lp[2] - sgn*size[1]};
      ray_quad(dot3(lv, lv), dot3(lv, lq), dot3(lq, lq) - size[0]*size[0], xx);
      for (int k = 0; k < 2; k++) if (xx[k] >= 0 && sgn*(lq[2] + xx[k]*lv[2]) >= 0 && (best < 0 || xx[k] < best)) best = xx[k];
    }
    return best;
  }
  if (type == GEOM_ELLIPSOID) {
    real sp[3] = {lp[0]/size[0], lp[1]/size[1], lp[2]/size[2]}, sv[3] = {lv[0]/size[0], lv[1]/size[1], lv[2]/size[2]};
    return ray_quad(dot3(sv, sv), dot3(sv, sp), dot3(sp, sp) - 1, xx);
  }
  return -1;
}

// acceleration-stage sensors: accelerometer (thorax site), 6 force sensors, 6 touch sensors
// FORCES (k_step_forces, fb_forces.hpp): xf = the environment's xfrc_applied rows (null: none); they enter cfrc_ext as in mj_rnePostConstraint
template <typename real, bool FORCES = false>
__device__ __forceinline__ void d_sensor_acc(const DevModel<real>& M, const WS<real>& w, int lane, const FB_GLOBAL real* xf = nullptr) {
  PROF_BEGIN();
  int ncon = w.istate()[IS_NCON];
  // wrench of each active contact about the tree CoM, in the lane that owns the contact (at most 64 contacts)
  int cb1 = -1, cb2 = -1;
  real cw[6] = {0, 0, 0, 0, 0, 0}, cfn = 0;
  real cnr[3] = {0, 0, 0}, cps[3] = {0, 0, 0};            // the lane's contact normal and position (the touch sensors read them by v_readlane)
  {
    // two rounds of loads: everything indexed by the contact (= lane), then what hangs off its pair id and row address
    const bool cv = lane < ncon; const int cs = cv ? lane : 0;
    const int adr = cv ? w.con_efc()[cs] : -1, p = w.con_pair()[cs], cdim = w.con_dim()[cs];
    real fr[9], cp[3], cm[3];
#pragma unroll
    for (int k = 0; k < 9; k++) fr[k] = w.con_frame()[9*cs + k];
#pragma unroll
    for (int k = 0; k < 3; k++) { cp[k] = w.con_pos()[3*cs + k]; cm[k] = w.com()[k]; }
#pragma unroll
    for (int k = 0; k < 3; k++) { cnr[k] = fr[k]; cps[k] = cp[k]; }
    const bool act = cv && adr >= 0;
    const int a0 = act ? adr : 0, ps = act ? p : 0;
    const int pb = M.pair_body[ps];
    const real f0 = w.efc_force()[a0], f1 = w.efc_force()[a0 + ((act && cdim > 1) ? 1 : 0)], f2 = w.efc_force()[a0 + ((act && cdim > 1) ? 2 : 0)];
    if (act) {
      cb1 = pb & 0xffff; cb2 = pb >> 16;
      cfn = f0;
      real lf[3] = {cfn, 0, 0};
      if (cdim > 1) { lf[1] = f1; lf[2] = f2; }
      real r[3];
      mulmatT3(cw + 3, fr, lf);
      sub3(r, cp, cm);
      cross3(cw, r, cw + 3);
    }
  }
  // Only the bodies the sensors read are needed: the accelerometer's body and the subtrees below the force-sensor bodies
  // (fruit fly: thorax + 6 x 5 tarsus segments = 31 of 68 bodies -> ONE pass of the wave instead of two, the second of which
  // would run the whole chain walk for four bodies).  A model with more than 64 such bodies takes the all-bodies passes.
  const int nsb = M.nsensbody;
  // body accelerations: -g + sum of cdof_dot qvel along the chain (cabias, from the velocity stage) + sum of cdof qacc (tree
  // prefix over the dofs in registers, fb_smooth.hpp), and body forces
  DofPair<real> Q;
  {
    const int ia = lane, ib = lane + FB_WAVE;
    const bool ha = ia < M.nv, hb = ib < M.nv;
    // (all twelve loads unconditional at clamped indices, then selects: one round trip instead of a branch per test)
    const int sa = min(ia, M.nv - 1), sb = min(ib, M.nv - 1);
    const real qa = w.qacc()[sa], qb = w.qacc()[sb];
    real da[6], db[6];
#pragma unroll
    for (int c = 0; c < 6; c++) { da[c] = w.cdof()[6*sa + c]; db[c] = w.cdof()[6*sb + c]; }
#pragma unroll
    for (int c = 0; c < 6; c++) { Q.a[c] = ha ? da[c]*qa : (real)0; Q.b[c] = hb ? db[c]*qb : (real)0; }
    tree_prefix6(M, Q, lane);
  }
  if (nsb > 0) {
    // ---- lane == sensor body: the external wrench, the acceleration and the body force stay in the lane's registers; the
    // accelerometer reads the thorax lane's acceleration by v_readlane, the force sensors sum their subtree (DFS-contiguous in the
    // body list, hence in the lanes) by ds_bpermute.  (Rounds 1-3 passed all three through the environment's global row.)
    const int b = lane < nsb ? M.sens_body[lane] : -1;
    real ext[6] = {0, 0, 0, 0, 0, 0};
    for (int c = 0; c < ncon; c++) {
      int rb1 = rdlane(cb1, c), rb2 = rdlane(cb2, c);
      if (rb1 < 0 || rb1 == rb2) continue;
      real wr[6];
      for (int k = 0; k < 6; k++) wr[k] = rdlane(cw[k], c);
      if (b > 0 && (b == rb1 || b == rb2)) {
        real sgn = (b == rb2) ? (real)1 : (real)-1;
        for (int k = 0; k < 6; k++) ext[k] += sgn*wr[k];
      }
    }
    if constexpr (FORCES) {
      if (xf && b > 0) { real xw[6]; applied_wrench(M, w, xf, b, xw); for (int k = 0; k < 6; k++) ext[k] += xw[k]; }
    }
    real qsum[6];
    dof_fetch6(Q, b >= 0 ? M.body_veldof[b] : -1, qsum);               // (wave collective)
    real a[6] = {0, 0, 0, -M.grav[0], -M.grav[1], -M.grav[2]}, frc[3] = {0, 0, 0};
    if (b > 0) {
      real ci[10], cv[6], t[6], t1[6], t2[6];
      for (int k = 0; k < 6; k++) a[k] += w.cabias()[6*b + k] + qsum[k];
      for (int k = 0; k < 10; k++) ci[k] = w.cinert()[10*b + k];
      for (int k = 0; k < 6; k++) cv[k] = w.cvel()[6*b + k];
      mulinertvec(t, ci, a);
      mulinertvec(t1, ci, cv);
      crossforce(t2, cv, t1);
      for (int k = 0; k < 3; k++) frc[k] = t[3 + k] + t2[3 + k] - ext[3 + k];
    }
    // accelerometer: the thorax site's body
    {
      const int s = M.site_thorax, bt = M.site_bodyid[s];
      const unsigned long long mt = __ballot(b == bt);
      const int src = mt ? __ffsll((long long)mt) - 1 : 0;
      real ca[6];
      for (int k = 0; k < 6; k++) ca[k] = rdlane(a[k], src);
      if (lane == 0) {
        real dif[3], t[3], lin[3], la[3], lvel[6], cor[3];
        sub3(dif, w.sxpos() + 3*s, w.com());
        cross3(t, dif, ca);
        sub3(lin, ca + 3, t);
        mulmatT3(la, w.sxmat() + 9*s, lin);
        object_velocity(w, bt, w.sxpos() + 3*s, w.sxmat() + 9*s, lvel);
        cross3(cor, lvel, lvel + 3);
        for (int k = 0; k < 3; k++) w.sens()[k] = la[k] + cor[k];
      }
    }
    // force sensors: interaction force of the site's body = subtree sum of body forces, deepest body first
    {
      const bool fs = lane >= 8 && lane < 8 + M.nforce;
      const int kf = fs ? lane - 8 : 0;
      const int s = fs ? M.force_sites[kf] : 0, bf = M.site_bodyid[s];
      const int n = fs ? M.body_nsub[bf] : 0;
      int first = 0, nmax = 0;                                    // lane of the sensor body inside the sensor-body list; longest subtree
      for (int q = 0; q < M.nforce; q++) {
        // (sensor q's body and subtree size sit in lane 8 + q: two v_readlane instead of three dependent table loads per sensor)
        const int bq = rdlane(bf, 8 + q);
        const unsigned long long mq = __ballot(b == bq);
        const int lq = mq ? __ffsll((long long)mq) - 1 : 0;
        if (kf == q) first = lq;
        const int nq = rdlane(n, 8 + q);
        nmax = nq > nmax ? nq : nmax;
      }
      real acc[3] = {0, 0, 0};
      for (int u = 0; u < nmax; u++) {
        const int d = n - 1 - u;                                  // (every lane takes part in the shuffles)
        const int srcl = first + (d >= 0 ? d : 0);
        const real f0 = __shfl(frc[0], srcl, 64), f1 = __shfl(frc[1], srcl, 64), f2 = __shfl(frc[2], srcl, 64);
        if (d >= 0) { acc[0] += f0; acc[1] += f1; acc[2] += f2; }
      }
      if (fs) mulmatT3(w.sens() + 9 + 3*kf, w.sxmat() + 9*s, acc);
    }
  } else {
  const int npass = (M.nbody + FB_WAVE - 1)/FB_WAVE;
  // external wrench per body: lane == body, the contacts are broadcast one at a time (in contact order)
  for (int ps = 0; ps < npass; ps++) {
    const int b = (ps*FB_WAVE + lane < M.nbody ? ps*FB_WAVE + lane : -1);
    real acc[6] = {0, 0, 0, 0, 0, 0};
    for (int c = 0; c < ncon; c++) {
      int rb1 = rdlane(cb1, c), rb2 = rdlane(cb2, c);
      if (rb1 < 0 || rb1 == rb2) continue;
      real wr[6];
      for (int k = 0; k < 6; k++) wr[k] = rdlane(cw[k], c);
      if (b > 0 && (b == rb1 || b == rb2)) {
        real sgn = (b == rb2) ? (real)1 : (real)-1;
        for (int k = 0; k < 6; k++) acc[k] += sgn*wr[k];
      }
    }
    if constexpr (FORCES) {
      if (xf && b > 0) { real xw[6]; applied_wrench(M, w, xf, b, xw); for (int k = 0; k < 6; k++) acc[k] += xw[k]; }
    }
    if (b >= 0) for (int k = 0; k < 6; k++) w.cfrc_ext()[6*b + k] = acc[k];
  }
  SYNC();
  for (int ps = 0; ps < npass; ps++) {
    const int b = (ps*FB_WAVE + lane < M.nbody ? ps*FB_WAVE + lane : -1);
    real qsum[6];
    dof_fetch6(Q, b >= 0 ? M.body_veldof[b] : -1, qsum);               // (wave collective: before any lane leaves the iteration)
    if (b < 0) continue;
    real a[6] = {0, 0, 0, -M.grav[0], -M.grav[1], -M.grav[2]};
    real* out = w.cfrc() + 6*b;
    if (b == 0) { for (int k = 0; k < 6; k++) { out[k] = 0; w.cacc()[k] = a[k]; } continue; }
    for (int k = 0; k < 6; k++) a[k] += w.cabias()[6*b + k] + qsum[k];
    for (int k = 0; k < 6; k++) w.cacc()[6*b + k] = a[k];
    real t[6], t1[6], t2[6];
    mulinertvec(t, w.cinert() + 10*b, a);
    mulinertvec(t1, w.cinert() + 10*b, w.cvel() + 6*b);
    crossforce(t2, w.cvel() + 6*b, t1);
    for (int k = 0; k < 6; k++) out[k] = t[k] + t2[k] - w.cfrc_ext()[6*b + k];
  }
  SYNC();
  if (lane == 0) {
    int s = M.site_thorax, b = M.site_bodyid[s];
    const real* ca = w.cacc() + 6*b;
    real dif[3], t[3], lin[3], la[3], lvel[6], cor[3];
    sub3(dif, w.sxpos() + 3*s, w.com());
    cross3(t, dif, ca);
    sub3(lin, ca + 3, t);
    mulmatT3(la, w.sxmat() + 9*s, lin);
    object_velocity(w, b, w.sxpos() + 3*s, w.sxmat() + 9*s, lvel);
    cross3(cor, lvel, lvel + 3);
    for (int k = 0; k < 3; k++) w.sens()[k] = la[k] + cor[k];
  }
  // force sensors: interaction force of the site's body = subtree sum of body forces
  if (lane >= 8 && lane < 8 + M.nforce) {
    int k = lane - 8;
    int s = M.force_sites[k], b = M.site_bodyid[s];
    real acc[3] = {0, 0, 0};
    int n = M.body_nsub[b];
    for (int d = n - 1; d >= 0; d--) { const real* c = w.cfrc() + 6*(b + d) + 3; acc[0] += c[0]; acc[1] += c[1]; acc[2] += c[2]; }
    mulmatT3(w.sens() + 9 + 3*k, w.sxmat() + 9*s, acc);
  }
  }
  {
    bool on = lane >= 16 && lane < 16 + M.ntouch;
    int k = lane - 16;
    int s = on ? M.touch_sites[k] : 0, b = on ? M.site_bodyid[s] : -2;
    // the site's pose and shape once, in one round of loads; the contacts' normals and positions come from the lanes that own them
    // (rounds 1-3 re-read both from the global row inside the loop: two dependent round trips per contact)
    real tpos[3], tmat[9], tsize[3];
#pragma unroll
    for (int q = 0; q < 3; q++) { tpos[q] = w.sxpos()[3*s + q]; tsize[q] = M.site_size[3*s + q]; }
#pragma unroll
    for (int q = 0; q < 9; q++) tmat[q] = w.sxmat()[9*s + q];
    const int ttype = M.site_type[s];
    real sum = 0;
    for (int c = 0; c < ncon; c++) {
      int rb1 = rdlane(cb1, c), rb2 = rdlane(cb2, c);
      real fn = rdlane(cfn, c);
      if (rb1 < 0 || fn <= 0) continue;
      real ray[3] = {rdlane(cnr[0], c), rdlane(cnr[1], c), rdlane(cnr[2], c)};
      const real pnt[3] = {rdlane(cps[0], c), rdlane(cps[1], c), rdlane(cps[2], c)};
      if (b != rb1 && b != rb2) continue;
      if (b == rb2) scl3(ray, ray, (real)-1);
      if (ray_site(tpos, tmat, tsize, ttype, pnt, ray) >= 0) sum += fn;
    }
    if (on) w.sens()[9 + 3*M.nforce + k] = sum;
  }
  SYNC();
}

// ------------------------------------------------------------------ integrator (semi-implicit Euler, implicit joint damping)
template <typename real>
__device__ __forceinline__ void d_integrate(const DevModel<real>& M, const WS<real>& w, int lane) {
  real h = M.timestep;
  // Round 5: in load rounds, and without the store -> fence -> reload of qvel between the velocity and the position update (the new
  // velocities reach the joints through the solve vector in LDS, which is dead after this stage).
  for (int i0 = 0; i0 < M.nu; i0 += FB_WAVE) {
    const int i = i0 + lane; const bool ok = i < M.nu; const int is = ok ? i : 0;
    const int aa = M.act_actadr[is], dt = M.act_dyntype[is]; const real prm = M.act_dynprm[is];
    const int as_ = (ok && aa >= 0) ? aa : 0;
    const real a0 = w.act()[as_], ad = w.act_dot()[as_];
    if (ok && aa >= 0) {
      real an;
      if (dt == DYN_FILTEREXACT) { real tau = fmax(FB_MINV, prm); an = a0 + ad*tau*(1 - exp(-h/tau)); }
      else an = a0 + h*ad;
      w.act()[aa] = an;
    }
  }
  for (int i = lane; i < M.nv; i += FB_WAVE) { const real v = w.qvel()[i] + h*w.lx()[i]; w.qvel()[i] = v; w.lx()[i] = v; }
  SYNC_LDS();
  {
    int jt[2], qa[2], da[2]; bool jok[2]; real qv[2][7], vv[2][6];
#pragma unroll
    for (int u = 0; u < 2; u++) {
      const int j = lane + u*FB_WAVE; jok[u] = j < M.njnt; const int js = jok[u] ? j : 0;
      jt[u] = M.jnt_type[js]; qa[u] = M.jnt_qposadr[js]; da[u] = M.jnt_dofadr[js];
    }
#pragma unroll
    for (int u = 0; u < 2; u++) {
      const int nq = M.nq, nv = M.nv;
      const int nqw = jt[u] == JNT_FREE ? 7 : (jt[u] == JNT_BALL ? 4 : 1), nvw = jt[u] == JNT_FREE ? 6 : (jt[u] == JNT_BALL ? 3 : 1);
#pragma unroll
      for (int k = 0; k < 7; k++) qv[u][k] = w.qpos()[min(qa[u] + min(k, nqw - 1), nq - 1)];
#pragma unroll
      for (int k = 0; k < 6; k++) vv[u][k] = w.lx()[min(da[u] + min(k, nvw - 1), nv - 1)];
    }
#pragma unroll
    for (int u = 0; u < 2; u++) {
      if (!jok[u]) continue;
      const int qa_ = qa[u];
      if (jt[u] == JNT_FREE) {
        for (int k = 0; k < 3; k++) w.qpos()[qa_ + k] = qv[u][k] + h*vv[u][k];
        real ax[3] = {vv[u][3], vv[u][4], vv[u][5]};
        real n = normalize3(ax);
        real q[4] = {qv[u][3], qv[u][4], qv[u][5], qv[u][6]}, qr[4], res[4];
        axisangle2quat(qr, ax, n*h);
        normquat(q);
        mulquat(res, q, qr);
        normquat(res);
        for (int k = 0; k < 4; k++) w.qpos()[qa_ + 3 + k] = res[k];
      } else if (jt[u] == JNT_BALL) {
        real ax[3] = {vv[u][0], vv[u][1], vv[u][2]};
        real n = normalize3(ax);
        real q[4] = {qv[u][0], qv[u][1], qv[u][2], qv[u][3]}, qr[4], res[4];
        axisangle2quat(qr, ax, n*h);
        normquat(q);
        mulquat(res, q, qr);
        normquat(res);
        for (int k = 0; k < 4; k++) w.qpos()[qa_ + k] = res[k];
      } else w.qpos()[qa_] = qv[u][0] + h*vv[u][0];
    }
  }
  if (lane == 0) sim_clock(w) += M.clock_timestep;
  SYNC();
}

// ------------------------------------------------------------------ the stage machine
// One launch = one pass of this interpreter.  Every stage is inlined exactly once; the factor and
// solve stages are shared by their three / two users through a return-stage register.  All stage
// selectors are wave-uniform.  Order per substep follows dm_control's legacy step: mj_step2
// (actuation, acceleration, constraint, acceleration-stage sensors), integrate, mj_step1
// (position + velocity stages for the new state).
enum { ST_ACT, ST_ACC_PRE, ST_SOLVE, ST_ACC_SOLVE, ST_ACC_POST, ST_CONSTR_A, ST_CONSTR_B, ST_SENS, ST_EULER_PRE, ST_FACTOR, ST_EULER_SOLVE,
       ST_EULER_POST, ST_KIN, ST_COLL, ST_SUBEND, ST_DONE };
enum { MODE_STEP = 0, MODE_SUBSTEP = 1, MODE_FORWARD = 2, MODE_RESET = 3, MODE_STAGE = 4 };
// MODE_STAGE (fb_batch_stage, profiling only): ONE stage of a control step per launch, so that rocprofv3's per-dispatch counters
// (instructions, active lanes, traffic) can be attributed to stages.  Stage word: stage id | damp << 8 | half << 9 | part mask << 12
// (ST_KIN: kinematics / com_pos / crb; ST_COLL: collision / rows / velocity; ST_ACC_POST: copy / projection; 0 = all parts);
// ST_PRE / ST_POST are the task hooks around the substeps.  The LDS pool is parked in global memory between launches (k_fly).
enum { ST_PRE = 32, ST_POST = 33 };

// ------------------------------------------------------------------ stage entry points
// Every stage of the step is compiled as a function of its own: the register allocator then works on one stage at a
// time instead of on the whole state machine (measured: the fully inlined kernel is ~25% slower).  A stage receives the
// model (constant memory) and a copy of the workspace descriptor; it moves the descriptor's pointers back to SGPRs.
// trailing-wave priority thresholds, in 32nds of the launch's environments (s_velocity)
#define FB_PRIO_T1 16
#define FB_PRIO_T2 28
#define FB_PRIO_T3 31
#define FB_LAT_PRIO 2     // issue priority of the latency-bound stage class (d_run)
#define FB_STAGE_C __device__ FB_NOINLINE
#define FB_STAGE_WRAP(name, ...) \
  template <typename real> FB_STAGE_C void name(const DevModel<real>& M_, const WS<real>& w_, int lane) { \
    const DevModel<real>& M = as_constant(M_); const WS<real> w = ws_uniform(w_, M); __VA_ARGS__; }
FB_STAGE_WRAP(s_kinematics, d_kinematics(M, w, lane))
FB_STAGE_WRAP(s_com_pos, d_com_pos(M, w, lane))
FB_STAGE_WRAP(s_crb, d_crb(M, w, lane))
FB_STAGE_WRAP(s_collision, d_collision(M, w, lane))
FB_STAGE_WRAP(s_make_constraint, d_make_constraint(M, w, lane))
// (the projection's stage keeps the smooth acceleration first: the solve that precedes it left M^-1 qfrc_smooth in lx, and every lane of it is fenced)
template <typename real> FB_STAGE_C void s_project_constraint(const DevModel<real>& M_, const WS<real>& w_, int parts, int lane) {
  const DevModel<real>& M = as_constant(M_); const WS<real> w = ws_uniform(w_, M);
  parts = uniform_int(parts);                                                            // (MODE_STAGE: 1 = the copy, 2 = the projection; the step passes 3)
  if (parts & 1) {
    for (int i = lane; i < M.nv; i += FB_WAVE) w.qacc_smooth()[i] = w.lx()[i];
    SYNC();
  }
  if (parts & 2) d_project_constraint(M, w, lane); }
// The velocity stage closes a substep: with `acc` the sensors it completes are added to the control step's accumulators, and with a progress
// counter (`ctr`, null: none) the wave counts itself in and gets its issue priority for the next substep (returned, -1: none; see ST_COLL in d_run).
template <typename real> FB_STAGE_C int s_velocity(const DevModel<real>& M_, const WS<real>& w_, bool acc, int* ctr_, int nslot, int lane) {
  const DevModel<real>& M = as_constant(M_); const WS<real> w = ws_uniform(w_, M);
  FB_LDS real* Lv = w.lLD + vel_off_v(M); FB_LDS real* X = w.lLD + vel_off_x(M);        // body velocities / per-body wrenches (fb_smooth.hpp)
  real ab[2][6];                                                                         // bias accelerations of the lane's two bodies
  d_com_vel(M, w, Lv, ab, lane); d_passive(M, w, Lv, X, lane); d_rne_bias(M, w, Lv, X, ab, lane); d_sensor_vel(M, w, lane);
  int prio = -1;
  if (uniform_int(acc ? 1 : 0) != 0) {
    if (lane < FB_NSENS) w.sens_acc()[lane] += w.sens()[lane];
    SYNC();
  }
  int* ctr = uniform_p(ctr_);
  if (ctr) {
    nslot = uniform_int(nslot);
    int before = 0;
    if (lane == 0) before = atomicAdd(ctr, 1);
    before = uniform_int(before);
    prio = (32*before < FB_PRIO_T1*nslot) ? 0 : (32*before < FB_PRIO_T2*nslot ? 1 : (32*before < FB_PRIO_T3*nslot ? 2 : 3));
    if (lane == 0) w.istate()[IS_PRIO] = prio;
  }
  return prio; }
FB_STAGE_WRAP(s_actuation, d_actuation(M, w, lane))
// a pass without controls (the forward pass of a reset): no actuator forces, no activation derivatives
template <typename real> FB_STAGE_C void s_actuation_zero(const DevModel<real>& M_, const WS<real>& w_, int lane) {
  const DevModel<real>& M = as_constant(M_); const WS<real> w = ws_uniform(w_, M);
  for (int i = lane; i < M.nv; i += FB_WAVE) { w.qfrc_actuator()[i] = 0; w.lx()[i] = 0; }
  for (int i = lane; i < M.na; i += FB_WAVE) w.act_dot()[i] = 0;
  SYNC(); }
FB_STAGE_WRAP(s_constraint_b, d_constraint_b(M, w, lane))
FB_STAGE_WRAP(s_sensor_acc, d_sensor_acc(M, w, lane))
FB_STAGE_WRAP(s_integrate, d_integrate(M, w, lane))
template <typename real> FB_STAGE_C void s_sensor_acc_forces(const DevModel<real>& M_, const WS<real>& w_, const real* xfrc_, int lane) {
  const DevModel<real>& M = as_constant(M_); const WS<real> w = ws_uniform(w_, M);
  d_sensor_acc<real, true>(M, w, lane, (const FB_GLOBAL real*)uniform_p(xfrc_)); }
template <typename real> FB_STAGE_C bool s_constraint_a(const DevModel<real>& M_, const WS<real>& w_, int lane) {
  const DevModel<real>& M = as_constant(M_); const WS<real> w = ws_uniform(w_, M); return d_constraint_a(M, w, lane); }
template <typename real> FB_STAGE_C void s_init(const DevModel<real>& M_, const WS<real>& w_, int env, int lane) {
  const DevModel<real>& M = as_constant(M_); const WS<real> w = ws_uniform(w_, M);
  if (lane == 0) w.istate()[IS_WARN_EVER] = 0;  d_task_init(M, w, env, lane); }
template <typename real> FB_STAGE_C void s_pre(const DevModel<real>& M_, const WS<real>& w_, const float* action, int lane) {
  const DevModel<real>& M = as_constant(M_); const WS<real> w = ws_uniform(w_, M); d_task_pre(M, w, action, lane); }
template <typename real> FB_STAGE_C void s_post(const DevModel<real>& M_, const WS<real>& w_, bool resetting, float* obs, float* reward, float* discount, int* step_type, int lane) {
  const DevModel<real>& M = as_constant(M_); const WS<real> w = ws_uniform(w_, M);
  // The flag and the environment's output rows are wave-uniform like the descriptor: SGPRs (otherwise the 12-per-CU FP64 build spills more than 503b35d's s_post did).
  d_task_post(M, w, uniform_int(resetting) != 0, uniform_p(obs), uniform_p(reward), uniform_p(discount), uniform_p(step_type), lane); }

// tk < 0: the whole call (all substeps of a control step, or what `mode` says).  tk >= 0: ONE substep of a control step handed out by
// the substep scheduler of k_fly (MODE_STEP only): bit 0 = first substep of the step (the action scatter, or the auto-reset, happens
// here), bit 1 = last (the task epilogue happens here); bit 2 = the FIRST HALF of a substep only (actuation .. acceleration sensors: stop where
// the integration would start), bit 3 = the SECOND HALF only (start at the integration: M + h D, Euler, mj_step1 of the next substep).  Nothing
// LDS-resident is alive at that boundary -- the factor of M is dead, the right-hand side of the Euler solve is assembled from the global row --
// so the two halves may run on different waves (k_fly hands the last substeps of a step out in halves).
// Returns true when the call was an auto-reset (the step is complete then).
// io: a callable that returns the step's StepIO (fb_types.hpp) -- the action, the output rows and, for the kernels that have them, the environment's rows of the applied-force arrays
// (FORCES, k_step_forces, fb_forces.hpp: every substep and a forward evaluation read them, the forward pass of a reset does not) and its
// coefficient block, the qpos addresses and its row of FB_QFRC_LAW (LAW, k_step_law, fb_law.hpp: read and written where the forces are read,
// zeroed by the forward pass of a reset).
//
// The interpreter keeps NO descriptor of its own: `wc` (a copy of the caller's descriptor, in memory) is handed to the stages by reference,
// the rows of `io` are formed where a stage that takes them is called, and every pass over the environment's data sits inside a stage -- the right-hand sides of the two solves in d_factor, the
// qacc_smooth copy in s_project_constraint, the sensor accumulation and the progress count in s_velocity, the zero fill of a reset's pass in
// s_actuation_zero.  Code that ran inline between the calls kept the descriptor's pointers alive across EVERY call, in scalar registers the
// kernel does not have: they were saved to vector lanes, and those to scratch, around each stage.
template <typename real, bool FORCES = false, bool LAW = false, typename IO>
__device__ __forceinline__ bool d_run(const DevModel<real>& M, const WS<real>& wc, const IO& io, int env, int mode, int nsub_arg, int nslot, int* sched,
                      int lane, int tk = -1, int only = -1) {
  // every selector of the stage machine is wave-uniform: say so (v_readfirstlane), otherwise the interpreter's state lives in
  // VGPRs + saved exec masks across every stage call and counts against the register budget of all stages
  mode = uniform_int(mode); nsub_arg = uniform_int(nsub_arg); tk = uniform_int(tk); only = uniform_int(only);
#if defined(FB_PROFILE) && !defined(FB_EMULATE)
  const WS<real> w = ws_uniform(wc, M);          // (the PROF() markers add to the environment's counters)
#endif
  const bool tk_first = tk < 0 || (tk & 1), tk_last = tk < 0 || (tk & 2), tk_half_a = tk >= 0 && (tk & 4), tk_half_b = tk >= 0 && (tk & 8);
  // Round 6 (+0.5 %, profiles/r6/ab_stage_priority.txt): issue priority by STAGE CLASS.  The stages that are chains of memory round trips with a few hundred
  // instructions between them (actuation, factorisations, solves, sensors, integration, kinematics, inertias, constraint rows, velocities) run at
  // max(ticket priority, FB_LAT_PRIO); the three stages that do nothing but issue (projection, solver, collision) at the ticket's own priority.
  const int base_prio_ = uniform_int((tk >= 0 && (tk & 16)) ? 3 : 0);
#define ST_LAT() FB_SETPRIO(base_prio_ > FB_LAT_PRIO ? base_prio_ : FB_LAT_PRIO)
#define ST_ISS() FB_SETPRIO(base_prio_)
  int parts = 15;
  bool resetting = (mode == MODE_RESET) || (mode == MODE_STEP && tk_first && uniform_int(ws_uniform(wc, M).istate()[IS_RESET_NEXT]) != 0);
  bool env_logic = (mode == MODE_STEP) || (mode == MODE_RESET);
  bool actuate = true, damp = false, half = false;
  int nsub = uniform_int(tk >= 0 ? 1 : ((mode == MODE_SUBSTEP) ? nsub_arg : M.nsubstep)), sub = 0;
  int pc, ret = ST_DONE, fret = ST_DONE;
  if (only >= 0) {
    // one stage of a control step (profiling): the host walks the stage sequence of d_run itself
    resetting = false; env_logic = true; nsub = 1;
    damp = (only >> 8) & 1; half = (only >> 9) & 1; parts = (only >> 12) & 15; if (parts == 0) parts = 15;
    pc = only & 0xff;
    if (pc == ST_PRE) { s_pre(M, wc, io().action, lane); return false; }
    if (pc == ST_POST) { const StepIO<real> o = io(); s_post(M, wc, false, o.obs, o.reward, o.discount, o.step_type, lane); return false; }
  } else
  if (resetting) {
    s_init(M, wc, env, lane);
    actuate = false; pc = ST_KIN;
  } else if (mode == MODE_FORWARD) {
    pc = ST_KIN;
  } else {
    PROF_BEGIN();
    if (mode == MODE_STEP && tk_first) s_pre(M, wc, io().action, lane);
    PROF(27);
    pc = (nsub > 0) ? (tk_half_b ? ST_EULER_PRE : ST_ACT) : ST_DONE;
  }
  bool single_pass = resetting || (mode == MODE_FORWARD);     // KIN..COLL then ACT..SENS once, no integration
  if (only >= 0) single_pass = false;
  while (pc != ST_DONE) {
    switch (pc) {
      case ST_ACT: {
        PROF_BEGIN();
        ST_LAT();
        if (actuate) s_actuation(M, wc, lane);      // (leaves qfrc_actuator in the solve vector lx as well as in the global row)
        else s_actuation_zero(M, wc, lane);
        PROF(P_ACT);
        pc = ST_ACC_PRE; break; }
      case ST_ACC_PRE: {
        // M is factorised HERE, not behind the inertia stage: the right-hand side of the smooth-acceleration solve is known
        // now, and the factorisation carries it along (d_factor: x leaves as L^-T x), so the solve is its root-to-leaf half
        // only.  The constraint projection, the factor's first consumer, follows.  Nothing LDS-resident crosses a launch
        // boundary any more (the factor and the Delassus matrix used to be parked in the global row between control steps).
        // (qfrc_smooth = lx = qfrc_passive - qfrc_bias + lx is the first thing that factorisation does: d_factor, damp = false)
        if constexpr (LAW) { const StepIO<real> o = io(); s_control_law(M, wc, o.law_coef, o.law_qadr, o.law_out, resetting, lane); }                                    // lx (= this substep's qfrc_actuator) += u, FB_QFRC_LAW = u (a reset: zeroed)
        if constexpr (FORCES) { if (!resetting) { const StepIO<real> o = io(); s_applied_forces(M, wc, o.qfrc_app, o.xfrc_app, lane); } }                     // lx += qfrc_applied + J' xfrc_applied
        damp = false; fret = ST_ACC_SOLVE; pc = ST_FACTOR; break; }
      case ST_ACC_SOLVE:
        half = true; ret = ST_ACC_POST; pc = ST_SOLVE; break;
      case ST_SOLVE: {
        PROF_BEGIN();
        d_solve(M, wc, half, lane);
        PROF(P_ACC);
        half = false;
        pc = ret; break; }
      case ST_ACC_POST: {
        PROF_BEGIN();
        ST_ISS();
        s_project_constraint(M, wc, parts & 3, lane);               // (qacc_smooth = lx first)
        PROF(P_PROJ);
        pc = ST_CONSTR_A; break; }
      case ST_CONSTR_A: {
        bool need = uniform_int(s_constraint_a(M, wc, lane) ? 1 : 0) != 0;
        ret = ST_CONSTR_B; pc = need ? ST_SOLVE : ST_CONSTR_B; break; }
      case ST_CONSTR_B: {
        PROF_BEGIN();
        ST_LAT();
        s_constraint_b(M, wc, lane);
        PROF(25);
        pc = ST_SENS; break; }
      case ST_SENS: {
        PROF_BEGIN();
        if constexpr (FORCES) s_sensor_acc_forces(M, wc, resetting ? (const real*)nullptr : io().xfrc_app, lane);
        else s_sensor_acc(M, wc, lane);
        PROF(P_SENS);
        pc = (single_pass || tk_half_a) ? ST_DONE : ST_EULER_PRE; break; }
      case ST_EULER_PRE: {
        // the factor of M is dead after the constraint solve: its LDS slot is reused for M + h*D
        // (lx = qfrc_smooth + qfrc_constraint is the first thing that factorisation does: d_factor, damp = true)
        damp = true; fret = ST_EULER_SOLVE; pc = ST_FACTOR; break; }
      case ST_FACTOR: {
        PROF_BEGIN();
        d_factor(M, wc, damp, lane);
        PROF(P_FACTOR);
        pc = fret; break; }
      case ST_EULER_SOLVE:
        half = true; ret = ST_EULER_POST; pc = ST_SOLVE; break;
      case ST_EULER_POST: {
        PROF_BEGIN();
        s_integrate(M, wc, lane);
        PROF(P_EULER);
        pc = ST_KIN; break; }
      case ST_KIN: {
        PROF_BEGIN();
        if (parts & 1) s_kinematics(M, wc, lane);
        PROF(P_KIN);
        if (parts & 2) s_com_pos(M, wc, lane);
        PROF(P_COMPOS);
        if (parts & 4) s_crb(M, wc, lane);
        PROF(P_CRB);
        pc = ST_COLL; break; }
      case ST_COLL: {
        PROF_BEGIN();
        ST_ISS();
        if (parts & 1) s_collision(M, wc, lane);
        PROF(P_COLL);
        ST_LAT();
        if (parts & 2) s_make_constraint(M, wc, lane);
        PROF(P_MAKEC);
        // The stage closes the substep (s_velocity): the sensors go to the control step's accumulators, and -- tail-aware issue priority --
        // the launch ends when its slowest environment ends, and every environment is resident from the start, so a wave that trails
        // the others is on the critical path.  Each wave counts itself into the substep's progress counter; the more waves were there
        // before it, the higher its priority for the next substep.
        if (parts & 4) {
          const bool closes = !single_pass;
          const int prio = uniform_int(s_velocity(M, wc, closes && env_logic, (closes && sched && sub < FB_NSCHED) ? sched + sub : (int*)nullptr, nslot, lane));
          if (prio >= 0) FB_SETPRIO(prio);
        }
        PROF(P_VEL);
        pc = single_pass ? ST_ACT : ST_SUBEND; break; }
      case ST_SUBEND: {
        sub++;
        pc = (sub < nsub) ? ST_ACT : ST_DONE; break; }
      default: pc = ST_DONE;
    }
    if (only >= 0) break;
  }
  if (only >= 0) return false;
  PROF_BEGIN();
  if (env_logic && (tk_last || resetting)) { const StepIO<real> o = io(); s_post(M, wc, resetting, o.obs, o.reward, o.discount, o.step_type, lane); }
  PROF(28);
  return resetting;
}
