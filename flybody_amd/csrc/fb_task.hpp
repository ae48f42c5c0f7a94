// The task layer: what an environment is beyond its physics.  A task (FB_TASK_*, fb_types.hpp) supplies three hooks -- episode init,
// before_step, and the reward / termination predicate of after_step.  Everything the reference keeps in one base class
// (flybody/tasks/base.py:206-225: step counter, termination -> step type and discount, observation) and everything the tasks' hooks
// have in common is stated once here; d_task_init / d_task_pre / d_task_post dispatch on the task id.
#pragma once
#include "fb_types.hpp"
#include "fb_math.hpp"
#include "fb_smooth.hpp"      // SYNC

// ------------------------------------------------------------------ the episode clock
// MuJoCo's d->time: a double that every substep advances by the model's timestep -- at EITHER precision.  The clock decides, it does not
// enter the physics: which dataset frame the reward is scored against and whether the trajectory has ended (clock_step), and the time
// limit (d_post_end).  Kept in `real` an FP32 build decided differently from FP64 and MuJoCo: its sum of 2e-4 falls half a control step
// behind after 5.4 s, so that walk_imitation scored the reward against the previous frame on 2285 of an episode's 5000 steps, and three of
// the four tasks ended their time-limited episodes one step off.  The slot (simtime) is two reals wide and starts its own cache line, so
// the double is aligned in the FP32 arena too; field FB_TIME reads and writes it.
template <typename real> FBD double& sim_clock(const WS<real>& w) { return *(double*)w.simtime(); }
// the control step the clock stands at (the reference's round(time / control_timestep))
template <typename real> FBD int clock_step(const DevModel<real>& M, const WS<real>& w) { return (int)floor(sim_clock(w) / M.clock_control_timestep + 0.5); }

// ------------------------------------------------------------------ reference trajectory of an environment
// inference mode: one root track shared by all environments (fb_batch_set_reference); training mode: the snippet the
// environment picked from the dataset at episode start, shifted to start at x = y = 0 (trajectory_loaders.py:249)
template <typename real> struct RefView { const real *q, *v; int stride, vstride, T, episode_steps; real sx, sy; };
template <typename real> FBD RefView<real> ref_view(const DevModel<real>& M, const WS<real>& w) {
  RefView<real> r;
  if (M.ds_qpos) {
    r.stride = 7 + M.ds_nj; r.vstride = 6 + M.ds_nj;
    r.q = M.ds_qpos + (size_t)w.istate()[IS_DS_OFF]*r.stride; r.v = M.ds_qvel + (size_t)w.istate()[IS_DS_OFF]*r.vstride;
    r.T = w.istate()[IS_DS_LEN];
    r.episode_steps = w.istate()[IS_EPSTEPS]; r.sx = w.dsshift()[0]; r.sy = w.dsshift()[1];
  } else { r.q = M.ref_qpos; r.v = M.ref_qvel; r.stride = 7; r.vstride = 6; r.T = M.T; r.episode_steps = M.episode_steps; r.sx = 0; r.sy = 0; }
  return r;
}
template <typename real> FBD void ref_vel(const RefView<real>& r, int idx, real* out6) {
  if (idx >= r.T) idx = r.T - 1;
  const real* p = r.v + (size_t)idx*r.vstride;
  for (int c = 0; c < 6; c++) out6[c] = p[c];
}
template <typename real> FBD void ref_root(const RefView<real>& r, int idx, real* out7) {
  if (idx >= r.T) idx = r.T - 1;
  const real* p = r.q + (size_t)idx*r.stride;
  out7[0] = p[0] - r.sx; out7[1] = p[1] - r.sy;
  for (int c = 2; c < 7; c++) out7[c] = p[c];
}

// ------------------------------------------------------------------ observation vector (engine.observation_layout)
template <typename real> FBD void d_pack_obs(const DevModel<real>& M, const WS<real>& w, const real* sm, float* obs, int lane) {
  int thorax = M.site_bodyid[M.site_thorax];
  real R[9];
  { const real tq[4] = {w.xquat()[4*thorax], w.xquat()[4*thorax + 1], w.xquat()[4*thorax + 2], w.xquat()[4*thorax + 3]}; quat2mat(R, tq); }   // (the kinematics stage stores quaternions only)
  const real* tp = w.xpos() + 3*thorax;
  int step = w.istate()[IS_STEP];
  int o = 0;
  if (lane < 3) obs[o + lane] = (float)sm[lane];
  o += 3;
  for (int i = lane; i < M.na; i += FB_WAVE) obs[o + i] = (float)w.act()[i];
  o += M.na;
  for (int k = lane; k < M.napp; k += FB_WAVE) {
    real dif[3], e[3]; sub3(dif, w.sxpos() + 3*M.app_sites[k], tp);
    mulmatT3(e, R, dif);
    for (int q = 0; q < 3; q++) obs[o + 3*k + q] = (float)e[q];
  }
  o += 3*M.napp;
  if (M.task == FB_TASK_WALK_ON_BALL) { if (lane < 3) obs[o + lane] = (float)w.qvel()[M.nv - 3 + lane]; o += 3; }      // ball_qvel (walk_on_ball.py:84-90)
  for (int k = lane; k < 3*M.nforce; k += FB_WAVE) obs[o + k] = (float)sm[9 + k];
  o += 3*M.nforce;
  if (lane < 3) obs[o + lane] = (float)sm[3 + lane];
  o += 3;
  for (int k = lane; k < M.nobsjnt; k += FB_WAVE) {
    int j = M.obs_jnt[k];
    obs[o + k] = (float)w.qpos()[M.jnt_qposadr[j]];
    obs[o + M.nobsjnt + k] = (float)w.qvel()[M.jnt_dofadr[j]];
  }
  o += 2*M.nobsjnt;
  int nf = (M.task == FB_TASK_WALK_ON_BALL || M.task == FB_TASK_TEMPLATE) ? 0 : M.future_steps + 1;        // walk_on_ball and template_task have no reference observables
  const RefView<real> rv = ref_view(M, w);
  for (int k = lane; k < nf; k += FB_WAVE) {
    real rr[7]; ref_root(rv, step + k, rr);
    real dif[3], e[3]; sub3(dif, rr, w.qpos());
    mulmatT3(e, R, dif);
    for (int q = 0; q < 3; q++) obs[o + 3*k + q] = (float)e[q];
  }
  o += 3*nf;
  if (nf > 0) {
    const real* q = w.qpos() + 3;
    real n2 = q[0]*q[0] + q[1]*q[1] + q[2]*q[2] + q[3]*q[3];
    real qi[4] = {q[0]/n2, -q[1]/n2, -q[2]/n2, -q[3]/n2};
    for (int k = lane; k < nf; k += FB_WAVE) {
      real rr[7]; ref_root(rv, step + k, rr);
      real e[4]; mulquat(e, qi, rr + 3);
      for (int c = 0; c < 4; c++) obs[o + 4*k + c] = (float)e[c];
    }
  }
  o += 4*nf;
  for (int k = lane; k < M.ntouch; k += FB_WAVE) obs[o + k] = (float)sm[9 + 3*M.nforce + k];
  o += M.ntouch;
  if (lane < 3) { obs[o + lane] = (float)sm[6 + lane]; obs[o + 3 + lane] = (float)R[6 + lane]; }
}

// ------------------------------------------------------------------ small helpers of the hooks
// first-minimum argmin of |x - v[i]| (mod1: of the fractional part of v[i]) over a table, searched by the 64 lanes cooperatively
template <typename real> FBD int wave_argmin_absdiff(const real* v, int n, real x, bool mod1, int lane) {
  real best = (real)1e30; int bi = 0x7fffffff;
  for (int i = lane; i < n; i += FB_WAVE) {
    real a = v[i];
    if (mod1) a = a - floor(a);
    real e = fabs(x - a);
    if (e < best) { best = e; bi = i; }
  }
  for (int m = 32; m >= 1; m >>= 1) {
    real ob = shfl_xor_any(best, m); int oi = __shfl_xor(bi, m, 64);
    if (ob < best || (ob == best && oi < bi)) { best = ob; bi = oi; }
  }
  return bi;
}
FBD float hash_uniform(unsigned seed, unsigned env, unsigned episode) {
  unsigned x = seed*0x9E3779B9u ^ (env*0x85EBCA6Bu) ^ (episode*0xC2B2AE35u);
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return (float)(x >> 8) * (1.0f/16777216.0f);
}
template <typename real> FBD real tolerance_linear(real x, real margin) { real d = fabs(x)/margin; return d < 1 ? 1 - d : (real)0; }
template <typename real> FBD real quat_dist_short_arc(const real* a, const real* b) {
  real na = sqrt(a[0]*a[0] + a[1]*a[1] + a[2]*a[2] + a[3]*a[3]), nb = sqrt(b[0]*b[0] + b[1]*b[1] + b[2]*b[2] + b[3]*b[3]);
  real dt = (a[0]*b[0] + a[1]*b[1] + a[2]*b[2] + a[3]*b[3])/(na*nb);
  real x = 2*dt*dt - 1; if (x > 1) x = 1;
  return acos(x);
}
// an action entry as the tasks read it: NaN counts as 0 (fruitfly.py:532-544)
FBD float sane_action(const float* action, int k) { float a = action[k]; return a != a ? 0.f : a; }

// ------------------------------------------------------------------ episode start: what every task's init does
// the environment at rest (v0: but for this linear velocity of the root): velocities, accelerations, the solver's warm start, activations and controls
template <typename real> FBD void d_clear_motion(const DevModel<real>& M, const WS<real>& w, int lane, const real* v0 = nullptr) {
  for (int i = lane; i < M.nv; i += FB_WAVE) { w.qvel()[i] = (v0 && i < 3) ? v0[i] : (real)0; w.qacc()[i] = 0; w.qacc_ws()[i] = 0; }
  for (int i = lane; i < M.nu; i += FB_WAVE) w.ctrl()[i] = 0;
  for (int i = lane; i < M.na; i += FB_WAVE) { w.act()[i] = 0; w.act_dot()[i] = 0; }
}
// joints folded to their spring reference: the wings of a walking fly (fruitfly.py:390-405), the legs of a flying one (flight_imitation.py:142-144)
template <typename real> FBD void d_retract(const DevModel<real>& M, const WS<real>& w, GP<const int> jnt, int n, int lane) {
  for (int k = lane; k < n; k += FB_WAVE) { int qa = M.jnt_qposadr[jnt[k]]; w.qpos()[qa] = M.qpos_spring[qa]; }
}
template <typename real> FBD void d_reset_counters(const WS<real>& w, int lane) {
  if (lane == 0) { w.istate()[IS_STEP] = 0; w.istate()[IS_RESET_NEXT] = 0; sim_clock(w) = 0; }
}
// a walker's episode starts (qpos is set): at rest, wings folded (fruitfly.py:390-405)
template <typename real> FBD void d_start_walker(const DevModel<real>& M, const WS<real>& w, int lane) {
  d_clear_motion(M, w, lane); SYNC(); d_retract(M, w, M.wing_jnt, 6, lane); d_reset_counters(w, lane); SYNC();
}
// dataset mode: the trajectory of this episode out of ds_select, a pure function of (seed, global environment id, episode) where the
// reference draws from a RandomState (walk_imitation.py:92-111, trajectory_loaders.py:110-141); rows [off, off + len) of the dataset
struct Snippet { int off, len; };
template <typename real> FBD Snippet pick_trajectory(const DevModel<real>& M, int env, int episode) {
  double u = (double)hash_uniform(M.seed, (unsigned)(M.ds_env_base + env), (unsigned)episode);
  int k = (int)(u*M.ds_nselect); if (k >= M.ds_nselect) k = M.ds_nselect - 1;
  int traj = M.ds_select[k];
  int off = M.ds_offset[traj];
  return {off, M.ds_offset[traj + 1] - off};
}

// ------------------------------------------------------------------ after_step: what every task's post does (base.py:206-225)
// Prologue: sensor means over the substeps, the step counter, |qacc|^2.  prev = the step counter before this control step.
template <typename real> struct PostHead { int prev; real qn; };
template <typename real> FBD PostHead<real> d_post_begin(const DevModel<real>& M, const WS<real>& w, int lane) {
  if (lane < FB_NSENS) w.sens_acc()[lane] = w.sens_acc()[lane] / (real)M.nsubstep;
  int prev = w.istate()[IS_STEP];
  SYNC();
  if (lane == 0) w.istate()[IS_STEP] = prev + 1;
  real qn = 0;
  for (int i = lane; i < M.nv; i += FB_WAVE) qn += w.qacc()[i]*w.qacc()[i];
  qn = wave_sum(qn);
  SYNC();
  return {prev, qn};
}
// physics error: the accelerations diverged or are NaN (every task's termination predicate has this clause)
template <typename real> FBD bool physics_error(real qn) { return (sqrt(qn) > (real)1e14) || (qn != qn); }
// What a task's post hook decides.  term: the episode terminates; traj_end: ... because the reference ran out, which is not a failure
// and keeps the discount at 1 (base.py:212-225).
template <typename real> struct Outcome { real reward; bool term, traj_end; };
// Epilogue: step type, discount, observation.  first: this is the FIRST step of an episode (the environment was just reset): the
// observation shows the sensors themselves, not their means; reward 0, discount 1, and IS_RESET_NEXT is the caller's business.
template <typename real> FBD void d_post_end(const DevModel<real>& M, const WS<real>& w, bool first, const Outcome<real>& out,
                    float* obs, float* reward, float* discount, int* step_type, int lane) {
  const bool terminating = out.term || (sim_clock(w) >= M.time_limit);
  const int type = first ? 0 : (terminating ? 2 : 1);
  d_pack_obs(M, w, first ? w.sens() : w.sens_acc(), obs, lane);
  if (lane == 0) {
    *reward = (float)out.reward;
    *discount = (out.term && !out.traj_end) ? 0.0f : 1.0f;
    *step_type = type;
    w.istate()[IS_STEP_TYPE] = type;
    if (!first) w.istate()[IS_RESET_NEXT] = terminating ? 1 : 0;
  }
  SYNC();
}

// ------------------------------------------------------------------ walk_imitation
// episode init (walk_imitation.py:112-136, fruitfly.py:390-405)
template <typename real> FBD void d_walk_init(const DevModel<real>& M, const WS<real>& w, int env, int lane) {
  if (M.ds_qpos) {
    // initialize_episode_mjcf (walk_imitation.py:92-111): the snippet of this episode
    int episode = w.istate()[IS_EPISODE];
    const Snippet s = pick_trajectory(M, env, episode);
    const real* q0 = M.ds_qpos + (size_t)s.off*(7 + M.ds_nj);
    for (int i = lane; i < M.nq; i += FB_WAVE) w.qpos()[i] = (i < 2) ? (real)0 : ((i < 7) ? q0[i] : M.qpos0[i]);
    SYNC();
    for (int j = lane; j < M.ds_nj; j += FB_WAVE) w.qpos()[M.jnt_qposadr[M.ds_jid[j]]] = q0[7 + j];     // every mocap joint (:118)
    int snippet = s.len - M.future_steps - 1;
    if (lane == 0) {
      w.istate()[IS_DS_OFF] = s.off; w.istate()[IS_DS_LEN] = s.len; w.istate()[IS_EPISODE] = episode + 1;
      w.istate()[IS_EPSTEPS] = M.max_episode_steps < snippet ? M.max_episode_steps : snippet;
      w.dsshift()[0] = q0[0]; w.dsshift()[1] = q0[1];
    }
  } else
  for (int i = lane; i < M.nq; i += FB_WAVE) w.qpos()[i] = (i < 7) ? M.ref_qpos[i] : M.qpos0[i];
  d_start_walker(M, w, lane);
}

// before_step (walk_imitation.py:138-150, fruitfly.py:532-544); walk_on_ball's as well
template <typename real> FBD void d_walk_pre(const DevModel<real>& M, const WS<real>& w, const float* action, int lane) {
  for (int k = lane; k < M.nu; k += FB_WAVE) w.ctrl()[M.action_to_ctrl[k]] = (real)sane_action(action, k);
  if (lane < FB_NSENS) w.sens_acc()[lane] = 0;
  SYNC();
}

// training-mode reward of walk_imitation (walk_imitation.py:152-177): DeepMimic factors of tasks/rewards.py:37-116 on
// (CoM, mocap qvel, egocentric root->site vectors, egocentric joint orientation quaternions) x (20,1,1,1) and the
// wing-retraction tolerance.  One lane per mocap joint / site, four wave reductions.
template <typename real> FBD real d_walk_training_reward(const DevModel<real>& M, const WS<real>& w, int step, int lane) {
  const int nj = M.ds_nj, ns = M.ds_ns;
  int len = w.istate()[IS_DS_LEN];
  if (step >= len) step = len - 1;
  size_t row = (size_t)w.istate()[IS_DS_OFF] + step;
  const real* rq = M.ds_qpos + row*(7 + nj); const real* rvel = M.ds_qvel + row*(6 + nj);
  const real* r2s = M.ds_r2s + row*3*ns; const real* rjq = M.ds_jq + row*4*nj;
  const real* root_quat = w.qpos() + 3;
  real n2 = root_quat[0]*root_quat[0] + root_quat[1]*root_quat[1] + root_quat[2]*root_quat[2] + root_quat[3]*root_quat[3];
  real qinv[4] = {root_quat[0]/n2, -root_quat[1]/n2, -root_quat[2]/n2, -root_quat[3]/n2};
  real d_com = 0, d_qvel = 0, d_site = 0, d_quat = 0;
  if (lane < 3) { real e = w.qpos()[lane] - (rq[lane] - (lane < 2 ? w.dsshift()[lane] : (real)0)); d_com = e*e; }
  if (lane < 6) { real e = w.qvel()[lane] - rvel[lane]; d_qvel = e*e; }
  if (lane == 0) { real e = quat_dist_short_arc(root_quat, rq + 3); d_quat = e*e; }
  for (int k = lane; k < nj; k += FB_WAVE) {
    int j = M.ds_jid[k];
    real e = w.qvel()[M.jnt_dofadr[j]] - rvel[6 + k]; d_qvel += e*e;
    // joint orientation quaternion (quaternions.py:310-333) of the egocentric joint axis: axis-angle(qpos) * z2vec(axis)
    real ax[3], qz[4], qa[4], jq[4];
    rotvecquat(ax, w.xaxis() + 3*j, qinv);
    real an = norm3(ax);
    real vx = ax[0]/an, vy = ax[1]/an, vz = ax[2]/an;
    real s = sqrt(vx*vx + vy*vy), zang = atan2(s, vz);          // z x v = (-vy, vx, 0)
    real cx = -vy, cy = vx;
    if (s > (real)1e-12) { cx /= s; cy /= s; } else { cx = 1; cy = 0; }
    real zs = sin(zang/2);
    qz[0] = cos(zang/2); qz[1] = cx*zs; qz[2] = cy*zs; qz[3] = 0;
    real ang = w.qpos()[M.jnt_qposadr[j]], sh = sin(ang/2);
    qa[0] = cos(ang/2); qa[1] = vx*sh; qa[2] = vy*sh; qa[3] = vz*sh;
    mulquat(jq, qa, qz);
    real eq = quat_dist_short_arc(jq, rjq + 4*k); d_quat += eq*eq;
  }
  for (int k = lane; k < ns; k += FB_WAVE) {
    real df[3], ego[3];
    sub3(df, w.sxpos() + 3*M.ds_sid[k], w.qpos());
    rotvecquat(ego, df, qinv);                                   // (quat2mat of a quaternion of norm^2 1/n2 is a rotation times 1/n2: undone below, get_egocentric_vec rotates whatever the norm)
    for (int c = 0; c < 3; c++) { real e = ego[c]*n2 - r2s[3*k + c]; d_site += e*e; }
  }
  d_com = wave_sum(d_com); d_qvel = wave_sum(d_qvel); d_site = wave_sum(d_site); d_quat = wave_sum(d_quat);
  const real s_com = (real)0.078487, s_qvel = (real)53.7801, s_site = (real)0.0735, s_quat = (real)1.2247;     // tasks/rewards.py:101-108
  real f0 = (real)20*exp(-(real)0.5/(s_com*s_com)*d_com), f1 = exp(-(real)0.5/(s_qvel*s_qvel)*d_qvel);
  real f2 = exp(-(real)0.5/(s_site*s_site)*d_site), f3 = exp(-(real)0.5/(s_quat*s_quat)*d_quat);
  real rw = 1;
  for (int k = 0; k < 6; k++) { int qa = M.jnt_qposadr[M.wing_jnt[k]]; rw *= tolerance_linear(w.qpos()[qa] - M.qpos_spring[qa], (real)3); }
  if (lane == 0) { w.rfac()[0] = f0; w.rfac()[1] = f1; w.rfac()[2] = f2; w.rfac()[3] = f3; w.rfac()[4] = rw; }
  return f0*f1*f2*f3*rw;
}

// reward / termination (walk_imitation.py:152-203)
template <typename real> FBD Outcome<real> d_walk_post(const DevModel<real>& M, const WS<real>& w, const PostHead<real>& h, int lane) {
  real linvel = norm3(w.sens() + 6), angvel = norm3(w.sens() + 3);
  int tstep = clock_step(M, w);
  const RefView<real> rv = ref_view(M, w);
  real rroot[7]; ref_root(rv, h.prev + 1, rroot);
  real dif[3]; sub3(dif, rroot, w.qpos());
  real com_dist = norm3(dif);
  bool traj_end = (tstep == rv.episode_steps);
  real rew = 1;
  if (M.ds_qpos) rew = d_walk_training_reward(M, w, tstep, lane);
  bool term = (linvel > (real)50) || (angvel > (real)200) || traj_end || (com_dist > M.terminal_com_dist) || physics_error(h.qn);
  return {rew, term, traj_end};
}

// ------------------------------------------------------------------ walk_on_ball (fly_envs.py:158-191, tasks/walk_on_ball.py)
// episode init: default pose with retracted wings (fruitfly.py:390-405); no reference trajectory
template <typename real> FBD void d_ball_init(const DevModel<real>& M, const WS<real>& w, int lane) {
  for (int i = lane; i < M.nq; i += FB_WAVE) w.qpos()[i] = M.qpos0[i];
  d_start_walker(M, w, lane);
}

// reward: ball spinning at (0, -5, 0) rad/s, linear tolerance with margin 6 per component (walk_on_ball.py:62-73);
// termination on sensor velocities / qacc (:75-80), never by a trajectory end
template <typename real> FBD Outcome<real> d_ball_post(const DevModel<real>& M, const WS<real>& w, const PostHead<real>& h, int lane) {
  real linvel = norm3(w.sens() + 6), angvel = norm3(w.sens() + 3);
  const real* bv = w.qvel() + M.nv - 3;
  real r = tolerance_linear(bv[0], (real)6)*tolerance_linear(bv[1] + (real)5, (real)6)*tolerance_linear(bv[2], (real)6);
  bool term = (linvel > (real)50) || (angvel > (real)200) || physics_error(h.qn);
  return {r, term, false};
}

// ------------------------------------------------------------------ template_task (fly_envs.py:194-247, tasks/template_task.py)
// The starting point for a user's own walking task: walk_imitation's walker and physics without a reference trajectory.  Episode init
// (d_template_init) IS d_walk_init's inference branch -- the root pose from row 0 of the "reference" (the factory's init_qpos), every
// other joint at qpos0, d_start_walker -- and the host refuses a dataset for this task (fb_batch_set_walk_dataset), so M.ds_qpos is null
// and d_task_init sends the task through d_walk_init itself: s_init keeps its code.  before_step (d_template_pre) is d_walk_pre.
// reward 1, termination on a physics error only (template_task.py:75-84, base.py:222-225); what a user builds on it is written from
// PyTorch (BatchedFlyEnv reward_fn / termination_fn, fb_batch_end_episode)
template <typename real> FBD Outcome<real> d_template_post(const PostHead<real>& h) { return {(real)1, physics_error(h.qn), false}; }

// ------------------------------------------------------------------ flight_imitation
// episode init (flight_imitation.py:112-144): root pose / linear velocity from the reference, wings from the wing-beat pattern
// generator (flybody/tasks/pattern_generators.py:131-203, one state machine per environment) at a per-episode phase
template <typename real> FBD void d_flight_init(const DevModel<real>& M, const WS<real>& w, int env, int lane) {
  int episode = w.istate()[IS_EPISODE];
  if (M.ds_qpos) {
    // HDF5FlightTrajectoryLoader.get_trajectory (trajectory_loaders.py:110-141): a trajectory out of traj_indices and, with
    // randomize_start_step, a start step in [0, len - 50).  x / y are re-centred on the first row of the slice.
    const Snippet s = pick_trajectory(M, env, episode);
    int start = 0;
    if (M.ds_random_start) {
      double u2 = (double)hash_uniform(M.seed ^ 0x5bd1e995u, (unsigned)(M.ds_env_base + env), (unsigned)episode);
      start = (int)(u2*(s.len - 50)); if (start > s.len - 51) start = s.len - 51; if (start < 0) start = 0;
    }
    int T = s.len - start, lim = (int)floor(M.time_limit / M.clock_control_timestep + 0.5);
    const real* q0 = M.ds_qpos + (size_t)(s.off + start)*7;
    if (lane == 0) {
      w.istate()[IS_DS_OFF] = s.off + start; w.istate()[IS_DS_LEN] = T;
      w.istate()[IS_EPSTEPS] = (T < lim ? T : lim) - (M.future_steps + 1);            // flight_imitation.py:101-105
      // the loader re-centres the CoM track (x, y of the first row -> 0) BEFORE the task converts it to the root joint:
      // the shift is the CoM position of the first row = root + R(quat) com_offset (task_utils.root2com)
      real qn[4] = {q0[3], q0[4], q0[5], q0[6]}, co[3];
      normquat(qn); rotvecquat(co, M.com_offset, qn);
      w.dsshift()[0] = q0[0] + co[0]; w.dsshift()[1] = q0[1] + co[1];
    }
    SYNC();
  }
  const RefView<real> rv = ref_view(M, w);
  real r0[7], v0[6]; ref_root(rv, 0, r0); ref_vel(rv, 0, v0);
  for (int i = lane; i < M.nq; i += FB_WAVE) w.qpos()[i] = (i < 7) ? r0[i] : M.qpos0[i];
  d_clear_motion(M, w, lane, v0);
  SYNC();
  d_retract(M, w, M.leg_jnt, M.nlegjnt, lane);
  real phase0 = (real)hash_uniform(M.seed, (unsigned)(M.ds_env_base + env), (unsigned)episode + 0x40000000u*(M.ds_qpos ? 1u : 0u));
  int fidx = wave_argmin_absdiff((const real*)M.wb_freqs, M.wb_nfreq, M.wb_base_freq, false, lane);
  int o = M.wb_offset[fidx], n = M.wb_offset[fidx + 1] - o;
  int st = wave_argmin_absdiff(M.wb_phase + o, n, phase0, false, lane);
  if (lane < 6) {
    int j = M.wing_jnt[lane];
    real q0 = M.wb_traj[6*(o + st) + lane], q1 = M.wb_traj[6*(o + st + 1) + lane];
    w.qpos()[M.jnt_qposadr[j]] = q0; w.qvel()[M.jnt_dofadr[j]] = (q1 - q0)/M.control_timestep;
  }
  d_reset_counters(w, lane);
  if (lane == 0) { w.istate()[IS_WB_STEP] = st; w.istate()[IS_WB_FREQ] = fidx; w.istate()[IS_EPISODE] = episode + 1; w.wbfreq()[0] = M.wb_base_freq; }
  SYNC();
}

// before_step (flight_imitation.py:146-168): pattern generator step at the requested frequency, wing action
// entries become position-error force commands
template <typename real> FBD void d_flight_pre(const DevModel<real>& M, const WS<real>& w, const float* action, int lane) {
  float au = sane_action(action, M.user_idx);
  real ctrl_freq = M.wb_base_freq*(1 + M.wb_rel_range*(real)au);
  int fidx = w.istate()[IS_WB_FREQ], st = w.istate()[IS_WB_STEP];
  real filt = w.wbfreq()[0];
  int o = M.wb_offset[fidx], n = M.wb_offset[fidx + 1] - o;
  st = (st + 1) % n;
  filt = (M.wb_rate == 0) ? ctrl_freq : filt*M.wb_rate + ctrl_freq*(1 - M.wb_rate);
  int fnew = wave_argmin_absdiff((const real*)M.wb_freqs, M.wb_nfreq, filt, false, lane);
  if (fnew != fidx) {
    real cur = M.wb_phase[o + st]; cur = cur - floor(cur);
    int o2 = M.wb_offset[fnew], n2 = M.wb_offset[fnew + 1] - o2;
    st = wave_argmin_absdiff(M.wb_phase + o2, n2, cur, true, lane);
    fidx = fnew; o = o2;
  }
  SYNC();
  for (int k = lane; k < M.nu; k += FB_WAVE) {
    real v = (real)sane_action(action, k);
    for (int q = 0; q < 6; q++) if (M.wing_act_idx[q] == k) v += M.wb_traj[6*(o + st) + q] - w.qpos()[M.jnt_qposadr[M.wing_jnt[q]]];
    w.ctrl()[M.action_to_ctrl[k]] = v;
  }
  if (lane < FB_NSENS) w.sens_acc()[lane] = 0;
  if (lane == 0) { w.istate()[IS_WB_STEP] = st; w.istate()[IS_WB_FREQ] = fidx; w.wbfreq()[0] = filt; }
  SYNC();
}

// reward / termination (flight_imitation.py:170-212)
template <typename real> FBD Outcome<real> d_flight_post(const DevModel<real>& M, const WS<real>& w, const PostHead<real>& h, int lane) {
  // ghost pose: set from ref[prev] before the physics and advanced by its velocity over the control step
  // (its ~1e-8 cm gravity sag is neglected)
  real gp[3], gq[4], qr[4], tmpq[4];
  const RefView<real> rview = ref_view(M, w);
  real rp[7], rv[6]; ref_root(rview, h.prev, rp); ref_vel(rview, h.prev, rv);
  for (int k = 0; k < 3; k++) gp[k] = rp[k] + M.control_timestep*rv[k];
  for (int k = 0; k < 4; k++) gq[k] = rp[3 + k];
  {
    real ax[3] = {rv[3], rv[4], rv[5]};
    real nn = normalize3(ax);
    axisangle2quat(qr, ax, nn*M.control_timestep);
    normquat(gq); mulquat(tmpq, gq, qr); normquat(tmpq);
  }
  real off[3], dif[3];
  rotvecquat(off, M.com_offset, tmpq);
  for (int k = 0; k < 3; k++) dif[k] = gp[k] + off[k] - w.com()[k];
  real r_disp = tolerance_linear((real)norm3(dif), (real)0.4);
  real rnext[7]; ref_root(rview, h.prev + 1, rnext);              // (clamped to the last row of the snippet)
  const real* q = w.qpos() + 3;
  real n2 = q[0]*q[0] + q[1]*q[1] + q[2]*q[2] + q[3]*q[3];
  real qi[4] = {q[0]/n2, -q[1]/n2, -q[2]/n2, -q[3]/n2}, dq[4];
  mulquat(dq, qi, rnext + 3);
  real nq = sqrt(dq[0]*dq[0] + dq[1]*dq[1] + dq[2]*dq[2] + dq[3]*dq[3]);
  real x = 2*(dq[0]/nq)*(dq[0]/nq) - 1; if (x > 1) x = 1;
  real r_quat = tolerance_linear((real)acos(x), (real)3.14159265358979323846);
  int thorax = M.site_bodyid[M.site_thorax];
  real height = w.xpos()[3*thorax + 2];
  real cd[3]; sub3(cd, rnext, w.qpos());
  int tstep = clock_step(M, w);
  bool traj_end = (tstep == rview.episode_steps);
  // enabled legs: reward for keeping them retracted (flight_imitation.py:196-203; 1 when the legs are disabled)
  real r_legs = 1;
  for (int k = 0; k < M.nlegjnt; k++) { int qa = M.jnt_qposadr[M.leg_jnt[k]]; r_legs *= tolerance_linear(w.qpos()[qa] - M.qpos_spring[qa], (real)4); }
  bool term = (height < (real)0.2) || (norm3(cd) > M.terminal_com_dist) || traj_end || physics_error(h.qn);
  return {r_disp*r_quat*r_legs, term, traj_end};
}

// ------------------------------------------------------------------ one dispatch per hook
// env.reset(), before the forward pass with actuation disabled that follows it (dm_control Physics.after_reset)
template <typename real> FBD void d_task_init(const DevModel<real>& M, const WS<real>& w, int env, int lane) {
  if (M.task == FB_TASK_FLIGHT_IMITATION) d_flight_init(M, w, env, lane); else if (M.task == FB_TASK_WALK_ON_BALL) d_ball_init(M, w, lane); else d_walk_init(M, w, env, lane);      // (template_task: the walker's inference branch)
}
template <typename real> FBD void d_task_pre(const DevModel<real>& M, const WS<real>& w, const float* action, int lane) {
  if (M.task == FB_TASK_FLIGHT_IMITATION) d_flight_pre(M, w, action, lane); else d_walk_pre(M, w, action, lane);      // (walk_on_ball, template_task: the walker's)
}
// first: the environment was reset in this call (s_init and the forward pass ran instead of a control step)
template <typename real> FBD void d_task_post(const DevModel<real>& M, const WS<real>& w, bool first, float* obs, float* reward, float* discount, int* step_type, int lane) {
  Outcome<real> out = {0, false, false};
  if (!first) {
    const PostHead<real> h = d_post_begin(M, w, lane);
    if (M.task == FB_TASK_FLIGHT_IMITATION) out = d_flight_post(M, w, h, lane); else if (M.task == FB_TASK_WALK_ON_BALL) out = d_ball_post(M, w, h, lane);
    else if (M.task == FB_TASK_TEMPLATE) out = d_template_post(h); else out = d_walk_post(M, w, h, lane);
  }
  d_post_end(M, w, first, out, obs, reward, discount, step_type, lane);
}
