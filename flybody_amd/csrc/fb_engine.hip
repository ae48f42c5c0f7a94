// libflybody_hip.so -- host side of the batched fly-physics engine and its C-ABI
// (include/flybody_engine.h).  One HIP workgroup of 64 threads (one CDNA4 wavefront) owns one
// environment; a single kernel launch advances every environment by one control step
// (nsubstep physics steps + observation/reward/termination epilogue).
#ifdef FB_EMULATE
#include "emu/hip_emu.hpp"
#else
#include <hip/hip_runtime.h>
#endif
#include <algorithm>
#include <array>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>
#if defined(FB_EMULATE) && defined(FB_STATS)
extern "C" { long long fb_stats[64]; }
#endif

#include "../../include/flybody_engine.h"
#include "fb_step.hpp"
#include "fb_ik.hpp"
#include "fb_inverse.hpp"
#include "fb_deriv.hpp"
#include "fb_rollout.hpp"
#include "fb_riccati.hpp"
#include "fb_ray.hpp"
#include "fb_host.hpp"                    // g_err / fail / HIPCHK, DevBuf, DevEvent
#include "fb_model.hpp"                   // fb_model and the C-ABI's model entry points

extern "C" const char* fb_last_error(void) { return g_err.c_str(); }

// Build identity of this shared object (the GPU test log / smoke() print it, so a log shows which binary ran)
#ifndef FB_BUILD_ID
#define FB_BUILD_ID "unversioned"
#endif
extern "C" const char* fb_version(void) {
#ifdef FB_EMULATE
  return "flybody_engine 2 (host emulation build, " FB_BUILD_ID ")";
#else
  return "flybody_engine 2 (gfx950, " FB_BUILD_ID ")";
#endif
}


// ------------------------------------------------------------------ kernels
template <typename real>
struct Batch {
  real* rarena; int* iarena;
  float *obs, *reward, *discount; int* step_type;
  int n_env, nobs;
  int* sched;                 // [FB_NSCHED] progress counters, zeroed before every launch
  int* cost;                  // [n_env] duration of the environment's last control step (wall-clock ticks), input of k_order
  int* tick;                  // substep scheduler (null = off): [nq][16] ticket counters, one per XCD, zeroed before every launch
  int* done;                  // ... [n_env] substeps of the running control step completed, zeroed before every launch
  int nq;                     // ... number of XCDs (ticket queues)
  int* sched_err;             // ... [1] tickets abandoned because the wait for the predecessor substep hit its cap (sticky; fb_batch_synchronize / fb_batch_get fail)
  const int* torder;          // ... [nq][ceil(n_env / nq)] environments of every XCD's share in the order their tickets are handed out (k_ticket_order:
                              //     largest constraint system of the previous step first); null = by id
  real* park;                 // MODE_STAGE (profiling): [n_env][POOL] the LDS pool between two single-stage launches
};

#ifndef FB_TICKET_SPLIT
#define FB_TICKET_SPLIT 0                 // final substeps of a control step handed out as two half tickets (0: whole substeps only; measured: profiles/r6/ab_tickets.txt)
#endif
#ifndef FB_SCHED_SPIN_CAP
#define FB_SCHED_SPIN_CAP (1 << 22)       // x s_sleep(32): seconds.  (Test builds lower it to provoke the abandon path.)
#endif
// XCD this wave runs on (HW_REG_XCC_ID, bits 3:0)
__device__ __forceinline__ int fb_xcc_id() {
#ifdef FB_EMULATE
  return 0;
#else
  return (int)(__builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11)) & 15u);
#endif
}
#ifndef FB_EMULATE
__global__ void k_probe_xcc(unsigned* mask) { if (threadIdx.x == 0) atomicOr(mask, 1u << fb_xcc_id()); }
#endif


// Grouped batch (fb_batch_create_group): Mp is an ARRAY of n_models model structs that share one tree, and environment e is
// stepped with Mp[env_model[e]].
struct GroupArgs { const int* env_model = nullptr; int n_models = 1; };

// The model an environment is stepped with.  MODELS off: the launch's one model.  On: element env_model[env] of the array, the id made
// wave-uniform (v_readfirstlane) and clamped with scalar compares, so that the struct is addressed through the constant path like the
// single model (as_constant: its fields stay scalar loads) and an id written out of range through the device pointer never becomes a
// wild pointer (`bad`: raise WARN_MODEL_ID).
template <typename real, bool MODELS>
__device__ __forceinline__ const DevModel<real>& model_of_env(const DevModel<real>* Mp, const DevModel<real>& M0, const GroupArgs& G, int env, bool& bad) {
  if constexpr (MODELS) {
    const int id = uniform_int(G.env_model[env]), n = uniform_int(G.n_models);
    const int k = id < 0 ? 0 : (id >= n ? n - 1 : id);
    bad = k != id;
    return as_constant(Mp[k]);
  } else { (void)Mp; (void)G; (void)env; bad = false; return M0; }
}

// The rows of one environment's step (StepIO, fb_types.hpp), formed from the kernel's arguments: action and outputs, FORCES: the two force
// rows, LAW: the law's rows.  The sizes are those of the launch's model M (element 0 of a group: its models agree in them).
template <typename real, bool FORCES, bool LAW>
__device__ __forceinline__ StepIO<real> step_io(const DevModel<real>& M, const Batch<real>& B, const float* action, const ForceArgs<real>& F, const LawArgs<real>& L, int env) {
  StepIO<real> o = {action ? action + (size_t)env*M.nact : nullptr, B.obs ? B.obs + (size_t)env*B.nobs : nullptr, B.reward + env, B.discount + env, B.step_type + env,
                    nullptr, nullptr, nullptr, nullptr, nullptr};
  if constexpr (FORCES) { o.qfrc_app = F.qfrc_applied + (size_t)env*M.nv; o.xfrc_app = F.xfrc_applied + (size_t)env*6*M.nbody; }
  if constexpr (LAW) { o.law_coef = L.coef + (L.per_env ? (size_t)env*LAW_NROW*M.nv : (size_t)0); o.law_qadr = L.qadr; o.law_out = L.out + (size_t)env*M.nv; }
  return o;
}

// An environment of a grouped batch whose model id was out of range (model_of_env: `bad`) was stepped with the clamped id: say so.
template <typename real>
__device__ __forceinline__ void flag_bad_model(const DevModel<real>& Me, const WS<real>& wc, bool bad_id, int lane) {
  if (bad_id && lane == 0) { int* is_ = ws_uniform(wc, Me).istate(); atomicOr(is_ + IS_WARN, (int)WARN_MODEL_ID); atomicOr(is_ + IS_WARN_EVER, (int)WARN_MODEL_ID); }
}

// The substep scheduler's counter of an environment's completed units (fly_kernel), read and published past the vector L1: a relaxed
// agent-scope load by lane 0, broadcast to the wave (d: the caller's last value, what the other lanes pass in -- starting them from zero
// here moves every step kernel's code), and a relaxed agent-scope atomic MAX.  Neither orders anything: acquire and release are in the
// protocol's text.  (Host emulation: plain memory.)
__device__ __forceinline__ int done_load(const int* done, int lane, int d) {
#ifndef FB_EMULATE
  if (lane == 0) d = __hip_atomic_load(done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  if (lane == 0) d = *done;
#endif
  return uniform_int(__shfl(d, 0, FB_WAVE));
}
__device__ __forceinline__ void done_publish_max(int* done, int v) {
#ifndef FB_EMULATE
  __hip_atomic_fetch_max(done, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  *done = max(*done, v);
#endif
}

// FORCES: the step kernel with applied forces (k_step_forces; F = the batch's two force arrays, fb_forces.hpp).  k_fly and k_fly_reset instantiate it false.
// MODELS: the kernels of a grouped batch (k_group_step, k_group_reset; G = the assignment).  The workgroup's LDS tables and the launch-wide
// quantities (substep count, dimensions, workspace layout) come from element 0 -- the models of a group agree in all of them -- and the
// model proper is bound once the environment is known: per launch on the per-wave path, per ticket under the substep scheduler.
// LAW: the step kernel with a substep control law (k_step_law; L = the law's coefficients, qpos addresses and output, fb_law.hpp).
template <typename real, bool FORCES = false, bool MODELS = false, bool LAW = false>
__device__ __forceinline__ void fly_kernel(const DevModel<real>* Mp, const Batch<real>& B, const float* action, const int* env_ids, int mode, int nsub, int nslot,
                                           const ForceArgs<real> F = ForceArgs<real>(), const GroupArgs G = GroupArgs(), const LawArgs<real> L = LawArgs<real>()) {
  // per-wave (per-environment) hot arrays
  constexpr int EPB = LdsCfg<real>::EPB;
  __shared__ real s_pool[EPB][LdsCfg<real>::POOL];          // [factor row | Delassus matrix | solve vector] of each environment
  // elimination-tree tables shared by the workgroup's environments ("joint tree staged in LDS")
  __shared__ LdsTab s_tab;
  // the model lives in constant memory: its fields (sizes, table pointers, workspace offsets) are scalar loads
  const DevModel<real>& M = as_constant(*Mp);
  int tid = threadIdx.x;
  for (int i = tid; i < M.nv; i += FB_WAVE*EPB) {
    s_tab.depth[i] = (uint8_t)M.dof_depth[i]; s_tab.cl[i] = (uint8_t)M.dof_cl[i]; s_tab.gen[i] = (uint8_t)M.dof_gen[i]; s_tab.madr[i] = (uint16_t)M.dof_Madr[i];
  }
  for (int i = tid; i < 2*FB_WAVE; i += FB_WAVE*EPB) s_tab.gen[FB_MAXNV + i] = (uint8_t)M.fac_dof[i];      // dof of a lane's first / second factor row (fb_smooth.hpp: fac_dof)
  for (int i = tid; i < FB_LGEN*FB_MAXCH; i += FB_WAVE*EPB) { s_tab.gk[i] = (uint32_t)M.gen_k[i]; s_tab.gm[2*i] = (uint32_t)M.gen_m[2*i]; s_tab.gm[2*i + 1] = (uint32_t)M.gen_m[2*i + 1]; }
  __syncthreads();                       // the only workgroup-wide barrier of the kernel
  // the wave index is wave-uniform: say so (v_readfirstlane), otherwise every per-environment base address is 64-bit VALU math
  int wave = uniform_int(tid / FB_WAVE), lane = tid % FB_WAVE;
  int slot = blockIdx.x*EPB + wave;
  if (slot >= nslot) return;
  if (B.tick && mode == MODE_STEP) {
    // ---- substep scheduler.  A batch larger than the resident wave slots used to run as "one environment per wave, start
    // to end": two environments per slot, and a launch as long as its unluckiest pair (1.18 x the mean load per slot with the
    // previous-step order, 1.13 x with perfect knowledge: tools/order_study.py).  Nothing LDS-resident crosses a substep
    // boundary any more, so the unit of work is ONE SUBSTEP of one environment: every wave draws tickets from the queue of
    // its XCD -- ticket t = substep t / cnt of environment (t % cnt) of that XCD's share -- until the queue is empty.  All
    // environments of an XCD advance together, the waves stay busy until the last round, and the launch ends within one
    // substep of sum(durations) / slots.  An environment's substeps are ordered by its `done` counter (a ticket waits for its
    // predecessor, which an earlier ticket -- a running wave -- holds: no deadlock; the wait is iteration-capped all the same).
    // An environment is bound to one XCD (env % nq), so its row only ever lives in one L2; the hand-over between waves of
    // different CUs needs the stores drained to that L2 (the vector L1 is write-through) and the reader's L1 invalidated
    // (acquire fence).  Protocol measured stand-alone in tools/microbench/ticket_proto.hip.
    const int nq = B.nq, xcc = fb_xcc_id() % nq, nsubm = uniform_int(M.nsubstep);
    const int cnt = (B.n_env - xcc + nq - 1)/nq;
    // Round 6: the LAST FB_TICKET_SPLIT substeps of the control step are handed out as two tickets each -- [actuation .. sensors] and
    // [integration .. velocity stage of the next substep's mj_step1], the boundary at which nothing LDS-resident is alive (the factor of M
    // is dead, M + h D is factorised behind it: fb_step.hpp) -- because the launch ends with a quantisation tail: 10 x 4096 tickets over
    // 3072 resident waves are 13.33 rounds, so a third of the waves run a 14th ticket while the rest idle, and the waves are out of phase
    // by then (mean idle = half a ticket).  Half-size units at the end halve both.  A unit index u = t / cnt counts them:
    // u < nsubm - split: whole substep u; beyond: halves.  `done` counts completed units.
    const int nsplit = uniform_int(FB_TICKET_SPLIT < nsubm ? FB_TICKET_SPLIT : nsubm), nfull = nsubm - nsplit, nunit = nsubm + nsplit;
    const int total = cnt*nunit;
    const int ostride = (B.n_env + nq - 1)/nq;
    for (int guard = 0; guard < (1 << 20); guard++) {
      int t = 0;
      if (lane == 0) t = atomicAdd(B.tick + 16*xcc, 1);
      t = uniform_int(__shfl(t, 0, FB_WAVE));
      if (t >= total || cnt <= 0) return;
      const int round = t / cnt;                      // unit index of this ticket
      int env = (t % cnt)*nq + xcc;
      if (B.torder) env = uniform_int(B.torder[xcc*ostride + (t % cnt)]);
      const int hk = round - nfull;                   // >= 0: a half ticket
      const int tkhalf = hk < 0 ? 0 : 1 + (hk & 1);   // 1: [actuation .. sensors], 2: [integration .. velocity]
      // wait for the predecessor substep (normally long done: it was drawn `cnt` tickets ago).  An environment whose predecessor is still
      // running when its next ticket comes up is BEHIND the round-robin: its ten substeps in sequence are what the launch will wait for
      // at the end (tools/ticket_trace.py), so that ticket runs at the highest issue priority.
      int d = 0, late = 0;
#if defined(FB_PROFILE) && !defined(FB_EMULATE)
      const long long tw0_ = wall_clock64();
#endif
      for (int spins = 0; spins < FB_SCHED_SPIN_CAP; spins++) {
        d = done_load(B.done + env, lane, d);
        if (d >= round) break;
        late = 3;
#ifndef FB_EMULATE
        __builtin_amdgcn_s_sleep(32);
#endif
      }
      if (d > round) continue;                       // the environment was auto-reset by its first ticket (or abandoned, below): nothing to do
      if (d < round) {
        // The wait was capped (~seconds): the predecessor substep has not been published.  Stepping the row now would race with
        // whoever still holds it, so the environment's control step is ABANDONED: flagged per environment (FB_WARN_SCHED_WAIT),
        // counted in the batch's sticky error counter (fb_batch_synchronize / fb_batch_get then fail), and its remaining tickets
        // are skipped.  Never observed; a launch that can get here has lost a wave.
        if (lane == 0) {
          int* is_ = (int*)(B.iarena + (size_t)env*M.off.nint + M.off.istate);
          // (the holder of the row may be writing IS_WARN itself: atomic OR.  The abandon mark nsubm + 2 must survive the holder's own
          // publication of `round + 1` when it finally finishes -- both sides publish with an atomic MAX -- so that every later
          // ticket of this environment is skipped at once (d > round) instead of spinning to the cap again.)
          atomicOr(is_ + IS_WARN, WARN_SCHED_WAIT); atomicOr(is_ + IS_WARN_EVER, WARN_SCHED_WAIT);
          atomicAdd(B.sched_err, 1);
          done_publish_max(B.done + env, nunit + 2);
        }
        continue;
      }
#ifndef FB_EMULATE
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
#endif
      bool bad_id;
      const DevModel<real>& Me = model_of_env<real, MODELS>(Mp, M, G, env, bad_id);
      const WS<real> w = ws_env(Me, B.rarena, B.iarena, env, s_pool, wave, &s_tab);
#ifdef FB_EMULATE
      // (host emulation, test infrastructure: every ticket starts from a POISONED LDS pool -- whatever a stage left there for a later ticket,
      //  against the claim that nothing LDS-resident crosses a ticket boundary, turns the state into NaN and fails the parity tests)
      for (int i = lane; i < LdsCfg<real>::POOL; i += FB_WAVE) w.lLD[i] = (real)NAN;
      SYNC();
#endif
      if (lane == 0) { w.istate()[IS_PRIO] = late; if (round == 0) w.istate()[IS_WARN] = 0; }
      FB_SETPRIO(late);
#if defined(FB_PROFILE) && !defined(FB_EMULATE)
      const long long tw1_ = wall_clock64();       // (tools/ticket_trace.py) per environment: wait for the predecessor, first start, last end, busy ticks
#endif
      // the stages read a copy of the descriptor, by reference, and the step's rows are formed where a stage takes them: neither stays in
      // registers across the stage calls (fb_step.hpp: d_run)
      const WS<real> wc = w;
      auto io = [&]() { return step_io<real, FORCES, LAW>(M, B, action, F, L, env); };
      const bool was_reset = d_run<real, FORCES, LAW>(Me, wc, io, env, mode, nsub, nslot, (int*)nullptr, lane,
                                   (round == 0 ? 1 : 0) | (round == nunit - 1 ? 2 : 0) | (tkhalf == 1 ? 4 : 0) | (tkhalf == 2 ? 8 : 0) | (late ? 16 : 0), -1);
      if constexpr (MODELS) flag_bad_model(Me, wc, bad_id, lane);
      // Release.  What the next holder of this environment (a wave of the SAME XCD: environments are bound to XCDs) must see is this
      // wave's global stores.  On gfx942 / gfx950 the vector L1 is write-through and an XCD has ONE L2, so "visible to the XCD" =
      // "acknowledged by the L2" = vmcnt(0); the workgroup-scope release fence keeps the compiler from sinking stores below it, the
      // relaxed agent-scope store then publishes the counter (atomics bypass the L1).  A formal agent-scope release would add
      // buffer_wbl2: a write-back of the WHOLE L2 to memory per ticket, for readers (other XCDs) that by construction do not
      // exist.  The hardware facts this leans on are checked where they can be (fb_batch_create: architecture, all XCDs visible;
      // launch: the stream reaches every XCD) and the scheduler is switched off otherwise.
#if defined(FB_PROFILE) && !defined(FB_EMULATE)
      if (lane == 0) {
        long long* pp_ = (long long*)ws_uniform(wc, Me).prof(); const long long tw2_ = wall_clock64();
        if (round == 0) { pp_[52] = 0; pp_[53] = tw0_; pp_[55] = 0; }
        pp_[52] += tw1_ - tw0_; pp_[54] = tw2_; pp_[55] += tw2_ - tw1_;
      }
#endif
#ifndef FB_EMULATE
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
#endif
      if (lane == 0) done_publish_max(B.done + env, was_reset ? nunit + 1 : round + 1);      // (MAX: an abandon mark stays)
    }
    return;
  }
  int env = uniform_int(env_ids ? env_ids[slot] : slot);
  bool bad_id;
  const DevModel<real>& Me = model_of_env<real, MODELS>(Mp, M, G, env, bad_id);
  const WS<real> w = ws_env(Me, B.rarena, B.iarena, env, s_pool, wave, &s_tab);
#if defined(FB_PROFILE) && !defined(FB_EMULATE)
  long long t0_ = clock64(), r0_ = wall_clock64();
#endif
#ifdef FB_EMULATE
  long long life0_ = 0;
#else
  long long life0_ = wall_clock64();
#endif
  // profiling (fb_batch_stage): ONE stage of a control step per launch; the LDS pool lives in B.park between launches
  const int only = uniform_int(mode == MODE_STAGE ? nsub : -1);
  if (only >= 0) {
    const FB_GLOBAL real* pk = (const FB_GLOBAL real*)(B.park + (size_t)env*LdsCfg<real>::POOL);
    for (int i = lane; i < LdsCfg<real>::POOL; i += FB_WAVE) w.lLD[i] = pk[i];
    SYNC();
  } else if (lane == 0) { w.istate()[IS_PRIO] = 0; if (mode == MODE_STEP || mode == MODE_RESET) w.istate()[IS_WARN] = 0; }
  const WS<real> wc = w;                  // (as on the ticket path: the stages' copy of the descriptor, the step's rows formed where they are used)
  auto io = [&]() { return step_io<real, FORCES, LAW>(M, B, action, F, L, env); };
  d_run<real, FORCES, LAW>(Me, wc, io, env, only >= 0 ? (int)MODE_STEP : mode, nsub, nslot, only >= 0 ? (int*)nullptr : B.sched, lane, -1, only);
  if constexpr (MODELS) flag_bad_model(Me, wc, bad_id, lane);
  if (only >= 0) {
    SYNC();
    FB_GLOBAL real* pk = (FB_GLOBAL real*)(B.park + (size_t)env*LdsCfg<real>::POOL);
    const FB_LDS real* pool = ws_uniform(wc, Me).lLD;
    for (int i = lane; i < LdsCfg<real>::POOL; i += FB_WAVE) pk[i] = pool[i];
    return;
  }
#if defined(FB_PROFILE) && !defined(FB_EMULATE)
  if (lane == 0) { long long* pp_ = (long long*)ws_uniform(wc, Me).prof(); pp_[29] += clock64() - t0_; pp_[30] += wall_clock64() - r0_; pp_[28] = r0_; /* start tick (replaces the env_post phase counter) */ }
#endif
  // how long this environment's control step took: the next launch starts the slow environments first (k_order)
  if (mode == MODE_STEP && B.cost && lane == 0) {
#ifdef FB_EMULATE
    B.cost[env] = (int)(((unsigned)env*2654435761u) >> 16);        // no clock on the host: an arbitrary permutation exercises the path
#else
    B.cost[env] = (int)(wall_clock64() - life0_);
#endif
  }
}

// The kernels proper.  k_fly: control steps, forward passes and single stages.  k_fly_reset: the (partial) resets of fb_batch_reset under a
// name of their own -- same device code with the mode folded in -- so that a kernel trace of k_fly holds control steps only (the staggered
// pre-roll of bench.py resets 1/235 of the batch between any two steps: 236 short launches that used to be averaged into the step kernel).
// Every step kernel runs under the same launch bounds (one wave per environment on k_fly's LDS layout: the residency batch_create_impl and
// launch_fly count on) and begins with the same arguments, a feature's own behind them; the reset kernels take neither action nor mode.
#define FB_STEP_KERNEL __global__ void __launch_bounds__(FB_WAVE*LdsCfg<real>::EPB, LdsCfg<real>::WAVES_PER_SIMD)
#define FB_STEP_PARAMS const DevModel<real>* Mp, Batch<real> B, const float* action, const int* env_ids, int mode, int nsub, int nslot
#define FB_STEP_ARGS Mp, B, action, env_ids, mode, nsub, nslot
#define FB_RESET_PARAMS const DevModel<real>* Mp, Batch<real> B, const int* env_ids, int nsub, int nslot
#define FB_RESET_ARGS Mp, B, nullptr, env_ids, (int)MODE_RESET, nsub, nslot
template <typename real> FB_STEP_KERNEL k_fly(FB_STEP_PARAMS) { fly_kernel<real>(FB_STEP_ARGS); }
template <typename real> FB_STEP_KERNEL k_fly_reset(FB_RESET_PARAMS) { fly_kernel<real>(FB_RESET_ARGS); }

// The step kernel with external forces (fb_forces.hpp): the same device code with the applied-force stage compiled in, under k_fly's launch bounds
// and on its LDS layout, ticket scheduler included.  The two arrays are an extra kernel argument, so k_fly's own arguments stay where they are.
// launch() uses it for control steps, substeps and forward evaluations while the batch's force arrays are allocated.
template <typename real> FB_STEP_KERNEL k_step_forces(FB_STEP_PARAMS, ForceArgs<real> F) { fly_kernel<real, true>(FB_STEP_ARGS, F); }

// The step kernel with a substep control law (fb_law.hpp): the forces kernel with the law stage compiled in as well -- setting a law allocates
// the force arrays -- under k_fly's launch bounds and on its LDS layout, ticket scheduler included.  The law is one more kernel argument.
template <typename real> FB_STEP_KERNEL k_step_law(FB_STEP_PARAMS, ForceArgs<real> F, LawArgs<real> L) { fly_kernel<real, true, false, true>(FB_STEP_ARGS, F, GroupArgs(), L); }

// Ends episodes from the device (fb_batch_end_episode): one thread per environment.  Where the mask is set and the environment's last
// step was MID, the step becomes LAST with the caller's discount and the next control step auto-resets the environment, exactly as after a
// LAST the step kernel decided itself.  FIRST and already-LAST environments are left alone.
__global__ void k_end_episode(int* iarena, unsigned nint, unsigned istate, int* step_type, float* discount, const uint8_t* mask, const float* disc, int n) {
  const int e = blockIdx.x*FB_WAVE + threadIdx.x;
  if (e >= n || !mask[e]) return;
  int* is = iarena + (size_t)e*nint + istate;
  if (is[IS_STEP_TYPE] != 1) return;
  is[IS_STEP_TYPE] = 2; is[IS_RESET_NEXT] = 1;
  step_type[e] = 2; discount[e] = disc ? disc[e] : 0.0f;
}

// Zeroes rows [words] of 32-bit words each: row ids[k] of `base`, one workgroup per listed row (fb_batch_reset of some environments
// clears their FB_QFRC_LAW rows; the ids are on the device already).
__global__ void k_zero_rows(uint32_t* base, const int* ids, int n, unsigned words) {
  const int k = blockIdx.x;
  if (k >= n) return;
  uint32_t* row = base + (size_t)ids[k]*words;
  for (unsigned i = threadIdx.x; i < words; i += FB_WAVE) row[i] = 0u;
}

// The kernels of a grouped batch (fb_batch_create_group): the same device code with the per-environment model compiled in, under k_fly's
// launch bounds and on its LDS layout, ticket scheduler included; with and without the applied-force stage, and the reset under a name of its
// own as above.  The assignment is an extra kernel argument.  launch_fly uses them while the batch holds more than one model, so the
// kernels above keep their arguments and their code.
template <typename real, bool FORCES> FB_STEP_KERNEL k_group_step(FB_STEP_PARAMS, ForceArgs<real> F, GroupArgs G) { fly_kernel<real, FORCES, true>(FB_STEP_ARGS, F, G); }
template <typename real> FB_STEP_KERNEL k_group_reset(FB_RESET_PARAMS, GroupArgs G) { fly_kernel<real, false, true>(FB_RESET_ARGS, ForceArgs<real>(), G); }

// The kernels launch_fly chooses among for a control step.  Same launch bounds and LDS layout, so the same residency
// (tests/test_step_kernel_resources.py); batch_create_impl takes the scheduler's resident-slot count as the minimum over this list all
// the same.  A new step kernel is one more entry.
template <typename real>
static std::array<const void*, 5> step_kernels() {
  return {(const void*)k_fly<real>, (const void*)k_step_forces<real>, (const void*)k_step_law<real>, (const void*)k_group_step<real, false>, (const void*)k_group_step<real, true>};
}

// Launch order for the next control step: environments sorted by the duration of their last step, longest first (counting
// sort over 256 duration bins, one workgroup).  Contact configurations persist from step to step, so the last duration
// predicts the next one well, and a launch with more environments than resident waves (FP64 build: 2048 slots per GPU)
// no longer ends with a few slow environments that started late: longest-processing-time-first packing.
#define FB_ORDER_THREADS 256
__global__ void __launch_bounds__(FB_ORDER_THREADS) k_order(const int* cost, int* order, int n) {
  __shared__ int s_red[FB_ORDER_THREADS];
  __shared__ int s_hist[256];
  int tid = threadIdx.x;
  int mx = 1;
  for (int e = tid; e < n; e += FB_ORDER_THREADS) mx = cost[e] > mx ? cost[e] : mx;
  s_red[tid] = mx; s_hist[tid & 255] = 0;
  __syncthreads();
  for (int st = FB_ORDER_THREADS/2; st >= 1; st >>= 1) {
    if (tid < st) s_red[tid] = s_red[tid] > s_red[tid + st] ? s_red[tid] : s_red[tid + st];
    __syncthreads();
  }
  mx = s_red[0];
  __syncthreads();
  // bin 0 = longest
  for (int e = tid; e < n; e += FB_ORDER_THREADS) {
    int c = cost[e]; c = c < 0 ? 0 : c;
    int bin = 255 - (int)(((long long)c*255)/mx);
    atomicAdd(&s_hist[bin], 1);
  }
  __syncthreads();
  if (tid == 0) { int acc = 0; for (int k = 0; k < 256; k++) { int h = s_hist[k]; s_hist[k] = acc; acc += h; } }
  __syncthreads();
  for (int e = tid; e < n; e += FB_ORDER_THREADS) {
    int c = cost[e]; c = c < 0 ? 0 : c;
    int bin = 255 - (int)(((long long)c*255)/mx);
    order[atomicAdd(&s_hist[bin], 1)] = e;
  }
}

// Ticket order of the substep scheduler: per XCD, the environments of its share (env % nq == xcc) by DECREASING size of the constraint
// system their last substep solved (counting sort, one workgroup per XCD).  The cost of a substep grows with that size (Newton: cubic),
// contact configurations persist from step to step, and the launch ends with the last tickets drawn: longest first means the stragglers
// of the final round are the cheap environments.  Scheduling only -- environments are independent, results do not depend on it.
__global__ void __launch_bounds__(FB_ORDER_THREADS) k_ticket_order(const int* iarena, int nint, int off_nefc, int* order, int n_env, int nq) {
  __shared__ int s_hist[256];
  const int tid = threadIdx.x, xcc = blockIdx.x;
  const int cnt = (n_env - xcc + nq - 1)/nq, stride = (n_env + nq - 1)/nq;
  s_hist[tid & 255] = 0;
  __syncthreads();
  for (int j = tid; j < cnt; j += FB_ORDER_THREADS) {
    int key = iarena[(size_t)(j*nq + xcc)*nint + off_nefc]; key = key < 0 ? 0 : (key > 255 ? 255 : key);
    atomicAdd(&s_hist[255 - key], 1);
  }
  __syncthreads();
  if (tid == 0) { int acc = 0; for (int k = 0; k < 256; k++) { int h = s_hist[k]; s_hist[k] = acc; acc += h; } }
  __syncthreads();
  for (int j = tid; j < cnt; j += FB_ORDER_THREADS) {
    const int e = j*nq + xcc;
    int key = iarena[(size_t)e*nint + off_nefc]; key = key < 0 ? 0 : (key > 255 ? 255 : key);
    order[xcc*stride + atomicAdd(&s_hist[255 - key], 1)] = e;
  }
}

// ------------------------------------------------------------------ synthetic actions
// Random-action rollouts ("per-env RNG = Philox(seed, stream = env_id)"): one counter-based stream per
// GLOBAL environment id, so what an environment is fed does not depend on the number of GPUs the batch is sharded over or on its
// position inside a rank's shard (the reference runs one independent environment per actor process,
// agents/ray_distributed_dmpo.py:232).  Philox4x32-10 (Salmon et al., SC'11) with key = seed and counter = (control step, global
// environment id, group of four action entries, distribution tag); outputs -> N(0,1) by Box-Muller in FP32, clipped to [-1, 1]
// (dist 0), or U(-1, 1) (dist 1).
FB_HD __forceinline__ void fb_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t* out) {
  for (int r = 0; r < 10; r++) {
    const uint64_t p0 = (uint64_t)0xD2511F53u*c0, p1 = (uint64_t)0xCD9E8D57u*c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
__global__ void __launch_bounds__(FB_WAVE) k_actions(float* out, const int* env_ids, int n_env, int nact, uint32_t seed_lo, uint32_t seed_hi, int step, int env_id_base, int dist) {
  const int ngrp = (nact + 3)/4;
  const int t = blockIdx.x*FB_WAVE + threadIdx.x;
  if (t >= n_env*ngrp) return;
  const int e = t / ngrp, g = t - e*ngrp;
  const int gid = env_ids ? env_ids[e] : env_id_base + e;
  uint32_t r[4];
  fb_philox4x32_10((uint32_t)step, (uint32_t)gid, (uint32_t)g, (uint32_t)dist, seed_lo, seed_hi, r);
  float v[4];
  if (dist == 1) {
    for (int k = 0; k < 4; k++) v[k] = ((float)(r[k] >> 8) + 0.5f)*(2.0f/16777216.0f) - 1.0f;
  } else {
    for (int k = 0; k < 4; k += 2) {
      const float u1 = ((float)(r[k] >> 8) + 0.5f)*(1.0f/16777216.0f), u2 = ((float)(r[k + 1] >> 8) + 0.5f)*(1.0f/16777216.0f);
      const float rad = sqrtf(-2.0f*logf(u1)), ang = 6.28318530717958647692f*u2;
      v[k] = rad*cosf(ang); v[k + 1] = rad*sinf(ang);
    }
    for (int k = 0; k < 4; k++) v[k] = fminf(1.0f, fmaxf(-1.0f, v[k]));
  }
  for (int k = 0; k < 4; k++) if (4*g + k < nact) out[(size_t)e*nact + 4*g + k] = v[k];
}

extern "C" int fb_random_actions(float* action, const int32_t* env_ids, int n_env, int nact, uint64_t seed, int step, int env_id_base, int dist, void* stream) {
  if (!action || n_env <= 0 || nact <= 0 || (dist != 0 && dist != 1)) return fail("fb_random_actions: bad arguments");
  const int total = n_env*((nact + 3)/4);
  hipLaunchKernelGGL(k_actions, dim3((total + FB_WAVE - 1)/FB_WAVE), dim3(FB_WAVE), 0, (hipStream_t)stream, action, (const int*)env_ids, n_env, nact,
                     (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), step, env_id_base, dist);
  HIPCHK(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------ batch
struct fb_batch {
  const fb_model* m;
  int n_env, device, precision, nobs;
  WSOff off;
  // Device memory and events: every one a DevBuf / DevEvent member (fb_host.hpp), released when the batch is deleted.  A new buffer is one
  // more such member and nothing else.  <void>: elements of the batch's precision, counted in bytes.
  DevBuf<void> rarena; DevBuf<int> iarena;
  DevBuf<float> obs, reward, discount; DevBuf<int> step_type;
  DevBuf<int> d_ids;
  DevBuf<int> sched;
  DevBuf<int> cost, order; bool order_valid = false, reorder = true, use_prio = true, ticket_order = true;
  DevBuf<int> tick, done, sched_err, torder; int nq = 0, slots = 0; bool tickets = false;      // substep scheduler (k_fly)
  unsigned xcc_mask = 0; std::vector<void*> probed_streams; DevBuf<unsigned> probe_word;  // ... the streams it was validated on, the probe's device word
  DevBuf<void> park;                  // MODE_STAGE: LDS pools between single-stage launches (allocated on first use)
  // model tables on the device (upload, upload_i).  A second fb_batch_set_wbpg or fb_batch_set_*_dataset adds its tables and the earlier ones
  // stay until the batch is destroyed: a launch in flight may still read them.
  std::vector<DevBuf<void>> allocs;
  DevModel<double> M64; DevModel<float> M32;   // the model at the batch's precision (with_model: only that one is built)
  // grouped batch (fb_batch_create_group): the models, the device structs of all of them at the batch's precision (element 0 follows
  // M64 / M32, which the setters change: sync_model) and the assignment FB_ENV_MODEL [n_env] (null: a batch made by fb_batch_create)
  std::vector<const fb_model*> models; std::vector<DevModel<double>> G64; std::vector<DevModel<float>> G32; DevBuf<int> env_model;
  int n_models() const { return models.empty() ? 1 : (int)models.size(); }
  DevBuf<void> dM;                    // the model struct in device memory (the kernels read it through the constant path)
  std::vector<char> dM_copy;          // ... what it currently holds (sync_model)
  DevBuf<void> ref_qpos, ref_qvel;
  bool have_ref = false, have_wbpg = false;
  DevEvent ev0, ev1; int timed_launches = 0; bool timing = false;
  std::vector<DevEvent> lev;          // per-launch event pairs of the timed region (fb_batch_timing_launches), created on first use
  DevBuf<double> ik_err; DevBuf<int> ik_steps;            // fb_batch_ik results (FB_IK_ERR / FB_IK_STEPS), allocated on the first call
  DevBuf<void> ik_buf;                                    // ... its tables and targets (grown as needed)
  DevBuf<double> inv_qfrc, inv_cforce;                           // fb_batch_inverse results (FB_QFRC_INVERSE / FB_CONTACT_FORCE), allocated on the first call
  DevBuf<void> qfrc_applied, xfrc_applied;                       // applied forces (FB_QFRC_APPLIED / FB_XFRC_APPLIED) at the batch's precision: both allocated by the first
                                                                 // fb_batch_set / fb_batch_device_ptr of either, freed by fb_batch_clear_forces; allocated = k_step_forces steps the batch
  // substep control law (fb_batch_set_control_law, fb_law.hpp): coefficients [law_rows][5][nv] (FB_CONTROL_LAW) and output [n_env][nv] (FB_QFRC_LAW) at the
  // batch's precision, qpos addresses [nv]; set = k_step_law steps the batch.  law_owns_forces: the law allocated the force arrays itself (no caller
  // touched them), so clearing the law frees them too and the batch is back on k_fly
  DevBuf<void> law_coef, law_out; DevBuf<int> law_qadr; int law_rows = 0; bool law_owns_forces = false;
  // fb_batch_transition_fd (fb_deriv.hpp), allocated on the first call: the pool of scratch rows (one real + one int arena row per resident wave),
  // the staging buffer of the tickets' raw results (at most FB_FD_STAGING_BYTES, grown as needed), the frames' environments, the counters
  DevBuf<double> fd_pool_r; DevBuf<int> fd_pool_i; int fd_slots = 0;
  DevBuf<double> fd_stage; DevBuf<int> fd_env, fd_counter;
  std::vector<int> fd_env_host;
  // fb_batch_rollout (fb_rollout.hpp): it runs on the scratch rows above (roll_slots of them: what its own kernel keeps resident, at most fd_slots);
  // the rollouts' source environments and its own counters
  DevBuf<int> roll_env, roll_counter, roll_sched; int roll_slots = 0;
  std::vector<int> roll_env_host;
  // fb_batch_rollout_feedback: the rows k_closedloop_rollout keeps resident, and the rollouts' nominals behind their environments in roll_env
  int roll_fb_slots = 0;
  // fb_batch_lqr_backward (fb_riccati.hpp): the products' workspace of all nominals, grown as needed
  DevBuf<double> lqr_ws;
  // fb_batch_ray (fb_ray.hpp): the call's small tables -- visible geoms, the frames' environments and terrain ids --, grown as needed
  DevBuf<int> ray_tab; std::vector<int> ray_tab_host;
};

// one table of n elements, converted to E (int, or the batch's real), in a device allocation of its own that the batch keeps
template <typename E, typename T, typename P>
static int upload(fb_batch* b, const T* src, size_t n, P* dst) {
  std::vector<E> tmp(n ? n : 1);      // an EMPTY table keeps one ZERO entry: the kernels read entry 0 of a table unpredicated in places
                                      // (flight_imitation has no force sensors: a garbage site id from here indexed site_bodyid wildly)
  for (size_t k = 0; k < n; k++) tmp[k] = (E)src[k];
  DevBuf<void> d;
  if (d.alloc(tmp.size()*sizeof(E))) return -1;
  HIPCHK(hipMemcpy(d.get(), tmp.data(), tmp.size()*sizeof(E), hipMemcpyHostToDevice));
  *dst = (const E*)d.get();
  b->allocs.push_back(std::move(d));
  return 0;
}
template <typename P> static int upload_i(fb_batch* b, const int* src, size_t n, P* dst) { return upload<int>(b, src, n, dst); }

// f(M) on the batch's model at its precision: M64 for an FP64 batch, M32 for an FP32 one (the other one is never built or read).
// Inside f, `using real = decltype(M.timestep);` names the precision.
template <typename F>
static auto with_model(fb_batch* b, F&& f) { return b->precision == 64 ? f(b->M64) : f(b->M32); }
static size_t real_size(fb_batch* b) { return with_model(b, [](auto& M) { return sizeof(M.timestep); }); }

// The device copy of the model struct follows the host copy (the setters only touch the host copy); a changed model is rare,
// so the refresh simply waits for the device to be idle
// (a grouped batch holds the structs of all its models as one array: element 0 is the setters' model, the task-level fields of the others follow it)
template <typename real>
static void copy_task_fields(DevModel<real>& d, const DevModel<real>& s) {
#define CP(f) d.f = s.f;
  CP(ref_qpos) CP(ref_qvel) CP(T) CP(future_steps) CP(episode_steps) CP(nobs) CP(terminal_com_dist) CP(time_limit) CP(seed)
  CP(wb_traj) CP(wb_phase) CP(wb_freqs) CP(wb_offset) CP(wb_nfreq) CP(wb_base_freq) CP(wb_rel_range) CP(wb_rate)
  CP(ds_qpos) CP(ds_qvel) CP(ds_r2s) CP(ds_jq) CP(ds_offset) CP(ds_jid) CP(ds_sid) CP(ds_select)
  CP(ds_nj) CP(ds_ns) CP(ds_ntraj) CP(ds_nselect) CP(ds_env_base) CP(max_episode_steps) CP(ds_random_start)
#undef CP
}
static std::vector<DevModel<double>>& group_models(fb_batch* b, DevModel<double>&) { return b->G64; }
static std::vector<DevModel<float>>& group_models(fb_batch* b, DevModel<float>&) { return b->G32; }

static int sync_model(fb_batch* b) {
  return with_model(b, [&](auto& M) {
    auto& G = group_models(b, M);
    const size_t bytes = sizeof(M)*(G.empty() ? 1 : G.size());
    if (!b->dM && b->dM.alloc(bytes)) return -1;
    if (!G.empty()) { G[0] = M; for (size_t k = 1; k < G.size(); k++) copy_task_fields(G[k], M); }
    const char* h = G.empty() ? (const char*)&M : (const char*)G.data();
    if (b->dM_copy.empty() || memcmp(h, b->dM_copy.data(), bytes) != 0) {
      HIPCHK(hipDeviceSynchronize());
      HIPCHK(hipMemcpy(b->dM.get(), h, bytes, hipMemcpyHostToDevice));
      b->dM_copy.assign(h, h + bytes);
    }
    return 0;
  });
}

// a zeroed device buffer of n elements, allocated on the first call that needs it
template <typename T>
static int alloc_zeroed_once(DevBuf<T>& d, size_t n) { return d ? 0 : d.alloc_zeroed(n); }

// a new, zeroed observation buffer of nobs floats per environment
static int alloc_obs(fb_batch* b, int nobs) {
  if (b->obs.alloc_zeroed((size_t)b->n_env*nobs)) return -1;
  b->nobs = nobs;
  return 0;
}

// The environment's test and measurement switches, read in one place, once, when a batch is created (batch_create_impl declares one).  Two truth
// rules, as ever: env_is1 -- in force when the variable's value begins with '1'; env_is_set -- in force when the variable exists, whatever it holds.
static bool env_is1(const char* n) { const char* e_ = getenv(n); return e_ && e_[0] == '1'; }
static bool env_is_set(const char* n) { return getenv(n) != nullptr; }
struct Switches {
  bool no_neighbour_list = env_is1("FB_NO_NEIGHBOUR_LIST");      // vl_delta = 0 (the tests compare the two mid phases bit for bit)
  bool no_ar_entry_lanes = env_is1("FB_NO_AR_ENTRY_LANES");      // ar_entry_lanes = 0 (... the two builds of the Delassus matrix bit for bit)
  bool no_solver_handover = env_is1("FB_NO_SOLVER_HANDOVER");    // solver_handover = 0 (... the two hand-overs against the oracle and each other)
  bool no_reorder = env_is1("FB_NO_REORDER");                    // environments and tickets keep their order
  bool no_fk_merge = env_is_set("FB_NO_FK_MERGE");               // fk_second = null: separate kinematics passes (the tests run both paths)
  bool no_tickets = env_is_set("FB_NO_TICKETS");                 // the per-wave path whatever the batch's size
  bool no_prio = env_is_set("FB_NO_PRIO");
  const char* ticket_slots = getenv("FB_TICKET_SLOTS");          // set: its value replaces the resident slot count (the tests pretend fewer slots)
};

// The device struct of model m at one precision: the scalars copied, the real ones converted, the switches applied, the tables uploaded.
// Nothing is derived here: whatever follows from the model alone is fb_model_load's (fb_model.hpp).
template <typename real>
static int build_devmodel(fb_batch* b, const fb_model* m, const Switches& sw, DevModel<real>& M) {
  memset(&M, 0, sizeof(M));
  M.nq = m->nq; M.nv = m->nv; M.nbody = m->nbody; M.njnt = m->njnt; M.ngeom = m->ngeom; M.nsite = m->nsite;
  M.nu = m->nu; M.na = m->na; M.ntendon = m->ntendon; M.npair = m->npair; M.nM = m->nM; M.nsubstep = m->nsubstep;
  M.nobsjnt = m->nobsjnt; M.napp = m->napp; M.nforce = m->nforce; M.ntouch = m->ntouch;
  M.site_thorax = m->i("sensor_site_thorax")[0]; M.nadh = (int)m->adh_act.size(); M.nplane = m->nplane; M.nsensbody = (int)m->sens_body.size();
  M.iterations = m->i("opt_iterations")[0]; M.noslip_iterations = m->i("opt_noslip_iterations")[0]; M.solver = m->solver;
  M.nlevel = m->nlevel; M.ntrunk = m->ntrunk; M.prefix_split = m->prefix_split; M.chmax = m->chmax; M.fk_dmax = m->fk_dmax; M.fk2_dlo = m->fk2_dlo;
  M.task = m->task_id; M.user_idx = m->i("user_action_idx")[0]; M.nact = m->nu + (M.user_idx >= 0 ? 1 : 0);
  M.timestep = (real)m->d("opt_timestep")[0]; M.control_timestep = (real)m->d("opt_control_timestep")[0];
  M.clock_timestep = m->d("opt_timestep")[0]; M.clock_control_timestep = m->d("opt_control_timestep")[0];
  for (int k = 0; k < 3; k++) { M.grav[k] = (real)m->d("opt_gravity")[k]; M.com_offset[k] = (real)m->d("com_offset")[k]; }
  M.density = (real)m->d("opt_density")[0]; M.viscosity = (real)m->d("opt_viscosity")[0]; M.impratio = (real)m->d("opt_impratio")[0]; M.tolerance = (real)m->d("opt_tolerance")[0];
  M.noslip_tolerance = (real)m->d("opt_noslip_tolerance")[0]; M.meaninertia = (real)m->d("stat_meaninertia")[0]; M.totalmass = (real)m->totalmass;
  M.vl_delta = sw.no_neighbour_list ? (real)0 : (real)m->vl_delta; M.ar_entry_lanes = sw.no_ar_entry_lanes ? 0 : 1; M.solver_handover = sw.no_solver_handover ? 0 : 1;
  size_t c;                             // the tables of FB_MODEL_TABLES (fb_types.hpp), one allocation each
#define FB_GET_int i
#define FB_GET_real d
#define FB_SRC_blob(kind, s) m->FB_GET_##kind(#s, &c)
#define FB_SRC_vec(kind, s) (c = m->s.size(), m->s.data())
#define X(member, kind, from, s) { const auto* s_ = FB_SRC_##from(kind, s); if (upload<kind>(b, s_, c, &M.member)) return -1; }
  FB_MODEL_TABLES(X)
#undef X
  // fk_second: a nullable raw pointer -- null where the model has no lane pairing (fb_model.hpp: derive_topology) or the switch is set
  if (!m->fk_second.empty() && !sw.no_fk_merge && upload_i(b, m->fk_second.data(), m->fk_second.size(), &M.fk_second)) return -1;
  // leg_jnt: an optional blob array (models compiled before the flight-with-legs variant do not carry it); without it a valid table that nobody reads
  const bool legs = m->has("leg_joints", 1);
  const int* lj = legs ? FB_SRC_blob(int, leg_joints) : FB_SRC_vec(int, adh_act);
  for (size_t k = 0; legs && k < c; k++) if (lj[k] < 0 || lj[k] >= m->njnt) return fail("fb_batch_create: leg_joints out of range");
  M.nlegjnt = legs ? (int)c : 0;
#undef FB_GET_int
#undef FB_GET_real
#undef FB_SRC_blob
#undef FB_SRC_vec
  return upload_i(b, lj, c, &M.leg_jnt);
}

template <typename real>
static void compute_offsets(const DevModel<real>& M, WSOff& o) {
  uint32_t r = 0, i = 0;
  auto al = [](uint32_t v) { return (v + 15u) & ~15u; };   // every array on a cache line of its own
#define X(name, n) o.name = r; r = al(r + (uint32_t)(n));
  FB_WS_REAL(X)
#undef X
#define X(name, n) o.name = i; i = al(i + (uint32_t)(n));
  FB_WS_INT(X)
#undef X
  o.nreal = (r + 15u) & ~15u; o.nint = (i + 15u) & ~15u;
}

static int batch_create_impl(fb_batch* b);

// fb_batch_create (models == null: the one model m) and fb_batch_create_group (m = models[0]) behind their argument checks
static int batch_create(const std::string& fn, const fb_model* m, const fb_model* const* models, int n_models, int n_env, int device, int precision, fb_batch** out) {
  if (precision != 32 && precision != 64) return fail(fn + ": precision must be 32 or 64");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(fn + ": no HIP device available (the engine has no CPU fallback)");
  if (device < 0 || device >= ndev) return fail(fn + ": bad device index");
  HIPCHK(hipSetDevice(device));
  fb_batch* b = new fb_batch();
  b->m = m; b->n_env = n_env; b->device = device; b->precision = precision;
  if (models) b->models.assign(models, models + n_models);
  int rc;
  try { rc = batch_create_impl(b); } catch (const std::exception& e_) { rc = fail(fn + ": " + e_.what()); }
  if (rc != 0) { std::string keep = g_err; fb_batch_destroy(b); g_err = keep; return rc; }     // every allocation made so far is released
  *out = b;
  return 0;
}

extern "C" int fb_batch_create(const fb_model* m, int n_env, int device, int precision, fb_batch** out) {
  if (!out) return fail("fb_batch_create: null output pointer");
  *out = nullptr;
  if (!m || n_env <= 0) return fail("fb_batch_create: bad arguments");
  return batch_create("fb_batch_create", m, nullptr, 1, n_env, device, precision, out);
}

// The first array in which model `o` is not compatible with model `m` (fb_batch_create_group), or null: the same arrays with the same
// types and shapes, integer arrays equal, of the real arrays the two time steps equal.
static const char* first_incompatible_array(const fb_model* m, const fb_model* o, std::string* why) {
  for (const auto& kv : m->idx) {
    const BlobEntry* a = kv.second;
    auto it = o->idx.find(kv.first);
    if (it == o->idx.end()) { *why = "is missing"; return a->name; }
    const BlobEntry* c = it->second;
    if (a->dtype != c->dtype || a->ndim != c->ndim || a->nbytes != c->nbytes || memcmp(a->shape, c->shape, sizeof(a->shape)) != 0) { *why = "has another type or shape"; return a->name; }
    const bool fixed = a->dtype == 1 || kv.first == "opt_timestep" || kv.first == "opt_control_timestep";
    if (fixed && memcmp(m->blob.data() + a->offset, o->blob.data() + c->offset, a->nbytes) != 0) { *why = "differs"; return a->name; }
  }
  for (const auto& kv : o->idx) if (m->idx.find(kv.first) == m->idx.end()) { *why = "is not an array of model 0"; return kv.second->name; }
  return nullptr;
}

extern "C" int fb_batch_create_group(const fb_model* const* models, int n_models, int n_env, int device, int precision, fb_batch** out) {
  if (!out) return fail("fb_batch_create_group: null output pointer");
  *out = nullptr;
  if (!models || n_models < 1 || n_env <= 0) return fail("fb_batch_create_group: bad arguments");
  if (n_models > FB_MAX_MODELS) return fail("fb_batch_create_group: more than FB_MAX_MODELS (" + std::to_string((int)FB_MAX_MODELS) + ") models");
  for (int k = 0; k < n_models; k++) if (!models[k]) return fail("fb_batch_create_group: model " + std::to_string(k) + " is null");
  for (int k = 1; k < n_models; k++) {
    std::string why;
    if (const char* name = first_incompatible_array(models[0], models[k], &why))
      return fail("fb_batch_create_group: model " + std::to_string(k) + " is not compatible with model 0: array '" + name + "' " + why +
                  " (the models of a group share dimensions, every integer array and the time steps)");
  }
  return batch_create("fb_batch_create_group", models[0], models, n_models, n_env, device, precision, out);
}

extern "C" int fb_batch_n_models(const fb_batch* b) {
  if (!b) return fail("fb_batch_n_models: null batch");
  return b->n_models();
}

static int batch_create_impl(fb_batch* b) {
  const fb_model* m = b->m; const int n_env = b->n_env;
  const Switches sw{};                  // (the environment as it is now)
  if (with_model(b, [&](auto& M) {
        if (build_devmodel(b, m, sw, M)) return -1;
        compute_offsets(M, b->off); M.off = b->off;
        // a group of more than one model: the structs of all of them (element 0 is refreshed from M by sync_model); every model gets tables of
        // its own, so whatever the host derives from real constants (vl_delta, body_box, geom_box, body_fluid_geom, totalmass) is per model
        if (b->models.size() > 1) {
          auto& G = group_models(b, M);
          G.assign(b->models.size(), M);
          for (size_t k = 1; k < G.size(); k++) { if (build_devmodel(b, b->models[k], sw, G[k])) return -1; G[k].off = b->off; }
        }
        return 0; })) return -1;
  if (!b->models.empty()) {
    std::vector<int> em(n_env);
    for (int e = 0; e < n_env; e++) em[e] = e % b->n_models();
    if (b->env_model.alloc(n_env)) return -1;
    HIPCHK(hipMemcpy(b->env_model.get(), em.data(), n_env*sizeof(int), hipMemcpyHostToDevice));
  }
  const size_t rs = real_size(b);
  if (b->rarena.alloc_zeroed((size_t)n_env*b->off.nreal*rs) || b->iarena.alloc_zeroed((size_t)n_env*b->off.nint)) return -1;
  if (b->reward.alloc_zeroed(n_env) || b->discount.alloc_zeroed(n_env) || b->step_type.alloc_zeroed(n_env)) return -1;
  if (b->d_ids.alloc(n_env) || b->sched.alloc(FB_NSCHED) || b->cost.alloc_zeroed(n_env) || b->order.alloc(n_env)) return -1;
  b->reorder = b->ticket_order = !sw.no_reorder;
  // substep scheduler: for batches larger than the resident wave slots (k_fly)
  {
#ifdef FB_EMULATE
    b->nq = 1; b->slots = 2;                                   // (host emulation: tiny, so that the test batches take the ticket path)
#else
    hipDeviceProp_t prop; HIPCHK(hipGetDeviceProperties(&prop, b->device));
    if (with_model(b, [&](auto& M) {
          using real = decltype(M.timestep);
          // launch_fly may launch any kernel of step_kernels(): the slot count that decides for tickets is the smallest of theirs
          int nb = INT_MAX, nbk = 0;
          for (const void* k : step_kernels<real>()) {
            HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nbk, k, FB_WAVE*LdsCfg<real>::EPB, 0));
            nb = std::min(nb, nbk);
          }
          b->slots = nb*prop.multiProcessorCount*LdsCfg<real>::EPB;
          return 0; })) return -1;
    DevBuf<unsigned> dmask; unsigned hmask = 0;
    if (dmask.alloc_zeroed(1)) return -1;
    hipLaunchKernelGGL(k_probe_xcc, dim3(4096), dim3(FB_WAVE), 0, 0, dmask.get());
    HIPCHK(hipMemcpy(&hmask, dmask.get(), sizeof(unsigned), hipMemcpyDeviceToHost)); dmask.reset();
    int nqq = __builtin_popcount(hmask);
    b->nq = (nqq > 0 && hmask == (1u << nqq) - 1u) ? nqq : 0;          // XCC ids 0 .. nq-1, all seen; anything else: scheduler off
    b->xcc_mask = hmask;
    // the hand-over protocol of the scheduler (k_fly) is written against the cache hierarchy of gfx942 / gfx950: write-through vector
    // L1, one L2 per XCD, HW_REG_XCC_ID.  Any other architecture takes the per-wave path.
    if (strncmp(prop.gcnArchName, "gfx942", 6) != 0 && strncmp(prop.gcnArchName, "gfx950", 6) != 0) b->nq = 0;
    if (sw.ticket_slots) b->slots = atoi(sw.ticket_slots);
#endif
    if (b->tick.alloc(16*16) || b->done.alloc(n_env) || b->torder.alloc((size_t)n_env + 16) || b->sched_err.alloc_zeroed(1) || b->probe_word.alloc(1)) return -1;
    // (round 3 kept flight_imitation -- equal-cost environments, short substeps -- on the per-wave path: tickets cost 3 % there.  With
    // the round-4 kernel they win for flight too: 8192 FP64 environments 2.21 -> 2.25 M env-steps/s on the default build, 2.52 -> 2.63 M
    // on the 12-per-CU build, profiles/r4/flight_variants.txt.  FB_NO_TICKETS=1 still forces the per-wave path.)
    b->tickets = b->nq > 0 && b->slots > 0 && n_env > b->slots && !sw.no_tickets;
  }
  b->use_prio = !sw.no_prio;
  // initial state: qpos0 everywhere (fb_batch_reset overrides it once a reference is set)
  if (with_model(b, [&](auto& M) {
        std::vector<decltype(M.timestep)> rows((size_t)n_env*m->nq);
        for (int e = 0; e < n_env; e++) {
          const double* q0 = (b->models.empty() ? m : b->models[e % b->n_models()])->d("qpos0");
          std::copy_n(q0, m->nq, rows.data() + (size_t)e*m->nq);
        }
        HIPCHK(hipMemcpy2D((char*)b->rarena.get() + (size_t)b->off.qpos*rs, (size_t)b->off.nreal*rs, rows.data(), (size_t)m->nq*rs, (size_t)m->nq*rs, n_env, hipMemcpyHostToDevice));
        return 0; })) return -1;
  b->nobs = 0;
  return 0;
}

extern "C" void fb_batch_destroy(fb_batch* b) {
  if (!b) return;
  (void)hipSetDevice(b->device);
  delete b;                             // (its DevBuf / DevEvent members release the device memory and the events)
}

extern "C" int fb_batch_set_reference(fb_batch* b, const double* ref_qpos, const double* ref_qvel, int T,
                                      int future_steps, double terminal_com_dist, double time_limit) {
  if (!b || !ref_qpos || !ref_qvel || T < 2) return fail("fb_batch_set_reference: bad arguments");
  if (T - future_steps - 1 < 1) return fail("fb_batch_set_reference: trajectory shorter than future_steps + 2");
  HIPCHK(hipSetDevice(b->device));
  b->ref_qpos.reset(); b->ref_qvel.reset(); b->have_ref = false;     // (a failure below leaves the batch without a reference)
  const fb_model* m = b->m;
  int max_steps = (int)floor(time_limit / m->d("opt_control_timestep")[0] + 0.5) + 1;
  int snippet = T - future_steps - 1;
  int episode_steps = max_steps < snippet ? max_steps : snippet;
  if (m->task_id == FB_TASK_FLIGHT_IMITATION) {          // flight_imitation.py:101-105
    int lim = max_steps - 1;
    episode_steps = (T < lim ? T : lim) - (future_steps + 1);
  }
  return with_model(b, [&](auto& M) {
    using real = decltype(M.timestep);
    const std::vector<real> q(ref_qpos, ref_qpos + (size_t)T*7), v(ref_qvel, ref_qvel + (size_t)T*6);
    if (b->ref_qpos.alloc(q.size()*sizeof(real)) || b->ref_qvel.alloc(v.size()*sizeof(real))) return -1;
    HIPCHK(hipMemcpy(b->ref_qpos.get(), q.data(), q.size()*sizeof(real), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(b->ref_qvel.get(), v.data(), v.size()*sizeof(real), hipMemcpyHostToDevice));
    if (alloc_obs(b, obs_width(m, m->task_id == FB_TASK_TEMPLATE ? 0 : future_steps + 1, false))) return -1;      // (template_task: the reference is the start pose only, no reference observables)
    M.ref_qpos = (const real*)b->ref_qpos.get(); M.ref_qvel = (const real*)b->ref_qvel.get(); M.T = T;
    M.future_steps = future_steps; M.episode_steps = episode_steps; M.nobs = b->nobs;
    M.terminal_com_dist = (real)terminal_com_dist; M.time_limit = time_limit;
    b->have_ref = true;
    return 0;
  });
}

extern "C" int fb_batch_set_time_limit(fb_batch* b, double time_limit) {
  if (!b || !(time_limit > 0)) return fail("fb_batch_set_time_limit: bad arguments");
  const fb_model* m = b->m;
  if (m->task_id != FB_TASK_WALK_ON_BALL) return fail("fb_batch_set_time_limit: only the walk_on_ball task has no reference trajectory");
  HIPCHK(hipSetDevice(b->device));
  if (alloc_obs(b, obs_width(m, 0, true))) return -1;
  return with_model(b, [&](auto& M) {
    using real = decltype(M.timestep);
    M.nobs = b->nobs; M.T = 0; M.future_steps = 0; M.episode_steps = 0; M.time_limit = time_limit;
    M.terminal_com_dist = (real)1e30;
    b->have_ref = true;
    return 0;
  });
}

extern "C" int fb_batch_set_wbpg(fb_batch* b, const double* traj, const double* phase, const int32_t* offset, const double* freqs,
                                 int nfreq, double base_freq, double rel_range, double rate, uint32_t seed) {
  if (!b || !traj || !phase || !offset || !freqs || nfreq <= 0) return fail("fb_batch_set_wbpg: bad arguments");
  HIPCHK(hipSetDevice(b->device));
  int rows = offset[nfreq];
  return with_model(b, [&](auto& M) {
    using real = decltype(M.timestep);
    const real *t_, *p_, *f_; const int* o_;
    if (upload<real>(b, traj, (size_t)rows*6, &t_) || upload<real>(b, phase, (size_t)rows, &p_) || upload<real>(b, freqs, (size_t)nfreq, &f_) ||
        upload_i(b, offset, (size_t)nfreq + 1, &o_)) return -1;
    M.wb_traj = t_; M.wb_phase = p_; M.wb_freqs = f_; M.wb_offset = o_; M.wb_nfreq = nfreq; M.wb_base_freq = (real)base_freq;
    M.wb_rel_range = (real)rel_range; M.wb_rate = (real)rate; M.seed = seed;
    b->have_wbpg = true;
    return 0;
  });
}

extern "C" int fb_batch_set_walk_dataset(fb_batch* b, const fb_walk_dataset* ds) {
  if (!b || !ds || !ds->traj_offset || !ds->qpos || !ds->qvel || !ds->root2site || !ds->joint_quat || !ds->joint_ids || !ds->site_ids || !ds->select)
    return fail("fb_batch_set_walk_dataset: null argument");
  if (ds->n_traj <= 0 || ds->n_select <= 0 || ds->n_joints < 0 || ds->n_sites < 0) return fail("fb_batch_set_walk_dataset: bad sizes");
  const fb_model* m = b->m;
  if (m->task_id != FB_TASK_WALK_IMITATION) return fail("fb_batch_set_walk_dataset: not a walk_imitation model");
  for (int k = 0; k < ds->n_joints; k++) if (ds->joint_ids[k] < 0 || ds->joint_ids[k] >= m->njnt) return fail("fb_batch_set_walk_dataset: joint id out of range");
  for (int k = 0; k < ds->n_sites; k++) if (ds->site_ids[k] < 0 || ds->site_ids[k] >= m->nsite) return fail("fb_batch_set_walk_dataset: site id out of range");
  for (int k = 0; k < ds->n_select; k++) {
    int t = ds->select[k];
    if (t < 0 || t >= ds->n_traj) return fail("fb_batch_set_walk_dataset: selected trajectory out of range");
    if (ds->traj_offset[t + 1] - ds->traj_offset[t] - ds->future_steps - 1 < 1) return fail("fb_batch_set_walk_dataset: trajectory shorter than future_steps + 2");
  }
  HIPCHK(hipSetDevice(b->device));
  size_t rows = (size_t)ds->traj_offset[ds->n_traj];
  int nj = ds->n_joints, ns = ds->n_sites, future_steps = ds->future_steps;
  int max_steps = (int)floor(ds->time_limit / m->d("opt_control_timestep")[0] + 0.5) + 1;
  if (alloc_obs(b, obs_width(m, future_steps + 1, false))) return -1;
  return with_model(b, [&](auto& M) {
    using real = decltype(M.timestep);
    const real *q_, *v_, *r_, *j_; const int *o_, *ji_, *si_, *se_;
    if (upload<real>(b, ds->qpos, rows*(7 + nj), &q_) || upload<real>(b, ds->qvel, rows*(6 + nj), &v_) || upload<real>(b, ds->root2site, rows*3*ns, &r_) ||
        upload<real>(b, ds->joint_quat, rows*4*nj, &j_) || upload_i(b, ds->traj_offset, (size_t)ds->n_traj + 1, &o_) || upload_i(b, ds->joint_ids, nj, &ji_) ||
        upload_i(b, ds->site_ids, ns, &si_) || upload_i(b, ds->select, ds->n_select, &se_)) return -1;
    M.ds_qpos = q_; M.ds_qvel = v_; M.ds_r2s = r_; M.ds_jq = j_; M.ds_offset = o_; M.ds_jid = ji_; M.ds_sid = si_; M.ds_select = se_;
    M.ds_nj = nj; M.ds_ns = ns; M.ds_ntraj = ds->n_traj; M.ds_nselect = ds->n_select; M.ds_env_base = ds->env_id_base; M.max_episode_steps = max_steps;
    M.seed = ds->seed; M.future_steps = future_steps; M.nobs = b->nobs; M.T = 0; M.episode_steps = 0;
    M.terminal_com_dist = (real)ds->terminal_com_dist; M.time_limit = ds->time_limit;
    b->have_ref = true;
    return 0;
  });
}

extern "C" int fb_batch_set_flight_dataset(fb_batch* b, const fb_flight_dataset* ds) {
  if (!b || !ds || !ds->traj_offset || !ds->qpos || !ds->qvel || !ds->select) return fail("fb_batch_set_flight_dataset: null argument");
  if (ds->n_traj <= 0 || ds->n_select <= 0 || ds->future_steps < 0) return fail("fb_batch_set_flight_dataset: bad sizes");
  const fb_model* m = b->m;
  if (m->task_id != FB_TASK_FLIGHT_IMITATION) return fail("fb_batch_set_flight_dataset: not a flight_imitation model");
  for (int k = 0; k < ds->n_select; k++) {
    int t = ds->select[k];
    if (t < 0 || t >= ds->n_traj) return fail("fb_batch_set_flight_dataset: selected trajectory out of range");
    int len = ds->traj_offset[t + 1] - ds->traj_offset[t];
    // the shortest slice a random start can leave is 51 rows (start < len - 50); it must still hold future_steps + 2 rows
    if (len < 52 || (ds->randomize_start_step ? 51 : len) - ds->future_steps - 1 < 1) return fail("fb_batch_set_flight_dataset: trajectory too short (needs > 51 rows and future_steps + 2 rows after any start)");
  }
  HIPCHK(hipSetDevice(b->device));
  size_t rows = (size_t)ds->traj_offset[ds->n_traj];
  int future_steps = ds->future_steps;
  if (alloc_obs(b, obs_width(m, future_steps + 1, false))) return -1;
  return with_model(b, [&](auto& M) {
    using real = decltype(M.timestep);
    const real *q_, *v_; const int *o_, *se_;
    if (upload<real>(b, ds->qpos, rows*7, &q_) || upload<real>(b, ds->qvel, rows*6, &v_) ||
        upload_i(b, ds->traj_offset, (size_t)ds->n_traj + 1, &o_) || upload_i(b, ds->select, ds->n_select, &se_)) return -1;
    M.ds_qpos = q_; M.ds_qvel = v_; M.ds_offset = o_; M.ds_select = se_; M.ds_nj = 0; M.ds_ns = 0; M.ds_ntraj = ds->n_traj;
    M.ds_nselect = ds->n_select; M.ds_env_base = ds->env_id_base; M.ds_random_start = ds->randomize_start_step ? 1 : 0;
    M.seed = ds->seed; M.future_steps = future_steps; M.nobs = b->nobs; M.T = 0; M.episode_steps = 0;
    M.terminal_com_dist = (real)ds->terminal_com_dist; M.time_limit = ds->time_limit;
    b->have_ref = true;
    return 0;
  });
}

// the step kernel launch of launch(): one of step_kernels(), or for a reset k_fly_reset / k_group_reset
template <typename real>
static void launch_fly(fb_batch* b, int mode, const float* action, const int* ids, int n, int nsub, hipStream_t st, bool tickets, const int* tord) {
  constexpr int EPB = LdsCfg<real>::EPB;
  const DevModel<real>* dM = (const DevModel<real>*)b->dM.get();    // (a grouped batch: the array of the group's model structs)
  Batch<real> B = {(real*)b->rarena.get(), b->iarena.get(), b->obs.get(), b->reward.get(), b->discount.get(), b->step_type.get(), b->n_env, b->nobs,
                   b->use_prio ? b->sched.get() : nullptr, b->cost.get(), tickets ? b->tick.get() : nullptr, b->done.get(), b->nq, b->sched_err.get(), tord, (real*)b->park.get()};
  const ForceArgs<real> F = {(const real*)b->qfrc_applied.get(), (const real*)b->xfrc_applied.get()};
  const LawArgs<real> L = {(const real*)b->law_coef.get(), b->law_qadr.get(), (real*)b->law_out.get(), b->law_rows > 1 || b->n_env == 1 ? 1 : 0};
  const GroupArgs G = {b->env_model.get(), b->n_models()};
  const dim3 grid((n + EPB - 1)/EPB), block(FB_WAVE*EPB);
  auto go = [&](auto kernel, auto... args) { hipLaunchKernelGGL(kernel, grid, block, 0, st, dM, B, args...); };
  if (b->n_models() > 1) {
    // a grouped batch: the kernels that bind the model per environment
    if (mode == MODE_RESET) go(k_group_reset<real>, ids, nsub, n, G);
    else if (b->qfrc_applied) go(k_group_step<real, true>, action, ids, mode, nsub, n, F, G);
    else go(k_group_step<real, false>, action, ids, mode, nsub, n, F, G);
  }
  else if (mode == MODE_RESET) go(k_fly_reset<real>, ids, nsub, n);
  else if (b->law_coef) go(k_step_law<real>, action, ids, mode, nsub, n, F, L);
  else if (b->qfrc_applied) go(k_step_forces<real>, action, ids, mode, nsub, n, F);
  else go(k_fly<real>, action, ids, mode, nsub, n);
}

static int launch(fb_batch* b, int mode, const float* action, const int* ids, int n, int nsub, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (sync_model(b)) return -1;
  HIPCHK(hipMemsetAsync(b->sched.get(), 0, FB_NSCHED*sizeof(int), st));
  // a control step of the whole batch: substep scheduler when the batch exceeds the resident slots, otherwise one environment per
  // wave in longest-first order
  bool tickets = (mode == MODE_STEP) && !ids && n == b->n_env && b->tickets;
#ifndef FB_EMULATE
  if (tickets && std::find(b->probed_streams.begin(), b->probed_streams.end(), stream) == b->probed_streams.end()) {
    // A stream with a CU mask may not reach every XCD: the ticket queues of the unreachable ones would never be drawn.  Every stream
    // is probed ONCE (the validated ones are remembered: a caller that alternates streams pays no blocking synchronisation per
    // step); a stream that does not see exactly the XCDs the batch was set up for puts this batch on the per-wave path for good.
    // The probe synchronises, so it cannot run while the stream is being captured into a graph: such a launch takes the per-wave
    // path (same results) and the stream stays unvalidated.
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) != hipSuccess) { (void)hipGetLastError(); cap = hipStreamCaptureStatusActive; }      // (the legacy stream under another stream's global-mode capture: the query fails -- treat as capturing, never synchronise)
    if (cap != hipStreamCaptureStatusNone) tickets = false;
    else {
      unsigned hmask = 0;
      HIPCHK(hipMemsetAsync(b->probe_word.get(), 0, sizeof(unsigned), st));
      hipLaunchKernelGGL(k_probe_xcc, dim3(4096), dim3(FB_WAVE), 0, st, b->probe_word.get());
      HIPCHK(hipMemcpyAsync(&hmask, b->probe_word.get(), sizeof(unsigned), hipMemcpyDeviceToHost, st)); HIPCHK(hipStreamSynchronize(st));
      if (hmask != b->xcc_mask) { b->tickets = false; tickets = false; }
      else { if (b->probed_streams.size() >= 64) b->probed_streams.clear(); b->probed_streams.push_back(stream); }
    }
  }
#endif
  const bool full_step = (mode == MODE_STEP) && !ids && n == b->n_env && b->reorder && !tickets;
  if (full_step && b->order_valid) ids = b->order.get();       // slowest environments of the previous step first
  if (tickets) {
    HIPCHK(hipMemsetAsync(b->tick.get(), 0, 16*16*sizeof(int), st)); HIPCHK(hipMemsetAsync(b->done.get(), 0, (size_t)n*sizeof(int), st));
    if (b->ticket_order) hipLaunchKernelGGL(k_ticket_order, dim3(b->nq), dim3(FB_ORDER_THREADS), 0, st, (const int*)b->iarena.get(), (int)b->off.nint, (int)(b->off.istate + IS_NEFC), b->torder.get(), n, b->nq);
  }
  const int* tord = (tickets && b->ticket_order) ? b->torder.get() : nullptr;
  const int FB_TIMED_MAX = 2048;
  const bool per_launch = b->timing && mode == MODE_STEP && b->timed_launches < FB_TIMED_MAX;
  if (per_launch) {
    while ((int)b->lev.size() < 2*(b->timed_launches + 1)) { DevEvent nev; if (nev.create()) return -1; b->lev.push_back(std::move(nev)); }
    HIPCHK(hipEventRecord(b->lev[2*b->timed_launches].get(), st));
  }
  with_model(b, [&](auto& M) { launch_fly<decltype(M.timestep)>(b, mode, action, ids, n, nsub, st, tickets, tord); });
  if (per_launch) HIPCHK(hipEventRecord(b->lev[2*b->timed_launches + 1].get(), st));
  if (full_step) { hipLaunchKernelGGL(k_order, dim3(1), dim3(FB_ORDER_THREADS), 0, st, b->cost.get(), b->order.get(), n); b->order_valid = true; }
  HIPCHK(hipGetLastError());
  if (b->timing) b->timed_launches++;
  return 0;
}

// the tables a control step reads are set: a reference (or dataset / time limit) and, with `wbpg`, flight's pattern generator
static int check_ready(const fb_batch* b, const char* fn, bool wbpg) {
  if (!b->have_ref) return fail(std::string(fn) + ": call fb_batch_set_reference first");
  if (wbpg && b->m->task_id == FB_TASK_FLIGHT_IMITATION && !b->have_wbpg) return fail(std::string(fn) + ": flight task needs fb_batch_set_wbpg first");
  return 0;
}

extern "C" int fb_batch_reset(fb_batch* b, const int32_t* env_ids, int n, void* stream) {
  if (!b) return fail("fb_batch_reset: null batch");
  if (check_ready(b, "fb_batch_reset", true)) return -1;
  HIPCHK(hipSetDevice(b->device));
  if (env_ids) {
    if (n <= 0 || n > b->n_env) return fail("fb_batch_reset: bad n");
    for (int k = 0; k < n; k++) if (env_ids[k] < 0 || env_ids[k] >= b->n_env) return fail("fb_batch_reset: env id out of range");
    HIPCHK(hipMemcpyAsync(b->d_ids.get(), env_ids, n*sizeof(int), hipMemcpyHostToDevice, (hipStream_t)stream));
    if (b->law_out) {                                   // a reset skips the law: FB_QFRC_LAW of the reset environments is zero (k_fly_reset knows no law)
      hipLaunchKernelGGL(k_zero_rows, dim3(n), dim3(FB_WAVE), 0, (hipStream_t)stream, (uint32_t*)b->law_out.get(), (const int*)b->d_ids.get(), n, (unsigned)(b->m->nv*real_size(b)/4));
    }
    return launch(b, MODE_RESET, nullptr, b->d_ids.get(), n, 0, stream);
  }
  if (b->law_out) HIPCHK(hipMemsetAsync(b->law_out.get(), 0, (size_t)b->n_env*b->m->nv*real_size(b), (hipStream_t)stream));
  return launch(b, MODE_RESET, nullptr, nullptr, b->n_env, 0, stream);
}

extern "C" int fb_batch_step(fb_batch* b, const float* action, void* stream) {
  if (!b || !action) return fail("fb_batch_step: null argument");
  if (check_ready(b, "fb_batch_step", true)) return -1;
  HIPCHK(hipSetDevice(b->device));
  return launch(b, MODE_STEP, action, nullptr, b->n_env, 0, stream);
}

extern "C" int fb_batch_substep(fb_batch* b, int nsub, void* stream) {
  if (!b || nsub < 0) return fail("fb_batch_substep: bad arguments");
  HIPCHK(hipSetDevice(b->device));
  return launch(b, MODE_SUBSTEP, nullptr, nullptr, b->n_env, nsub, stream);
}

extern "C" int fb_batch_forward(fb_batch* b, void* stream) {
  if (!b) return fail("fb_batch_forward: null batch");
  HIPCHK(hipSetDevice(b->device));
  return launch(b, MODE_FORWARD, nullptr, nullptr, b->n_env, 0, stream);
}

// The streams a batch was validated on are remembered by handle.  A caller that DESTROYS a stream must say so: a new stream (possibly with a
// CU mask that hides an XCD) may reuse the handle and would skip the probe -- its unreachable ticket queues would never be drawn.
extern "C" int fb_batch_forget_stream(fb_batch* b, void* stream) {
  if (!b) return fail("fb_batch_forget_stream: null batch");
  b->probed_streams.erase(std::remove(b->probed_streams.begin(), b->probed_streams.end(), stream), b->probed_streams.end());
  return 0;
}

// substep scheduler: a control step that abandoned tickets (capped wait, k_fly) left environments half-stepped -- sticky failure
static int check_sched_errors(fb_batch* b) {
  int n = 0;
  HIPCHK(hipMemcpy(&n, b->sched_err.get(), sizeof(int), hipMemcpyDeviceToHost));
  if (n) return fail("substep scheduler: " + std::to_string(n) + " ticket(s) were abandoned because the wait for an environment's previous substep hit its cap; "
                     "the flagged environments (FB_WARN_SCHED_WAIT) are not in a valid state and this batch fails from now on (sticky, include/flybody_engine.h): "
                     "destroy it and create a new one; FB_NO_TICKETS=1 selects the per-wave path");
  return 0;
}

extern "C" int fb_batch_synchronize(fb_batch* b, void* stream) {
  if (!b) return fail("fb_batch_synchronize: null batch");
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  return check_sched_errors(b);
}

// Profiling / debug: ONE stage of a control step for every environment (fb_step.hpp MODE_STAGE).  The caller walks the stage sequence
// of a control step itself (tools/stage_profile.py); results equal fb_batch_step's as long as no environment ends its episode.
extern "C" int fb_batch_stage(fb_batch* b, int stage_word, const float* action, void* stream) {
  if (!b || stage_word < 0) return fail("fb_batch_stage: bad arguments");
  if (check_ready(b, "fb_batch_stage", false)) return -1;
  if (b->n_models() > 1) return fail("fb_batch_stage: single-stage profiling runs k_fly, which steps one model; this batch is a group of " + std::to_string(b->n_models()) + " models (fb_batch_create_group)");
  if (b->law_coef) return fail("fb_batch_stage: single-stage profiling runs k_fly, which knows no control law; call fb_batch_set_control_law(batch, NULL) first");
  if (b->qfrc_applied) return fail("fb_batch_stage: single-stage profiling runs k_fly, which knows no applied forces; call fb_batch_clear_forces first");
  HIPCHK(hipSetDevice(b->device));
  const size_t pool = with_model(b, [](auto& M) { return sizeof(M.timestep)*LdsCfg<decltype(M.timestep)>::POOL; });
  if (alloc_zeroed_once(b->park, (size_t)b->n_env*pool)) return -1;
  return launch(b, MODE_STAGE, action, nullptr, b->n_env, stage_word, stream);
}

// ------------------------------------------------------------------ inverse kinematics
// Multi-site IK, one frame per environment (fb_ik.hpp: k_ik).  Not a control step: it does not go through launch(), is not a timed launch
// and changes nothing of the environment's state but qpos and the position-stage outputs computed from it.
extern "C" int fb_batch_ik(fb_batch* b, const fb_ik_config* cfg, const double* target_xpos, void* stream) {
  if (!b || !cfg || !target_xpos) return fail("fb_batch_ik: null argument");
  if (b->precision != 64) return fail("fb_batch_ik: inverse kinematics needs an FP64 batch (precision 64)");
  if (b->n_models() > 1) return fail("fb_batch_ik: per-model inverse kinematics is not supported: this batch is a group of " + std::to_string(b->n_models()) + " models (fb_batch_create_group)");
  if (b->law_coef) return fail("fb_batch_ik: the IK kernel knows no control law, and its position-stage outputs would not be the law kernel's; call fb_batch_set_control_law(batch, NULL) first");
  const fb_model* m = b->m;
  const int ns = cfg->n_site, nj = cfg->n_joint, n = b->n_env;
  if (ns < 1 || !cfg->site_ids || !cfg->include) return fail("fb_batch_ik: at least one site (and its include mask) is required");
  if (nj < 0 || (nj > 0 && !cfg->joint_ids)) return fail("fb_batch_ik: bad joint list");
  if (!std::isfinite(cfg->reg_strength) || !std::isfinite(cfg->lr) || !std::isfinite(cfg->beta) || !std::isfinite(cfg->progress_threshold))
    return fail("fb_batch_ik: hyper-parameters must be finite");
  if (cfg->max_steps < 1) return fail("fb_batch_ik: max_steps must be >= 1");
  if (std::max({7*m->nbody + 10*m->njnt, 6*m->nv + 10*m->nbody, 7*m->nv + 6*m->nbody}) > FB_IK_POOL) return fail("fb_batch_ik: model exceeds the IK LDS pool (FB_IK_POOL)");
  FB_GUARD_BEGIN
  const int *sbody = m->i("site_bodyid"), *jt = m->i("jnt_type"), *jda = m->i("jnt_dofadr"), *jqa = m->i("jnt_qposadr");
  std::vector<char> seen(std::max(m->nsite, m->njnt), 0);
  for (int k = 0; k < ns; k++) {
    const int s = cfg->site_ids[k];
    if (s < 0 || s >= m->nsite) return fail("fb_batch_ik: site id out of range");
    if (seen[s]) return fail("fb_batch_ik: duplicate site id");
    seen[s] = 1;
  }
  for (int k = 0; k < 3*ns; k++) if (cfg->include[k] != 0 && cfg->include[k] != 1) return fail("fb_batch_ik: include mask entries must be 0 or 1");
  std::fill(seen.begin(), seen.end(), 0);
  // joints -> dofs (the reference's dof_jntid row indexer), hinge dofs carry their qpos address (regularisation)
  std::vector<int> dof, dof_hq;
  for (int k = 0; k < nj; k++) {
    const int j = cfg->joint_ids[k];
    if (j < 0 || j >= m->njnt) return fail("fb_batch_ik: joint id out of range");
    if (seen[j]) return fail("fb_batch_ik: duplicate joint id");
    seen[j] = 1;
    const int nd = jt[j] == JNT_FREE ? 6 : (jt[j] == JNT_BALL ? 3 : 1);
    for (int d = 0; d < nd; d++) { dof.push_back(jda[j] + d); dof_hq.push_back(jt[j] == JNT_HINGE ? jqa[j] : -1); }
  }
  if ((int)dof.size() > 2*FB_WAVE) return fail("fb_batch_ik: more than 128 dofs");
  for (size_t k = 0; k < (size_t)n*3*ns; k++) if (std::isnan(target_xpos[k])) return fail("fb_batch_ik: target_xpos holds NaN");
  // the sites of every body (the kernel sums a body's point forces on one lane, in site-list order)
  std::vector<int> boff(m->nbody + 1, 0), bsite(ns);
  for (int k = 0; k < ns; k++) boff[sbody[cfg->site_ids[k]] + 1]++;
  for (int bb = 0; bb < m->nbody; bb++) boff[bb + 1] += boff[bb];
  { std::vector<int> fill(boff.begin(), boff.end() - 1); for (int k = 0; k < ns; k++) bsite[fill[sbody[cfg->site_ids[k]]]++] = k; }
  // one device buffer: int tables, then the targets
  const size_t nd = dof.size();
  std::vector<int> it;
  auto put = [&](const int* p, size_t c) { size_t o = it.size(); it.insert(it.end(), p, p + c); return o; };
  const size_t o_site = put(cfg->site_ids, ns), o_boff = put(boff.data(), boff.size()), o_bsite = put(bsite.data(), ns),
               o_inc = put(cfg->include, 3*(size_t)ns), o_dof = put(dof.data(), nd), o_hq = put(dof_hq.data(), nd);
  const size_t tgt_off = ((it.size()*sizeof(int) + 255) & ~(size_t)255), bytes = tgt_off + (size_t)n*3*ns*sizeof(double);
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipDeviceSynchronize());                      // (a previous IK launch may still read the buffer)
  if (alloc_zeroed_once(b->ik_err, (size_t)n*2) || alloc_zeroed_once(b->ik_steps, (size_t)n*2) || b->ik_buf.reserve(bytes)) return -1;
  HIPCHK(hipMemcpy(b->ik_buf.get(), it.data(), it.size()*sizeof(int), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy((char*)b->ik_buf.get() + tgt_off, target_xpos, (size_t)n*3*ns*sizeof(double), hipMemcpyHostToDevice));
  if (sync_model(b)) return -1;
  const int* ib = (const int*)b->ik_buf.get();
  IKArgs<double> A;
  A.site = ib + o_site; A.bsite_off = ib + o_boff; A.bsite = ib + o_bsite; A.include = ib + o_inc; A.dof = ib + o_dof; A.dof_hq = ib + o_hq;
  A.target = (const double*)((const char*)b->ik_buf.get() + tgt_off); A.err = b->ik_err.get(); A.steps = b->ik_steps.get();
  A.n_site = ns; A.n_dof = (int)nd; A.max_steps = cfg->max_steps; A.n_env = n;
  A.reg = cfg->reg_strength; A.lr = cfg->lr; A.beta = cfg->beta; A.thr = cfg->progress_threshold;
  hipLaunchKernelGGL((k_ik<double>), dim3(n), dim3(FB_WAVE), 0, (hipStream_t)stream, (const DevModel<double>*)b->dM.get(), (double*)b->rarena.get(), b->iarena.get(), A);
  HIPCHK(hipGetLastError());
  return 0;
  FB_GUARD_END
}

// ------------------------------------------------------------------ the calls beside the step (the kernels of fb_side.hpp)
// fb_batch_inverse, fb_batch_transition_fd and the two rollout calls do not go through launch() and are not timed launches.  Each keeps its own
// body; what they literally repeated is stated here.

// The refusals of an FP64 side call, in their order.  The texts' words: needs "<what> need(s)", per_model "<what> is / are", kernel the
// kernel's name, law_why what the inverse adds about the law; forces: applied forces are refused too (the inverse allows them).
static int side_refusals(const fb_batch* b, const std::string& fn, const char* needs, const char* per_model, const char* kernel, const char* law_why, bool forces) {
  if (b->precision != 64) return fail(fn + ": " + needs + " an FP64 batch (precision 64)");
  if (b->n_models() > 1) return fail(fn + ": per-model " + per_model + " not supported: this batch is a group of " + std::to_string(b->n_models()) + " models (fb_batch_create_group)");
  if (b->law_coef) return fail(fn + ": the " + kernel + " knows no control law" + law_why + "; call fb_batch_set_control_law(batch, NULL) first");
  if (forces && b->qfrc_applied) return fail(fn + ": the " + kernel + " knows no applied forces; call fb_batch_clear_forces first");
  return 0;
}
// An optional list of n source environments (null: 0 .. n-1); count / item: the texts' names ("n_frames" / "frame").
static int side_check_env_ids(const fb_batch* b, const std::string& fn, const int32_t* env_ids, int n, const char* count, const char* item) {
  if (!env_ids && n > b->n_env) return fail(fn + ": environment id out of range (" + count + " exceeds the batch and env_ids is NULL)");
  if (env_ids) for (int k = 0; k < n; k++) if (env_ids[k] < 0 || env_ids[k] >= b->n_env)
    return fail(fn + ": environment id " + std::to_string(env_ids[k]) + " out of range (" + item + " " + std::to_string(k) + ")");
  return 0;
}
// Rows `kernel` keeps resident (occupancy x CUs x EPB), at most `cap` where cap > 0, at least 1; cached in `slots`.
static int side_resident_rows(fb_batch* b, const void* kernel, int cap, int& slots) {
  if (slots > 0) return 0;
#ifdef FB_EMULATE
  (void)kernel; (void)cap; slots = 8;                        // (host emulation has no residency: a few rows, so that the tests can vary the pool)
#else
  hipDeviceProp_t prop; HIPCHK(hipGetDeviceProperties(&prop, b->device));
  constexpr int EPB = LdsCfg<double>::EPB;
  int nbk = 0;
  HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nbk, kernel, FB_WAVE*EPB, 0));
  const int own = nbk*prop.multiProcessorCount*EPB;
  slots = std::max(1, cap > 0 ? std::min(cap, own) : own);
#endif
  return 0;
}
// The pool of scratch rows: as many as k_transition_fd keeps resident, at most the step kernel's slots; allocated by the first call that gets that far.
static int side_pool_rows(fb_batch* b) { return side_resident_rows(b, (const void*)k_transition_fd<double>, b->slots, b->fd_slots); }
static int side_pool(fb_batch* b) {
  return alloc_zeroed_once(b->fd_pool_r, (size_t)b->fd_slots*b->off.nreal) || alloc_zeroed_once(b->fd_pool_i, (size_t)b->fd_slots*b->off.nint) ? -1 : 0;
}
// Word [1] of a ticket counter {next ticket, tickets finished since the call began}.  Synchronises the device.
static int side_tickets_done(fb_batch* b, const DevBuf<int>& counter, int64_t* n) {
  *n = 0;
  if (!counter) return 0;
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipDeviceSynchronize());
  int c[2] = {0, 0};
  HIPCHK(hipMemcpy(c, counter.get(), sizeof(c), hipMemcpyDeviceToHost));
  *n = c[1];
  return 0;
}

// ------------------------------------------------------------------ inverse dynamics
// mj_inverse, one frame per environment (fb_inverse.hpp: k_inverse).  It reads FB_QPOS / FB_QVEL / FB_QACC and changes nothing a later
// control step reads (see fb_inverse.hpp).
extern "C" int fb_batch_inverse(fb_batch* b, int flags, void* stream) {
  if (!b) return fail("fb_batch_inverse: null batch");
  if (side_refusals(b, "fb_batch_inverse", "inverse dynamics needs", "inverse dynamics is", "inverse", ": qfrc_inverse would count the law's force as external", false)) return -1;
  if (flags & ~FB_INV_DISCRETE) return fail("fb_batch_inverse: unknown flags");
  FB_GUARD_BEGIN
  const int n = b->n_env, nv = b->m->nv;
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipDeviceSynchronize());                      // (the qacc check below reads what earlier launches wrote)
  {
    std::vector<double> qacc((size_t)n*nv);
    HIPCHK(hipMemcpy2D(qacc.data(), (size_t)nv*8, (char*)b->rarena.get() + (size_t)b->off.qacc*8, (size_t)b->off.nreal*8, (size_t)nv*8, n, hipMemcpyDeviceToHost));
    for (size_t k = 0; k < qacc.size(); k++)
      if (!std::isfinite(qacc[k])) return fail("fb_batch_inverse: FB_QACC of environment " + std::to_string(k/nv) + " is not finite");
  }
  if (alloc_zeroed_once(b->inv_qfrc, (size_t)n*nv) || alloc_zeroed_once(b->inv_cforce, (size_t)n*3*FB_MAXCON_)) return -1;
  if (sync_model(b)) return -1;
  InvArgs<double> A;
  A.qfrc_inverse = b->inv_qfrc.get(); A.contact_force = b->inv_cforce.get(); A.n_env = n;
  A.flags = (flags & FB_INV_DISCRETE) ? FB_INV_FLAG_DISCRETE : 0;
  constexpr int EPB = LdsCfg<double>::EPB;
  hipLaunchKernelGGL((k_inverse<double>), dim3((n + EPB - 1)/EPB), dim3(FB_WAVE*EPB), 0, (hipStream_t)stream, (const DevModel<double>*)b->dM.get(),
                     (double*)b->rarena.get(), b->iarena.get(), A);
  HIPCHK(hipGetLastError());
  return 0;
  FB_GUARD_END
}

// ------------------------------------------------------------------ transition derivatives
// mjd_transitionFD for the listed environments (fb_deriv.hpp: k_transition_fd draws (frame, column, side) tickets onto a pool of scratch rows,
// k_fd_assemble forms the quotients).  The environments' rows are only read: state, caches, warm start, warnings, size statistics and step
// ticks stay as they were.
extern "C" int fb_batch_transition_fd(fb_batch* b, const fb_fd_config* cfg, double* A, double* Bm, double* Cm, double* Dm, int32_t* status, void* stream) {
  if (!b) return fail("fb_batch_transition_fd: null batch");
  if (!cfg) return fail("fb_batch_transition_fd: null config");
  if (side_refusals(b, "fb_batch_transition_fd", "transition derivatives need", "derivatives are", "derivative kernel", "", true)) return -1;
  if (!A && !Bm && !Cm && !Dm) return fail("fb_batch_transition_fd: all four outputs are NULL");
  if (!std::isfinite(cfg->eps) || !(cfg->eps > 0)) return fail("fb_batch_transition_fd: eps must be finite and > 0");
  if (cfg->n_substeps < 1) return fail("fb_batch_transition_fd: n_substeps must be >= 1");
  if (cfg->n_frames < 1) return fail("fb_batch_transition_fd: n_frames must be >= 1");
  if (cfg->centered != 0 && cfg->centered != 1) return fail("fb_batch_transition_fd: centered must be 0 or 1");
  if (side_check_env_ids(b, "fb_batch_transition_fd", cfg->env_ids, cfg->n_frames, "n_frames", "frame")) return -1;
  FB_GUARD_BEGIN
  HIPCHK(hipSetDevice(b->device));
  if (side_pool_rows(b)) return -1;
  if (cfg->pool_rows < 0 || cfg->pool_rows > b->fd_slots) return fail("fb_batch_transition_fd: pool_rows out of range (0, or 1 .. " + std::to_string(b->fd_slots) + " resident slots)");
  hipStream_t st = (hipStream_t)stream;
  const fb_model* m = b->m;
  const int nf = cfg->n_frames, ndx = 2*m->nv + m->na, nst = m->nq + m->nv + m->na + FB_NSENS;
  const int c0 = (A || Cm) ? 0 : ndx, c1 = (Bm || Dm) ? ndx + m->nu : ndx, sides = cfg->centered ? 2 : 1, per_frame = 1 + sides*(c1 - c0);
  if (c1 <= c0) return fail("fb_batch_transition_fd: the outputs asked for have no column (a model without controls has no B or D)");
  if (side_pool(b) || alloc_zeroed_once(b->fd_counter, 2)) return -1;
  // frames per chunk: the tickets' staging slots stay inside the budget
  const size_t frame_bytes = (size_t)per_frame*nst*sizeof(double);
  const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)nf, FB_FD_STAGING_BYTES/frame_bytes));
  const size_t stage_n = chunk*frame_bytes/sizeof(double);
  if (b->fd_stage.count() < stage_n || b->fd_env.count() < (size_t)nf) {
    HIPCHK(hipDeviceSynchronize());                    // (an earlier call may still use the buffers)
    if (b->fd_stage.reserve(stage_n) || b->fd_env.reserve(nf)) return -1;
  }
  b->fd_env_host.resize(nf);
  for (int k = 0; k < nf; k++) b->fd_env_host[k] = cfg->env_ids ? cfg->env_ids[k] : k;
  HIPCHK(hipMemcpyAsync(b->fd_env.get(), b->fd_env_host.data(), (size_t)nf*sizeof(int), hipMemcpyHostToDevice, st));
  if (sync_model(b)) return -1;
  if (status) HIPCHK(hipMemsetAsync(status, 0, (size_t)nf*sizeof(int32_t), st));
  HIPCHK(hipMemsetAsync(b->fd_counter.get(), 0, 2*sizeof(int), st));
  constexpr int EPB = LdsCfg<double>::EPB;
  const int pool = cfg->pool_rows > 0 ? cfg->pool_rows : b->fd_slots;
  for (int lo = 0; lo < nf; lo += chunk) {
    const int n = std::min(chunk, nf - lo);
    FdArgs<double> F;
    F.rarena = (const double*)b->rarena.get(); F.iarena = b->iarena.get(); F.pool_r = b->fd_pool_r.get(); F.pool_i = b->fd_pool_i.get();
    F.frame_env = b->fd_env.get() + lo; F.stage = b->fd_stage.get(); F.counter = b->fd_counter.get(); F.status = status ? (int*)status + lo : nullptr;
    F.A = A ? A + (size_t)lo*ndx*ndx : nullptr; F.B = Bm ? Bm + (size_t)lo*ndx*m->nu : nullptr;
    F.C = Cm ? Cm + (size_t)lo*FB_NSENS*ndx : nullptr; F.D = Dm ? Dm + (size_t)lo*FB_NSENS*m->nu : nullptr;
    F.eps = cfg->eps; F.n_frames = n; F.c0 = c0; F.c1 = c1; F.centered = cfg->centered; F.n_substeps = cfg->n_substeps;
    F.skip_tail = (!Cm && !Dm) ? 1 : 0;
    const long long tickets = (long long)n*per_frame;
    F.nwave = (int)std::min<long long>(pool, tickets);
    if (lo > 0) HIPCHK(hipMemsetAsync(b->fd_counter.get(), 0, sizeof(int), st));      // (the next-ticket word; the run count goes on)
    hipLaunchKernelGGL((k_transition_fd<double>), dim3((F.nwave + EPB - 1)/EPB), dim3(FB_WAVE*EPB), 0, st, (const DevModel<double>*)b->dM.get(), F);
    hipLaunchKernelGGL((k_fd_assemble<double>), dim3(n*(c1 - c0)), dim3(FB_WAVE), 0, st, (const DevModel<double>*)b->dM.get(), F);
  }
  HIPCHK(hipGetLastError());
  return 0;
  FB_GUARD_END
}

// Tickets the last fb_batch_transition_fd call ran (perturbed and nominal transitions; a ctrl side that a range limit forbids is not run).
// Synchronises the device.  A debug counter: the tests count columns with it instead of timing them.
extern "C" int fb_batch_fd_tickets(fb_batch* b, int64_t* n) {
  if (!b || !n) return fail("fb_batch_fd_tickets: null argument");
  return side_tickets_done(b, b->fd_counter, n);
}

// ------------------------------------------------------------------ rollouts, open and closed loop
// MuJoCo's rollout for the listed environments (fb_rollout.hpp: k_rollout / k_closedloop_rollout draw one ticket per rollout onto the scratch
// rows fb_batch_transition_fd owns too); the environments' rows are only read.  Steady state: no host synchronisation, one upload (the rollouts' source environments, and their nominals behind them).
// Both entry points are run_rollout: fbk == NULL is the open-loop one.  fn: the entry point's name, for the refusals.
static int run_rollout(fb_batch* b, const std::string& fn, const fb_rollout_config* cfg, const double* ctrl, const float* action, const fb_feedback* fbk,
                       bool feedback, double* state, double* sensordata, double* ctrl_out, int32_t* status, void* stream) {
  if (!b) return fail(fn + ": null batch");
  if (!cfg) return fail(fn + ": null config");
  if (side_refusals(b, fn, "rollouts need", "rollouts are", "rollout kernel", "", true)) return -1;
  if (!state) return fail(fn + ": the state output is NULL");
  if (!feedback) {
    if (ctrl && action) return fail(fn + ": both ctrl and action are given; a rollout takes exactly one of them");
    if (!ctrl && !action) return fail(fn + ": neither ctrl nor action is given; a rollout takes exactly one of them");
  }
  if (cfg->n_roll < 1) return fail(fn + ": n_roll must be >= 1");
  if (cfg->horizon < 1) return fail(fn + ": horizon must be >= 1");
  if (cfg->n_substeps < 0) return fail(fn + ": n_substeps must be >= 0 (0: the model's own)");
  if (side_check_env_ids(b, fn, cfg->env_ids, cfg->n_roll, "n_roll", "rollout")) return -1;
  if (action && b->m->task_id == FB_TASK_FLIGHT_IMITATION && !b->have_wbpg) return fail(fn + ": an action rollout of the flight task needs fb_batch_set_wbpg first");
  if (feedback) {
    if (!fbk) return fail(fn + ": null feedback");
    if (!fbk->x_nom) return fail(fn + ": x_nom is NULL");
    if (!fbk->u_nom) return fail(fn + ": u_nom is NULL");
    if (fbk->n_nom < 1) return fail(fn + ": n_nom must be >= 1");
    if (!fbk->nom_ids && fbk->n_nom != cfg->n_roll) return fail(fn + ": nom_ids is NULL and n_nom (" + std::to_string(fbk->n_nom) + ") is not n_roll (" + std::to_string(cfg->n_roll) + ")");
    if (fbk->nom_ids) for (int k = 0; k < cfg->n_roll; k++) if (fbk->nom_ids[k] < 0 || fbk->nom_ids[k] >= fbk->n_nom)
      return fail(fn + ": nominal id " + std::to_string(fbk->nom_ids[k]) + " out of range (rollout " + std::to_string(k) + ")");
    if (2*b->m->nv + b->m->na > FB_WAVE*FeedbackArgs<double>::DXSLOTS)
      return fail(fn + ": the model's tangent space (2 nv + na) exceeds the feedback kernel's " + std::to_string(FB_WAVE*FeedbackArgs<double>::DXSLOTS) + " dx registers");
  }
  FB_GUARD_BEGIN
  HIPCHK(hipSetDevice(b->device));
  int& slots = feedback ? b->roll_fb_slots : b->roll_slots;       // the rows this call's own kernel keeps resident, at most the pool's
  if (side_pool_rows(b) ||
      side_resident_rows(b, feedback ? (const void*)k_closedloop_rollout<double> : (const void*)k_rollout<double>, b->fd_slots, slots)) return -1;
  if (cfg->pool_rows < 0 || cfg->pool_rows > slots) return fail(fn + ": pool_rows out of range (0, or 1 .. " + std::to_string(slots) + " scratch rows)");
  hipStream_t st = (hipStream_t)stream;
  const int nr = cfg->n_roll;
  if (side_pool(b) || alloc_zeroed_once(b->roll_counter, 2)) return -1;
  const int nsub = cfg->n_substeps > 0 ? cfg->n_substeps : b->m->nsubstep;
  const size_t nctr = (size_t)cfg->horizon*nsub;        // one progress counter per substep of a rollout (k_rollout: tail-aware priorities)
  const size_t nids = (size_t)nr*(feedback ? 2 : 1);    // the environments, and for a closed-loop call the nominals behind them: one upload
  if (b->roll_env.count() < nids || b->roll_sched.count() < nctr) {
    HIPCHK(hipDeviceSynchronize());                    // (an earlier call may still read them)
    if (b->roll_env.reserve(nids) || b->roll_sched.reserve(nctr)) return -1;
  }
  b->roll_env_host.resize(nids);
  for (int k = 0; k < nr; k++) b->roll_env_host[k] = cfg->env_ids ? cfg->env_ids[k] : k;
  if (feedback) for (int k = 0; k < nr; k++) b->roll_env_host[nr + k] = fbk->nom_ids ? fbk->nom_ids[k] : k;
  HIPCHK(hipMemcpyAsync(b->roll_env.get(), b->roll_env_host.data(), nids*sizeof(int), hipMemcpyHostToDevice, st));
  if (sync_model(b)) return -1;
  HIPCHK(hipMemsetAsync(b->roll_counter.get(), 0, 2*sizeof(int), st));
  HIPCHK(hipMemsetAsync(b->roll_sched.get(), 0, nctr*sizeof(int), st));
  constexpr int EPB = LdsCfg<double>::EPB;
  RolloutArgs<double> R;
  R.rarena = (const double*)b->rarena.get(); R.iarena = b->iarena.get(); R.pool_r = b->fd_pool_r.get(); R.pool_i = b->fd_pool_i.get();
  R.roll_env = b->roll_env.get(); R.ctrl = ctrl; R.action = action; R.state = state; R.sens = sensordata; R.status = (int*)status;
  R.counter = b->roll_counter.get();
  R.n_roll = nr; R.horizon = cfg->horizon; R.n_substeps = nsub;
  R.nwave = std::min(cfg->pool_rows > 0 ? cfg->pool_rows : slots, nr);
  R.sched = nr <= R.nwave ? b->roll_sched.get() : nullptr;      // (a wave with a second rollout would count into the first one's substeps)
  if (feedback) {
    FeedbackArgs<double> F;
    F.roll_nom = b->roll_env.get() + nr; F.x_nom = fbk->x_nom; F.u_nom = fbk->u_nom; F.Kt = fbk->K; F.k = fbk->k; F.alpha = fbk->alpha; F.ctrl_out = ctrl_out;
    hipLaunchKernelGGL((k_closedloop_rollout<double>), dim3((R.nwave + EPB - 1)/EPB), dim3(FB_WAVE*EPB), 0, st, (const DevModel<double>*)b->dM.get(), R, F);
  }
  else hipLaunchKernelGGL((k_rollout<double>), dim3((R.nwave + EPB - 1)/EPB), dim3(FB_WAVE*EPB), 0, st, (const DevModel<double>*)b->dM.get(), R);
  HIPCHK(hipGetLastError());
  return 0;
  FB_GUARD_END
}

extern "C" int fb_batch_rollout(fb_batch* b, const fb_rollout_config* cfg, const double* ctrl, const float* action, double* state, double* sensordata,
                                int32_t* status, void* stream) {
  return run_rollout(b, "fb_batch_rollout", cfg, ctrl, action, nullptr, false, state, sensordata, nullptr, status, stream);
}

// Closed-loop rollouts: the input of interval t is a time-varying affine feedback on the state the rollout has reached (fb_rollout.hpp).
extern "C" int fb_batch_rollout_feedback(fb_batch* b, const fb_rollout_config* cfg, const fb_feedback* fbk, double* state, double* sensordata,
                                         double* ctrl_out, int32_t* status, void* stream) {
  return run_rollout(b, "fb_batch_rollout_feedback", cfg, nullptr, nullptr, fbk, true, state, sensordata, ctrl_out, status, stream);
}

// Rollouts the last fb_batch_rollout / fb_batch_rollout_feedback call finished.  Synchronises the device.  A debug counter, like fb_batch_fd_tickets.
extern "C" int fb_batch_rollouts_run(fb_batch* b, int64_t* n) {
  if (!b || !n) return fail("fb_batch_rollouts_run: null argument");
  return side_tickets_done(b, b->roll_counter, n);
}

// ------------------------------------------------------------------ LQR / iLQR backward pass
// fb_riccati.hpp: the horizon loop runs here and enqueues the interval's products, its gain kernel and the symmetrisation on the caller's
// stream.  The batch gives the device and owns the workspace; no environment is read.  Steady state (the shapes of the call before): no
// allocation, no upload, no synchronisation.
static void ric_gemm(hipStream_t st, int n_nom, int M, int N, int K, const double* X, long long sX, long long xi, long long xk,
                     const double* Y, long long sY, long long yk, long long yj, const double* D, long long sD, int ldd, double* C, long long sC,
                     const int* status) {
  RicGemm g;
  g.X = X; g.Y = Y; g.D = D; g.C = C; g.sX = sX; g.sY = sY; g.sD = sD; g.sC = sC; g.xi = xi; g.xk = xk; g.yk = yk; g.yj = yj;
  g.M = M; g.N = N; g.K = K; g.ldd = ldd; g.ldc = N; g.tm = (M + FB_RIC_TILE - 1)/FB_RIC_TILE; g.tn = (N + FB_RIC_TILE - 1)/FB_RIC_TILE; g.status = status;
  hipLaunchKernelGGL(k_riccati_gemm, dim3((unsigned)((size_t)n_nom*g.tm*g.tn)), dim3(64), 0, st, g);
}

// doubles of workspace per nominal (the header states the layout)
static size_t lqr_ws_per_nominal(int ndx, int nu) { return 3*(size_t)ndx*ndx + 3*(size_t)ndx*nu + (size_t)nu*nu + 2*(size_t)ndx; }

extern "C" int fb_batch_lqr_backward(fb_batch* b, const fb_lqr_config* cfg, const double* A, const double* B, const double* Q, const double* R,
                                     const double* Qf, const double* q, const double* r, const double* mu, double* Kt, double* k, double* P,
                                     double* p, double* dV, int32_t* status, void* stream) {
  const std::string fn = "fb_batch_lqr_backward";
  if (!b) return fail(fn + ": null batch");
  if (!cfg) return fail(fn + ": null config");
  if (!A) return fail(fn + ": A is NULL");
  if (!B) return fail(fn + ": B is NULL");
  if (!Q) return fail(fn + ": Q is NULL");
  if (!R) return fail(fn + ": R is NULL");
  if (!Kt) return fail(fn + ": the Kt output is NULL");
  if (!status) return fail(fn + ": the status output is NULL");
  if (cfg->n_nom < 1) return fail(fn + ": n_nom must be >= 1");
  if (cfg->horizon < 1) return fail(fn + ": horizon must be >= 1");
  if (cfg->ndx < 1) return fail(fn + ": ndx must be >= 1");
  if (cfg->nu < 1) return fail(fn + ": nu must be >= 1");
  if (cfg->ndx > FB_RIC_NDXMAX) return fail(fn + ": ndx " + std::to_string(cfg->ndx) + " exceeds the gain kernel's " + std::to_string(FB_RIC_NDXMAX) + " Qx registers per workgroup");
  if (cfg->nu > FB_RIC_NUMAX) return fail(fn + ": nu " + std::to_string(cfg->nu) + " exceeds the " + std::to_string(FB_RIC_NUMAX) + " rows of the Cholesky factor in LDS and of a lane's right-hand side");
  if (cfg->stationary != 0 && cfg->stationary != 1) return fail(fn + ": stationary must be 0 or 1");
  const int n = cfg->n_nom, T = cfg->horizon, ndx = cfg->ndx, nu = cfg->nu; const bool stat = cfg->stationary == 1;
  const size_t nn = (size_t)ndx*ndx, nm = (size_t)ndx*nu;
  if ((size_t)n*((nn + 32*32 - 1)/(32*32) + 1) > (size_t)INT_MAX/4 || (size_t)n*(T + 1)*nn > ((size_t)1 << 46))
    return fail(fn + ": n_nom " + std::to_string(n) + " x horizon x ndx^2 exceeds the kernels' grids");
  FB_GUARD_BEGIN
  HIPCHK(hipSetDevice(b->device));
  hipStream_t st = (hipStream_t)stream;
  const size_t need = (size_t)n*lqr_ws_per_nominal(ndx, nu);
  if (b->lqr_ws.count() < need) {
    HIPCHK(hipDeviceSynchronize());                    // (an earlier call may still use the block)
    if (b->lqr_ws.reserve(need)) return -1;
  }
  // the workspace, one array [n_nom][..] after the other: three ndx x ndx buffers whose roles rotate (P_{t+1}, W then P_t, S), Y, Qux, G, Quu, p x 2
  double* w = b->lqr_ws.get();
  double* big[3]; for (int i = 0; i < 3; i++) { big[i] = w; w += (size_t)n*nn; }
  double* Yb = w; w += (size_t)n*nm; double* Qux = w; w += (size_t)n*nm; double* G = w; w += (size_t)n*nm;
  double* Quu = w; w += (size_t)n*nu*nu; double* pv[2]; pv[0] = w; w += (size_t)n*ndx; pv[1] = w;
  const int Tout = stat ? 1 : T, TP = stat ? 2 : T + 1;
  // outputs start from zero: a failed nominal's intervals are never written
  HIPCHK(hipMemsetAsync(Kt, 0, (size_t)n*Tout*nm*sizeof(double), st));
  if (k) HIPCHK(hipMemsetAsync(k, 0, (size_t)n*Tout*nu*sizeof(double), st));
  if (P) HIPCHK(hipMemsetAsync(P, 0, (size_t)n*TP*nn*sizeof(double), st));
  if (p) HIPCHK(hipMemsetAsync(p, 0, (size_t)n*TP*ndx*sizeof(double), st));
  // where P_j and p_j live: in the output when it has a slot for them, else in the workspace
  auto P_out = [&](int j, long long* s) -> double* { if (!P || (stat && j > 1)) return nullptr; *s = (long long)TP*nn; return P + (size_t)j*nn; };
  auto p_slot = [&](int j, long long* s) -> double* { if (!p || (stat && j > 1)) return nullptr; *s = (long long)TP*ndx; return p + (size_t)j*ndx; };
  const int chunks = (int)std::min<size_t>(64, (nn + FB_RIC_THREADS - 1)/FB_RIC_THREADS);
  const int* stat_ro = (const int*)status;
  long long sPn = (long long)nn, spn = ndx; int cur = 0, pcur = 0;          // P_{t+1}: big[cur] unless in the output; p_{t+1} likewise
  double* Pn = P_out(T, &sPn); if (Pn) cur = -1; else Pn = big[0];
  double* pn = p_slot(T, &spn); if (pn) pcur = -1; else pn = pv[0];
  const long long qT = stat ? 1 : T;                                         // q: [n_nom][T + 1][ndx]; stationary: [n_nom][2][ndx] (running, terminal)
  {
    RicInit g;
    g.Qf = Qf ? Qf : Q; g.P = Pn; g.sP = sPn; g.qT = q ? q + (size_t)qT*ndx : nullptr; g.sqT = (qT + 1)*ndx; g.p = pn; g.sp = spn;
    g.dV = dV; g.status = (int*)status; g.ndx = ndx; g.chunks = chunks;
    hipLaunchKernelGGL(k_riccati_init, dim3((unsigned)(n*chunks)), dim3(FB_RIC_THREADS), 0, st, g);
  }
  const long long sA = (long long)(stat ? 1 : T)*nn, sB = (long long)(stat ? 1 : T)*nm, sN = (long long)nn, sM = (long long)nm;
  for (int t = T - 1; t >= 0; t--) {
    const int to = stat ? 0 : t;
    const double* At = A + (size_t)to*nn; const double* Bt = B + (size_t)to*nm;
    const int iw = cur == 0 ? 1 : 0; int is = 0;                       // two workspace buffers that do not hold P_{t+1}
    while (is == cur || is == iw) is++;
    double* W = big[iw]; double* S = big[is];
    double* Ktt = Kt + (size_t)to*nm; const long long sK = (long long)Tout*nm;
    ric_gemm(st, n, ndx, ndx, ndx, Pn, sPn, ndx, 1, At, sA, ndx, 1, nullptr, 0, 0, W, sN, stat_ro);              // W = P A
    ric_gemm(st, n, ndx, nu, ndx, Pn, sPn, ndx, 1, Bt, sB, nu, 1, nullptr, 0, 0, Yb, sM, stat_ro);               // Y = P B
    ric_gemm(st, n, ndx, ndx, ndx, At, sA, 1, ndx, W, sN, ndx, 1, Q, 0, ndx, S, sN, stat_ro);                    // S = Q + A'W   (Qxx)
    ric_gemm(st, n, nu, ndx, ndx, Bt, sB, 1, nu, W, sN, ndx, 1, nullptr, 0, 0, Qux, sM, stat_ro);                // Qux = B'W
    ric_gemm(st, n, nu, nu, ndx, Bt, sB, 1, nu, Yb, sM, nu, 1, R, 0, nu, Quu, (long long)nu*nu, stat_ro);        // Quu = R + B'Y
    long long spo = ndx; double* po = p_slot(t, &spo); int pnext = -1;
    if (!po) { pnext = pcur == 0 ? 1 : 0; po = pv[pnext]; }
    {
      RicGain g;
      g.A = At; g.B = Bt; g.sA = sA; g.sB = sB; g.Qux = Qux; g.Quu = Quu; g.sQux = sM; g.sQuu = (long long)nu*nu;
      g.q = q ? q + (size_t)to*ndx : nullptr; g.sq = (qT + 1)*ndx; g.r = r ? r + (size_t)to*nu : nullptr; g.sr = (long long)Tout*nu; g.mu = mu;
      g.p_next = pn; g.sp_next = spn; g.p_out = po; g.sp_out = spo; g.Kt = Ktt; g.sKt = sK; g.k = k ? k + (size_t)to*nu : nullptr; g.sk = (long long)Tout*nu;
      g.dV = dV; g.status = (int*)status; g.ndx = ndx; g.nu = nu; g.t = t;
      hipLaunchKernelGGL(k_riccati_gain, dim3((unsigned)n), dim3(FB_RIC_THREADS), 0, st, g);
    }
    if (mu) {                                                                                                     // the general form (header)
      ric_gemm(st, n, nu, ndx, nu, Quu, (long long)nu*nu, nu, 1, Ktt, sK, 1, nu, Qux, sM, ndx, G, sM, stat_ro);   // G = Qux + Quu K
      ric_gemm(st, n, ndx, ndx, nu, Ktt, sK, nu, 1, G, sM, ndx, 1, S, sN, ndx, S, sN, stat_ro);                   // S += K'G
    }
    ric_gemm(st, n, ndx, ndx, nu, Qux, sM, 1, ndx, Ktt, sK, 1, nu, S, sN, ndx, S, sN, stat_ro);                   // S += Qux'K
    long long sPo = sN; double* Po = P_out(t, &sPo); int next = -1;
    if (!Po) { next = iw; Po = W; }                                                                              // (W is dead behind Qux)
    {
      RicSym g; g.S = S; g.sS = sN; g.P = Po; g.sP = sPo; g.status = stat_ro; g.ndx = ndx; g.chunks = chunks;
      hipLaunchKernelGGL(k_riccati_sym, dim3((unsigned)(n*chunks)), dim3(FB_RIC_THREADS), 0, st, g);
    }
    Pn = Po; sPn = sPo; cur = next; pn = po; spn = spo; pcur = pnext;
  }
  HIPCHK(hipGetLastError());
  return 0;
  FB_GUARD_END
}

// The product kernel of fb_batch_lqr_backward alone, for the tests of its tile map and edges: C = op(X) op(Y) (+ D), one matrix each.
extern "C" int fb_riccati_gemm(fb_batch* b, int m, int n, int k, int trans_x, int trans_y, const double* X, const double* Y, const double* D,
                               double* C, void* stream) {
  if (!b) return fail("fb_riccati_gemm: null batch");
  if (!X || !Y || !C) return fail("fb_riccati_gemm: X, Y or C is NULL");
  if (m < 1 || n < 1 || k < 1 || m > 4096 || n > 4096 || k > 4096) return fail("fb_riccati_gemm: m, n and k must be 1 .. 4096");
  FB_GUARD_BEGIN
  HIPCHK(hipSetDevice(b->device));
  ric_gemm((hipStream_t)stream, 1, m, n, k, X, 0, trans_x ? 1 : k, trans_x ? m : 1, Y, 0, trans_y ? 1 : n, trans_y ? k : 1, D, 0, n, C, 0, nullptr);
  HIPCHK(hipGetLastError());
  return 0;
  FB_GUARD_END
}

// ------------------------------------------------------------------ ray casting
// mj_ray / mj_multiRay for n_ray rays in each of n_frames live environments (fb_ray.hpp: k_raycast), against the geoms as the last step left
// them and an optional height field.  Not a control step and not a timed launch; the environments' rows are only read.  Everything the
// kernel indexes with is validated HERE: it has no check of its own to fall back on.
extern "C" int fb_batch_ray(fb_batch* b, const fb_ray_config* cfg, const double* rays, const fb_terrain* terrain, float* dist, int32_t* geomid, void* stream) {
  const std::string fn = "fb_batch_ray";
  if (!b || !cfg || !rays || !dist || !geomid) return fail(fn + ": null argument (batch, cfg, rays, dist or geomid)");
  if (b->n_models() > 1) return fail(fn + ": per-model ray casting is not supported: this batch is a group of " + std::to_string(b->n_models()) + " models (fb_batch_create_group)");
  const fb_model* m = b->m;
  const int nf = cfg->n_frames, nr = cfg->n_ray;
  if (nf < 1 || nr < 1) return fail(fn + ": n_frames and n_ray must be >= 1");
  const long long tiles = ((long long)nr + FB_RAY_TILE - 1)/FB_RAY_TILE;
  if (tiles*nf > (1ll << 23)) return fail(fn + ": too many rays for one call (more than 2^23 workgroups of " + std::to_string(FB_RAY_TILE) + " rays)");
  if (cfg->per_frame != 0 && cfg->per_frame != 1) return fail(fn + ": per_frame must be 0 or 1");
  if (side_check_env_ids(b, fn, cfg->env_ids, nf, "n_frames", "frame")) return -1;
  if (cfg->body < -1 || cfg->body >= m->nbody) return fail(fn + ": body " + std::to_string(cfg->body) + " out of range (-1, or 0 .. " + std::to_string(m->nbody - 1) + ")");
  if (cfg->bodyexclude < -1 || cfg->bodyexclude >= m->nbody) return fail(fn + ": bodyexclude " + std::to_string(cfg->bodyexclude) + " out of range (-1, or 0 .. " + std::to_string(m->nbody - 1) + ")");
  if (!(cfg->cutoff >= 0)) return fail(fn + ": cutoff must be >= 0 (0 or +inf: none) and not NaN");
  if (terrain) {
    const fb_terrain& t = *terrain;
    if (!t.data) return fail(fn + ": terrain data is NULL");
    if (t.nrow < 2 || t.ncol < 2 || t.nrow > FB_RAY_MAXGRID || t.ncol > FB_RAY_MAXGRID) return fail(fn + ": terrain nrow and ncol must be 2 .. " + std::to_string(FB_RAY_MAXGRID));
    if (t.n_terrain < 1) return fail(fn + ": n_terrain must be >= 1");
    for (int k = 0; k < 4; k++) if (!std::isfinite(t.size[k])) return fail(fn + ": terrain size must be finite");
    for (int k = 0; k < 3; k++) if (!std::isfinite(t.pos[k])) return fail(fn + ": terrain pos must be finite");
    if (!(t.size[0] > 0) || !(t.size[1] > 0) || t.size[2] < 0 || t.size[3] < 0) return fail(fn + ": terrain size must be (rx > 0, ry > 0, elevation_z >= 0, base_z >= 0)");
    if (t.terrain_ids) for (int k = 0; k < nf; k++) if (t.terrain_ids[k] < 0 || t.terrain_ids[k] >= t.n_terrain)
      return fail(fn + ": terrain id " + std::to_string(t.terrain_ids[k]) + " out of range (frame " + std::to_string(k) + ")");
  }
  FB_GUARD_BEGIN
  HIPCHK(hipSetDevice(b->device));
  hipStream_t st = (hipStream_t)stream;
  // the call's tables: [visible geoms | frame -> environment | frame -> terrain]
  const int* gbody = m->i("geom_bodyid");
  std::vector<int>& tab = b->ray_tab_host;
  tab.clear();
  for (int g = 0; g < m->ngeom; g++) if ((!cfg->geom_mask || cfg->geom_mask[g]) && (cfg->bodyexclude < 0 || gbody[g] != cfg->bodyexclude)) tab.push_back(g);
  const int n_vis = (int)tab.size();
  for (int k = 0; k < nf; k++) tab.push_back(cfg->env_ids ? cfg->env_ids[k] : k);
  const bool tids = terrain && terrain->terrain_ids;
  if (tids) tab.insert(tab.end(), terrain->terrain_ids, terrain->terrain_ids + nf);
  if (b->ray_tab.count() < tab.size()) {
    HIPCHK(hipDeviceSynchronize());                    // (an earlier call may still read the block)
    if (b->ray_tab.reserve(tab.size() + 256)) return -1;
  }
  HIPCHK(hipMemcpyAsync(b->ray_tab.get(), tab.data(), tab.size()*sizeof(int), hipMemcpyHostToDevice, st));
  with_model(b, [&](auto& M) {
    using real = decltype(M.timestep);
    RayArgs<real> A;
    A.rarena = (const real*)b->rarena.get(); A.nreal = b->off.nreal;
    A.o_gxpos = b->off.gxpos; A.o_gxmat = b->off.gxmat; A.o_xpos = b->off.xpos; A.o_xquat = b->off.xquat;
    A.geom_size = M.geom_size; A.geom_rbound = M.geom_rbound; A.geom_type = M.geom_type;
    A.vis = b->ray_tab.get(); A.n_vis = n_vis; A.frame_env = A.vis + n_vis; A.frame_terrain = tids ? A.frame_env + nf : nullptr;
    A.rays = rays; A.dist = dist; A.geomid = (int*)geomid;
    A.n_frames = nf; A.n_ray = nr; A.per_frame = cfg->per_frame; A.body = cfg->body; A.ngeom = m->ngeom; A.tiles = (int)tiles;
    A.cutoff = cfg->cutoff > 0 ? (real)cfg->cutoff : (real)INFINITY;
    A.hdata = terrain ? terrain->data : nullptr; A.nrow = terrain ? terrain->nrow : 2; A.ncol = terrain ? terrain->ncol : 2;
    A.rx = terrain ? (real)terrain->size[0] : 1; A.ry = terrain ? (real)terrain->size[1] : 1;
    A.elev = terrain ? (real)terrain->size[2] : 0; A.base = terrain ? (real)terrain->size[3] : 0;
    for (int k = 0; k < 3; k++) A.tpos[k] = terrain ? (real)terrain->pos[k] : 0;
    hipLaunchKernelGGL((k_raycast<real>), dim3((unsigned)(tiles*nf)), dim3(FB_RAY_THREADS), 0, st, A);
    return 0;
  });
  HIPCHK(hipGetLastError());
  return 0;
  FB_GUARD_END
}

// ------------------------------------------------------------------ field access
enum FieldKind { REAL_ARENA, F64_ARENA /* doubles in the real arena at either precision: the episode clock */, INT_ARENA, F32_ARRAY, I32_ARRAY, F64_ARRAY, REAL_ARRAY /* caller-owned input at the batch's precision: the applied forces */ };
// rows of `width` at offset `off` of an arena row, or an array [n_env][width] of its own at `base`; `unset`: why such an array is not
// allocated yet (the ones allocated with the batch need none)
struct FieldDesc { FieldKind kind; size_t off, width; void* base = nullptr; const char* unset = nullptr; };

static int field_desc(fb_batch* b, int field, FieldDesc* f) {
  const fb_model* m = b->m; const WSOff& o = b->off;
  const char* no_ref = "fb_batch_get: field not allocated yet (set a reference first)";
  const char* no_ik = "fb_batch_get: field not allocated yet (run fb_batch_ik first)";
  const char* no_inv = "fb_batch_get: field not allocated yet (run fb_batch_inverse first)";
  const char* no_grp = "FB_ENV_MODEL needs a grouped batch (fb_batch_create_group); this one was made by fb_batch_create";
  const char* no_frc = "fb_batch_get: no applied forces (fb_batch_set / fb_batch_device_ptr of FB_QFRC_APPLIED or FB_XFRC_APPLIED allocates them)";
  switch (field) {
    case FB_QPOS: *f = {REAL_ARENA, o.qpos, (size_t)m->nq}; break;
    case FB_QVEL: *f = {REAL_ARENA, o.qvel, (size_t)m->nv}; break;
    case FB_ACT: *f = {REAL_ARENA, o.act, (size_t)m->na}; break;
    case FB_CTRL: *f = {REAL_ARENA, o.ctrl, (size_t)m->nu}; break;
    case FB_QACC: *f = {REAL_ARENA, o.qacc, (size_t)m->nv}; break;
    case FB_XPOS: *f = {REAL_ARENA, o.xpos, (size_t)3*m->nbody}; break;
    case FB_XQUAT: *f = {REAL_ARENA, o.xquat, (size_t)4*m->nbody}; break;
    case FB_SENSORDATA: *f = {REAL_ARENA, o.sens, FB_NSENS}; break;
    case FB_QFRC_BIAS: *f = {REAL_ARENA, o.qfrc_bias, (size_t)m->nv}; break;
    case FB_QFRC_PASSIVE: *f = {REAL_ARENA, o.qfrc_passive, (size_t)m->nv}; break;
    case FB_QACC_SMOOTH: *f = {REAL_ARENA, o.qacc_smooth, (size_t)m->nv}; break;
    case FB_QM: *f = {REAL_ARENA, o.qM, (size_t)m->nM}; break;
    case FB_EFC_FORCE: *f = {REAL_ARENA, o.efc_force, FB_MAXEFC_}; break;
    case FB_QFRC_ACTUATOR: *f = {REAL_ARENA, o.qfrc_actuator, (size_t)m->nv}; break;
    case FB_QFRC_CONSTRAINT: *f = {REAL_ARENA, o.qfrc_constraint, (size_t)m->nv}; break;
    case FB_SUBTREE_COM: *f = {REAL_ARENA, o.com, 3}; break;
    case FB_TIME: *f = {F64_ARENA, o.simtime, 1}; break;
    case FB_NCON: *f = {INT_ARENA, o.istate + IS_NCON, 1}; break;
    case FB_NEFC: *f = {INT_ARENA, o.istate + IS_NEFC, 1}; break;
    case FB_SOLVER_NITER: *f = {INT_ARENA, o.istate + IS_NITER, 1}; break;
    case FB_STEP_COUNT: *f = {INT_ARENA, o.istate + IS_STEP, 1}; break;
    case FB_PROF: *f = {INT_ARENA, o.prof, 2*FB_NPROF}; break;
    case FB_REWARD_FACTORS: *f = {REAL_ARENA, o.rfac, 5}; break;
    case FB_GEOM_XPOS: *f = {REAL_ARENA, o.gxpos, (size_t)3*m->ngeom}; break;
    case FB_GEOM_XMAT: *f = {REAL_ARENA, o.gxmat, (size_t)9*m->ngeom}; break;
    case FB_CVEL: *f = {REAL_ARENA, o.cvel, (size_t)6*m->nbody}; break;
    case FB_OBS: *f = {F32_ARRAY, 0, (size_t)b->nobs, b->obs.get(), no_ref}; break;
    case FB_REWARD: *f = {F32_ARRAY, 0, 1, b->reward.get()}; break;
    case FB_DISCOUNT: *f = {F32_ARRAY, 0, 1, b->discount.get()}; break;
    case FB_STEP_TYPE: *f = {I32_ARRAY, 0, 1, b->step_type.get()}; break;
    case FB_WARN: *f = {INT_ARENA, o.istate + IS_WARN, 1}; break;
    case FB_WARN_EVER: *f = {INT_ARENA, o.istate + IS_WARN_EVER, 1}; break;
    case FB_SIZE_STATS: *f = {INT_ARENA, o.istate + IS_MAX_NCON, 4}; break;
    case FB_STEP_TICKS: *f = {I32_ARRAY, 0, 1, b->cost.get()}; break;
    case FB_LAUNCH_ORDER: *f = {I32_ARRAY, 0, 1, b->order.get()}; break;
    case FB_SITE_XPOS: *f = {REAL_ARENA, o.sxpos, (size_t)3*m->nsite}; break;
    case FB_IK_ERR: *f = {F64_ARRAY, 0, 2, b->ik_err.get(), no_ik}; break;
    case FB_IK_STEPS: *f = {I32_ARRAY, 0, 2, b->ik_steps.get(), no_ik}; break;
    case FB_QFRC_INVERSE: *f = {F64_ARRAY, 0, (size_t)m->nv, b->inv_qfrc.get(), no_inv}; break;
    case FB_CONTACT_FORCE: *f = {F64_ARRAY, 0, (size_t)3*FB_MAXCON_, b->inv_cforce.get(), no_inv}; break;
    case FB_QFRC_APPLIED: *f = {REAL_ARRAY, 0, (size_t)m->nv, b->qfrc_applied.get(), no_frc}; break;
    case FB_XFRC_APPLIED: *f = {REAL_ARRAY, 0, (size_t)6*m->nbody, b->xfrc_applied.get(), no_frc}; break;
    case FB_ENV_MODEL: *f = {I32_ARRAY, 0, 1, b->env_model.get(), no_grp}; break;
    case FB_QFRC_LAW: *f = {REAL_ARRAY, 0, (size_t)m->nv, b->law_out.get(), "fb_batch_get: no control law (fb_batch_set_control_law sets one)"}; break;
    case FB_CONTROL_LAW: return fail("FB_CONTROL_LAW is [n_rows][5][nv], not one row per environment: read and write it through fb_batch_device_ptr, set it with fb_batch_set_control_law");
    default: return fail("unknown field");
  }
  return 0;
}

// The applied-force arrays, zeroed, on the first fb_batch_set / fb_batch_device_ptr of either field.  From then on launch() steps the batch with
// k_step_forces.  (Both or neither: the kernel takes them as one argument.)
static int alloc_forces(fb_batch* b) {
  if (b->qfrc_applied && b->xfrc_applied) return 0;
  const size_t rs = real_size(b);
  HIPCHK(hipDeviceSynchronize());
  DevBuf<void> q, x;                                   // (both or neither: a failure gives back what it got)
  if (q.alloc_zeroed((size_t)b->n_env*b->m->nv*rs) || x.alloc_zeroed((size_t)b->n_env*6*b->m->nbody*rs)) return fail("applied forces: device allocation failed");
  HIPCHK(hipDeviceSynchronize());                      // (the zeroes are there before a launch on any stream reads them)
  b->qfrc_applied = std::move(q); b->xfrc_applied = std::move(x);
  return 0;
}

extern "C" int fb_batch_clear_forces(fb_batch* b) {
  if (!b) return fail("fb_batch_clear_forces: null batch");
  if (b->law_coef) return fail("fb_batch_clear_forces: a control law is set, and its kernel (k_step_law) reads the force arrays; call fb_batch_set_control_law(batch, NULL) first");
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipDeviceSynchronize());                      // (a launch in flight may still read the arrays)
  b->qfrc_applied.reset(); b->xfrc_applied.reset();
  return 0;
}

extern "C" int fb_batch_forces_active(const fb_batch* b) {
  if (!b) return fail("fb_batch_forces_active: null batch");
  return b->qfrc_applied ? 1 : 0;
}

// ------------------------------------------------------------------ substep control law (fb_law.hpp)
extern "C" int fb_batch_set_control_law(fb_batch* b, const fb_control_law* law) {
  if (!b) return fail("fb_batch_set_control_law: null batch");
  FB_GUARD_BEGIN
  HIPCHK(hipSetDevice(b->device));
  if (!law) {
    HIPCHK(hipDeviceSynchronize());                    // (a launch in flight may still read the law)
    b->law_coef.reset(); b->law_out.reset(); b->law_qadr.reset(); b->law_rows = 0;
    if (b->law_owns_forces) { b->law_owns_forces = false; return fb_batch_clear_forces(b); }
    return 0;
  }
  if (b->n_models() > 1) return fail("fb_batch_set_control_law: a control law in a grouped batch is not supported: this batch is a group of " + std::to_string(b->n_models()) +
                                     " models (fb_batch_create_group); give every model a batch of its own (fb_batch_create)");
  const fb_model* m = b->m;
  const int nv = m->nv, n = b->n_env, nr = law->n_rows;
  if (nr != 1 && nr != n) return fail("fb_batch_set_control_law: n_rows must be 1 (one law for the batch) or n_env = " + std::to_string(n) + ", got " + std::to_string(nr));
  const double* rows[LAW_NROW] = {law->bias, law->act_gain, law->pos_gain, law->pos_ref, law->vel_gain};
  const char* names[LAW_NROW] = {"bias", "act_gain", "pos_gain", "pos_ref", "vel_gain"};
  // qpos address of every hinge's dof; pos_gain must be zero everywhere else (the free root's and a ball's dofs have no scalar position)
  const int *djnt = m->i("dof_jntid"), *jt = m->i("jnt_type"), *jqa = m->i("jnt_qposadr");
  std::vector<int> qadr(nv, 0);
  for (int i = 0; i < nv; i++) if (jt[djnt[i]] == JNT_HINGE) qadr[i] = jqa[djnt[i]];
  for (int r = 0; r < LAW_NROW; r++) {
    if (!rows[r]) continue;
    for (size_t k = 0; k < (size_t)nr*nv; k++) {
      if (!std::isfinite(rows[r][k])) return fail(std::string("fb_batch_set_control_law: ") + names[r] + " of dof " + std::to_string(k % nv) + " (row " + std::to_string(k/nv) + ") is not finite");
      if (r == LAW_POS_GAIN && rows[r][k] != 0 && jt[djnt[k % nv]] != JNT_HINGE)
        return fail("fb_batch_set_control_law: pos_gain of dof " + std::to_string(k % nv) + " (row " + std::to_string(k/nv) + ") is not zero, but the dof belongs to a " +
                    (jt[djnt[k % nv]] == JNT_FREE ? "free" : "ball") + " joint, which has no scalar position; position feedback is for hinge dofs only");
    }
  }
  const bool had_forces = (bool)b->qfrc_applied;
  if (alloc_forces(b)) return -1;
  if (!had_forces) b->law_owns_forces = true;
  HIPCHK(hipDeviceSynchronize());
  // Whatever the new law needs and the batch does not have yet is allocated in locals, filled, and moved in last: a failure on the way leaves
  // the batch as it was, the previous law included (a block of another row count is a new block; the move frees the old one).
  const size_t rs = real_size(b);
  const bool reuse = b->law_coef && b->law_rows == nr;
  DevBuf<void> new_coef, new_out; DevBuf<int> new_qa;
  auto undo = [&](const char* why) {                   // (the locals free themselves; the forces this call brought are the batch's by now)
    if (!had_forces && !b->law_coef) { b->law_owns_forces = false; (void)fb_batch_clear_forces(b); }
    (void)hipGetLastError();
    return fail(std::string("fb_batch_set_control_law: ") + why);
  };
  if ((!reuse && new_coef.alloc((size_t)nr*LAW_NROW*nv*rs)) || (!b->law_qadr && new_qa.alloc(nv)) || (!b->law_out && new_out.alloc_zeroed((size_t)n*nv*rs)))
    return undo("device allocation failed");
  void* coef = reuse ? b->law_coef.get() : new_coef.get(); int* qa = b->law_qadr ? b->law_qadr.get() : new_qa.get();
  if (hipMemcpy(qa, qadr.data(), nv*sizeof(int), hipMemcpyHostToDevice) != hipSuccess) return undo("copy to the device failed");
  const int rc = with_model(b, [&](auto& M) {
    std::vector<decltype(M.timestep)> tmp((size_t)nr*LAW_NROW*nv, 0);
    for (int e = 0; e < nr; e++) for (int r = 0; r < LAW_NROW; r++) if (rows[r])
      for (int i = 0; i < nv; i++) tmp[((size_t)e*LAW_NROW + r)*nv + i] = (decltype(M.timestep))rows[r][(size_t)e*nv + i];
    return hipMemcpy(coef, tmp.data(), tmp.size()*sizeof(tmp[0]), hipMemcpyHostToDevice) == hipSuccess ? 0 : -1;
  });
  if (rc || hipDeviceSynchronize() != hipSuccess) return undo("copy to the device failed");
  if (new_coef) b->law_coef = std::move(new_coef);
  if (new_out) b->law_out = std::move(new_out);
  if (new_qa) b->law_qadr = std::move(new_qa);
  b->law_rows = nr;
  return 0;
  FB_GUARD_END
}

extern "C" int fb_batch_control_law_active(const fb_batch* b) {
  if (!b) return fail("fb_batch_control_law_active: null batch");
  return b->law_coef ? 1 : 0;
}

extern "C" int fb_batch_end_episode(fb_batch* b, const uint8_t* mask_dev, const float* discount_dev, void* stream) {
  if (!b || !mask_dev) return fail("fb_batch_end_episode: null argument");
  HIPCHK(hipSetDevice(b->device));
  hipLaunchKernelGGL(k_end_episode, dim3((b->n_env + FB_WAVE - 1)/FB_WAVE), dim3(FB_WAVE), 0, (hipStream_t)stream, b->iarena.get(), (unsigned)b->off.nint, (unsigned)b->off.istate,
                     b->step_type.get(), b->discount.get(), mask_dev, discount_dev, b->n_env);
  HIPCHK(hipGetLastError());
  return 0;
}

// a REAL_ARENA field of every environment, between the arena (the batch's precision) and FP64 rows [n_env][width] on the host
static int real_rows(fb_batch* b, const FieldDesc& f, double* host, bool to_device) {
  return with_model(b, [&](auto& M) {
    using real = decltype(M.timestep);
    const size_t row = f.width*sizeof(real), pitch = (size_t)b->off.nreal*sizeof(real);
    char* dev = (char*)b->rarena.get() + f.off*sizeof(real);
    std::vector<real> tmp((size_t)b->n_env*f.width);
    if (to_device) std::copy(host, host + tmp.size(), tmp.begin());
    HIPCHK(to_device ? hipMemcpy2D(dev, pitch, tmp.data(), row, row, b->n_env, hipMemcpyHostToDevice)
                     : hipMemcpy2D(tmp.data(), row, dev, pitch, row, b->n_env, hipMemcpyDeviceToHost));
    if (!to_device) std::copy(tmp.begin(), tmp.end(), host);
    return 0;
  });
}

extern "C" int fb_batch_get(fb_batch* b, int field, void* dst, size_t bytes) {
  if (!b || !dst) return fail("fb_batch_get: null argument");
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipDeviceSynchronize());
  if (field != FB_WARN && field != FB_WARN_EVER && check_sched_errors(b)) return -1;      // (the flags stay readable: they say WHICH environments)
  int n = b->n_env;
  if (field == FB_CONTACT) {
    // [n_env][64][8]: dist, pos3, normal3, pair id  (FP64)
    if (bytes != (size_t)n*FB_MAXCON_*8*sizeof(double)) return fail("fb_batch_get: size mismatch");
    return with_model(b, [&](auto& M) {
      std::vector<decltype(M.timestep)> rr((size_t)n*b->off.nreal);
      std::vector<int> ii((size_t)n*b->off.nint);
      HIPCHK(hipMemcpy(rr.data(), b->rarena.get(), rr.size()*sizeof(rr[0]), hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(ii.data(), b->iarena.get(), ii.size()*sizeof(int), hipMemcpyDeviceToHost));
      double* out = (double*)dst;
      for (int e = 0; e < n; e++) for (int c = 0; c < FB_MAXCON_; c++) {
        double* o = out + ((size_t)e*FB_MAXCON_ + c)*8;
        const auto* r = rr.data() + (size_t)e*b->off.nreal;
        o[0] = r[b->off.con_dist + c];
        for (int k = 0; k < 3; k++) { o[1+k] = r[b->off.con_pos + 3*c + k]; o[4+k] = r[b->off.con_frame + 9*c + k]; }
        o[7] = ii[(size_t)e*b->off.nint + b->off.con_pair + c];
      }
      return 0;
    });
  }
  FieldDesc f;
  if (field_desc(b, field, &f)) return -1;
  if (f.kind == REAL_ARENA) {
    if (bytes != (size_t)n*f.width*sizeof(double)) return fail("fb_batch_get: size mismatch (physics fields are returned as FP64)");
    return real_rows(b, f, (double*)dst, false);
  } else if (f.kind == F64_ARENA) {
    if (bytes != (size_t)n*f.width*sizeof(double)) return fail("fb_batch_get: size mismatch");
    const size_t rs = real_size(b);
    HIPCHK(hipMemcpy2D(dst, f.width*8, (char*)b->rarena.get() + f.off*rs, (size_t)b->off.nreal*rs, f.width*8, n, hipMemcpyDeviceToHost));
  } else if (f.kind == INT_ARENA) {
    if (bytes != (size_t)n*f.width*sizeof(int)) return fail("fb_batch_get: size mismatch");
    HIPCHK(hipMemcpy2D(dst, f.width*4, (char*)b->iarena.get() + f.off*4, (size_t)b->off.nint*4, f.width*4, n, hipMemcpyDeviceToHost));
  } else if (f.kind == REAL_ARRAY) {
    if (!f.base) return fail(f.unset);
    if (bytes != (size_t)n*f.width*sizeof(double)) return fail("fb_batch_get: size mismatch (physics fields are returned as FP64)");
    return with_model(b, [&](auto& M) {
      std::vector<decltype(M.timestep)> tmp((size_t)n*f.width);
      HIPCHK(hipMemcpy(tmp.data(), f.base, tmp.size()*sizeof(tmp[0]), hipMemcpyDeviceToHost));
      std::copy(tmp.begin(), tmp.end(), (double*)dst);
      return 0;
    });
  } else {
    if (!f.base) return fail(f.unset);
    if (bytes != (size_t)n*f.width*(f.kind == F64_ARRAY ? 8 : 4)) return fail("fb_batch_get: size mismatch");
    HIPCHK(hipMemcpy(dst, f.base, bytes, hipMemcpyDeviceToHost));
  }
  return 0;
}

extern "C" int fb_batch_set(fb_batch* b, int field, const void* src, size_t bytes) {
  if (!b || !src) return fail("fb_batch_set: null argument");
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipDeviceSynchronize());
  FieldDesc f;
  if (field_desc(b, field, &f)) return -1;
  int n = b->n_env;
  if (f.kind == REAL_ARENA) {
    if (bytes != (size_t)n*f.width*sizeof(double)) return fail("fb_batch_set: size mismatch (physics fields are passed as FP64)");
    return real_rows(b, f, (double*)src, true);
  } else if (f.kind == F64_ARENA) {
    if (bytes != (size_t)n*f.width*sizeof(double)) return fail("fb_batch_set: size mismatch");
    const size_t rs = real_size(b);
    HIPCHK(hipMemcpy2D((char*)b->rarena.get() + f.off*rs, (size_t)b->off.nreal*rs, src, f.width*8, f.width*8, n, hipMemcpyHostToDevice));
  } else if (f.kind == INT_ARENA) {
    if (bytes != (size_t)n*f.width*sizeof(int)) return fail("fb_batch_set: size mismatch");
    HIPCHK(hipMemcpy2D((char*)b->iarena.get() + f.off*4, (size_t)b->off.nint*4, src, f.width*4, f.width*4, n, hipMemcpyHostToDevice));
  } else if (field == FB_QFRC_LAW) {
    return fail("fb_batch_set: FB_QFRC_LAW is read-only (the law stage writes it; fb_batch_set_control_law sets the law)");
  } else if (f.kind == REAL_ARRAY) {
    // applied forces: validated on the host (size, finite), then both arrays exist and k_step_forces steps the batch
    const char* name = field == FB_QFRC_APPLIED ? "FB_QFRC_APPLIED" : "FB_XFRC_APPLIED";
    if (bytes != (size_t)n*f.width*sizeof(double))
      return fail(std::string("fb_batch_set: size mismatch: ") + name + " is [n_env][" + std::to_string(f.width) + "] FP64 = " + std::to_string((size_t)n*f.width*sizeof(double)) + " bytes, got " + std::to_string(bytes));
    const double* v = (const double*)src;
    for (size_t k = 0; k < (size_t)n*f.width; k++)
      if (!std::isfinite(v[k])) return fail(std::string("fb_batch_set: ") + name + " of environment " + std::to_string(k/f.width) + " is not finite");
    if (alloc_forces(b)) return -1;
    b->law_owns_forces = false;
    void* dev = field == FB_QFRC_APPLIED ? b->qfrc_applied.get() : b->xfrc_applied.get();
    return with_model(b, [&](auto& M) {
      const std::vector<decltype(M.timestep)> tmp(v, v + (size_t)n*f.width);
      HIPCHK(hipMemcpy(dev, tmp.data(), tmp.size()*sizeof(tmp[0]), hipMemcpyHostToDevice));
      return 0;
    });
  } else if (field == FB_ENV_MODEL) {
    // the assignment of a grouped batch: validated on the host (the kernels clamp what arrives through the device pointer)
    if (!f.base) return fail(f.unset);
    if (bytes != (size_t)n*sizeof(int)) return fail("fb_batch_set: size mismatch: FB_ENV_MODEL is [n_env] int32");
    const int* v = (const int*)src;
    for (int e = 0; e < n; e++)
      if (v[e] < 0 || v[e] >= b->n_models()) return fail("fb_batch_set: FB_ENV_MODEL of environment " + std::to_string(e) + " is " + std::to_string(v[e]) + ", outside [0, " + std::to_string(b->n_models()) + ")");
    HIPCHK(hipMemcpy(b->env_model.get(), v, bytes, hipMemcpyHostToDevice));
  } else return fail("fb_batch_set: field is read-only");
  return 0;
}

extern "C" void* fb_batch_device_ptr(fb_batch* b, int field) {
  if (!b) return nullptr;
  switch (field) {
    case FB_OBS: return b->obs.get();
    case FB_REWARD: return b->reward.get();
    case FB_DISCOUNT: return b->discount.get();
    case FB_STEP_TYPE: return b->step_type.get();
    case FB_ENV_MODEL: return b->env_model.get();           // (null on a batch made by fb_batch_create)
    case FB_QFRC_APPLIED: case FB_XFRC_APPLIED:        // (allocates both arrays on first use: the batch is stepped by k_step_forces from then on)
      if (hipSetDevice(b->device) != hipSuccess || alloc_forces(b)) return nullptr;
      b->law_owns_forces = false;
      return field == FB_QFRC_APPLIED ? b->qfrc_applied.get() : b->xfrc_applied.get();
    case FB_QPOS: case FB_QVEL:                        // rows of the arena: environment e's row starts e x (fb_batch_row's row_bytes of the real arena) further on
      return (char*)b->rarena.get() + (size_t)(field == FB_QPOS ? b->off.qpos : b->off.qvel)*real_size(b);
    case FB_QFRC_LAW: return b->law_out.get();         // (null while no law is set)
    case FB_CONTROL_LAW: return b->law_coef.get();
    default: return nullptr;
  }
}

extern "C" int fb_batch_row(fb_batch* b, int which, int env, void* host, size_t bytes, int write, size_t* row_bytes) {
  if (!b || which < 0 || which > 1 || env < 0 || env >= b->n_env) return fail("fb_batch_row: bad argument");
  const size_t rs = which == 0 ? real_size(b) : 4;
  const size_t rb = (which == 0 ? (size_t)b->off.nreal : (size_t)b->off.nint)*rs;
  if (row_bytes) *row_bytes = rb;
  if (bytes == 0) return 0;
  if (!host || bytes != rb) return fail("fb_batch_row: size mismatch");
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipDeviceSynchronize());
  char* dev = (which == 0 ? (char*)b->rarena.get() : (char*)b->iarena.get()) + (size_t)env*rb;
  if (write) HIPCHK(hipMemcpy(dev, host, rb, hipMemcpyHostToDevice)); else HIPCHK(hipMemcpy(host, dev, rb, hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int fb_batch_scheduler(const fb_batch* b, int* slots) {
  if (!b) return fail("fb_batch_scheduler: null batch");
  if (slots) *slots = b->slots;
  return b->tickets ? 1 : 0;
}

extern "C" int fb_batch_timing_begin(fb_batch* b, void* stream) {
  if (!b) return fail("fb_batch_timing_begin: null batch");
  HIPCHK(hipSetDevice(b->device));
  if ((!b->ev0 && b->ev0.create()) || (!b->ev1 && b->ev1.create())) return -1;
  b->timed_launches = 0; b->timing = true;
  HIPCHK(hipEventRecord(b->ev0.get(), (hipStream_t)stream));
  return 0;
}

extern "C" int fb_batch_timing_end(fb_batch* b, void* stream, float* total_ms, int* n_launches) {
  if (!b || !b->timing) return fail("fb_batch_timing_end: timing not started");
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipEventRecord(b->ev1.get(), (hipStream_t)stream));
  HIPCHK(hipEventSynchronize(b->ev1.get()));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, b->ev0.get(), b->ev1.get()));
  if (total_ms) *total_ms = ms;
  if (n_launches) *n_launches = b->timed_launches;
  b->timing = false;
  return 0;
}

extern "C" int fb_batch_timing_launches(fb_batch* b, float* ms, int cap) {
  if (!b || b->timing) return fail("fb_batch_timing_launches: call after fb_batch_timing_end");
  HIPCHK(hipSetDevice(b->device));
  const int n = std::min((int)b->lev.size()/2, std::min(b->timed_launches, cap));
  for (int k = 0; k < n && ms; k++) HIPCHK(hipEventElapsedTime(ms + k, b->lev[2*k].get(), b->lev[2*k + 1].get()));
  return n;
}
