// Host-only model loading of libflybody_hip.so (included by fb_engine.hip): the model blob and its table of contents, the checks of every
// array the engine reads, the tables the host derives from the tree once (fb_model), and the C-ABI's fb_model_load / fb_model_destroy /
// fb_model_dim.  Nothing here touches the device; build_devmodel (fb_engine.hip) uploads what the kernels read.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>
#include "../../include/flybody_engine.h"
#include "fb_types.hpp"
#include "fb_host.hpp"

// ------------------------------------------------------------------ blob
struct BlobEntry { char name[40]; uint32_t dtype, ndim, shape[4]; uint64_t offset, nbytes; };

struct fb_model {
  std::vector<char> blob;
  std::map<std::string, const BlobEntry*> idx;
  // host-side derived tables
  int nq, nv, nbody, njnt, ngeom, nsite, nu, na, ntendon, npair, nM, nsubstep, nobsjnt, napp, nforce, ntouch;
  int task_id;                           // FB_TASK_* (fb_types.hpp)
  std::vector<int> body_nsub, body_depth, body_chlen, body_chain, body_common, dof_depth, dof_ndesc, lvl_dof, lvl_start, adh_act;
  std::vector<int> wrap_qadr, act_wn, act_wdof, act_lenadr; std::vector<double> act_wcoef;
  std::vector<int> pair_word, pair_body, plane_geoms;
  std::vector<double> geom_box;          // [ngeom][3] oriented-box half extents by geom type (constant: one lookup instead of type -> size -> switch)
  std::vector<int> dof_cl, dof_gen, gen_k, gen_m, fwd_tab, fwd_pack, fac_w, fac_band, fac_dof; int ngen = 0, ntrunk = 1, prefix_split = 0;
  int nlevel;
  std::vector<double> body_box, body_rec;
  std::vector<int> body_fluid_geom, sens_body, dof_jump, dof_vbef, body_veldof;
  double totalmass; int solver;          // solver: FB_SOLVER_*
  int chmax, fk_dmax, fk2_dlo;           // longest dof chain of a body; deepest body level; shallowest level among bodies >= 64
  std::vector<int> fk_second;            // [64] second body of each lane in the kinematics level loop (-1: none); empty: the model has no such pairing
  int nplane;                            // geoms of type plane (plane_geoms holds one entry even when there is none)
  double vl_delta;                       // neighbour-list slack of this model (0: no list)
  // A missing or ill-typed array is an error of the caller's blob, never a reason to take the process down: the accessors
  // throw, every extern "C" entry point that reads the model catches and returns -1 with the message in fb_last_error().
  // fb_model_load checks every array the engine reads (name, type, minimum length) up front, so a loaded model cannot throw.
  const double* d(const char* n, size_t* cnt = nullptr) const {
    auto it = idx.find(n);
    if (it == idx.end() || it->second->dtype != 0) throw std::runtime_error(std::string("model blob: missing f64 array '") + n + "'");
    if (cnt) *cnt = it->second->nbytes/8;
    return (const double*)(blob.data() + it->second->offset);
  }
  const int* i(const char* n, size_t* cnt = nullptr) const {
    auto it = idx.find(n);
    if (it == idx.end() || it->second->dtype != 1) throw std::runtime_error(std::string("model blob: missing i32 array '") + n + "'");
    if (cnt) *cnt = it->second->nbytes/4;
    return (const int*)(blob.data() + it->second->offset);
  }
  bool has(const char* n, int dtype) const { auto it = idx.find(n); return it != idx.end() && (int)it->second->dtype == dtype; }
  void need(const char* n, int dtype, size_t min_count) const {
    auto it = idx.find(n);
    if (it == idx.end()) throw std::runtime_error(std::string("model blob: missing array '") + n + "'");
    if ((int)it->second->dtype != dtype) throw std::runtime_error(std::string("model blob: array '") + n + "' has the wrong type (expected " + (dtype ? "i32" : "f64") + ")");
    size_t c = it->second->nbytes/(dtype ? 4 : 8);
    if (c < min_count) throw std::runtime_error(std::string("model blob: array '") + n + "' has " + std::to_string(c) + " elements, expected at least " + std::to_string(min_count));
  }
};

static int model_load_impl(fb_model* m, size_t n);

extern "C" int fb_model_load(const void* blob, size_t n, fb_model** out) {
  if (!out) return fail("fb_model_load: null output pointer");
  *out = nullptr;
  if (!blob || n < 8 || memcmp(blob, "FBM1", 4) != 0) return fail("fb_model_load: bad blob magic");
  fb_model* m = new fb_model();
  int rc;
  try {
    m->blob.assign((const char*)blob, (const char*)blob + n);
    rc = model_load_impl(m, n);
  } catch (const std::exception& e_) { rc = fail(std::string("fb_model_load: ") + e_.what()); }
  if (rc != 0) { delete m; return rc; }
  *out = m;
  return 0;
}

// every array the engine reads, with its element type and the minimum length the model's dimensions imply
static void check_model_arrays(const fb_model* m) {
  const size_t nq = m->nq, nv = m->nv, nb = m->nbody, nj = m->njnt, ng = m->ngeom, ns = m->nsite, nu = m->nu, nt = m->ntendon, np = m->npair;
  struct Req { const char* name; int dtype; size_t n; };
  size_t nwrap = 0; { size_t c = 0; m->i("wrap_dofid", &c); nwrap = c; }
  const Req req[] = {
    {"body_mass", 0, nb}, {"body_inertia", 0, 3*nb}, {"body_invweight0", 0, 2*nb}, {"body_pos", 0, 3*nb}, {"body_quat", 0, 4*nb},
    {"body_ipos", 0, 3*nb}, {"body_iquat", 0, 4*nb}, {"jnt_pos", 0, 3*nj}, {"jnt_axis", 0, 3*nj}, {"jnt_stiffness", 0, nj},
    {"jnt_range", 0, 2*nj}, {"jnt_solref", 0, 2*nj}, {"jnt_solimp", 0, 5*nj}, {"jnt_margin", 0, nj}, {"qpos0", 0, nq}, {"qpos_spring", 0, nq},
    {"dof_armature", 0, nv}, {"dof_damping", 0, nv}, {"dof_invweight0", 0, nv}, {"geom_pos", 0, 3*ng}, {"geom_quat", 0, 4*ng},
    {"geom_size", 0, 3*ng}, {"geom_rbound", 0, ng}, {"geom_fluid", 0, 12*ng}, {"site_pos", 0, 3*ns}, {"site_quat", 0, 4*ns}, {"site_size", 0, 3*ns},
    {"wrap_coef", 0, nwrap}, {"actuator_dynprm", 0, nu}, {"actuator_gainprm", 0, 3*nu}, {"actuator_biasprm", 0, 3*nu},
    {"actuator_ctrlrange", 0, 2*nu}, {"actuator_forcerange", 0, 2*nu}, {"pair_friction", 0, 5*np}, {"pair_solref", 0, 2*np},
    {"pair_solimp", 0, 5*np}, {"pair_margin", 0, np}, {"pair_gap", 0, np}, {"opt_timestep", 0, 1}, {"opt_control_timestep", 0, 1},
    {"opt_gravity", 0, 3}, {"opt_density", 0, 1}, {"opt_viscosity", 0, 1}, {"opt_impratio", 0, 1}, {"opt_tolerance", 0, 1},
    {"opt_noslip_tolerance", 0, 1}, {"stat_meaninertia", 0, 1}, {"com_offset", 0, 3},
    {"body_parent", 1, nb}, {"body_dofadr", 1, nb}, {"body_dofnum", 1, nb}, {"body_jntadr", 1, nb}, {"body_jntnum", 1, nb},
    {"jnt_type", 1, nj}, {"jnt_qposadr", 1, nj}, {"jnt_dofadr", 1, nj}, {"jnt_bodyid", 1, nj}, {"jnt_limited", 1, nj},
    {"dof_bodyid", 1, nv}, {"dof_jntid", 1, nv}, {"dof_parentid", 1, nv}, {"dof_Madr", 1, nv + 1}, {"geom_type", 1, ng}, {"geom_bodyid", 1, ng},
    {"site_bodyid", 1, ns}, {"site_type", 1, ns}, {"tendon_adr", 1, nt}, {"tendon_num", 1, nt}, {"actuator_trntype", 1, nu},
    {"actuator_trnid", 1, nu}, {"actuator_dyntype", 1, nu}, {"actuator_biastype", 1, nu}, {"actuator_ctrllimited", 1, nu},
    {"actuator_forcelimited", 1, nu}, {"actuator_actadr", 1, nu}, {"action_to_ctrl", 1, nu}, {"pair_geom1", 1, np}, {"pair_geom2", 1, np},
    {"pair_condim", 1, np}, {"observable_joints", 1, 0}, {"appendage_sites", 1, 0}, {"sensor_force_sites", 1, 0}, {"sensor_touch_sites", 1, 0},
    {"wing_jnt", 1, 6}, {"wing_action_idx", 1, 0}, {"task_id", 1, 1}, {"user_action_idx", 1, 1}, {"sensor_site_thorax", 1, 1},
    {"opt_iterations", 1, 1}, {"opt_noslip_iterations", 1, 1}, {"wrap_dofid", 1, 0},
  };
  for (const Req& r : req) m->need(r.name, r.dtype, r.n);
  // index ranges the kernels rely on
  auto in_range = [&](const char* name, size_t cnt, int lo, int hi) {
    const int* v = m->i(name);
    for (size_t k = 0; k < cnt; k++) if (v[k] < lo || v[k] >= hi) throw std::runtime_error(std::string("model blob: '") + name + "' holds an index out of range");
  };
  in_range("body_parent", nb, -1, (int)nb); in_range("dof_bodyid", nv, 0, (int)nb); in_range("dof_jntid", nv, 0, (int)nj);
  in_range("jnt_qposadr", nj, 0, (int)nq); in_range("jnt_dofadr", nj, 0, (int)nv); in_range("jnt_bodyid", nj, 0, (int)nb);
  in_range("geom_bodyid", ng, 0, (int)nb); in_range("site_bodyid", ns, 0, (int)nb); in_range("pair_geom1", np, 0, (int)ng); in_range("pair_geom2", np, 0, (int)ng);
  in_range("action_to_ctrl", nu, 0, (int)nu); in_range("wrap_dofid", nwrap, 0, (int)nv);
  in_range("observable_joints", m->nobsjnt, 0, (int)nj); in_range("appendage_sites", m->napp, 0, (int)ns);
  in_range("sensor_force_sites", m->nforce, 0, (int)ns); in_range("sensor_touch_sites", m->ntouch, 0, (int)ns);
  in_range("wing_jnt", 6, 0, (int)nj); in_range("sensor_site_thorax", 1, 0, (int)ns);
}

// The derivations of fb_model_load, one step per family of tables, each with its own capacity checks.  A step reads the blob, the dimensions
// and what EARLIER steps filled (model_load_impl gives the order); none reads a table that a later step fills.

// reads: the blob.  fills: idx, the dimensions, task_id, nM, nsubstep, na, solver -- and checks every array the engine reads
static int derive_dims(fb_model* m, size_t n) {
  uint32_t narr; memcpy(&narr, m->blob.data() + 4, 4);
  if (narr > 4096 || 8 + (size_t)narr*sizeof(BlobEntry) > n) return fail("fb_model_load: corrupt table of contents");
  const BlobEntry* e = (const BlobEntry*)(m->blob.data() + 8);
  for (uint32_t k = 0; k < narr; k++) {
    if (!memchr(e[k].name, 0, sizeof(e[k].name))) return fail("fb_model_load: unterminated array name");
    if (e[k].dtype > 1) return fail(std::string("fb_model_load: array '") + e[k].name + "' has an unknown element type");
    if (e[k].offset > n || e[k].nbytes > n - e[k].offset) return fail(std::string("fb_model_load: array '") + e[k].name + "' lies outside the blob");
    if (e[k].offset % 8 != 0) return fail(std::string("fb_model_load: array '") + e[k].name + "' is misaligned");
    m->idx[std::string(e[k].name)] = e + k;
  }
  auto len = [&](const char* name) { size_t c; m->i(name, &c); return (int)c; };      // (a dimension is the length of an i32 array)
  { size_t c; m->d("qpos0", &c); m->nq = (int)c; }
  m->nv = len("dof_bodyid"); m->nbody = len("body_parent"); m->njnt = len("jnt_type"); m->ngeom = len("geom_type"); m->nsite = len("site_bodyid");
  m->nu = len("actuator_trntype"); m->ntendon = len("tendon_adr"); m->npair = len("pair_geom1");
  m->nobsjnt = len("observable_joints"); m->napp = len("appendage_sites"); m->nforce = len("sensor_force_sites"); m->ntouch = len("sensor_touch_sites");
  if (m->nq <= 0 || m->nv <= 0 || m->nbody <= 1 || m->njnt <= 0) return fail("fb_model_load: empty model");
  check_model_arrays(m);
  m->task_id = m->i("task_id")[0];
  m->nM = m->i("dof_Madr")[m->nv];
  if (!(m->d("opt_timestep")[0] > 0) || !(m->d("opt_control_timestep")[0] >= m->d("opt_timestep")[0])) return fail("fb_model_load: bad timestep / control timestep");
  m->nsubstep = (int)floor(m->d("opt_control_timestep")[0] / m->d("opt_timestep")[0] + 0.5);
  const int* actadr = m->i("actuator_actadr");
  m->na = 0; for (int k = 0; k < m->nu; k++) if (actadr[k] >= 0) m->na++;
  // opt_solver is optional: a blob without it gets MuJoCo's default, Newton -- what the reference XML selects (fruitfly.xml:4)
  m->solver = (m->has("opt_solver", 1) && m->i("opt_solver")[0] == FB_SOLVER_PGS) ? FB_SOLVER_PGS : FB_SOLVER_NEWTON;
  return 0;
}

// reads: body_parent, body_dofadr, body_dofnum, dof_parentid, dof_Madr.  fills: body_depth, body_nsub, fk_dmax, fk2_dlo, fk_second, dof_depth,
// body_chain, body_chlen, chmax, body_common, dof_ndesc, nlevel, lvl_dof, lvl_start
static int derive_topology(fb_model* m) {
  const int nb = m->nbody, nv = m->nv;
  const int *parent = m->i("body_parent"), *dofadr = m->i("body_dofadr"), *dofnum = m->i("body_dofnum"), *dofpar = m->i("dof_parentid");
  m->body_depth.assign(nb, 0); m->body_nsub.assign(nb, 1); m->fk_dmax = 0; m->fk2_dlo = 1 << 20;
  for (int b = 1; b < nb; b++) m->body_depth[b] = m->body_depth[parent[b]] + 1;
  for (int b = nb - 1; b > 0; b--) m->body_nsub[parent[b]] += m->body_nsub[b];
  for (int b = 1; b < nb; b++) { m->fk_dmax = std::max(m->fk_dmax, m->body_depth[b]); if (b >= FB_WAVE) m->fk2_dlo = std::min(m->fk2_dlo, m->body_depth[b]); }
  if (m->fk_dmax > FB_MAXDEPTH) return fail("fb_model_load: body tree deeper than FB_MAXDEPTH");
  // LDS staging of the position / velocity stages (fb_smooth.hpp): frames + joint rotations + anchors / axes; motion axes + inertias;
  // motion axes + body velocities + per-body wrenches -- all inside the smallest LDS pool of this build
  const int pool = std::min(LdsCfg<double>::POOL, LdsCfg<float>::POOL);
  if (nb > 2*FB_WAVE || 7*nb + 10*m->njnt > pool || 6*nv + 10*nb > pool || 6*nv + 12*nb > pool || m->nM + 1 > FB_LDS_SCRATCH) return fail("fb_model_load: model exceeds the per-environment LDS pool (bodies / joints / dofs)");
  if (m->nM > FB_MAXNM || nv > FB_MAXNV) return fail("fb_model_load: model exceeds the LDS capacity constants FB_MAXNM / FB_MAXNV");
  // DFS contiguity: every body in (b, b+nsub) must descend from b
  for (int b = 1; b < nb; b++)
    for (int d = b + 1; d < b + m->body_nsub[b]; d++) {
      int a = d; while (a > b) a = parent[a];
      if (a != b) return fail("fb_model_load: bodies are not in DFS order");
    }
  // kinematics level loop: bodies beyond the wavefront width ride along on lanes whose own body sits on a
  // SHALLOWER level, so one trip down the levels covers every body (fb_smooth.hpp fk_pass)
  if (nb > FB_WAVE) {
    m->fk_second.assign(FB_WAVE, -1);
    for (int b = FB_WAVE; b < nb && !m->fk_second.empty(); b++) {
      int pick = -1;
      for (int l = 0; l < FB_WAVE && pick < 0; l++) if (m->fk_second[l] < 0 && (l == 0 || m->body_depth[l] < m->body_depth[b])) pick = l;      // (deeper than the lane's own body: fk_pass reuses the record registers)
      if (pick < 0) m->fk_second.clear(); else m->fk_second[pick] = b;
    }
  }
  m->dof_depth.assign(nv, 0);
  for (int k = 0; k < nv; k++) { int a = dofpar[k], n_ = 0; while (a >= 0) { n_++; a = dofpar[a]; } m->dof_depth[k] = n_; }
  m->body_chlen.assign(nb, 0); m->body_chain.assign((size_t)nb*FB_MAXCH, 0); m->chmax = 0;
  for (int b = 1; b < nb; b++) {
    int a = b; while (a > 0 && dofnum[a] == 0) a = parent[a];
    if (a <= 0) continue;
    int last = dofadr[a] + dofnum[a] - 1;
    int len = m->dof_depth[last] + 1;
    if (len > FB_MAXCH) return fail("fb_model_load: dof chain longer than FB_MAXCH");
    m->body_chlen[b] = len; m->chmax = std::max(m->chmax, len);
    for (int k = last, s = len - 1; k >= 0; k = dofpar[k], s--) m->body_chain[(size_t)b*FB_MAXCH + s] = k;
  }
  m->body_common.assign((size_t)nb*nb, 0);
  for (int a = 0; a < nb; a++) for (int b = 0; b < nb; b++) {
    int n_ = 0, la = m->body_chlen[a], lb = m->body_chlen[b];
    while (n_ < la && n_ < lb && m->body_chain[(size_t)a*FB_MAXCH + n_] == m->body_chain[(size_t)b*FB_MAXCH + n_]) n_++;
    m->body_common[(size_t)a*nb + b] = n_;
  }
  // descendant ranges (dofs are in DFS order) and depth levels
  m->dof_ndesc.assign(nv, 0);
  for (int k = nv - 1; k >= 0; k--) if (dofpar[k] >= 0) m->dof_ndesc[dofpar[k]] += m->dof_ndesc[k] + 1;
  for (int k = 0; k < nv; k++)
    for (int q = k + 1; q <= k + m->dof_ndesc[k]; q++) {
      int a = q; while (a > k) a = dofpar[a];
      if (a != k) { return fail("fb_model_load: dofs are not in DFS order"); }
    }
  m->nlevel = 0;
  for (int k = 0; k < nv; k++) if (m->dof_depth[k] + 1 > m->nlevel) m->nlevel = m->dof_depth[k] + 1;
  m->lvl_start.assign(m->nlevel + 1, 0);
  for (int d = 0; d < m->nlevel; d++) {
    m->lvl_start[d] = (int)m->lvl_dof.size();
    for (int k = 0; k < nv; k++) if (m->dof_depth[k] == d) m->lvl_dof.push_back(k);
    if ((int)m->lvl_dof.size() - m->lvl_start[d] > FB_WAVE) { return fail("fb_model_load: more than 64 dofs on one depth level"); }
  }
  m->lvl_start[m->nlevel] = (int)m->lvl_dof.size();
  // The factor is stored ROW-major like qM: row k = [1/D[k], L[k,parent], L[k,grandparent], ...] at dof_Madr[k].
  // Along an unbranched chain consecutive rows grow by one entry, so the row start of the descendant of dof i on
  // depth level d is  dof_Madr[i] - T(depth[i]) + T(d)  with T(d) = d(d+1)/2 -- no table lookup.
  const int* madr = m->i("dof_Madr");
  int adr = 0;
  for (int k = 0; k < nv; k++) { if (madr[k] != adr) return fail("fb_model_load: dof_Madr does not match the dof tree"); adr += m->dof_depth[k] + 1; }
  if (adr != m->nM) return fail("fb_model_load: dof_Madr does not match the dof tree");
  return 0;
}

// reads: dof_parentid, dof_Madr, dof_depth, dof_ndesc, nlevel, lvl_dof, lvl_start.  fills: dof_cl, ntrunk, dof_gen, ngen, gen_k, gen_m, fwd_tab, fwd_pack
// Pure-chain length below each dof (descendants i+1 .. i+cl are one unbranched chain).  The unbranched chain
// that starts at dof 0 is the "trunk" (the free joint): its rows are handled wave-parallel.  Other dofs whose
// subtree branches further down ("general" dofs: head, ...) get a per-level list of their descendants.
static int derive_trunk_and_ancestors(fb_model* m) {
  const int nv = m->nv; const int* dofpar = m->i("dof_parentid"); const int* madr = m->i("dof_Madr");
  std::vector<int> nchild(nv, 0);
  for (int k = 0; k < nv; k++) if (dofpar[k] >= 0) nchild[dofpar[k]]++;
  m->dof_cl.assign(nv, 0);
  for (int k = nv - 2; k >= 0; k--) m->dof_cl[k] = (nchild[k] == 1) ? m->dof_cl[k + 1] + 1 : 0;
  // the trunk optimisation needs ONE dof tree whose root chain is an ancestor of every other dof (free-joint models);
  // a forest (tethered fly: every limb is its own tree) has no trunk
  int nroots = 0; for (int k = 0; k < nv; k++) if (dofpar[k] < 0) nroots++;
  m->ntrunk = (nroots == 1) ? std::min(m->dof_cl[0] + 1, FB_MAXTRUNK) : 0;
  m->dof_gen.assign(nv, -1);
  for (int k = m->ntrunk; k < nv; k++) if (m->dof_ndesc[k] > m->dof_cl[k]) m->dof_gen[k] = m->ngen++;
  if (m->ngen > 15 || m->ngen > FB_MAXGEN || m->ngen > FB_LGEN) { return fail("fb_model_load: more than FB_MAXGEN branching dofs"); }
  m->gen_k.assign((size_t)FB_MAXGEN*FB_MAXCH, -1);            // 4 descendant dof ids per (general dof, level), 0xff = none
  m->gen_m.assign((size_t)FB_MAXGEN*FB_MAXCH*2, -1);          // ... and their row starts, 4 x u16, 0xffff = none
  for (int k = 0; k < nv; k++) {
    if (m->dof_gen[k] < 0) continue;
    for (int d = 0; d < m->nlevel; d++) {
      unsigned pk = 0xffffffffu; unsigned long long pm = ~0ull; int cnt = 0;
      for (int t = m->lvl_start[d]; t < m->lvl_start[d + 1]; t++) {
        int q = m->lvl_dof[t];
        if (q > k && q <= k + m->dof_ndesc[k]) {
          if (cnt == 4) { return fail("fb_model_load: a branching dof has more than 4 descendants on one level"); }
          pk = (pk & ~(0xffu << (8*cnt))) | ((unsigned)q << (8*cnt));
          pm = (pm & ~(0xffffull << (16*cnt))) | ((unsigned long long)madr[q] << (16*cnt));
          cnt++;
        }
      }
      size_t o = (size_t)m->dof_gen[k]*FB_MAXCH + d;
      m->gen_k[o] = (int)pk; m->gen_m[2*o] = (int)(unsigned)(pm & 0xffffffffu); m->gen_m[2*o + 1] = (int)(unsigned)(pm >> 32);
    }
  }
  // forward-substitution table: ancestor of dof k on level d
  m->fwd_tab.assign((size_t)FB_MAXCH*FB_MAXNV, 0);
  for (int k = 0; k < nv; k++)
    for (int a = dofpar[k]; a >= 0; a = dofpar[a]) m->fwd_tab[(size_t)m->dof_depth[a]*FB_MAXNV + k] = a;
  // ... the same, four levels per word (8-bit dof ids): the solve's root-to-leaf loop fetches one word per four levels, one block
  // ahead, instead of one table entry per level with a global-memory latency on every level
  if (nv > 255) return fail("fb_model_load: more than 255 dofs (packed ancestor table)");
  if (m->nbody > 2*FB_WAVE || 6*nv + 10*m->nbody > FB_LDS_SCRATCH + 276) return fail("fb_model_load: bodies / dofs exceed the LDS staging of the inertia stages");
  m->fwd_pack.assign((size_t)((FB_MAXCH + 3)/4)*FB_MAXNV, 0);
  for (int k = 0; k < nv; k++)
    for (int a = dofpar[k]; a >= 0; a = dofpar[a]) { int d = m->dof_depth[a]; m->fwd_pack[(size_t)(d >> 2)*FB_MAXNV + k] |= (int)((unsigned)a << (8*(d & 3))); }
  return 0;
}

// reads: dof_parentid, dof_Madr, dof_depth, dof_ndesc, dof_cl, dof_gen, ntrunk.  fills: fac_w, fac_band, fac_dof
// Factorisation work list: every off-diagonal entry (i, j) of the lower triangle with i outside the trunk is
// owned by one (lane, slot); the diagonal of dof j belongs to lane j & 63.  Entries are spread so that the number
// of triple products (= ndesc[i] per entry) is balanced over the 64 lanes.  Entries of general dofs need the
// descendant lists and may only sit in the first FB_FGEN slots.  One packed word per slot (fb_smooth.hpp).
static int derive_factor_list(fb_model* m) {
  const int nv = m->nv; const int* dofpar = m->i("dof_parentid"); const int* madr = m->i("dof_Madr");
  struct Ent { int i, j, work; bool gen; };
  std::vector<Ent> gen_ents, chain_ents;
  for (int i = m->ntrunk; i < nv; i++)
    for (int j = dofpar[i]; j >= 0; j = dofpar[j]) (m->dof_gen[i] >= 0 ? gen_ents : chain_ents).push_back({i, j, m->dof_ndesc[i] + 1, m->dof_gen[i] >= 0});
  m->fac_w.assign((size_t)FB_FSLOT*FB_WAVE, (31 << 13) | (int)(15u << 28));        // depth 31: empty slot
  auto put = [&](const Ent& e, int lane_, int slot) -> bool {
    int dep = m->dof_depth[e.i], base = madr[e.i] - dep*(dep + 1)/2, ee = dep - m->dof_depth[e.j];
    if (base < -4096 || base > 4095 || dep > 30) return false;
    m->fac_w[(size_t)slot*FB_WAVE + lane_] = (base & 0x1fff) | (dep << 13) | (m->dof_cl[e.i] << 18) | (ee << 23) | (int)((unsigned)(e.gen ? m->dof_gen[e.i] : 15) << 28);
    return true;
  };
  // Entries of branching dofs: the first FB_FGEN slots, spread over the lanes.
  std::vector<int> ngs(FB_WAVE, 0);
  if ((int)gen_ents.size() > FB_FGEN*FB_WAVE) { return fail("fb_model_load: lower triangle of M does not fit the factor work list"); }
  for (size_t k = 0; k < gen_ents.size(); k++) { int l = (int)(k % FB_WAVE); if (!put(gen_ents[k], l, ngs[l]++)) return fail("fb_model_load: factor work list field overflow"); }
  // Chain entries: sorted deepest dof first and DEALT to the lanes in turn, so slot s of every lane holds entries of (nearly) the
  // same depth.  An entry publishes on level dep and pulls on levels dep+1 .. dep+cl; with this order the slots that do
  // anything on a level form a narrow band that is the same for all lanes, and the level loop skips the rest (fac_band).
  // (first key: the deepest level the entry still pulls on -- the abdomen's rows, which alone reach the last levels, then share a
  // few slots instead of being spread over all of them by their depth)
  std::stable_sort(chain_ents.begin(), chain_ents.end(), [&](const Ent& a, const Ent& b) {
    int da = m->dof_depth[a.i], db = m->dof_depth[b.i], la = da + m->dof_cl[a.i], lb = db + m->dof_cl[b.i];
    if (la != lb) return la > lb; if (da != db) return da > db; return a.work > b.work; });
  const int nchain_slots = FB_FSLOT - FB_FGEN; size_t placed = 0;
  for (; placed < chain_ents.size() && placed < (size_t)nchain_slots*FB_WAVE; placed++)
    if (!put(chain_ents[placed], (int)(placed % FB_WAVE), FB_FGEN + (int)(placed / FB_WAVE))) return fail("fb_model_load: factor work list field overflow");
  // what does not fit the chain slots (the shallowest entries) goes to free slots of the first FB_FGEN (never skipped)
  for (; placed < chain_ents.size(); placed++) {
    int best = -1;
    for (int l = 0; l < FB_WAVE; l++) if (ngs[l] < FB_FGEN && (best < 0 || ngs[l] < ngs[best])) best = l;
    if (best < 0) { return fail("fb_model_load: lower triangle of M does not fit the factor work list"); }
    if (!put(chain_ents[placed], best, ngs[best]++)) return fail("fb_model_load: factor work list field overflow");
  }
  // per level: bit masks of the chain slots that publish (dep == d) and that pull (dep < d <= dep + cl), over all lanes
  m->fac_band.assign(64, 0);
  for (int d = 0; d < 32; d++) {
    unsigned pub = 0, pull = 0;
    for (int s = FB_FGEN; s < FB_FSLOT; s++)
      for (int l = 0; l < FB_WAVE; l++) {
        int wd = m->fac_w[(size_t)s*FB_WAVE + l], dep = (wd >> 13) & 31, cl_ = (wd >> 18) & 31;
        if (dep == 31) continue;
        if (dep == d) pub |= 1u << s;
        if (dep < d && d <= dep + cl_) pull |= 1u << s;
      }
    m->fac_band[2*d] = (int)pub; m->fac_band[2*d + 1] = (int)pull;
  }
  // rows of the factorisation / the solves per lane, dealt by depth: the 64 shallowest dofs outside the trunk are the lanes' first rows
  // (in dof order, so that neighbouring lanes still hold neighbouring rows), the deeper ones their second rows (fb_smooth.hpp: fac_dof)
  std::vector<int> order;
  for (int i = m->ntrunk; i < nv; i++) order.push_back(i);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return m->dof_depth[a] < m->dof_depth[b]; });
  if ((int)order.size() > 2*FB_WAVE) { return fail("fb_model_load: more dofs than two rows per lane"); }
  std::vector<int> first(order.begin(), order.begin() + std::min<size_t>(order.size(), FB_WAVE)), second(order.begin() + std::min<size_t>(order.size(), FB_WAVE), order.end());
  std::sort(first.begin(), first.end()); std::sort(second.begin(), second.end());
  m->fac_dof.assign(2*FB_WAVE, 255);
  for (size_t k = 0; k < first.size(); k++) m->fac_dof[k] = first[k];
  for (size_t k = 0; k < second.size(); k++) m->fac_dof[FB_WAVE + k] = second[k];
  return 0;
}

// reads: pair_geom1, pair_geom2, geom_type, geom_bodyid, geom_size, geom_rbound.  fills: plane_geoms, nplane, pair_word, pair_body, geom_box, vl_delta
// Collision mid phase: one packed word per candidate pair; the geoms' bounding spheres (and the plane normals) are
// staged in LDS (the Delassus-matrix slot, free at that point of the step), fb_collide.hpp: d_collision
static int derive_collision(fb_model* m) {
  const int *g1 = m->i("pair_geom1"), *g2 = m->i("pair_geom2"), *gt = m->i("geom_type"), *gb = m->i("geom_bodyid");
  std::vector<int> slot(m->ngeom, 0);
  for (int g = 0; g < m->ngeom; g++) if (gt[g] == GEOM_PLANE) { m->plane_geoms.push_back(g); slot[g] = m->ngeom + (int)m->plane_geoms.size() - 1; }
  m->nplane = (int)m->plane_geoms.size();
  if (m->ngeom + m->nplane > 1023 || 4*(m->ngeom + m->nplane) > LdsCfg<double>::AR_ELEMS + FB_MAXNV) { return fail("fb_model_load: too many geoms for the LDS staging area of the collision mid phase"); }
  m->pair_word.assign(std::max(m->npair, 1), 0);
  // the two bodies of a pair, packed (b1 | b2 << 16): constant, so that a contact's bodies are one lookup behind its pair id
  // instead of pair -> geom -> body
  m->pair_body.assign(std::max(m->npair, 1), 0);
  for (int q = 0; q < m->npair; q++) m->pair_body[q] = gb[g1[q]] | (gb[g2[q]] << 16);
  for (int q = 0; q < m->npair; q++) {
    if (gt[g2[q]] == GEOM_PLANE) { return fail("fb_model_load: a plane must be the first geom of a pair"); }
    // bit 30: the pair goes through the convex narrow phase (MPR) -- everything but plane-x, sphere-sphere, sphere-capsule and
    // capsule-capsule, which have closed forms (fb_collide.hpp: narrow_phase)
    const int t1 = gt[g1[q]], t2 = gt[g2[q]];
    const bool analytic = t1 == GEOM_PLANE || (t1 == GEOM_SPHERE && (t2 == GEOM_SPHERE || t2 == GEOM_CAPSULE)) || (t1 == GEOM_CAPSULE && t2 == GEOM_CAPSULE);
    m->pair_word[q] = g1[q] | (g2[q] << 10) | (slot[g1[q]] << 20) | (analytic ? 0 : (1 << 30));
  }
  if (m->plane_geoms.empty()) m->plane_geoms.push_back(0);
  const double* gs = m->d("geom_size");
  m->geom_box.assign(3*std::max(m->ngeom, 1), 0.0);
  for (int g = 0; g < m->ngeom; g++) {
    double* e = &m->geom_box[3*g]; const double* sz = gs + 3*g;
    if (gt[g] == GEOM_CAPSULE) { e[0] = e[1] = sz[0]; e[2] = sz[1] + sz[0]; }
    else if (gt[g] == GEOM_CYLINDER) { e[0] = e[1] = sz[0]; e[2] = sz[1]; }
    else if (gt[g] == GEOM_ELLIPSOID) { e[0] = sz[0]; e[1] = sz[1]; e[2] = sz[2]; }
    else { e[0] = e[1] = e[2] = sz[0]; }
  }
  // neighbour-list slack: half the median bounding radius of the geoms that have one (planes: 0) -- the fruit fly: 0.0083 model units; measured best of
  // 0.002 ... 0.06 (profiles/r6/ab_neighbour_list.txt).  No list for models whose pair count fits a few wave passes anyway.
  std::vector<double> rb; const double* r_ = m->d("geom_rbound");
  for (int g = 0; g < m->ngeom; g++) if (r_[g] > 0) rb.push_back(r_[g]);
  std::sort(rb.begin(), rb.end());
  m->vl_delta = (rb.empty() || m->npair <= 4*FB_WAVE) ? 0.0 : FB_VL_SCALE*rb[rb.size()/2];
  // the list's validity test watches the geom centres only: a plane on a moving body could turn its normal without moving its centre -- no list then
  for (int g = 0; g < m->ngeom; g++) if (gt[g] == GEOM_PLANE && gb[g] != 0) m->vl_delta = 0;
  return 0;
}

// reads: actuator_trntype, actuator_trnid, wrap_dofid, wrap_coef, tendon_adr, tendon_num, dof_jntid, jnt_qposadr, jnt_dofadr.
// fills: adh_act, wrap_qadr, act_wn, act_wdof, act_wcoef, act_lenadr
// Flattened actuator transmissions and tendon wraps: one padded record per actuator / wrap, so that the kernel fetches
// them with a fixed number of independent loads instead of walking tendon_adr -> wrap_dofid -> dof_jntid -> jnt_qposadr
static int derive_transmissions(fb_model* m) {
  const int* trn = m->i("actuator_trntype");
  for (int k = 0; k < m->nu; k++) if (trn[k] == TRN_BODY) m->adh_act.push_back(k);
  size_t nw_ = 0; const int *wd = m->i("wrap_dofid", &nw_), *tadr = m->i("tendon_adr"), *tnum = m->i("tendon_num"), *tid = m->i("actuator_trnid");
  const int *djnt = m->i("dof_jntid"), *jqa = m->i("jnt_qposadr"), *jda = m->i("jnt_dofadr");
  const double* wc = m->d("wrap_coef");
  m->wrap_qadr.assign(std::max<size_t>(nw_, 1), 0);
  for (size_t k = 0; k < nw_; k++) m->wrap_qadr[k] = jqa[djnt[wd[k]]];
  for (int t = 0; t < m->ntendon; t++) if (tnum[t] > FB_MAXWRAP) { return fail("fb_model_load: tendon with more than FB_MAXWRAP joints"); }
  m->act_wn.assign(m->nu, 0); m->act_lenadr.assign(m->nu, 0);
  m->act_wdof.assign((size_t)m->nu*FB_MAXWRAP, 0); m->act_wcoef.assign((size_t)m->nu*FB_MAXWRAP, 0.0);
  std::vector<int> owner(m->nv, -1);
  for (int k = 0; k < m->nu; k++) {
    int n_ = 0;
    if (trn[k] == TRN_JOINT) { m->act_wdof[(size_t)k*FB_MAXWRAP] = jda[tid[k]]; m->act_wcoef[(size_t)k*FB_MAXWRAP] = 1.0; m->act_lenadr[k] = jqa[tid[k]]; n_ = 1; }
    else if (trn[k] == TRN_TENDON) {
      for (int q = 0; q < tnum[tid[k]]; q++) { m->act_wdof[(size_t)k*FB_MAXWRAP + q] = wd[tadr[tid[k]] + q]; m->act_wcoef[(size_t)k*FB_MAXWRAP + q] = wc[tadr[tid[k]] + q]; }
      m->act_lenadr[k] = tid[k]; n_ = tnum[tid[k]];
    }
    m->act_wn[k] = n_;
    // the kernel scatters joint / tendon actuator forces with plain stores (one lane per actuator): dofs must not be shared
    for (int q = 0; q < n_; q++) {
      int dq = m->act_wdof[(size_t)k*FB_MAXWRAP + q];
      if (owner[dq] >= 0) { return fail("fb_model_load: two joint/tendon actuators drive the same dof"); }
      owner[dq] = k;
    }
  }
  return 0;
}

// reads: body_parent, body_pos / quat / ipos / iquat, body_jntadr, body_jntnum, jnt_pos, jnt_axis, jnt_type, jnt_qposadr, body_mass, body_inertia.
// fills: body_rec, body_box, totalmass
// Per-body kinematics record: every constant the frame composition of one body needs, contiguous, so that a
// tree level costs one round of independent loads instead of a chain of table lookups (fb_smooth.hpp: fk_pass)
static int derive_body_records(fb_model* m) {
  const int nb = m->nbody; const int* parent = m->i("body_parent");
  const double* mass = m->d("body_mass"); const double* inert = m->d("body_inertia");
  const double *bp = m->d("body_pos"), *bq = m->d("body_quat"), *bip = m->d("body_ipos"), *biq = m->d("body_iquat");
  const double *jp = m->d("jnt_pos"), *jx = m->d("jnt_axis");
  const int *bja = m->i("body_jntadr"), *bjn = m->i("body_jntnum"), *jt = m->i("jnt_type"), *jqa = m->i("jnt_qposadr");
  m->body_rec.assign((size_t)nb*FB_BODYREC, 0);
  for (int b = 0; b < nb; b++) {
    double* R = m->body_rec.data() + (size_t)b*FB_BODYREC;
    int jn = bjn[b], ja = bja[b];
    if (jn > 3) { return fail("fb_model_load: more than 3 joints on one body"); }
    bool fr = jn > 0 && jt[ja] == JNT_FREE;
    if (fr && jn != 1) { return fail("fb_model_load: a free joint must be the only joint of its body"); }
    R[0] = parent[b]; R[1] = ja; R[2] = jn; R[3] = fr ? 1 : 0;
    for (int k = 0; k < 3; k++) { R[4 + k] = bp[3*b + k]; R[11 + k] = bip[3*b + k]; }
    for (int k = 0; k < 4; k++) { R[7 + k] = bq[4*b + k]; R[14 + k] = biq[4*b + k]; }
    for (int q = 0; q < jn; q++) for (int k = 0; k < 3; k++) { R[18 + 6*q + k] = jp[3*(ja + q) + k]; R[21 + 6*q + k] = jx[3*(ja + q) + k]; }
    R[36] = fr ? jqa[ja] : 0;
  }
  m->body_box.assign((size_t)nb*3, 0); m->totalmass = 0;
  for (int b = 1; b < nb; b++) {
    m->totalmass += mass[b];
    if (mass[b] < 1e-15) continue;
    const double* I = inert + 3*b;
    m->body_box[3*b+0] = sqrt(fmax(1e-15, I[1] + I[2] - I[0]) / mass[b] * 6.0);
    m->body_box[3*b+1] = sqrt(fmax(1e-15, I[0] + I[2] - I[1]) / mass[b] * 6.0);
    m->body_box[3*b+2] = sqrt(fmax(1e-15, I[0] + I[1] - I[2]) / mass[b] * 6.0);
  }
  return 0;
}

// reads: dof_parentid, dof_jntid, jnt_type, jnt_dofadr, dof_depth, ntrunk, body_chain, body_chlen.  fills: dof_jump, prefix_split, dof_vbef, body_veldof
// Tree prefix sums over the dofs (body velocities, bias accelerations): ancestors at distance 2^k, the dof whose inclusive
// velocity prefix is the velocity "before" a dof (mj_comVel: the parent body's velocity plus the earlier dofs of the same body;
// a free joint's rotational axes see its three translations, a ball joint none of its own dofs), the last dof of a body's chain
static int derive_prefix_tables(fb_model* m) {
  const int nb = m->nbody, nv = m->nv; const int* dofpar = m->i("dof_parentid");
  if (FB_MAXCH > (1 << FB_NJUMP) || nv > 2*FB_WAVE) return fail("fb_model_load: dof tree too deep / too wide for the prefix tables");
  m->dof_jump.assign((size_t)FB_NJUMP*nv, -1);
  for (int i = 0; i < nv; i++) {
    if (dofpar[i] >= i) return fail("fb_model_load: dof_parentid must number parents before children (the prefix sums exchange one slot for the ancestors of the first 64 dofs)");
    m->dof_jump[i] = dofpar[i];
  }
  // Round 6: when every chain is at most 2^(FB_NJUMP - 1) dofs long BELOW the trunk (the fruit fly: 6 trunk dofs + <= 14), the jumps of the other dofs
  // stop at the trunk: four rounds finish the trunk's own prefixes and everybody else's sum over their non-trunk ancestors, and the trunk's total -- common
  // to all of them -- is added by one broadcast (tree_prefix6).  One round of lane exchanges less in each of the three prefix sums of a substep.
  const int nT = m->ntrunk; int below = 0; m->prefix_split = 0;
  for (int i = nT; i < nv; i++) below = std::max(below, m->dof_depth[i] + 1 - nT);
  if (nT > 0 && nT <= (1 << (FB_NJUMP - 1)) && below <= (1 << (FB_NJUMP - 1))) {
    bool ok = true;
    for (int i = nT; i < nv; i++) { int a = i; while (dofpar[a] >= nT) a = dofpar[a]; ok = ok && dofpar[a] == nT - 1; }      // (everything hangs off the last trunk dof)
    if (ok) { m->prefix_split = 1; for (int i = nT; i < nv; i++) if (dofpar[i] < nT) m->dof_jump[i] = -1; }
  }
  for (int k = 1; k < FB_NJUMP; k++)
    for (int i = 0; i < nv; i++) { int a = m->dof_jump[(size_t)(k - 1)*nv + i]; m->dof_jump[(size_t)k*nv + i] = a >= 0 ? m->dof_jump[(size_t)(k - 1)*nv + a] : -1; }
  const int *djnt = m->i("dof_jntid"), *jt = m->i("jnt_type"), *jda = m->i("jnt_dofadr");
  m->dof_vbef.assign(nv, -1);
  for (int i = 0; i < nv; i++) {
    int j = djnt[i];
    if (jt[j] == JNT_FREE) m->dof_vbef[i] = (i - jda[j] < 3) ? -2 : jda[j] + 2;
    else if (jt[j] == JNT_BALL) m->dof_vbef[i] = dofpar[jda[j]];
    else m->dof_vbef[i] = dofpar[i];
  }
  m->body_veldof.assign(nb, -1);
  for (int b = 1; b < nb; b++) if (m->body_chlen[b] > 0) m->body_veldof[b] = m->body_chain[(size_t)b*FB_MAXCH + m->body_chlen[b] - 1];
  return 0;
}

// reads: site_bodyid, sensor_site_thorax, sensor_force_sites, body_nsub, geom_fluid, geom_bodyid.  fills: sens_body, body_fluid_geom
// Bodies whose acceleration / force the sensors need: the accelerometer's body and the subtrees below the force-sensor bodies
// (none listed when there are more than 64: all bodies are processed then); the fluid geom of each body
static int derive_sensor_and_fluid_bodies(fb_model* m) {
  const int nb = m->nbody; const int* sb = m->i("site_bodyid");
  std::vector<char> need(nb, 0);
  need[sb[m->i("sensor_site_thorax")[0]]] = 1;
  size_t nf = 0; const int* fs = m->i("sensor_force_sites", &nf);
  for (size_t k = 0; k < nf; k++) { int b = sb[fs[k]]; for (int d = 0; d < m->body_nsub[b]; d++) need[b + d] = 1; }
  for (int b = 0; b < nb; b++) if (need[b]) m->sens_body.push_back(b);
  if ((int)m->sens_body.size() > FB_WAVE) m->sens_body.clear();
  m->body_fluid_geom.assign(nb, -1);
  { const double* gfl = m->d("geom_fluid"); const int* gb = m->i("geom_bodyid");
    for (int g = 0; g < m->ngeom; g++) if (gfl[12*g] > 0) m->body_fluid_geom[gb[g]] = g; }
  return 0;
}

static int model_load_impl(fb_model* m, size_t n) {
  return derive_dims(m, n) || derive_topology(m) || derive_trunk_and_ancestors(m) || derive_factor_list(m) || derive_collision(m) ||
         derive_transmissions(m) || derive_body_records(m) || derive_prefix_tables(m) || derive_sensor_and_fluid_bodies(m) ? -1 : 0;
}

extern "C" void fb_model_destroy(fb_model* m) { delete m; }

// Width of the observation vector (engine.observation_layout; fb_task.hpp: d_pack_obs writes it): the walker's own observables, 7 per reference frame
// of the imitation tasks (nref = future_steps + 1 of them) and, for walk_on_ball, the ball's velocity
static int obs_width(const fb_model* m, int nref, bool ball) {
  return 3 + m->na + 3*m->napp + (ball ? 3 : 0) + 3*m->nforce + 3 + 2*m->nobsjnt + 7*nref + m->ntouch + 3 + 3;
}

extern "C" int fb_model_dim(const fb_model* m, const char* name) {
  if (!m || !name) return -1;
#define X(f) if (!strcmp(name, #f)) return m->f
  X(nq); X(nv); X(nbody); X(njnt); X(ngeom); X(nsite); X(nu); X(na); X(ntendon); X(npair); X(nM); X(nsubstep);
  X(nobsjnt); X(napp); X(nforce); X(ntouch); X(task_id);
#undef X
  if (!strcmp(name, "nact")) return m->nu + (m->i("user_action_idx")[0] >= 0 ? 1 : 0);
  if (!strcmp(name, "nobs_base")) return obs_width(m, 0, false);
  // where this build places the Delassus matrix (LdsCfg; d_constraint_a): rows of the LDS matrix slot, rows of the wide LDS placement
  if (!strcmp(name, "lds_ar_rows_f64")) return LdsCfg<double>::AR_ROWS;
  if (!strcmp(name, "lds_wide_rows_f64")) return LdsCfg<double>::WIDE_ROWS;
  if (!strcmp(name, "lds_ar_rows_f32")) return LdsCfg<float>::AR_ROWS;
  if (!strcmp(name, "lds_wide_rows_f32")) return LdsCfg<float>::WIDE_ROWS;
  return -1;
}
