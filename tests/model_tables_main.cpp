// TEST INFRASTRUCTURE ONLY -- what a batch's DevModel holds, as text (tests/test_model_tables.py builds this program with -DFB_EMULATE
// -DFB_EMU_NO_LAUNCH -fsanitize=address,undefined and compares its output with a recording of the parent commit's).  It loads one blob
// written by pack_model, or two for a group, creates an FP64 and an FP32 batch and prints, for every model of the batch: each table of
// FB_MODEL_TABLES and the two tables beside it (leg_jnt, fk_second) with element kind, byte count and an FNV-1a digest of the bytes, and
// every scalar member of DevModel.  In the emulation build a device pointer is a host pointer; the DevBuf in b->allocs that owns it
// gives the byte count.
//   model_tables BLOB [BLOB2]   -> one line per table and scalar, exit 0
#include "../flybody_amd/csrc/fb_engine.hip"

static unsigned long long fnv1a(const void* p, size_t n) {
  unsigned long long h = 1469598103934665603ull;
  for (size_t k = 0; k < n; k++) { h ^= ((const unsigned char*)p)[k]; h *= 1099511628211ull; }
  return h;
}

static int print_table(const fb_batch* b, const char* tag, const char* name, const char* kind, const void* p) {
  for (const auto& d : b->allocs)
    if (d.get() == p) { printf("%s table %s %s %zu %016llx\n", tag, name, kind, d.count(), fnv1a(p, d.count())); return 0; }
  fprintf(stderr, "%s: table %s is no allocation of the batch (%p)\n", tag, name, p);
  return 1;
}

static void print_scalar(const char* tag, const char* name, int v) { printf("%s scalar %s %d\n", tag, name, v); }
static void print_scalar(const char* tag, const char* name, unsigned v) { printf("%s scalar %s %u\n", tag, name, v); }
static void print_scalar(const char* tag, const char* name, double v) { printf("%s scalar %s %.17g\n", tag, name, v); }     // (a float prints exactly too)

template <typename real>
static int print_model(const fb_batch* b, const char* tag, const DevModel<real>& M) {
  int bad = 0;
#define X(member, kind, from, source) bad += print_table(b, tag, #member, #kind, (const void*)(const kind*)M.member);
  FB_MODEL_TABLES(X)
#undef X
  bad += print_table(b, tag, "leg_jnt", "int", (const void*)(const int*)M.leg_jnt);
  printf("%s fk_second %s\n", tag, M.fk_second ? "set" : "null");
  if (M.fk_second) bad += print_table(b, tag, "fk_second", "int", M.fk_second);
#define S(f) print_scalar(tag, #f, M.f);
  S(nq) S(nv) S(nbody) S(njnt) S(ngeom) S(nsite) S(nu) S(na) S(ntendon) S(npair) S(nM) S(nsubstep)
  S(nobsjnt) S(napp) S(nforce) S(ntouch) S(site_thorax) S(nadh) S(iterations) S(noslip_iterations) S(solver)
  S(timestep) S(control_timestep) S(grav[0]) S(grav[1]) S(grav[2]) S(density) S(viscosity) S(impratio) S(tolerance) S(noslip_tolerance)
  S(meaninertia) S(totalmass) S(vl_delta) S(ar_entry_lanes) S(solver_handover)
  S(nlevel) S(ntrunk) S(prefix_split) S(chmax) S(fk_dmax) S(fk2_dlo) S(nplane) S(nsensbody)
  S(T) S(future_steps) S(episode_steps) S(nobs) S(terminal_com_dist) S(time_limit) S(task) S(nact) S(user_idx) S(seed)
  S(com_offset[0]) S(com_offset[1]) S(com_offset[2]) S(wb_nfreq) S(wb_base_freq) S(wb_rel_range) S(wb_rate)
  S(ds_nj) S(ds_ns) S(ds_ntraj) S(ds_nselect) S(ds_env_base) S(max_episode_steps) S(ds_random_start) S(nlegjnt)
  S(off.nreal) S(off.nint)
#undef S
  printf("%s offsets %016llx\n", tag, fnv1a(&M.off, sizeof(M.off)));
  // the tables a setter fills later are null in a new batch
  const void* later[] = {(const real*)M.ref_qpos, (const real*)M.ref_qvel, (const real*)M.wb_traj, (const real*)M.wb_phase, (const real*)M.wb_freqs,
                         (const int*)M.wb_offset, (const real*)M.ds_qpos, (const real*)M.ds_qvel, (const real*)M.ds_r2s, (const real*)M.ds_jq,
                         (const int*)M.ds_offset, (const int*)M.ds_jid, (const int*)M.ds_sid, (const int*)M.ds_select};
  for (const void* p : later) if (p) { fprintf(stderr, "%s: a setter's table is set in a new batch\n", tag); bad++; }
  return bad;
}

static int read_blob(const char* path, std::vector<char>& blob) {
  FILE* f = fopen(path, "rb"); if (!f) { perror(path); return 1; }
  char buf[65536]; size_t n; while ((n = fread(buf, 1, sizeof(buf), f)) > 0) blob.insert(blob.end(), buf, buf + n);
  fclose(f);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 2 && argc != 3) { fprintf(stderr, "usage: %s MODEL_BLOB [SECOND_MODEL_BLOB]\n", argv[0]); return 2; }
  const int nm = argc - 1;
  fb_model* models[2] = {nullptr, nullptr};
  for (int k = 0; k < nm; k++) {
    std::vector<char> blob;
    if (read_blob(argv[1 + k], blob)) return 2;
    if (fb_model_load(blob.data(), blob.size(), &models[k])) { fprintf(stderr, "fb_model_load: %s\n", fb_last_error()); return 1; }
  }
  int bad = 0;
  for (int precision : {64, 32}) {
    fb_batch* b = nullptr;
    const int rc = nm == 1 ? fb_batch_create(models[0], 3, 0, precision, &b) : fb_batch_create_group(models, nm, 3, 0, precision, &b);
    if (rc) { fprintf(stderr, "batch creation: %s\n", fb_last_error()); return 1; }
    bad += with_model(b, [&](auto& M) {
      auto& G = group_models(b, M);
      int bad_ = 0;
      for (int k = 0; k < nm; k++) {
        char tag[16]; snprintf(tag, sizeof(tag), "f%d.m%d", precision, k);
        bad_ += print_model(b, tag, G.empty() ? M : G[k]);
      }
      return bad_; });
    fb_batch_destroy(b);
  }
  for (int k = 0; k < nm; k++) fb_model_destroy(models[k]);
  return bad ? 1 : 0;
}
