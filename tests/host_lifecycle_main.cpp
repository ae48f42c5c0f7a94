// TEST INFRASTRUCTURE ONLY -- the engine's host layer as a stand-alone program (tests/test_host_ownership_emulation.py builds it with
// -DFB_EMULATE -DFB_EMU_NO_LAUNCH -fsanitize=address,undefined and runs it on a blob written by pack_model).  Through the C-ABI: the life
// cycle of a batch with every entry point that allocates, for an FP64 batch, an FP32 batch and a group of two models, and one failed
// allocation per entry point.  Kernel launches are compiled out (the emulation's fibers switch stacks by hand, which AddressSanitizer's
// stack bookkeeping does not follow): ownership, growth and the error paths are what is under test.
//   host_lifecycle BLOB   -> "host lifecycle ok", exit 0
#include "../flybody_amd/csrc/fb_engine.hip"

#define OK(x) do { if ((x) != 0) { fprintf(stderr, "line %d: %s failed: %s\n", __LINE__, #x, fb_last_error()); return 1; } } while (0)
#define REQUIRE(x) do { if (!(x)) { fprintf(stderr, "line %d: %s does not hold (%s)\n", __LINE__, #x, fb_last_error()); return 1; } } while (0)
// the next allocation fails: the call reports it with a message
#define FAILS(x) do { fb_emu_fail_alloc(0); const int rc_ = (x); fb_emu_fail_alloc(-1); \
                      if (rc_ == 0 || !fb_last_error()[0]) { fprintf(stderr, "line %d: %s did not fail with a message\n", __LINE__, #x); return 1; } } while (0)

static const int N = 3;

struct Inputs {
  std::vector<double> ref_qpos, ref_qvel, zeros, law_rows, target;
  std::vector<float> action;
  std::vector<int32_t> sites, include;
};

static int set_reference(fb_batch* b, const Inputs& in) { return fb_batch_set_reference(b, in.ref_qpos.data(), in.ref_qvel.data(), 8, 2, 1e30, 10.0); }
static int set_law(fb_batch* b, const Inputs& in, int rows) {
  fb_control_law law = {in.law_rows.data(), nullptr, nullptr, nullptr, in.law_rows.data(), rows};
  return fb_batch_set_control_law(b, &law);
}
static int ik(fb_batch* b, const Inputs& in, int n_site) {
  fb_ik_config cfg = {n_site, 0, in.sites.data(), nullptr, in.include.data(), 0.0, 0.01, 0.99, 0.01, 3};
  return fb_batch_ik(b, &cfg, in.target.data(), nullptr);
}
static int transition_fd(fb_batch* b, const fb_model* m, int n_frames) {
  const int ndx = 2*fb_model_dim(m, "nv") + fb_model_dim(m, "na"), nu = fb_model_dim(m, "nu");
  std::vector<double> Bm((size_t)n_frames*ndx*nu);
  fb_fd_config cfg = {1e-6, 0, 1, n_frames, nullptr, 0};
  return fb_batch_transition_fd(b, &cfg, nullptr, Bm.data(), nullptr, nullptr, nullptr, nullptr);
}

// the life cycle; full: what an FP64 batch of one model allows (IK, inverse dynamics, derivatives), law: a batch of one model
static int lifecycle(fb_batch* b, const fb_model* m, const Inputs& in, bool full, bool law) {
  const int nv = fb_model_dim(m, "nv"), nbody = fb_model_dim(m, "nbody");
  OK(set_reference(b, in)); OK(fb_batch_reset(b, nullptr, 0, nullptr)); OK(fb_batch_step(b, in.action.data(), nullptr));
  OK(fb_batch_set(b, FB_XFRC_APPLIED, in.zeros.data(), (size_t)N*6*nbody*sizeof(double)));
  REQUIRE(fb_batch_forces_active(b) == 1);
  if (law) {
    OK(set_law(b, in, 1)); OK(set_law(b, in, N)); OK(set_law(b, in, N)); REQUIRE(fb_batch_control_law_active(b) == 1);
    OK(fb_batch_step(b, in.action.data(), nullptr));
    OK(fb_batch_set_control_law(b, nullptr)); REQUIRE(fb_batch_control_law_active(b) == 0 && fb_batch_forces_active(b) == 1);
  }
  if (full) { OK(ik(b, in, 1)); OK(ik(b, in, 3)); OK(fb_batch_inverse(b, 0, nullptr)); }
  OK(fb_batch_clear_forces(b)); REQUIRE(fb_batch_forces_active(b) == 0);
  if (law) {                                          // a law on a batch without forces brings its own, and takes them along when it goes
    OK(set_law(b, in, 1)); REQUIRE(fb_batch_forces_active(b) == 1);
    OK(fb_batch_set_control_law(b, nullptr)); REQUIRE(fb_batch_forces_active(b) == 0);
  }
  if (full) { OK(transition_fd(b, m, 1)); OK(transition_fd(b, m, 3)); int64_t t = 0; OK(fb_batch_fd_tickets(b, &t)); }
  if (law) OK(fb_batch_stage(b, 32, in.action.data(), nullptr));
  OK(fb_batch_timing_begin(b, nullptr)); OK(fb_batch_step(b, in.action.data(), nullptr));
  float ms = 0; int nl = 0;
  OK(fb_batch_timing_end(b, nullptr, &ms, &nl)); REQUIRE(nl == 1);
  OK(set_reference(b, in));                          // a second reference replaces the first
  std::vector<double> q((size_t)N*fb_model_dim(m, "nq"));
  OK(fb_batch_get(b, FB_QPOS, q.data(), q.size()*sizeof(double)));
  (void)nv;
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s MODEL_BLOB\n", argv[0]); return 2; }
  std::vector<char> blob;
  { FILE* f = fopen(argv[1], "rb"); if (!f) { perror(argv[1]); return 2; }
    char buf[65536]; size_t n; while ((n = fread(buf, 1, sizeof(buf), f)) > 0) blob.insert(blob.end(), buf, buf + n); fclose(f); }
  fb_model *m = nullptr, *m2 = nullptr;
  OK(fb_model_load(blob.data(), blob.size(), &m)); OK(fb_model_load(blob.data(), blob.size(), &m2));
  const int nv = fb_model_dim(m, "nv"), nbody = fb_model_dim(m, "nbody"), nact = fb_model_dim(m, "nact");
  Inputs in;
  in.ref_qpos.assign(8*7, 0.0); in.ref_qvel.assign(8*6, 0.0);
  for (int t = 0; t < 8; t++) { in.ref_qpos[7*t] = 0.01*t; in.ref_qpos[7*t + 2] = 0.13; in.ref_qpos[7*t + 3] = 1.0; }
  in.zeros.assign((size_t)N*std::max(6*nbody, nv), 0.0); in.law_rows.assign((size_t)N*nv, 1e-6); in.target.assign((size_t)N*3*3, 0.1);
  in.action.assign((size_t)N*nact, 0.25f); in.sites = {0, 1, 2}; in.include.assign(9, 1);
  const int base_allocs = fb_emu_live_allocs(), base_events = fb_emu_live_events();
  auto clean = [&]() { return fb_emu_live_allocs() == base_allocs && fb_emu_live_events() == base_events; };

  // ---- the life cycle: FP64, FP32, a group of two models
  fb_batch* b = nullptr;
  OK(fb_batch_create(m, N, 0, 64, &b)); if (lifecycle(b, m, in, true, true)) return 1;
  REQUIRE(fb_emu_live_allocs() > base_allocs + 20 && fb_emu_live_events() >= base_events + 4);
  fb_batch_destroy(b); REQUIRE(clean());
  OK(fb_batch_create(m, N, 0, 32, &b)); if (lifecycle(b, m, in, false, true)) return 1;
  fb_batch_destroy(b); REQUIRE(clean());
  const fb_model* group[2] = {m, m2};
  OK(fb_batch_create_group(group, 2, N, 0, 64, &b)); if (lifecycle(b, m, in, false, false)) return 1;
  fb_batch_destroy(b); REQUIRE(clean());

  // ---- every allocation of fb_batch_create fails in turn
  int failed = 0;
  for (int k = 0; k < 500; k++) {
    fb_emu_fail_alloc(k);
    const int rc = fb_batch_create(m, N, 0, 64, &b);
    fb_emu_fail_alloc(-1);
    if (rc == 0) break;
    REQUIRE(b == nullptr && fb_last_error()[0] && clean());
    failed++;
  }
  REQUIRE(b != nullptr && failed >= 20);

  // ---- one failed allocation per entry point on the live batch; the same call then succeeds
  OK(set_reference(b, in)); OK(fb_batch_reset(b, nullptr, 0, nullptr));
  FAILS(set_law(b, in, 1)); REQUIRE(fb_batch_control_law_active(b) == 0 && fb_batch_forces_active(b) == 0);
  OK(set_law(b, in, 1));
  FAILS(set_law(b, in, N)); REQUIRE(fb_batch_control_law_active(b) == 1);       // (the law of one row stays)
  OK(set_law(b, in, N)); OK(fb_batch_set_control_law(b, nullptr)); REQUIRE(fb_batch_forces_active(b) == 0);
  FAILS(fb_batch_set(b, FB_QFRC_APPLIED, in.zeros.data(), (size_t)N*nv*sizeof(double))); REQUIRE(fb_batch_forces_active(b) == 0);
  OK(fb_batch_set(b, FB_QFRC_APPLIED, in.zeros.data(), (size_t)N*nv*sizeof(double))); OK(fb_batch_clear_forces(b));
  FAILS(ik(b, in, 2)); OK(ik(b, in, 2)); FAILS(ik(b, in, 3)); OK(ik(b, in, 3));
  FAILS(fb_batch_inverse(b, 0, nullptr)); OK(fb_batch_inverse(b, 0, nullptr));
  FAILS(transition_fd(b, m, 1)); OK(transition_fd(b, m, 1)); FAILS(transition_fd(b, m, 2)); OK(transition_fd(b, m, 2));
  FAILS(fb_batch_stage(b, 32, in.action.data(), nullptr)); OK(fb_batch_stage(b, 32, in.action.data(), nullptr));
  FAILS(set_reference(b, in));
  REQUIRE(fb_batch_step(b, in.action.data(), nullptr) != 0 && strstr(fb_last_error(), "call fb_batch_set_reference first"));
  OK(set_reference(b, in)); OK(fb_batch_reset(b, nullptr, 0, nullptr)); OK(fb_batch_step(b, in.action.data(), nullptr));
  fb_batch_destroy(b); REQUIRE(clean());
  fb_model_destroy(m); fb_model_destroy(m2);
  printf("host lifecycle ok\n");
  return 0;
}
