// host build of the prior term's plan (banet_amd/csrc/prior_plan.hpp) for tests/test_prior_cpu.py: where its regions lie, asked of
// the code itself.  No ROCm needed.
#include "../../banet_amd/csrc/prior_plan.hpp"

#define PRIOR_PLAN_FIELDS(X)                                                                                                  \
  X(rc) X(on) X(coef) X(eta) X(obs) X(weight) X(K) X(m) X(P) X(add_grid) X(fit.NR) X(fit.NP) X(fit.chunk) X(fit.rows) X(fit.pstride) \
  X(off_Le) X(off_ee) X(off_part) X(off_G) X(off_g) X(bytes)

extern "C" const char* banet_test_prior_plan_fields() {
#define X(f) #f " "
  return "desc_ints=12 " PRIOR_PLAN_FIELDS(X);
#undef X
}

// one prior per row of `desc`: B, N, K, pairs, variant, has Lambda, has eta, has obs_depth, has obs_weight, reserved_, base (bytes), and
// which plan (0: plan_prior_layout, the queries; 1: plan_prior, the calls); scale[i] next to it.  out: one row of PRIOR_PLAN_FIELDS
extern "C" void banet_test_prior_plan_sweep(const int64_t* desc, const float* scale, int n, int64_t* out) {
  static const float dummy[1] = {0.f};
  for (int i = 0; i < n; ++i, desc += 12) {
    banet_level_t lv = {};
    lv.B = (int)desc[0], lv.N = (int)desc[1], lv.K = (int)desc[2], lv.pairs = (int)desc[3], lv.variant = (int)desc[4];
    banet_prior_t pr = {};
    pr.Lambda = desc[5] ? dummy : nullptr;
    pr.eta = desc[6] ? dummy : nullptr;
    pr.obs_depth = desc[7] ? dummy : nullptr;
    pr.obs_weight = desc[8] ? dummy : nullptr;
    pr.reserved_ = (int32_t)desc[9];
    pr.scale = scale[i];
    struct : banet::PriorPlan { int rc; } p;
    p.rc = desc[11] ? banet::plan_prior(&lv, &pr, (size_t)desc[10], &p) : banet::plan_prior_layout(&lv, &pr, (size_t)desc[10], &p);
#define X(f) *out++ = (int64_t)p.f;
    PRIOR_PLAN_FIELDS(X)
#undef X
  }
}
