// host build of the plan of the prior term's backward (banet_amd/csrc/prior_grad_plan.hpp) for tests/test_prior_grad_cpu.py: its
// regions, LDS image and grid, asked of the code itself.  No ROCm needed.
#include "../../banet_amd/csrc/prior_grad_plan.hpp"

#define PRIOR_GRAD_PLAN_FIELDS(X) \
  X(rc) X(on) X(coef) X(eta) X(obs) X(weight) X(K) X(m) X(P) X(NR) X(NP) X(pixel) X(tiles) X(grid) X(lds) X(add_grid) X(off_Gh) X(off_gh) X(bytes)

extern "C" const char* banet_test_prior_grad_plan_fields() {
#define X(f) #f " "
  return "desc_ints=12 " PRIOR_GRAD_PLAN_FIELDS(X);
#undef X
}

extern "C" int banet_test_prior_grad_threads(int NR) { return banet::prior_grad_threads(NR); }

// one call per row of `desc`: B, N, K, pairs, variant, has Lambda, has eta, has obs_depth, has obs_weight, a bit mask of the
// outputs asked for (gLambda 1, geta 2, gscale 4, gobs 8, gweight 16, gdepth 32, gbasis 64), in->flags, and which plan (0:
// plan_prior_grad_layout, the query; 1: plan_prior_terms_grad, the call; 2: plan_prior_add_grad with flags); scale[i] next to it.
// 256 CUs.  out: one row of PRIOR_GRAD_PLAN_FIELDS
extern "C" void banet_test_prior_grad_plan_sweep(const int64_t* desc, const float* scale, int n, int64_t* out) {
  static float dummy[1] = {0.f};
  for (int i = 0; i < n; ++i, desc += 12) {
    banet_level_t lv = {};
    lv.B = (int)desc[0], lv.N = (int)desc[1], lv.K = (int)desc[2], lv.pairs = (int)desc[3], lv.variant = (int)desc[4];
    lv.depth = lv.basis = dummy;
    banet_prior_t pr = {};
    pr.Lambda = desc[5] ? dummy : nullptr;
    pr.eta = desc[6] ? dummy : nullptr;
    pr.obs_depth = desc[7] ? dummy : nullptr;
    pr.obs_weight = desc[8] ? dummy : nullptr;
    pr.scale = scale[i];
    banet_prior_grad_in_t in = {};
    in.gLe = in.gee = in.Le = in.ee = dummy;
    in.flags = (int32_t)desc[10];
    banet_prior_grad_out_t o = {};
    const int64_t w = desc[9];
    o.gLambda = (w & 1) ? dummy : nullptr;
    o.geta = (w & 2) ? dummy : nullptr;
    o.gscale = (w & 4) ? dummy : nullptr;
    o.gobs = (w & 8) ? dummy : nullptr;
    o.gweight = (w & 16) ? dummy : nullptr;
    o.gdepth = (w & 32) ? dummy : nullptr;
    o.gbasis = (w & 64) ? dummy : nullptr;
    struct : banet::PriorGradPlan { int rc; } p;
    p.rc = desc[11] == 2   ? banet::plan_prior_add_grad(&lv, (int)desc[10], &p)
           : desc[11] == 1 ? banet::plan_prior_terms_grad(&lv, &pr, &in, &o, 256, &p)
                           : banet::plan_prior_grad_layout(&lv, &pr, 256, &p);
#define X(f) *out++ = (int64_t)p.f;
    PRIOR_GRAD_PLAN_FIELDS(X)
#undef X
  }
}
