// host build of the pose prior's plan (banet_amd/csrc/pose_prior_plan.hpp) for tests/test_pose_prior_cpu.py: the struct checks, the
// empty test, the refusals and the grid, asked of the code itself.  No ROCm needed.
#include "../../banet_amd/csrc/pose_prior_plan.hpp"

#define POSE_PRIOR_PLAN_FIELDS(X) X(rc) X(on) X(pairs) X(m) X(K) X(P) X(grid)

extern "C" const char* banet_test_pose_prior_plan_fields() {
#define X(f) #f " "
  return "desc_ints=9 threads=256 pairs_max=8 " POSE_PRIOR_PLAN_FIELDS(X);
#undef X
}

extern "C" int banet_test_pose_prior_threads() { return banet::kPosePriorThreads; }
extern "C" int banet_test_pose_prior_pairs_max() { return banet::kPosePriorPairsMax; }

// one pose prior per row of `desc`: B, K, pairs, variant, has R0, has T0, has Lambda, reserved_, and whether pp is given at all;
// scale[i] next to it.  out: one row of POSE_PRIOR_PLAN_FIELDS
extern "C" void banet_test_pose_prior_plan_sweep(const int64_t* desc, const float* scale, int n, int64_t* out) {
  static const float dummy[1] = {0.f};
  for (int i = 0; i < n; ++i, desc += 9) {
    banet_level_t lv = {};
    lv.B = (int)desc[0], lv.K = (int)desc[1], lv.pairs = (int)desc[2], lv.variant = (int)desc[3];
    banet_pose_prior_t pp = {};
    pp.R0 = desc[4] ? dummy : nullptr;
    pp.T0 = desc[5] ? dummy : nullptr;
    pp.Lambda = desc[6] ? dummy : nullptr;
    pp.reserved_ = (int32_t)desc[7];
    pp.scale = scale[i];
    struct : banet::PosePriorPlan { int rc; } p;
    p.rc = banet::plan_pose_prior(&lv, desc[8] ? &pp : nullptr, &p);
#define X(f) *out++ = (int64_t)p.f;
    POSE_PRIOR_PLAN_FIELDS(X)
#undef X
  }
}
