// host build of the pose prior backward's plan (banet_amd/csrc/pose_prior_grad_plan.hpp) for tests/test_pose_prior_grad_cpu.py:
// the refusals, the grid and the phases per output set, asked of the code itself.  No ROCm needed.
#include "../../banet_amd/csrc/pose_prior_grad_plan.hpp"

#define POSE_PRIOR_GRAD_PLAN_FIELDS(X) X(rc) X(on) X(pairs) X(m) X(K) X(P) X(grid) X(work) X(lanes) X(overwrite_state) X(overwrite_prior)

extern "C" const char* banet_test_pose_prior_grad_plan_fields() {
#define X(f) #f " "
  return "desc_ints=11 " POSE_PRIOR_GRAD_PLAN_FIELDS(X);
#undef X
}

extern "C" int banet_test_pose_prior_grad_threads() { return banet::kPosePriorGradThreads; }
extern "C" int banet_test_pose_prior_grad_entries() { return banet::kPosePriorGradEntries; }
extern "C" int banet_test_pose_prior_grad_work_bit(int i) {
  const int bits[6] = {banet::kPoseGradA, banet::kPoseGradX, banet::kPoseGradXt, banet::kPoseGradLambda, banet::kPoseGradScale, banet::kPoseGradPose};
  return i >= 0 && i < 6 ? bits[i] : 0;
}

// one call per row of `desc`: B, K, pairs, variant, prior (0: pp NULL, 1: complete, 2: no pointers, 3: T0 missing), pp.reserved_,
// outputs (bit 0..5: gR gT gR0 gT0 gLambda gscale), flags, out.reserved_, whether lv is given, whether out is given; scale[i] next to
// it.  out: one row of POSE_PRIOR_GRAD_PLAN_FIELDS
extern "C" void banet_test_pose_prior_grad_plan_sweep(const int64_t* desc, const float* scale, int n, int64_t* out) {
  static const float dummy[1] = {0.f};
  static float sink[1] = {0.f};
  for (int i = 0; i < n; ++i, desc += 11) {
    banet_level_t lv = {};
    lv.B = (int)desc[0], lv.K = (int)desc[1], lv.pairs = (int)desc[2], lv.variant = (int)desc[3];
    banet_pose_prior_t pp = {};
    if (desc[4] == 1 || desc[4] == 3) pp.R0 = dummy, pp.Lambda = dummy;
    if (desc[4] == 1) pp.T0 = dummy;
    pp.reserved_ = (int32_t)desc[5];
    pp.scale = scale[i];
    banet_pose_prior_grad_t o = {};
    o.gR = (desc[6] & 1) ? sink : nullptr;
    o.gT = (desc[6] & 2) ? sink : nullptr;
    o.gR0 = (desc[6] & 4) ? sink : nullptr;
    o.gT0 = (desc[6] & 8) ? sink : nullptr;
    o.gLambda = (desc[6] & 16) ? sink : nullptr;
    o.gscale = (desc[6] & 32) ? sink : nullptr;
    o.flags = (int32_t)desc[7];
    o.reserved_ = (int32_t)desc[8];
    struct : banet::PosePriorGradPlan { int rc; } p;
    p.rc = banet::plan_pose_prior_grad(desc[9] ? &lv : nullptr, desc[4] ? &pp : nullptr, desc[10] ? &o : nullptr, &p);
#define X(f) *out++ = (int64_t)p.f;
    POSE_PRIOR_GRAD_PLAN_FIELDS(X)
#undef X
  }
}
