// The host-side plan of the pose prior (pose_prior.hip; include/banet_hip.h (5f)): the struct checks, whether a prior is empty,
// which levels the term exists on, and the one launch's grid.  The term needs no workspace and no once-per-level pass: it touches
// the m x m pose block of AtA and Atb[0:m] only (m = 6 max(pairs, 1)), between launch_assemble and launch_solve.  Host-only, plain
// C++17 (no HIP include), in the manner of prior_plan.hpp: tests/native/pose_prior_plan_host.cpp compiles this header with g++.
#pragma once
#include <cmath>

#include "plan.hpp"

namespace banet {

constexpr int kPosePriorThreads = 256;   // ba_pose_prior_add_kernel: one workgroup of 4 waves per window, whatever the shape
constexpr int kPosePriorPairsMax = 8;    // target frames per window: m <= 48 (Lambda, Lambda Jr and the Jr blocks live in LDS)

struct PosePriorPlan {
  int on;          // 0: the empty prior -- nothing is launched
  int pairs, m;    // m = 6 pairs: the pose block
  int K, P;        // P = m + K: the row stride of AtA
  int grid;        // workgroups: one per window
};

namespace plan_detail {

// some but not all of the three pointers, a bad scale, reserved_ != 0: BANET_ERR_INVALID_ARG whatever else holds
inline int pose_prior_struct_ok(const banet_pose_prior_t* pp) {
  if (!pp) return BANET_OK;
  const int given = (pp->R0 != nullptr) + (pp->T0 != nullptr) + (pp->Lambda != nullptr);
  if (given != 0 && given != 3) return BANET_ERR_INVALID_ARG;
  if (!(pp->scale >= 0.f) || std::isinf(pp->scale)) return BANET_ERR_INVALID_ARG;   // (NaN fails the comparison)
  if (pp->reserved_ != 0) return BANET_ERR_INVALID_ARG;
  return BANET_OK;
}

}  // namespace plan_detail

// pp == NULL, no pointers, or scale == 0 (of a struct that passed pose_prior_struct_ok)
inline bool pose_prior_empty(const banet_pose_prior_t* pp) { return !pp || !pp->Lambda || pp->scale == 0.f; }

// What a call runs.  BANET_OK with on = 0 for the empty prior on any level with B >= 1; BANET_ERR_INVALID_ARG for a struct the
// entries refuse; BANET_ERR_UNSUPPORTED for a level the term does not exist on (a legacy variant, more than kPosePriorPairsMax
// target frames).  Reads lv->B, K, pairs and variant only.
inline int plan_pose_prior(const banet_level_t* lv, const banet_pose_prior_t* pp, PosePriorPlan* pl) {
  *pl = PosePriorPlan{};
  const int rc = plan_detail::pose_prior_struct_ok(pp);
  if (rc != BANET_OK) return rc;
  if (!lv || lv->B < 1) return BANET_ERR_INVALID_ARG;
  if (pose_prior_empty(pp)) return BANET_OK;
  if (lv->K < 0 || lv->pairs < 0) return BANET_ERR_INVALID_ARG;
  const bool bundle = lv->variant == BANET_BUNDLE && lv->K >= 1, camera = lv->variant == BANET_BUNDLE_CAMERA && lv->K == 0;
  if ((!bundle && !camera) || npairs(lv) > kPosePriorPairsMax) return BANET_ERR_UNSUPPORTED;
  pl->on = 1;
  pl->pairs = npairs(lv);
  pl->m = 6 * pl->pairs;
  pl->K = lv->K;
  pl->P = pl->m + lv->K;
  pl->grid = lv->B;
  return BANET_OK;
}

}  // namespace banet
