// The host-side plan of the pose prior's backward (pose_prior_grad.hip; include/banet_hip.h (5g)): the checks of the one entry, the
// launch's grid, and which intermediates and phases a set of outputs needs.  No workspace.  Host-only, plain C++17 (no HIP include),
// in the manner of pose_prior_plan.hpp, whose struct stays as it is: tests/native/pose_prior_grad_plan_host.cpp compiles this header
// with g++.
#pragma once
#include "pose_prior_plan.hpp"

namespace banet {

constexpr int kPosePriorGradThreads = 256;   // ba_pose_prior_grad_kernel: one workgroup of 4 waves per window, whatever the shape
constexpr int kPosePriorGradEntries = 24;    // input entries of one pose: R 9, T 3, R0 9, T0 3 -- one lane of phase 3 each
constexpr int kPosePriorGradFlags = BANET_POSE_PRIOR_GRAD_OVERWRITE_STATE | BANET_POSE_PRIOR_GRAD_OVERWRITE_PRIOR;

// what the kernel forms (PosePriorGradPlan::work); y = Jr g is always formed
enum {
  kPoseGradA = 1,        // A = Jr G                              gLambda, gscale
  kPoseGradX = 2,        // X = Lambda Jr and u = Lambda r        gscale, the pose outputs
  kPoseGradXt = 4,       // Xt = Lambda^T Jr                      the pose outputs
  kPoseGradLambda = 8,   // phase 2: gLambda
  kPoseGradScale = 16,   // phase 2: gscale (float64 chains, fixed tree)
  kPoseGradPose = 32,    // phase 2: gr, gJr; phase 3: the tangents and gR / gT / gR0 / gT0
};

struct PosePriorGradPlan {
  int on;          // 1: the launch runs (the entry refuses everything else)
  int pairs, m;    // m = 6 pairs: the pose block
  int K, P;        // P = m + K: the row stride of gAtA
  int grid;        // workgroups: one per window
  int work;        // kPoseGrad* bits
  int lanes;       // phase 3: 24 pairs <= 192 lanes, one per (pose, input entry)
  int overwrite_state, overwrite_prior;
};

// What banet_pose_prior_add_grad_f32 runs.  BANET_ERR_INVALID_ARG, before anything else: a NULL level / pp / out, a struct (5f)
// refuses, the empty prior (it has no backward), an unknown flag bit, reserved_ != 0, no output at all.  BANET_ERR_UNSUPPORTED: a
// level the forward refuses.  Reads lv->B, K, pairs and variant only.  (R / T / gAtA / gAtb are the entry's to check.)
inline int plan_pose_prior_grad(const banet_level_t* lv, const banet_pose_prior_t* pp, const banet_pose_prior_grad_t* out,
                                PosePriorGradPlan* pl) {
  *pl = PosePriorGradPlan{};
  if (!lv || !pp || !out) return BANET_ERR_INVALID_ARG;
  if ((out->flags & ~kPosePriorGradFlags) || out->reserved_ != 0) return BANET_ERR_INVALID_ARG;
  const bool pose = out->gR || out->gT || out->gR0 || out->gT0;
  if (!pose && !out->gLambda && !out->gscale) return BANET_ERR_INVALID_ARG;
  PosePriorPlan fw;
  const int rc = plan_pose_prior(lv, pp, &fw);
  if (rc != BANET_OK) return rc;
  if (!fw.on) return BANET_ERR_INVALID_ARG;   // the empty prior
  pl->on = 1;
  pl->pairs = fw.pairs, pl->m = fw.m, pl->K = fw.K, pl->P = fw.P;
  pl->grid = fw.grid;
  pl->lanes = kPosePriorGradEntries * fw.pairs;
  int w = 0;
  if (out->gLambda) w |= kPoseGradLambda | kPoseGradA;
  if (out->gscale) w |= kPoseGradScale | kPoseGradA | kPoseGradX;
  if (pose) w |= kPoseGradPose | kPoseGradX | kPoseGradXt;
  pl->work = w;
  pl->overwrite_state = (out->flags & BANET_POSE_PRIOR_GRAD_OVERWRITE_STATE) != 0;
  pl->overwrite_prior = (out->flags & BANET_POSE_PRIOR_GRAD_OVERWRITE_PRIOR) != 0;
  return BANET_OK;
}

}  // namespace banet
