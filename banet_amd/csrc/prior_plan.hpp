// The host-side plan of the depth-observation / coefficient-prior term (prior.hip; include/banet_hip.h (5d)): which halves a prior
// has, whether it is empty, and where its regions lie in the workspace -- behind `base` bytes of somebody else's layout (the LM
// level's carve, or 0 for banet_prior_apply_f32 alone).  Also the partial-row geometry of the Gram pass (basisfit.hip), which the
// observation half runs and whose rows are the largest region.  Host-only, plain C++17 (no HIP include), in the manner of
// adjoint_plan.hpp: tests/native/prior_plan_host.cpp compiles this header with g++ (tests/test_prior_cpu.py pins the offsets).
#pragma once
#include <cmath>

#include "plan.hpp"

namespace banet {

constexpr int kPriorKMax = 256;           // the Gram pass's limit (kFitKMax)
constexpr int kPriorThreads = 256;        // ba_prior_add_kernel / prior_combine_kernel: 4 waves
constexpr int kFitRowsMax = 64;           // Gram pass: partial rows per window at most
constexpr int kFitRowPixels = 256;        // ... and never fewer pixels than this per row

// The Gram pass's summation tree: functions of N and K alone, never of B.
struct FitRows {
  int NR, NP;       // NR 32-column blocks, NP = NR (NR + 1) / 2 lower 32 x 32 blocks of G
  int chunk, rows;  // pixels per partial row, partial rows per window
  int pstride;      // floats per partial row: the blocks, g, (sum w, sum w r^2) + padding
};

inline FitRows fit_rows(int N, int K) {
  FitRows f;
  f.NR = (K + 31) / 32;
  f.NP = f.NR * (f.NR + 1) / 2;
  int rows = (N + kFitRowPixels - 1) / kFitRowPixels;
  if (rows > kFitRowsMax) rows = kFitRowsMax;
  int chunk = (N + rows - 1) / rows;
  chunk = (chunk + 1) / 2 * 2;                       // whole two-pixel steps
  f.chunk = chunk;
  f.rows = (N + chunk - 1) / chunk;
  f.pstride = f.NP * 1024 + f.NR * 32 + 32;
  return f;
}

struct PriorPlan {
  int on;                     // 0: the empty prior -- nothing is launched, no region exists, bytes == base
  int coef, eta, obs, weight; // which pointers of banet_prior_t are given
  int K, m, P;                // m = 6 max(pairs, 1): first row / column of the depth block; P = m + K: row stride of AtA
  FitRows fit;                // obs: the Gram pass
  int add_grid;               // ba_prior_add_kernel: workgroups (one wave per row of Le, B K rows)
  // Regions, each at a 256-byte boundary behind `base`; every one is written before it is read.  Le / ee live for the call (the
  // level's iterations); part / G / g only until the combine launch.
  size_t off_Le, off_ee;            // [B][K][K], [B][K]
  size_t off_part, off_G, off_g;    // obs only: the Gram pass's partial rows [B][rows][pstride], G [B][K][K], g [B][K]
  size_t bytes;                     // base + the regions
};

namespace plan_detail {

// eta without Lambda, obs_weight without obs_depth, a bad scale, reserved_ != 0: BANET_ERR_INVALID_ARG whatever else holds
inline int prior_struct_ok(const banet_prior_t* pr) {
  if (!pr) return BANET_OK;
  if (pr->eta && !pr->Lambda) return BANET_ERR_INVALID_ARG;
  if (pr->obs_weight && !pr->obs_depth) return BANET_ERR_INVALID_ARG;
  if (!(pr->scale >= 0.f) || std::isinf(pr->scale)) return BANET_ERR_INVALID_ARG;   // (NaN fails the comparison)
  if (pr->reserved_ != 0) return BANET_ERR_INVALID_ARG;
  return BANET_OK;
}

}  // namespace plan_detail

// The layout of a prior's regions from its pointers and the level's shape alone -- what the queries report (the scale is not
// read: a caller sizes one workspace for every scale).  BANET_OK with on = 0 for a prior without pointers; BANET_ERR_INVALID_ARG
// for a pointer combination the entries refuse; BANET_ERR_UNSUPPORTED for a level the term does not exist on.
inline int plan_prior_layout(const banet_level_t* lv, const banet_prior_t* pr, size_t base, PriorPlan* pl) {
  *pl = PriorPlan{};
  pl->bytes = base;
  if (!lv || lv->B < 1) return BANET_ERR_INVALID_ARG;
  if (!pr || (!pr->Lambda && !pr->eta && !pr->obs_depth && !pr->obs_weight)) return BANET_OK;
  if ((pr->eta && !pr->Lambda) || (pr->obs_weight && !pr->obs_depth)) return BANET_ERR_INVALID_ARG;
  if (lv->variant != BANET_BUNDLE || lv->K < 1 || lv->K > kPriorKMax || lv->pairs < 0) return BANET_ERR_UNSUPPORTED;
  if (pr->obs_depth && lv->N < 1) return BANET_ERR_UNSUPPORTED;
  const size_t B = lv->B, K = lv->K;
  pl->on = 1;
  pl->coef = pr->Lambda != nullptr;
  pl->eta = pr->eta != nullptr;
  pl->obs = pr->obs_depth != nullptr;
  pl->weight = pr->obs_weight != nullptr;
  pl->K = lv->K;
  pl->m = 6 * npairs(lv);
  pl->P = pl->m + lv->K;
  pl->add_grid = (int)((B * K + kPriorThreads / kWave - 1) / (kPriorThreads / kWave));
  Arena ar;
  ar.off = align_up(base, 256);
  pl->off_Le = ar.take(B * K * K * sizeof(float));
  pl->off_ee = ar.take(B * K * sizeof(float));
  if (pl->obs) {
    pl->fit = fit_rows(lv->N, lv->K);
    pl->off_part = ar.take(B * pl->fit.rows * pl->fit.pstride * sizeof(float));
    pl->off_G = ar.take(B * K * K * sizeof(float));
    pl->off_g = ar.take(B * K * sizeof(float));
  }
  pl->bytes = ar.off;
  return BANET_OK;
}

// What a call runs: the layout above, the struct checks, and the empty prior by its scale as well (on = 0, bytes = base).
inline int plan_prior(const banet_level_t* lv, const banet_prior_t* pr, size_t base, PriorPlan* pl) {
  *pl = PriorPlan{};
  pl->bytes = base;
  int rc = plan_detail::prior_struct_ok(pr);
  if (rc != BANET_OK) return rc;
  if (!pr || pr->scale == 0.f) return (lv && lv->B >= 1) ? BANET_OK : BANET_ERR_INVALID_ARG;
  rc = plan_prior_layout(lv, pr, base, pl);
  if (rc != BANET_OK) {
    *pl = PriorPlan{};
    pl->bytes = base;
  }
  return rc;
}

}  // namespace banet
