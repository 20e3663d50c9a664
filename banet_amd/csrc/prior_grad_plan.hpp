// The host-side plan of the prior term's backward (prior_grad.hip; include/banet_hip.h (5e)): which outputs a call forms, whether
// the per-pixel kernel runs, its LDS image and grid, and where Gh / gh lie in the workspace.  Host-only, plain C++17 (no HIP
// include), in the manner of prior_plan.hpp, whose structs stay as they are: tests/native/prior_grad_plan_host.cpp compiles this
// header with g++ (tests/test_prior_grad_cpu.py pins the offsets).
#pragma once
#include "prior_plan.hpp"

namespace banet {

// prior_grad_pixel_kernel: 32 pixels per wave and step; 8 waves up to K = 128 (NR <= 4), 4 waves above
constexpr int prior_grad_threads(int NR) { return NR <= 4 ? 512 : 256; }
constexpr int kPriorPrepThreads = 1024;       // prior_grad_prep_kernel: one workgroup per window
constexpr int kPriorGradFlags = BANET_PRIOR_GRAD_OVERWRITE | BANET_PRIOR_GRAD_ACCUMULATE;

struct PriorGradPlan {
  int on;                     // 0: the empty prior (the call refuses it; the query reports 0)
  int coef, eta, obs, weight; // which pointers of banet_prior_t are given
  int K, m, P;                // as PriorPlan
  int NR, NP;                 // 32-column blocks of Gh, lower 32 x 32 blocks kept in LDS
  int pixel;                  // the per-pixel kernel runs: observations and one of gobs / gweight / gdepth / gbasis
  int tiles, grid;            // 32-pixel tiles per window, workgroups per window (2 CUs / B, capped by the tile count)
  size_t lds;                 // its dynamic LDS: NP 4 KB blocks + gh padded to NR 32 floats
  int add_grid;               // prior_add_grad_kernel: workgroups (one wave per row of Le, B K rows)
  size_t off_Gh, off_gh;      // [B][K][K], [B][K]: each at a 256-byte boundary
  size_t bytes;
};

// The shape checks every entry of (5e) shares (the level's, not the prior's): BANET_OK / _INVALID_ARG / _UNSUPPORTED
inline int prior_grad_level_ok(const banet_level_t* lv) {
  if (!lv || lv->B < 1) return BANET_ERR_INVALID_ARG;
  if (lv->variant != BANET_BUNDLE || lv->K < 1 || lv->K > kPriorKMax || lv->pairs < 0) return BANET_ERR_UNSUPPORTED;
  return BANET_OK;
}

// banet_prior_add_grad_f32: the level alone decides
inline int plan_prior_add_grad(const banet_level_t* lv, int flags, PriorGradPlan* pl) {
  *pl = PriorGradPlan{};
  const int rc = prior_grad_level_ok(lv);
  if (rc != BANET_OK) return rc;
  if (flags & ~BANET_PRIOR_GRAD_OVERWRITE) return BANET_ERR_INVALID_ARG;
  pl->on = 1;
  pl->K = lv->K;
  pl->m = 6 * npairs(lv);
  pl->P = pl->m + lv->K;
  pl->add_grid = (int)(((size_t)lv->B * lv->K + kPriorThreads / kWave - 1) / (kPriorThreads / kWave));
  return BANET_OK;
}

// The layout from the prior's pointers and the level's shape alone -- what the query reports (num_cus: the device's, for the grid)
inline int plan_prior_grad_layout(const banet_level_t* lv, const banet_prior_t* pr, int num_cus, PriorGradPlan* pl) {
  *pl = PriorGradPlan{};
  PriorPlan pp;
  const int rc = plan_prior_layout(lv, pr, 0, &pp);
  if (rc != BANET_OK || !pp.on) return rc;
  const size_t B = lv->B, K = lv->K;
  pl->on = 1;
  pl->coef = pp.coef, pl->eta = pp.eta, pl->obs = pp.obs, pl->weight = pp.weight;
  pl->K = pp.K, pl->m = pp.m, pl->P = pp.P;
  pl->NR = (lv->K + 31) / 32;
  pl->NP = pl->NR * (pl->NR + 1) / 2;
  pl->lds = ((size_t)pl->NP * 1024 + (size_t)pl->NR * 32) * sizeof(float);
  pl->add_grid = pp.add_grid;
  if (pl->obs) {
    pl->tiles = (lv->N + 31) / 32;
    int G = (int)((2 * (size_t)num_cus + B - 1) / B);
    const int waves = prior_grad_threads(pl->NR) / kWave;
    const int steps = (pl->tiles + waves - 1) / waves;
    if (G > steps) G = steps;
    if (G < 1) G = 1;
    pl->grid = G;
  }
  Arena ar;
  pl->off_Gh = ar.take(B * K * K * sizeof(float));
  pl->off_gh = ar.take(B * K * sizeof(float));
  pl->bytes = ar.off;
  return BANET_OK;
}

// What banet_prior_terms_grad_f32 runs: the layout, the struct checks of (5d), and which outputs the prior allows
inline int plan_prior_terms_grad(const banet_level_t* lv, const banet_prior_t* pr, const banet_prior_grad_in_t* in,
                                 const banet_prior_grad_out_t* out, int num_cus, PriorGradPlan* pl) {
  *pl = PriorGradPlan{};
  if (!lv || !pr || !in || !out) return BANET_ERR_INVALID_ARG;
  int rc = plan_detail::prior_struct_ok(pr);
  if (rc != BANET_OK) return rc;
  if (pr->scale == 0.f) return BANET_ERR_INVALID_ARG;                     // the empty prior has no backward
  rc = plan_prior_grad_layout(lv, pr, num_cus, pl);
  if (rc != BANET_OK) {
    *pl = PriorGradPlan{};
    return rc;
  }
  if (!pl->on) return BANET_ERR_INVALID_ARG;
  if ((in->flags & ~BANET_PRIOR_GRAD_ACCUMULATE) || in->reserved_ != 0 || !in->gLe || !in->gee) return BANET_ERR_INVALID_ARG;
  if (!out->gLambda && !out->geta && !out->gscale && !out->gobs && !out->gweight && !out->gdepth && !out->gbasis) return BANET_ERR_INVALID_ARG;
  if ((out->gLambda && !pl->coef) || (out->geta && !pl->eta) || (out->gweight && !pl->weight)) return BANET_ERR_INVALID_ARG;
  if ((out->gobs || out->gdepth || out->gbasis) && !pl->obs) return BANET_ERR_INVALID_ARG;
  if (out->gscale && (!in->Le || !in->ee)) return BANET_ERR_INVALID_ARG;
  pl->pixel = pl->obs && (out->gobs || out->gweight || out->gdepth || out->gbasis);
  if (pl->pixel && (!lv->depth || !lv->basis)) return BANET_ERR_INVALID_ARG;
  return BANET_OK;
}

}  // namespace banet
