// banet_lm_solve_f32: the whole coarse -> fine schedule in one call (include/banet_hip.h (5c); the reference's level loop,
// bundlenet.py:376-399 / legacy/ba.py:106-145).  Every level is validated and planned on the host first (lm_level_plan, api.hip);
// then the levels are enqueued one after another on the caller's stream (lm_level_enqueue: the launches of banet_lm_level_ex_f32),
// each followed by one trace launch.  No allocation, no synchronisation, one stream.  banet_lm_solve_prior_f32 is the same loop with
// a prior per level (lm_level_prior_plan; header (5d)), banet_lm_solve_pose_prior_f32 with a pose prior per level as well
// (lm_level_pose_prior_plan; header (5f)).
#include "kernels.hpp"

namespace banet {

constexpr int kMaxLevels = 16;

// One workgroup per window: the window's state after a level -> row l of the trace.  Plain loads and stores; every destination
// (and Wc / its source for K == 0) may be nullptr.
__global__ __launch_bounds__(64) void lm_trace_kernel(TraceRow r, int B) {
  const int b = blockIdx.x, tid = threadIdx.x;
  if (b >= B) return;
  if (r.to.R)
    for (int i = tid; i < r.nR; i += 64) r.to.R[(size_t)b * r.nR + i] = r.from.R[(size_t)b * r.nR + i];
  if (r.to.T)
    for (int i = tid; i < r.nT; i += 64) r.to.T[(size_t)b * r.nT + i] = r.from.T[(size_t)b * r.nT + i];
  if (r.to.Wc)
    for (int i = tid; i < r.K; i += 64) r.to.Wc[(size_t)b * r.K + i] = r.from.Wc[(size_t)b * r.K + i];
  if (r.to.delta)
    for (int i = tid; i < r.P; i += 64) r.to.delta[(size_t)b * r.P + i] = r.from.delta[(size_t)b * r.P + i];
  if (tid == 0) {
    if (r.to.lambda_out) r.to.lambda_out[b] = r.from.lambda_out[b];
    if (r.to.ratio) r.to.ratio[b] = r.from.ratio[b];
    if (r.to.iters) r.to.iters[b] = r.from.iters[b];
  }
}

void launch_lm_trace(const TraceRow& row, int B, hipStream_t s) {
  hipLaunchKernelGGL(lm_trace_kernel, dim3(B), dim3(64), 0, s, row, B);
}

// the fields every level of a schedule shares: they fix the state's layout and the batch every selection is taken from
static bool same_problem(const banet_level_t& a, const banet_level_t& b) {
  return a.B == b.B && a.K == b.K && npairs(&a) == npairs(&b) && a.variant == b.variant && a.policy == b.policy;
}

static bool schedule_shape_ok(const banet_schedule_t* s) {
  return s && s->levels && s->n_levels >= 1 && s->n_levels <= kMaxLevels;
}

static TraceRow trace_row(const banet_solve_trace_t* tr, const banet_level_t* lv, const banet_state_t* st, int l) {
  TraceRow r;
  const size_t B = (size_t)lv->B, row = (size_t)l * B;
  r.nR = 9 * npairs(lv);
  r.nT = 3 * npairs(lv);
  r.K = lv->K;
  r.P = 6 * npairs(lv) + lv->K;
  r.from = *st;
  r.to.R = tr->R ? tr->R + row * r.nR : nullptr;
  r.to.T = tr->T ? tr->T + row * r.nT : nullptr;
  r.to.Wc = (tr->Wc && lv->K > 0) ? tr->Wc + row * r.K : nullptr;
  r.to.iters = tr->iters ? tr->iters + row : nullptr;
  r.to.ratio = tr->ratio ? tr->ratio + row : nullptr;
  r.to.lambda_out = tr->lambda_out ? tr->lambda_out + row : nullptr;
  r.to.delta = tr->delta ? tr->delta + row * r.P : nullptr;
  return r;
}

// banet_lm_solve_f32 (with_priors = false: lm_level_plan, early termination allowed) and banet_lm_solve_prior_f32 (with_priors:
// lm_level_pose_prior_plan with priors[l] and pose_priors[l], or none where the array is nullptr)
static int lm_solve_run(const banet_schedule_t* s, bool with_priors, const banet_prior_t* priors, const banet_pose_prior_t* pose_priors,
                        banet_state_t* st, banet_stream_t stream) {
  if (!schedule_shape_ok(s) || !s->max_iters) return BANET_ERR_INVALID_ARG;
  if (with_priors && s->early_termination != 0) return BANET_ERR_INVALID_ARG;
  // validate + plan every level; nothing is enqueued before the last one has passed
  LevelRun runs[kMaxLevels];
  for (int l = 0; l < s->n_levels; ++l) {
    const banet_mlp_t* mlp = s->mlps ? s->mlps[l] : nullptr;
    const int rc = with_priors ? lm_level_pose_prior_plan(&s->levels[l], mlp, s->l2_base, s->max_iters[l], s->params, priors ? &priors[l] : nullptr,
                                                          pose_priors ? &pose_priors[l] : nullptr, st, s->workspace, s->workspace_bytes, &runs[l])
                               : lm_level_plan(&s->levels[l], mlp, s->l2_base, s->max_iters[l], s->early_termination, s->params, st,
                                               s->workspace, s->workspace_bytes, &runs[l]);
    if (rc != BANET_OK) return rc;
    if (!same_problem(s->levels[l], s->levels[0])) return BANET_ERR_INVALID_ARG;
  }
  const banet_solve_trace_t* tr = s->trace;
  const banet_level_t* lv0 = &s->levels[0];
  if (tr && tr->depth && (lv0->variant != BANET_BUNDLE || lv0->K <= 0)) return BANET_ERR_INVALID_ARG;
  const bool rows = tr && (tr->R || tr->T || (tr->Wc && lv0->K > 0) || tr->lambda_out || tr->delta || tr->ratio || tr->iters);
  hipStream_t hs = static_cast<hipStream_t>(stream);
  for (int l = 0; l < s->n_levels; ++l) {
    int rc = lm_level_enqueue(runs[l], hs);
    if (rc != BANET_OK) return rc;
    const banet_level_t* lv = &s->levels[l];
    if (rows) {
      launch_lm_trace(trace_row(tr, lv, st, l), lv->B, hs);
      if (hipGetLastError() != hipSuccess) return BANET_ERR_LAUNCH;
    }
    if (tr && tr->depth && tr->depth[l]) {
      rc = launch_depth_output(lv->depth, lv->basis, st->Wc, tr->depth[l], lv->B, lv->N, lv->K, hs);
      if (rc != BANET_OK) return rc;
    }
  }
  return BANET_OK;
}

}  // namespace banet

using namespace banet;

extern "C" {

size_t banet_lm_solve_workspace_bytes(const banet_schedule_t* s) {
  if (!schedule_shape_ok(s)) return 0;
  size_t need = 0;
  for (int l = 0; l < s->n_levels; ++l) {
    const size_t nb = banet_lm_level_workspace_bytes(&s->levels[l]);
    if (nb == 0 || !same_problem(s->levels[l], s->levels[0])) return 0;
    if (nb > need) need = nb;
  }
  return need;
}

int banet_lm_solve_f32(const banet_schedule_t* s, banet_state_t* st, banet_stream_t stream) {
  return lm_solve_run(s, false, nullptr, nullptr, st, stream);
}

size_t banet_lm_solve_prior_workspace_bytes(const banet_schedule_t* s, const banet_prior_t* priors) {
  if (!schedule_shape_ok(s)) return 0;
  size_t need = 0;
  for (int l = 0; l < s->n_levels; ++l) {
    const size_t nb = lm_level_prior_bytes(&s->levels[l], priors ? &priors[l] : nullptr);
    if (nb == 0 || !same_problem(s->levels[l], s->levels[0])) return 0;
    if (nb > need) need = nb;
  }
  return need;
}

int banet_lm_solve_prior_f32(const banet_schedule_t* s, const banet_prior_t* priors, banet_state_t* st, banet_stream_t stream) {
  return lm_solve_run(s, true, priors, nullptr, st, stream);
}

size_t banet_lm_solve_pose_prior_workspace_bytes(const banet_schedule_t* s, const banet_prior_t* priors, const banet_pose_prior_t* pose_priors) {
  if (!schedule_shape_ok(s)) return 0;
  size_t need = 0;
  for (int l = 0; l < s->n_levels; ++l) {
    const size_t nb = lm_level_pose_prior_bytes(&s->levels[l], priors ? &priors[l] : nullptr, pose_priors ? &pose_priors[l] : nullptr);
    if (nb == 0 || !same_problem(s->levels[l], s->levels[0])) return 0;
    if (nb > need) need = nb;
  }
  return need;
}

int banet_lm_solve_pose_prior_f32(const banet_schedule_t* s, const banet_prior_t* priors, const banet_pose_prior_t* pose_priors,
                                  banet_state_t* st, banet_stream_t stream) {
  return lm_solve_run(s, true, priors, pose_priors, st, stream);
}

}  // extern "C"
