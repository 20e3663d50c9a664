// C-ABI entry points of libbanet_hip.so (see include/banet_hip.h).  Argument checking,
// workspace carving and kernel enqueue only -- no allocation, no synchronisation.
#include "kernels.hpp"

namespace banet {

static bool aligned256(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 255u) == 0; }

static int check_level(const banet_level_t* lv) {
  if (!lv || !lv->src || !lv->tgt || !lv->depth) return BANET_ERR_INVALID_ARG;
  if (lv->variant < BANET_LEGACY_LM || lv->variant > BANET_BUNDLE) return BANET_ERR_INVALID_ARG;
  if (lv->K > 0 && !lv->basis) return BANET_ERR_INVALID_ARG;
  if ((lv->variant == BANET_BUNDLE) != (lv->K > 0)) return BANET_ERR_INVALID_ARG;
  if (lv->pairs < 0 || (lv->policy != BANET_POLICY_THROUGHPUT && lv->policy != BANET_POLICY_BATCH_INVARIANT)) return BANET_ERR_INVALID_ARG;
  if (lv->pairs > 1 && lv->variant != BANET_BUNDLE && lv->variant != BANET_BUNDLE_CAMERA) return BANET_ERR_INVALID_ARG;
  if (lv->dense) {
    if (!lv->intr || !(lv->scale > 0.f)) return BANET_ERR_INVALID_ARG;
  } else {
    if (!lv->rays || !lv->fx || !lv->fy || !lv->ox || !lv->oy) return BANET_ERR_INVALID_ARG;
  }
  return BANET_OK;
}

// the solve's plan for a level: P = 6 pairs + K unknowns, the level's variant and flags, lm.solver
static int plan_level_solve(const banet_level_t* lv, int solver, SolvePlan* sp) {
  return plan_solve(lv->variant, 6 * npairs(lv) + lv->K, lv->C, solver, lv->flags, sp);
}

// (LevelWs: kernels.hpp)  sp: plan_level_solve's (the matrix of a big solve is the last region)
static LevelWs carve_level(const banet_level_t* lv, const AsmPlan& pl, const SolvePlan& sp, void* ws) {
  LevelWs w;
  char* p = static_cast<char*>(ws);
  Arena ar;
  auto take = [&](size_t bytes) {
    const size_t at = ar.take(bytes);
    return p ? p + at : nullptr;   // (ws == nullptr: the size query)
  };
  w.partials = reinterpret_cast<float*>(take(pl.ws_bytes));
  w.AtA = reinterpret_cast<float*>(take((size_t)lv->B * pl.P * pl.P * sizeof(float)));
  w.Atb = reinterpret_cast<float*>(take((size_t)lv->B * pl.P * sizeof(float)));
  w.absres = reinterpret_cast<float*>(take((size_t)lv->B * lv->C * sizeof(float)));
  w.nvalid = reinterpret_cast<float*>(take((size_t)lv->B * sizeof(float)));
  w.ctl = reinterpret_cast<LmCtl*>(take((size_t)lv->B * sizeof(LmCtl)));
  w.mlp_y = reinterpret_cast<float*>(take((size_t)lv->B * sizeof(float)));
  w.bigA = sp.big ? reinterpret_cast<float*>(take((size_t)lv->B * sp.big_floats * sizeof(float))) : nullptr;
  w.total = ar.off;
  return w;
}

static SolveArgs make_solve_args(const banet_level_t* lv, const banet_mlp_t* mlp, float l2_base, const float* AtA,
                                 const float* Atb, const float* absres, const float* nvalid, const banet_state_t* st) {
  SolveArgs a;
  a.B = lv->B;
  a.N = lv->N;
  a.C = lv->C;
  a.K = lv->K;
  a.pairs = npairs(lv);
  a.P = 6 * a.pairs + lv->K;
  a.variant = lv->variant;
  a.l2_base = l2_base;
  a.max_iters = 0;
  a.use_mlp = lv->variant != BANET_LEGACY_FIXED;
  if (mlp) a.mlp = *mlp;
  else
    for (int i = 0; i < 5; ++i) a.mlp.w[i] = a.mlp.b[i] = nullptr;
  a.AtA = AtA;
  a.Atb = Atb;
  a.absres = absres;
  a.nvalid = nvalid;
  a.st = *st;
  a.ctl = nullptr;
  a.queue = nullptr;
  a.nqueue = 0;
  a.bigA = nullptr;
  a.mlp_y = nullptr;
  banet_lm_params_default(&a.lm);
  a.pl = SolvePlan{};   // (the caller's: plan_level_solve)
  return a;
}

static int check_state(const banet_level_t* lv, const banet_mlp_t* mlp, const banet_state_t* st) {
  if (!st || !st->R || !st->T || !st->iters || !st->ratio || !st->lambda_out || !st->delta) return BANET_ERR_INVALID_ARG;
  if (lv->K > 0 && !st->Wc) return BANET_ERR_INVALID_ARG;
  if (lv->variant != BANET_LEGACY_FIXED) {
    if (!mlp) return BANET_ERR_INVALID_ARG;
    for (int i = 0; i < 5; ++i)
      if (!mlp->w[i] || !mlp->b[i]) return BANET_ERR_INVALID_ARG;
  }
  return BANET_OK;
}


int lm_level_plan(const banet_level_t* lv, const banet_mlp_t* mlp, float l2_base, int max_iters, int early_termination,
                  const banet_lm_params_t* params, const banet_state_t* st, void* ws, size_t ws_bytes, LevelRun* run) {
  int rc = check_level(lv);
  if (rc != BANET_OK) return rc;
  rc = check_state(lv, mlp, st);
  if (rc != BANET_OK) return rc;
  if (max_iters < 0) return BANET_ERR_INVALID_ARG;
  AsmPlan& pl = run->pl;
  rc = plan_assemble(lv, num_cus(), &pl);
  if (rc != BANET_OK) return rc;
  // the solve, planned once per level (an lm.solver that is refused below plans like BANET_SOLVER_QR; the workspace need does
  // not depend on it)
  SolvePlan sp;
  const int solve_rc = plan_level_solve(lv, params ? params->solver : BANET_SOLVER_QR, &sp);
  if (!ws || !aligned256(ws)) return BANET_ERR_WORKSPACE;
  LevelWs& w = run->w;
  w = carve_level(lv, pl, sp, ws);
  if (ws_bytes < w.total) return BANET_ERR_WORKSPACE;
  SolveArgs& a = run->a;
  a = make_solve_args(lv, mlp, l2_base, w.AtA, w.Atb, w.absres, w.nvalid, st);
  a.max_iters = max_iters;
  a.bigA = w.bigA;
  a.pl = sp;
  if (params) {
    if (params->solver != BANET_SOLVER_QR && params->solver != BANET_SOLVER_INVERSE) return BANET_ERR_INVALID_ARG;
    if (!(params->angle_change >= 0.f) || !(params->translation_change >= 0.f) || !(params->residual_ratio > 0.f))
      return BANET_ERR_INVALID_ARG;   // also rejects NaN
    a.lm = *params;
  }
  if (solve_rc != BANET_OK) return solve_rc;   // vectors and scratch alone beyond the LDS (hundreds of target frames)
  run->lv = lv;
  run->mlp = mlp;
  run->prior = PriorRun{};   // (off: lm_level_prior_plan turns it on)
  run->pose = PosePriorRun{};   // (off: lm_level_pose_prior_plan turns it on)
  run->max_iters = max_iters;
  run->lm = early_termination && lv->variant == BANET_LEGACY_LM;
  run->role = SyrkRole{0, pl.s.Gs};
  if (run->lm) {
    a.ctl = w.ctl;
  } else {
    // the tile queue is reset once per level; afterwards every solve kernel leaves it zeroed for the next gather
    a.queue = assemble_queue(pl, w.partials);
    a.nqueue = 8 * npairs(lv);
    // the lambda MLP as a role workgroup of the SYRK launch, off the solve kernel's critical path: plan_syrk_role (plan.hpp)
    run->role = plan_syrk_role(pl.s, lv->variant == BANET_BUNDLE && mlp != nullptr && a.use_mlp, selection_batch(lv), lv->N, lv->C,
                               lv->flags, num_cus());
    if (run->role.on) a.mlp_y = w.mlp_y;
  }
  return BANET_OK;
}

size_t lm_level_prior_bytes(const banet_level_t* lv, const banet_prior_t* pr) {
  AsmPlan apl;
  if (plan_assemble(lv, num_cus(), &apl) != BANET_OK) return 0;
  SolvePlan sp;
  (void)plan_level_solve(lv, BANET_SOLVER_QR, &sp);
  PriorPlan pl;
  if (plan_prior_layout(lv, pr, carve_level(lv, apl, sp, nullptr).total, &pl) != BANET_OK) return 0;
  return pl.bytes;
}

int lm_level_prior_plan(const banet_level_t* lv, const banet_mlp_t* mlp, float l2_base, int max_iters, const banet_lm_params_t* params,
                        const banet_prior_t* pr, const banet_state_t* st, void* ws, size_t ws_bytes, LevelRun* run) {
  int rc = plan_detail::prior_struct_ok(pr);
  if (rc != BANET_OK) return rc;
  rc = lm_level_plan(lv, mlp, l2_base, max_iters, 0, params, st, ws, ws_bytes, run);
  if (rc != BANET_OK) return rc;
  PriorPlan pl;
  rc = plan_prior(lv, pr, run->w.total, &pl);
  if (rc != BANET_OK) return rc;
  if (!pl.on) return BANET_OK;   // the empty prior: banet_lm_level_ex_f32's launches and workspace need
  if (ws_bytes < pl.bytes) return BANET_ERR_WORKSPACE;
  run->prior = make_prior_run(lv, pr, pl, ws);
  return BANET_OK;
}

size_t lm_level_pose_prior_bytes(const banet_level_t* lv, const banet_prior_t* pr, const banet_pose_prior_t* pp) {
  if (pp) {   // what the entry refuses whatever the scale: a partial struct, or a prior with pointers on a level without the term
    banet_pose_prior_t q = *pp;
    q.scale = 1.f;
    q.reserved_ = 0;
    PosePriorPlan pl;
    if (plan_pose_prior(lv, &q, &pl) != BANET_OK) return 0;
  }
  return lm_level_prior_bytes(lv, pr);
}

int lm_level_pose_prior_plan(const banet_level_t* lv, const banet_mlp_t* mlp, float l2_base, int max_iters, const banet_lm_params_t* params,
                             const banet_prior_t* pr, const banet_pose_prior_t* pp, const banet_state_t* st, void* ws, size_t ws_bytes,
                             LevelRun* run) {
  int rc = plan_detail::pose_prior_struct_ok(pp);
  if (rc != BANET_OK) return rc;
  rc = lm_level_prior_plan(lv, mlp, l2_base, max_iters, params, pr, st, ws, ws_bytes, run);
  if (rc != BANET_OK) return rc;
  PosePriorPlan pl;
  rc = plan_pose_prior(lv, pp, &pl);
  if (rc != BANET_OK) return rc;
  if (!pl.on) return BANET_OK;   // the empty pose prior: banet_lm_level_prior_f32's launches
  run->pose.pl = pl;
  run->pose.pp = *pp;
  return BANET_OK;
}

int lm_level_enqueue(const LevelRun& run, hipStream_t s) {
  const banet_level_t* lv = run.lv;
  const AsmPlan& pl = run.pl;
  const LevelWs& w = run.w;
  const SolveArgs& a = run.a;
  const banet_state_t* st = &a.st;
  const int max_iters = run.max_iters;
  int rc;
  if (run.lm) {
    // device-side loop control: max_iters + 1 evaluation rounds; the last one only runs the
    // pending accept/reject test (legacy/ba.py:304-345), see solve.hip
    launch_ctl_init(w.ctl, st->iters, lv->B, s);
    const int stride = (int)(sizeof(LmCtl) / sizeof(int32_t));
    for (int it = 0; it <= max_iters; ++it) {
      rc = launch_assemble(lv, pl, st->R, st->T, st->Wc, &w.ctl->active, stride, w.partials, w.AtA, w.Atb, w.absres,
                           w.nvalid, s);
      if (rc != BANET_OK) return rc;
      {
        RangeScope r("solve", lv->N);
        rc = launch_solve(a, s);
      }
      if (rc != BANET_OK) return rc;
    }
  } else {
    launch_zero_iters(st->iters, lv->B, s);
    if (a.queue) launch_zero_iters(a.queue, lv->B * a.nqueue, s);   // a kernel, not hipMemsetAsync: see prepare_gather
    if (run.prior.pl.on && max_iters > 0) {   // Le, ee: constant over the level's iterations (prior.hip)
      RangeScope r("prior_setup", lv->N);
      rc = launch_prior_setup(lv, run.prior, s);
      if (rc != BANET_OK) return rc;
    }
    for (int it = 0; it < max_iters; ++it) {
      rc = launch_assemble(lv, pl, st->R, st->T, st->Wc, nullptr, 0, w.partials, w.AtA, w.Atb, w.absres, w.nvalid, s,
                           syrk_stats_of_iteration(pl.s, it, max_iters), a.queue == nullptr, &run.role, run.mlp, w.mlp_y);
      if (rc != BANET_OK) return rc;
      if (run.prior.pl.on) {   // the depth block of AtA / Atb, before the damping
        RangeScope r("prior", lv->N);
        rc = launch_prior_add(run.prior, st->Wc, w.AtA, w.Atb, s);
        if (rc != BANET_OK) return rc;
      }
      if (run.pose.pl.on) {   // the pose block of AtA / Atb at the iteration's R, T, before the damping
        RangeScope r("pose_prior", lv->N);
        rc = launch_pose_prior_add(run.pose, st->R, st->T, w.AtA, w.Atb, s);
        if (rc != BANET_OK) return rc;
      }
      {
        RangeScope r("solve", lv->N);
        rc = launch_solve(a, s);
      }
      if (rc != BANET_OK) return rc;
    }
  }
  return BANET_OK;
}

static size_t solve_update_ws_bytes(int B, const SolvePlan& sp) { return align_up((size_t)B * sp.big_floats * sizeof(float), 256); }

// banet_ba_solve_update_f32 (has_ws = false) and banet_ba_solve_update_ws_f32: the checks, the plan, the launch.  A system whose
// matrix does not fit the LDS is BANET_ERR_UNSUPPORTED without a workspace, and BANET_ERR_WORKSPACE with one that is missing, too
// small or misaligned.
static int solve_update(const banet_level_t* lv, const banet_mlp_t* mlp, float l2_base, const float* AtA, const float* Atb,
                        const float* absres, const float* nvalid, banet_state_t* st, bool has_ws, void* ws, size_t ws_bytes,
                        banet_stream_t stream) {
  if (!lv || !AtA || !Atb || !absres || !nvalid) return BANET_ERR_INVALID_ARG;
  if (lv->variant < BANET_LEGACY_LM || lv->variant > BANET_BUNDLE || lv->B <= 0 || lv->N <= 0 || lv->C <= 0 || lv->K < 0 ||
      lv->pairs < 0)
    return BANET_ERR_INVALID_ARG;
  int rc = check_state(lv, mlp, st);
  if (rc != BANET_OK) return rc;
  SolveArgs a = make_solve_args(lv, mlp, l2_base, AtA, Atb, absres, nvalid, st);
  rc = plan_level_solve(lv, a.lm.solver, &a.pl);
  if (a.pl.big) {
    if (!has_ws) return BANET_ERR_UNSUPPORTED;
    if (!ws || ws_bytes < solve_update_ws_bytes(lv->B, a.pl) || !aligned256(ws)) return BANET_ERR_WORKSPACE;
    a.bigA = static_cast<float*>(ws);
  }
  if (rc != BANET_OK) return rc;
  return launch_solve(a, static_cast<hipStream_t>(stream));
}

}  // namespace banet

using namespace banet;

extern "C" {

int banet_version(void) { return BANET_VERSION; }

const char* banet_error_string(int code) {
  switch (code) {
    case BANET_OK: return "ok";
    case BANET_ERR_INVALID_ARG: return "invalid argument";
    case BANET_ERR_WORKSPACE: return "workspace too small or misaligned";
    case BANET_ERR_UNSUPPORTED: return "shape not supported by the compiled kernel set";
    case BANET_ERR_LAUNCH: return "kernel launch failed";
    default: return "unknown error";
  }
}

size_t banet_equation_construction_workspace_bytes(int B, int N, int C, int P) {
  EqPlan pl;
  if (plan_eq(B, N, C, P, &pl) != BANET_OK) return 0;
  return pl.partial_bytes;
}

int banet_equation_construction_f32(const float* J, const float* G, const float* d, float* AtA, float* Atb, int B,
                                    int N, int C, int P, void* ws, size_t ws_bytes, banet_stream_t stream) {
  if (!J || !G || !d || !AtA || !Atb) return BANET_ERR_INVALID_ARG;
  EqPlan pl;
  const int rc = plan_eq(B, N, C, P, &pl);
  if (rc != BANET_OK) return rc;
  if (!ws || ws_bytes < pl.partial_bytes || !aligned256(ws)) return BANET_ERR_WORKSPACE;
  return launch_eq(J, G, d, AtA, Atb, B, N, C, P, pl, static_cast<float*>(ws), static_cast<hipStream_t>(stream));
}

size_t banet_equation_construction_grad_workspace_bytes(int B, int N, int C, int P) {
  if (B <= 0 || N <= 0 || C <= 0 || P <= 0) return 0;
  return eq_grad_fast_ws_bytes(B, N, P);
}

int banet_equation_construction_grad_f32(const float* J, const float* G, const float* d, const float* g0,
                                         const float* g1, float* gJ, float* gG, float* gd, int B, int N, int C, int P,
                                         void* ws, size_t ws_bytes, banet_stream_t stream) {
  if (!J || !G || !d || !g0 || !g1 || !gJ || !gG || !gd) return BANET_ERR_INVALID_ARG;
  if (B <= 0 || N <= 0 || C <= 0 || P <= 0) return BANET_ERR_INVALID_ARG;
  // with a workspace (P <= 304): the matrix-pipe kernels of eqcon_grad.hip; without: the first-generation kernel
  const size_t need = eq_grad_fast_ws_bytes(B, N, P);
  if (need > 0 && ws != nullptr && ws_bytes >= need && aligned256(ws))
    return launch_eq_grad_fast(J, G, d, g0, g1, gJ, gG, gd, B, N, C, P, ws, static_cast<hipStream_t>(stream));
  return launch_eq_grad(J, G, d, g0, g1, gJ, gG, gd, B, N, C, P, static_cast<hipStream_t>(stream));
}

size_t banet_ba_assemble_workspace_bytes(const banet_level_t* lv) {
  AsmPlan pl;
  if (plan_assemble(lv, num_cus(), &pl) != BANET_OK) return 0;
  return align_up(pl.ws_bytes, 256);
}

int banet_ba_assemble_f32(const banet_level_t* lv, const float* R, const float* T, const float* Wc, float* AtA,
                          float* Atb, float* absres, float* nvalid, void* ws, size_t ws_bytes, banet_stream_t stream) {
  int rc = check_level(lv);
  if (rc != BANET_OK) return rc;
  if (!R || !T || !AtA || !Atb || !absres || !nvalid || (lv->K > 0 && !Wc)) return BANET_ERR_INVALID_ARG;
  AsmPlan pl;
  rc = plan_assemble(lv, num_cus(), &pl);
  if (rc != BANET_OK) return rc;
  if (!ws || ws_bytes < pl.ws_bytes || !aligned256(ws)) return BANET_ERR_WORKSPACE;
  return launch_assemble(lv, pl, R, T, Wc, nullptr, 0, ws, AtA, Atb, absres, nvalid,
                         static_cast<hipStream_t>(stream), syrk_stats_of_single_pass(pl.s));
}

int banet_ba_assemble_mask_f32(const banet_level_t* lv, const float* R, const float* T, const float* Wc, float* AtA,
                               float* Atb, float* absres, float* nvalid, unsigned char* mask_out, void* ws, size_t ws_bytes,
                               banet_stream_t stream) {
  int rc = check_level(lv);
  if (rc != BANET_OK) return rc;
  if (!R || !T || !AtA || !Atb || !absres || !nvalid || !mask_out || (lv->K > 0 && !Wc)) return BANET_ERR_INVALID_ARG;
  AsmPlan pl;
  rc = plan_assemble(lv, num_cus(), &pl);
  if (rc != BANET_OK) return rc;
  if (!ws || ws_bytes < pl.ws_bytes || !aligned256(ws)) return BANET_ERR_WORKSPACE;
  return launch_assemble(lv, pl, R, T, Wc, nullptr, 0, ws, AtA, Atb, absres, nvalid, static_cast<hipStream_t>(stream),
                         syrk_stats_of_single_pass(pl.s), true, nullptr, nullptr, nullptr, mask_out);
}

int banet_ba_residual_f32(const banet_level_t* lv, const float* R, const float* T, const float* Wc, const banet_residual_out_t* out,
                          banet_stream_t stream) {
  // the checks of banet_ba_assemble_f32, in its order and with its codes (flags / policy only select kernels there: ignored here,
  // but an unknown policy is refused like there)
  int rc = check_level(lv);
  if (rc != BANET_OK) return rc;
  if (!R || !T || !out || !out->sq || !out->ab || !out->mask || (lv->K > 0 && !Wc)) return BANET_ERR_INVALID_ARG;
  AsmPlan pl;
  rc = plan_assemble(lv, num_cus(), &pl);
  if (rc != BANET_OK) return rc;
  rc = residual_shape_supported(lv);
  if (rc != BANET_OK) return rc;
  return launch_residual(lv, R, T, Wc, out, static_cast<hipStream_t>(stream));
}

// the level checks of banet_ba_residual_f32, in its order and with its codes
static int residual_level_check(const banet_level_t* lv) {
  int rc = check_level(lv);
  if (rc != BANET_OK) return rc;
  AsmPlan pl;
  rc = plan_assemble(lv, num_cus(), &pl);
  if (rc != BANET_OK) return rc;
  return residual_shape_supported(lv);
}

size_t banet_ba_residual_grad_workspace_bytes(const banet_level_t* lv, int want_dtgt) {
  if (residual_level_check(lv) != BANET_OK) return 0;
  if (want_dtgt && !residual_grad_dtgt_supported(lv)) return 0;
  ResGradPlan pl;
  plan_residual_grad(lv, want_dtgt != 0, &pl);
  return pl.bytes;
}

int banet_ba_residual_grad_f32(const banet_level_t* lv, const float* R, const float* T, const float* Wc, const banet_residual_grad_in_t* g,
                               const banet_residual_grad_out_t* out, int flags, void* ws, size_t ws_bytes, banet_stream_t stream) {
  int rc = check_level(lv);
  if (rc != BANET_OK) return rc;
  if (!R || !T || !g || !out || (!g->gsq && !g->gab && !g->gproj) || (lv->K > 0 && !Wc)) return BANET_ERR_INVALID_ARG;
  if (flags & ~(BANET_ADJOINT_OVERWRITE | BANET_ADJOINT_OVERWRITE_MAP)) return BANET_ERR_INVALID_ARG;
  rc = residual_level_check(lv);
  if (rc != BANET_OK) return rc;
  if (out->dtgt && !residual_grad_dtgt_supported(lv)) return BANET_ERR_UNSUPPORTED;
  ResGradPlan pl;
  plan_residual_grad(lv, out->dtgt != nullptr, &pl);
  if (!ws || ws_bytes < pl.bytes || !aligned256(ws)) return BANET_ERR_WORKSPACE;
  return launch_residual_grad(lv, R, T, Wc, g, out, flags, ws, static_cast<hipStream_t>(stream));
}

size_t banet_ba_marginals_workspace_bytes(const banet_level_t* lv, int want_depth_var) {
  MargPlan pl;
  if (plan_marginals(lv, want_depth_var, &pl) != BANET_OK) return 0;
  return pl.bytes;
}

int banet_ba_marginals_f32(const banet_level_t* lv, const float* AtA, const float* damping, const float* sigma2,
                           const banet_marginals_out_t* out, void* ws, size_t workspace_bytes, banet_stream_t stream) {
  if (!lv || !AtA || !out || !out->pose_cov || !out->status) return BANET_ERR_INVALID_ARG;
  if (lv->B < 1 || lv->K < 0 || lv->pairs < 0) return BANET_ERR_INVALID_ARG;
  const bool want_dv = out->depth_var != nullptr && lv->K > 0;   // depth_var / wfactor of a level without a basis: ignored
  if (want_dv && (!lv->basis || lv->N < 1)) return BANET_ERR_INVALID_ARG;
  MargPlan pl;
  const int rc = plan_marginals(lv, want_dv, &pl);
  if (rc != BANET_OK) return rc;
  if (!ws || workspace_bytes < pl.bytes || !aligned256(ws)) return BANET_ERR_WORKSPACE;
  return launch_marginals(lv, pl, AtA, damping, sigma2, out, ws, static_cast<hipStream_t>(stream));
}

size_t banet_ba_marginals_grad_workspace_bytes(const banet_level_t* lv, int want_gbasis) {
  MargGradPlan pl;
  if (plan_marginals_grad(lv, want_gbasis, &pl) != BANET_OK) return 0;
  return pl.bytes;
}

int banet_ba_marginals_grad_f32(const banet_level_t* lv, const float* AtA, const float* damping, const float* sigma2,
                                const banet_marginals_grad_in_t* in, const banet_marginals_grad_out_t* out, void* ws,
                                size_t workspace_bytes, banet_stream_t stream) {
  if (!lv || !AtA || !in || !out || !out->status) return BANET_ERR_INVALID_ARG;
  if (lv->B < 1 || lv->K < 0 || lv->pairs < 0) return BANET_ERR_INVALID_ARG;
  const bool want_gb = out->gbasis != nullptr && lv->K > 0;      // gbasis / g_depth_var of a level without a basis: ignored
  const bool reads_basis = lv->K > 0 && (in->g_depth_var != nullptr || out->gbasis != nullptr);
  if (reads_basis && (!lv->basis || lv->N < 1)) return BANET_ERR_INVALID_ARG;
  MargGradPlan pl;
  const int rc = plan_marginals_grad(lv, want_gb, &pl);
  if (rc != BANET_OK) return rc;
  if (!ws || workspace_bytes < pl.bytes || !aligned256(ws)) return BANET_ERR_WORKSPACE;
  return launch_marginals_grad(lv, pl, AtA, damping, sigma2, in, out, ws, static_cast<hipStream_t>(stream));
}

size_t banet_depth_reproject_workspace_bytes(const banet_level_t* lv) {
  size_t bytes = 0;
  if (plan_reproject(lv, &bytes) != BANET_OK) return 0;
  return bytes;
}

int banet_depth_reproject_f32(const banet_level_t* lv, const float* R, const float* T, const float* Wc,
                              const banet_reproject_out_t* out, void* ws, size_t workspace_bytes, banet_stream_t stream) {
  if (!lv || !R || !T || !out || !out->depth || !out->index) return BANET_ERR_INVALID_ARG;
  size_t bytes = 0;
  const int rc = plan_reproject(lv, &bytes);
  if (rc != BANET_OK) return rc;
  if (!lv->depth || !lv->intr || (lv->K > 0 && Wc && !lv->basis)) return BANET_ERR_INVALID_ARG;
  if (!ws || workspace_bytes < bytes || !aligned256(ws)) return BANET_ERR_WORKSPACE;
  return launch_reproject(lv, R, T, Wc, out, ws, static_cast<hipStream_t>(stream));
}

size_t banet_basis_fit_workspace_bytes(const banet_level_t* lv) {
  FitPlan pl;
  if (plan_basis_fit(lv, &pl) != BANET_OK) return 0;
  return pl.bytes;
}

int banet_basis_fit_f32(const banet_level_t* lv, const float* target, const float* weight, const float* damping,
                        const banet_basis_fit_out_t* out, void* ws, size_t workspace_bytes, banet_stream_t stream) {
  if (!lv || !target || !out || !out->Wc || !out->status) return BANET_ERR_INVALID_ARG;
  FitPlan pl;
  const int rc = plan_basis_fit(lv, &pl);
  if (rc != BANET_OK) return rc;
  if (!lv->depth || !lv->basis) return BANET_ERR_INVALID_ARG;
  if (!ws || workspace_bytes < pl.bytes || !aligned256(ws)) return BANET_ERR_WORKSPACE;
  return launch_basis_fit(lv, pl, target, weight, damping, out, ws, static_cast<hipStream_t>(stream));
}

int banet_ba_solve_update_f32(const banet_level_t* lv, const banet_mlp_t* mlp, float l2_base, const float* AtA,
                              const float* Atb, const float* absres, const float* nvalid, banet_state_t* st,
                              banet_stream_t stream) {
  return solve_update(lv, mlp, l2_base, AtA, Atb, absres, nvalid, st, false, nullptr, 0, stream);
}

size_t banet_ba_solve_update_workspace_bytes(const banet_level_t* lv) {
  if (!lv || lv->B <= 0 || lv->C <= 0 || lv->K < 0 || lv->pairs < 0) return 0;
  SolvePlan sp;
  (void)plan_level_solve(lv, BANET_SOLVER_QR, &sp);   // (big / big_floats: filled whatever it returns)
  return solve_update_ws_bytes(lv->B, sp);
}

int banet_ba_solve_update_ws_f32(const banet_level_t* lv, const banet_mlp_t* mlp, float l2_base, const float* AtA,
                                 const float* Atb, const float* absres, const float* nvalid, banet_state_t* st, void* ws,
                                 size_t ws_bytes, banet_stream_t stream) {
  return solve_update(lv, mlp, l2_base, AtA, Atb, absres, nvalid, st, true, ws, ws_bytes, stream);
}

size_t banet_lm_level_workspace_bytes(const banet_level_t* lv) {
  AsmPlan pl;
  if (plan_assemble(lv, num_cus(), &pl) != BANET_OK) return 0;
  SolvePlan sp;
  (void)plan_level_solve(lv, BANET_SOLVER_QR, &sp);   // (big / big_floats: filled whatever it returns)
  return carve_level(lv, pl, sp, nullptr).total;
}

void banet_lm_params_default(banet_lm_params_t* p) {
  if (!p) return;
  p->angle_change = (float)(0.002 * (3.14 / 180.0));   // legacy/ba.py:6 (3.14, not pi)
  p->translation_change = 0.0002f;                      // legacy/ba.py:7
  p->residual_ratio = 1.0f;                             // legacy/ba.py:8
  p->solver = BANET_SOLVER_QR;                          // legacy/ba.py:9
}

int banet_lm_level_f32(const banet_level_t* lv, const banet_mlp_t* mlp, float l2_base, int max_iters,
                       int early_termination, banet_state_t* st, void* ws, size_t ws_bytes, banet_stream_t stream) {
  return banet_lm_level_ex_f32(lv, mlp, l2_base, max_iters, early_termination, nullptr, st, ws, ws_bytes, stream);
}

int banet_lm_level_ex_f32(const banet_level_t* lv, const banet_mlp_t* mlp, float l2_base, int max_iters,
                          int early_termination, const banet_lm_params_t* params, banet_state_t* st, void* ws,
                          size_t ws_bytes, banet_stream_t stream) {
  LevelRun run;
  const int rc = lm_level_plan(lv, mlp, l2_base, max_iters, early_termination, params, st, ws, ws_bytes, &run);
  if (rc != BANET_OK) return rc;
  return lm_level_enqueue(run, static_cast<hipStream_t>(stream));
}

size_t banet_lm_level_prior_workspace_bytes(const banet_level_t* lv, const banet_prior_t* pr) { return lm_level_prior_bytes(lv, pr); }

int banet_lm_level_prior_f32(const banet_level_t* lv, const banet_mlp_t* mlp, float l2_base, int max_iters,
                             const banet_lm_params_t* params, const banet_prior_t* pr, banet_state_t* st, void* ws,
                             size_t workspace_bytes, banet_stream_t stream) {
  LevelRun run;
  const int rc = lm_level_prior_plan(lv, mlp, l2_base, max_iters, params, pr, st, ws, workspace_bytes, &run);
  if (rc != BANET_OK) return rc;
  return lm_level_enqueue(run, static_cast<hipStream_t>(stream));
}

size_t banet_lm_level_pose_prior_workspace_bytes(const banet_level_t* lv, const banet_prior_t* pr, const banet_pose_prior_t* pp) {
  return lm_level_pose_prior_bytes(lv, pr, pp);
}

int banet_lm_level_pose_prior_f32(const banet_level_t* lv, const banet_mlp_t* mlp, float l2_base, int max_iters,
                                  const banet_lm_params_t* params, const banet_prior_t* pr, const banet_pose_prior_t* pp,
                                  banet_state_t* st, void* ws, size_t workspace_bytes, banet_stream_t stream) {
  LevelRun run;
  const int rc = lm_level_pose_prior_plan(lv, mlp, l2_base, max_iters, params, pr, pp, st, ws, workspace_bytes, &run);
  if (rc != BANET_OK) return rc;
  return lm_level_enqueue(run, static_cast<hipStream_t>(stream));
}

int banet_pose_prior_add_grad_f32(const banet_level_t* lv, const banet_pose_prior_t* pp, const float* R, const float* T,
                                  const float* gAtA, const float* gAtb, const banet_pose_prior_grad_t* out, banet_stream_t stream) {
  if (!R || !T || !gAtA || !gAtb) return BANET_ERR_INVALID_ARG;
  PosePriorGradPlan pl;
  const int rc = plan_pose_prior_grad(lv, pp, out, &pl);
  if (rc != BANET_OK) return rc;
  return launch_pose_prior_grad(pl, *pp, R, T, gAtA, gAtb, *out, static_cast<hipStream_t>(stream));
}

int banet_resample_f32(const float* data, const float* warp, float* out, int B, int N, int C, int H, int W, int mode,
                       banet_stream_t stream) {
  if (!data || !warp || !out) return BANET_ERR_INVALID_ARG;
  return launch_resample(data, warp, out, B, N, C, H, W, mode, static_cast<hipStream_t>(stream));
}

int banet_target_map_f32(const float* img, float* out, int B, int H, int W, int C, banet_stream_t stream) {
  if (!img || !out) return BANET_ERR_INVALID_ARG;
  return launch_target_map(img, out, B, H, W, C, static_cast<hipStream_t>(stream));
}

int banet_depth_output_f32(const float* init_depth, const float* basis, const float* Wc, float* out, int B, int N, int K,
                           banet_stream_t stream) {
  if (!init_depth || !basis || !Wc || !out) return BANET_ERR_INVALID_ARG;
  return launch_depth_output(init_depth, basis, Wc, out, B, N, K, static_cast<hipStream_t>(stream));
}

size_t banet_resample_grad_workspace_bytes(int B, int N, int C, int H, int W, int mode) {
  if (B <= 0 || N <= 0 || C <= 0 || H <= 0 || W <= 0 || (mode != BANET_RESAMPLE_ZERO_PAD && mode != BANET_RESAMPLE_CLAMP)) return 0;
  if (!resample_grad_supported(B, N, C, H, W)) return 0;
  return resample_grad_workspace_bytes(B, N, C, H, W);
}

int banet_resample_grad_f32(const float* data, const float* warp, const float* gout, float* ddata, float* dwarp, int B, int N, int C,
                            int H, int W, int mode, int flags, void* ws, size_t ws_bytes, banet_stream_t stream) {
  if (!data || !warp || !gout) return BANET_ERR_INVALID_ARG;
  if (B <= 0 || N <= 0 || C <= 0 || H <= 0 || W <= 0 || (mode != BANET_RESAMPLE_ZERO_PAD && mode != BANET_RESAMPLE_CLAMP))
    return BANET_ERR_INVALID_ARG;
  if (flags & ~BANET_ADJOINT_OVERWRITE) return BANET_ERR_INVALID_ARG;
  if (!resample_grad_supported(B, N, C, H, W)) return BANET_ERR_UNSUPPORTED;
  if (!ws || ws_bytes < resample_grad_workspace_bytes(B, N, C, H, W) || (reinterpret_cast<uintptr_t>(ws) & 255) != 0)
    return BANET_ERR_WORKSPACE;
  return launch_resample_grad(data, warp, gout, ddata, dwarp, B, N, C, H, W, mode, flags & BANET_ADJOINT_OVERWRITE, ws,
                              static_cast<hipStream_t>(stream));
}

size_t banet_depth_output_grad_workspace_bytes(int B, int N, int K) {
  if (B <= 0 || N <= 0 || K <= 0) return 0;
  return depth_output_grad_workspace_bytes(B, N, K);
}

int banet_depth_output_grad_f32(const float* basis, const float* Wc, const float* gout, float* dinit, float* dbasis, float* dWc, int B,
                                int N, int K, int flags, void* ws, size_t ws_bytes, banet_stream_t stream) {
  if (!basis || !Wc || !gout) return BANET_ERR_INVALID_ARG;
  if (B <= 0 || N <= 0 || K <= 0 || (flags & ~BANET_ADJOINT_OVERWRITE)) return BANET_ERR_INVALID_ARG;
  if (!ws || ws_bytes < depth_output_grad_workspace_bytes(B, N, K) || (reinterpret_cast<uintptr_t>(ws) & 255) != 0)
    return BANET_ERR_WORKSPACE;
  return launch_depth_output_grad(basis, Wc, gout, dinit, dbasis, dWc, B, N, K, flags & BANET_ADJOINT_OVERWRITE, ws,
                                  static_cast<hipStream_t>(stream));
}

int banet_grid_resample_f32(const float* data, int B, int H, int W, int C, int mode, const banet_grid_level_t* levels, int n_levels,
                            banet_stream_t stream) {
  return launch_grid_resample(data, B, H, W, C, mode, levels, n_levels, static_cast<hipStream_t>(stream));
}

int banet_grid_resample_grad_f32(float* ddata, int B, int H, int W, int C, int mode, const banet_grid_level_t* levels, int n_levels,
                                 int flags, banet_stream_t stream) {
  if (flags & ~BANET_ADJOINT_OVERWRITE) return BANET_ERR_INVALID_ARG;
  return launch_grid_resample_grad(ddata, B, H, W, C, mode, levels, n_levels, flags & BANET_ADJOINT_OVERWRITE,
                                   static_cast<hipStream_t>(stream));
}

int banet_sample_stats_blocks(int N) { return N > 0 ? sample_stats_blocks(N) : 0; }

static bool sstats_shape_ok(int B, int N, int C, int H, int W) {
  return B > 0 && N > 0 && C > 0 && H > 0 && W > 0 && (unsigned long long)B * H * W * 3ull * C < (1ull << 32);
}

int banet_sample_stats_f32(const float* conv1, const float* conv2, const float* px, const float* py, int B, int N, int C, int H,
                           int W, float* stats, float* absd_part, banet_stream_t stream) {
  if (!conv1 || !conv2 || !px || !py || !stats || !absd_part) return BANET_ERR_INVALID_ARG;
  if (!sstats_shape_ok(B, N, C, H, W)) return BANET_ERR_INVALID_ARG;
  return launch_sample_stats(conv1, conv2, px, py, B, N, C, H, W, stats, absd_part, static_cast<hipStream_t>(stream));
}

int banet_sample_stats_grad_f32(const float* conv1, const float* conv2, const float* px, const float* py, int B, int N, int C,
                                int H, int W, const float* dstats, const float* dabs, float* dconv1, float* dconv2, float* dpos,
                                banet_stream_t stream) {
  if (!conv1 || !conv2 || !px || !py || !dstats || !dabs || !dconv1 || !dconv2 || !dpos) return BANET_ERR_INVALID_ARG;
  if (!sstats_shape_ok(B, N, C, H, W)) return BANET_ERR_INVALID_ARG;
  return launch_sample_stats_grad(conv1, conv2, px, py, B, N, C, H, W, dstats, dabs, dconv1, dconv2, dpos,
                                  static_cast<hipStream_t>(stream));
}

int banet_spd_solve_f32(const float* A, const float* rhs, float* x, int B, int P, banet_stream_t stream) {
  if (!A || !rhs || !x || B <= 0 || P <= 0) return BANET_ERR_INVALID_ARG;
  return launch_spd_solve(A, rhs, x, B, P, static_cast<hipStream_t>(stream));
}

size_t banet_sample_stats_grad_workspace_bytes(int B, int N, int C, int H, int W) {
  if (!sstats_shape_ok(B, N, C, H, W)) return 0;
  return sample_stats_grad_det_workspace_bytes(B, N, C, H, W);
}

int banet_sample_stats_grad_det_f32(const float* conv1, const float* conv2, const float* px, const float* py, int B, int N, int C,
                                    int H, int W, const float* dstats, const float* dabs, float* dconv1, float* dconv2,
                                    float* dpos, void* ws, size_t ws_bytes, banet_stream_t stream) {
  if (!conv1 || !conv2 || !px || !py || !dstats || !dabs || !dconv1 || !dconv2 || !dpos) return BANET_ERR_INVALID_ARG;
  if (!sstats_shape_ok(B, N, C, H, W)) return BANET_ERR_INVALID_ARG;
  const size_t need = sample_stats_grad_det_workspace_bytes(B, N, C, H, W);
  if (need == 0) return BANET_ERR_UNSUPPORTED;
  if (!ws || ws_bytes < need || !aligned256(ws)) return BANET_ERR_WORKSPACE;   // a missing workspace is a workspace error, as everywhere
  return launch_sample_stats_grad_det(conv1, conv2, px, py, B, N, C, H, W, dstats, dabs, dconv1, dconv2, dpos, ws,
                                      static_cast<hipStream_t>(stream));
}

size_t banet_dense_adjoint_workspace_bytes(const banet_level_t* lv) {
  if (!lv || lv->B <= 0 || lv->N <= 0) return 0;
  return dense_adjoint_workspace_bytes(lv);
}

size_t banet_dense_adjoint_workspace_bytes_ex(const banet_level_t* lv, int flags) {
  if (!lv || lv->B <= 0 || lv->N <= 0) return 0;
  if (flags & ~(BANET_ADJOINT_OVERWRITE | BANET_ADJOINT_OVERWRITE_MAP | BANET_ADJOINT_FOLD_TARGET | BANET_ADJOINT_REUSE_DEPTH_SEED | BANET_ADJOINT_TILE_SHAPE(15))) return 0;
  return dense_adjoint_workspace_bytes(lv, flags);
}

int banet_dense_adjoint_ex_f32(const banet_level_t* lv, const float* R, const float* T, const float* Wc, const float* gAtA,
                               const float* gAtb, const float* gabs, float* dsrc, float* dmap3, float* ddepth, float* dbasis,
                               float* dpose, int flags, void* ws, size_t ws_bytes, banet_stream_t stream) {
  if (!lv || !R || !T || !gAtA || !gAtb || !gabs || !dsrc || !dmap3 || !ddepth || !dpose) return BANET_ERR_INVALID_ARG;
  if (lv->K > 0 && (!Wc || !dbasis || !lv->basis)) return BANET_ERR_INVALID_ARG;     // K = 0 (pose only): no coefficient / basis tensors
  if (lv->B <= 0 || lv->N <= 0 || !lv->src || !lv->tgt || !lv->depth) return BANET_ERR_INVALID_ARG;
  if (lv->dense ? !lv->intr : (!lv->rays || !lv->fx || !lv->fy || !lv->ox || !lv->oy)) return BANET_ERR_INVALID_ARG;
  if (flags & ~(BANET_ADJOINT_OVERWRITE | BANET_ADJOINT_OVERWRITE_MAP | BANET_ADJOINT_FOLD_TARGET | BANET_ADJOINT_REUSE_DEPTH_SEED | BANET_ADJOINT_TILE_SHAPE(15))) return BANET_ERR_INVALID_ARG;
  const size_t need = dense_adjoint_workspace_bytes(lv, flags);
  if (need == 0) return BANET_ERR_UNSUPPORTED;
  if (!ws || ws_bytes < need || !aligned256(ws)) return BANET_ERR_WORKSPACE;
  return launch_dense_adjoint(lv, R, T, Wc, gAtA, gAtb, gabs, dsrc, dmap3, ddepth, dbasis, dpose, flags, ws,
                              static_cast<hipStream_t>(stream));
}

int banet_dense_adjoint_f32(const banet_level_t* lv, const float* R, const float* T, const float* Wc, const float* gAtA,
                            const float* gAtb, const float* gabs, float* dsrc, float* dmap3, float* ddepth, float* dbasis,
                            float* dpose, void* ws, size_t ws_bytes, banet_stream_t stream) {
  return banet_dense_adjoint_ex_f32(lv, R, T, Wc, gAtA, gAtb, gabs, dsrc, dmap3, ddepth, dbasis, dpose, 0, ws, ws_bytes, stream);
}

int banet_target_map_adjoint_ex_f32(const float* dmap3, float* dimg, int B, int H, int W, int C, int flags, banet_stream_t stream) {
  if (!dmap3 || !dimg || B <= 0 || H <= 0 || W <= 0 || C <= 0 || (flags & ~BANET_ADJOINT_OVERWRITE)) return BANET_ERR_INVALID_ARG;
  return launch_target_map_adjoint(dmap3, dimg, B, H, W, C, flags & BANET_ADJOINT_OVERWRITE, static_cast<hipStream_t>(stream));
}

int banet_target_map_adjoint_f32(const float* dmap3, float* dimg, int B, int H, int W, int C, banet_stream_t stream) {
  return banet_target_map_adjoint_ex_f32(dmap3, dimg, B, H, W, C, 0, stream);
}

size_t banet_small_step_adjoint_workspace_bytes(int variant, int B, int N, int C, int K, int pairs) {
  return small_step_workspace_bytes(variant, B, N, C, K, pairs);
}

int banet_small_step_adjoint_f32(int variant, int B, int N, int C, int K, int pairs, float l2_regularizer_base, const banet_mlp_t* mlp,
                                 const float* AtA, const float* Atb, const float* absres, const float* delta, const float* R,
                                 const float* T, const float* gR, const float* gT, const float* gW, float* gAtA, float* gAtb, float* gabs,
                                 float* dR, float* dT, const banet_mlp_t* gmlp, void* ws, size_t ws_bytes, banet_stream_t stream) {
  if (!mlp || !gmlp || !AtA || !Atb || !absres || !delta || !R || !T || !gR || !gT || !gAtA || !gAtb || !gabs || !dR || !dT)
    return BANET_ERR_INVALID_ARG;
  if (K > 0 && !gW) return BANET_ERR_INVALID_ARG;
  for (int i = 0; i < 5; ++i)
    if (!mlp->w[i] || !mlp->b[i] || !gmlp->w[i] || !gmlp->b[i]) return BANET_ERR_INVALID_ARG;
  if (B <= 0 || N <= 0 || C <= 0 || K < 0 || pairs < 1) return BANET_ERR_INVALID_ARG;
  const size_t need = small_step_workspace_bytes(variant, B, N, C, K, pairs);
  if (need == 0) return BANET_ERR_UNSUPPORTED;
  if (!ws || ws_bytes < need || !aligned256(ws)) return BANET_ERR_WORKSPACE;
  return launch_small_step_adjoint(variant, B, N, C, K, pairs, l2_regularizer_base, mlp, AtA, Atb, absres, delta, R, T, gR, gT, gW, gAtA,
                                   gAtb, gabs, dR, dT, gmlp, ws, static_cast<hipStream_t>(stream));
}

#include "build_id.h"   // generated by build.sh: BANET_BUILD_ID
const char* banet_build_id(void) { return BANET_BUILD_ID; }

int banet_profile_ranges(int enable) { return profile_ranges(enable); }

int banet_gather_selection(const banet_level_t* lv) {
  GatherPlan pl;
  const int rc = plan_gather(lv, num_cus(), &pl);
  if (rc != BANET_OK) return rc;
  return pl.quad ? 4 : pl.strip ? 3 : pl.patch ? 2 : pl.c128 ? 1 : 0;
}

int banet_syrk_selection(const banet_level_t* lv) {
  AsmPlan pl;
  const int rc = plan_assemble(lv, num_cus(), &pl);
  if (rc != BANET_OK) return rc;
  if (lv->K == 0) return -1000;
  return pl.s.f16 ? 4 : pl.s.direct;
}

int banet_profile_begin(int max_launches) { return profile_begin(max_launches); }

int banet_profile_end(int max_tags, int32_t* tag_points, int32_t* tag_launches, double* tag_ms, int32_t* ntags) {
  return profile_end(max_tags, tag_points, tag_launches, tag_ms, ntags);
}

}  // extern "C"
