// Launchers / argument blocks shared by the translation units of libbanet_hip.so (the host-only launch plans: plan.hpp).
#pragma once
#include "common.hpp"
#include "grid_plan.hpp"   // the grid resampler's geometry (host-only like plan.hpp)
#include "prior_plan.hpp"  // the prior term's regions and the Gram pass's partial rows (host-only like plan.hpp)
#include "prior_grad_plan.hpp"  // its backward: outputs, per-pixel grid, Gh / gh regions (host-only like plan.hpp)
#include "pose_prior_plan.hpp"  // the pose prior: struct checks, the empty test, the grid (host-only like plan.hpp)
#include "pose_prior_grad_plan.hpp"  // its backward: checks, grid, the phases per output set (host-only like plan.hpp)
#include "solve_plan.hpp"  // the solve: method, LDS-or-workspace switch, LDS layout (host-only like plan.hpp)

namespace banet {

constexpr int kUStrideS = 8;    // per-pixel record: u0..u5, s, r

// compute units of the current device (hipDeviceAttributeMultiprocessorCount, queried once per device; 256 = MI355X when no
// device is visible, e.g. the host-only plan / workspace arithmetic of the CPU tests).  The launch plans size their grids by it.
int num_cus();

// ---- gather.hip (driver; the step list: plan.hpp, kernels: gather_generic / gather128 / 128p / 128s / 128q.hip) ----------
// (GatherPlan / plan_gather / plan_gather_steps: plan.hpp)
// prepare (reset the tile queue) -> launch (the gather kernel alone: this is what the profiler times)
// -> finish (fold the tile partials; returns the rows ba_reduce2_kernel should read): each enqueues its steps of `steps`
void prepare_gather(const GatherSteps& steps, const GatherPlan& pl, float* partials, hipStream_t s);
int launch_gather(const GatherSteps& steps, const banet_level_t* lv, const GatherPlan& pl, const float* R, const float* T, const float* Wc,
                  const int32_t* active, int active_stride, float* rec, float* partials, hipStream_t s,
                  unsigned char* mask_out = nullptr);
const float* finish_gather(const GatherSteps& steps, const banet_level_t* lv, const GatherPlan& pl, const int32_t* active,
                           int active_stride, float* partials, hipStream_t s);

// ---- syrk.hip (driver; the step list: plan.hpp, kernels: syrk_lds / _mfma32 / _bf16x6 / _wide / _stats.hip) -------------
struct MlpRole {        // one extra workgroup per window of the SYRK launch evaluates the lambda MLP (mlp.hpp); y == nullptr: off
  const float* gpart;   // folded gather partial rows [B * pairs][grows][gstride]
  int grows, gstride;
  banet_mlp_t mlp;
  int C, pairs;
  float Nf;             // residual rows per window (N * pairs)
  float* y;             // [B] MLP output
};
// (SyrkPlan / plan_syrk / SyrkStats / SyrkRole / plan_syrk_steps: plan.hpp)  Enqueues the steps of plan_syrk_steps.  role: plan_syrk_role's
// (or {0, pl.Gs}): role.Gs partial rows per window are written; mr: the role's arguments where role.on; stats: which form runs and
// what becomes of the basis column maxima (syrk_stats_of_iteration / syrk_stats_of_single_pass)
int launch_syrk(const float* basis, const float* rec, int B, int N, int K, int pairs, const SyrkPlan& pl, const int32_t* active,
                int active_stride, float* partials, hipStream_t s, const SyrkRole& role, const MlpRole* mr, SyrkStats stats);
// ---- syrk_reduce.hip ---------------------------------------------------------------------
void launch_reduce2(const float* gpart, int Gg, int gstride, const float* spart, int Gs, int sstride,
                    const int32_t* active, int active_stride, int B, int K, int C, int pairs, float* AtA, float* Atb,
                    float* absres, float* nvalid, hipStream_t s);

// ---- assemble.hip: one assembly pass = gather + syrk + reduce ------------------------------
// (AsmPlan / plan_assemble: plan.hpp)
int launch_assemble(const banet_level_t* lv, const AsmPlan& pl, const float* R, const float* T, const float* Wc,
                    const int32_t* active, int active_stride, void* ws, float* AtA, float* Atb, float* absres,
                    float* nvalid, hipStream_t s, SyrkStats stats = kSyrkStatsExact, bool reset_queue = true,
                    const SyrkRole* role = nullptr, const banet_mlp_t* role_mlp = nullptr, float* role_y = nullptr,
                    unsigned char* mask_out = nullptr);   // role (with role_mlp / role_y): plan_syrk_role's, where it is on
int* assemble_queue(const AsmPlan& pl, void* ws);   // the gather's tile-queue heads inside the workspace (or nullptr)
int profile_ranges(int enable);             // roctx ranges around the launches (banet_profile_ranges)
struct RangeScope {                         // pushes "banet.<role>[ N=<n>]" when ranges are on
  bool on;
  RangeScope(const char* role, int n = -1);
  ~RangeScope();
};
int profile_begin(int max_launches);
int profile_end(int max_tags, int32_t* tag_points, int32_t* tag_launches, double* tag_ms, int32_t* ntags);

// ---- residual.hip: per-pixel error maps, mask and their sums at a state (banet_ba_residual_f32; no workspace) ----
int residual_shape_supported(const banet_level_t* lv);   // the assembly's launch-time refusals (odd C / K above 128), as its code
int launch_residual(const banet_level_t* lv, const float* R, const float* T, const float* Wc, const banet_residual_out_t* out,
                    hipStream_t s);

// ---- residual_grad.hip: the backward of the above (banet_ba_residual_grad_f32) ----
constexpr int kResGradLdsFrames = 32;   // windows of up to this many target frames keep the kernel's pose slots in LDS (16 x 12 doubles = 1536 bytes per frame)
struct ResGradPlan {   // the workspace of one call; host memory only
  int pairs, units, G, cols;   // G: workgroups = partial rows per window (512 points each); cols = 12 pairs + K floats per row
  int slots_in_ws;             // pairs > kResGradLdsFrames: the pose slots [B][G][16][pairs][12] (doubles) live in the workspace
  size_t off_part, off_slots, off_erow, off_eproj, off_rg, bytes;
};
bool residual_grad_dtgt_supported(const banet_level_t* lv);   // C-channel target map within the resampler gradient's limits
void plan_residual_grad(const banet_level_t* lv, int want_dtgt, ResGradPlan* pl);   // a level the forward accepts
int launch_residual_grad(const banet_level_t* lv, const float* R, const float* T, const float* Wc, const banet_residual_grad_in_t* gin,
                         const banet_residual_grad_out_t* out, int flags, void* ws, hipStream_t s);

// ---- marginals.hip: pose covariance and per-pixel depth variance from a normal matrix (banet_ba_marginals_f32) ----
constexpr int kMargKMax = 256, kMargPMax = 304;   // the project's largest system (8 target frames, K = 256)
struct MargPlan {   // the workspace of one call; host memory only
  int P, m, K;      // m = 6 pairs pose coefficients
  bool big;         // the factor kernel's matrix (packed lower triangle, doubles) lives in the workspace (P >= 200: it does not fit the LDS)
  size_t lds;       // the factor kernel's dynamic LDS
  size_t off_T, off_big, bytes;   // T = L_WW^-1 [B][K][K] for the depth-variance kernel
};
// reads lv->B / K / pairs only; BANET_ERR_INVALID_ARG (NULL, B < 1, negative K / pairs) or BANET_ERR_UNSUPPORTED (K > 256, P > 304)
int plan_marginals(const banet_level_t* lv, int want_depth_var, MargPlan* pl);
int launch_marginals(const banet_level_t* lv, const MargPlan& pl, const float* AtA, const float* damping, const float* sigma2,
                     const banet_marginals_out_t* out, void* ws, hipStream_t s);

// ---- marginals_grad.hip: the backward of the above (banet_ba_marginals_grad_f32) ----
struct MargGradPlan {   // the workspace of one call; host memory only
  int P, m, K, NR, NP;  // NR 32-column blocks of the depth block, NP = NR (NR + 1) / 2 lower 32 x 32 blocks of M = sum g b b^T
  int chunk, rows;      // M's partial rows per window (pixels per row, rows): functions of N alone
  bool big;             // the factor kernel's packed triangle of Y lives in the workspace: P >= 200, MargPlan's switch by the same
                        // arithmetic (P (P + 1) / 2 + 2 P doubles against 160 KB of LDS).  Hinv (a second packed triangle) and
                        // X = Hinv Gbar [P][P] are in the workspace at every P
  size_t lds;           // the factor kernel's dynamic LDS
  size_t off_part, off_M, off_T, off_Hinv, off_X, off_big, bytes;
};
// reads lv->B / N / K / pairs only (N sizes M's partial rows; < 1 counts as 1); the return codes of plan_marginals
int plan_marginals_grad(const banet_level_t* lv, int want_gbasis, MargGradPlan* pl);
int launch_marginals_grad(const banet_level_t* lv, const MargGradPlan& pl, const float* AtA, const float* damping, const float* sigma2,
                          const banet_marginals_grad_in_t* in, const banet_marginals_grad_out_t* out, void* ws, hipStream_t s);

// ---- reproject.hip: the key frame's depth map in the target frames' pixel grids, z-buffered (banet_depth_reproject_f32) ----
// reads lv->B / N / K / H / W / dense / scale / pairs only; BANET_ERR_INVALID_ARG (NULL, a non-positive size, N != H W, scale <= 0)
// or BANET_ERR_UNSUPPORTED (a sparse level); *bytes = the 64-bit keys [B][max(pairs, 1)][H][W]
int plan_reproject(const banet_level_t* lv, size_t* bytes);
int launch_reproject(const banet_level_t* lv, const float* R, const float* T, const float* Wc, const banet_reproject_out_t* out,
                     void* ws, hipStream_t s);

// ---- basisfit.hip: weighted, damped least squares of a depth map on a level's basis (banet_basis_fit_f32) ----
constexpr int kFitKMax = 256;
struct FitPlan {    // the workspace of one call; host memory only
  int K, NR, NP;    // NR 32-column blocks, NP = NR (NR + 1) / 2 lower 32 x 32 blocks of G
  int chunk, rows;  // pixels per partial row, partial rows per window: functions of N alone
  int pstride;      // floats per partial row
  bool big;         // the solve kernel's matrix (packed lower triangle, doubles) lives in the workspace (K >= 200)
  size_t lds;       // the solve kernel's dynamic LDS
  size_t off_part, off_G, off_g, off_big, bytes;
};
// reads lv->B / N / K only; BANET_ERR_INVALID_ARG (NULL, B < 1) or BANET_ERR_UNSUPPORTED (K outside 1 .. 256, N < 1)
int plan_basis_fit(const banet_level_t* lv, FitPlan* pl);
int launch_basis_fit(const banet_level_t* lv, const FitPlan& pl, const float* target, const float* weight, const float* damping,
                     const banet_basis_fit_out_t* out, void* ws, hipStream_t s);
// its first two launches (Gram pass over the rows `fr` = fit_rows(N, K), fold): G / g to Gws / gws, and to normal / rhs / stats where given
int launch_fit_gram_fold(const banet_level_t* lv, const FitRows& fr, const float* target, const float* weight, float* part, float* Gws,
                         float* gws, float* normal, float* rhs, float* stats, hipStream_t s);

// ---- prior.hip: depth observations and coefficient priors between assembly and solve (banet_prior_apply_f32, the *_prior_ LM entries;
//      plan: prior_plan.hpp) ----
struct PriorRun {   // a planned prior next to its pointers; host memory only.  pl.on == 0: nothing is launched
  PriorPlan pl;
  banet_prior_t pr;
  int B;
  float* Le;        // [B][K][K] inside the workspace
  float* ee;        // [B][K]
  float* part;      // pl.obs: the Gram pass's partial rows, G and g (nullptr otherwise)
  float* G;
  float* g;
};
// pl: plan_prior's for (lv, pr), its offsets relative to `ws`
PriorRun make_prior_run(const banet_level_t* lv, const banet_prior_t* pr, const PriorPlan& pl, void* ws);
int launch_prior_setup(const banet_level_t* lv, const PriorRun& run, hipStream_t s);   // once per level: Le, ee
int launch_prior_add(const PriorRun& run, const float* Wc, float* AtA, float* Atb, hipStream_t s);   // every iteration

// ---- pose_prior.hip: the SE(3) log residual on the pose block between assembly and solve (banet_pose_prior_apply_f32, the
//      *_pose_prior_ LM entries; plan: pose_prior_plan.hpp) ----
struct PosePriorRun {   // a planned pose prior next to its pointers; host memory only.  pl.on == 0: nothing is launched
  PosePriorPlan pl;
  banet_pose_prior_t pp;
};
int launch_pose_prior_add(const PosePriorRun& run, const float* R, const float* T, float* AtA, float* Atb, hipStream_t s);   // every iteration
// ---- pose_prior_grad.hip: its backward, one launch per iteration (banet_pose_prior_add_grad_f32; plan: pose_prior_grad_plan.hpp) ----
int launch_pose_prior_grad(const PosePriorGradPlan& pl, const banet_pose_prior_t& pp, const float* R, const float* T, const float* gAtA,
                           const float* gAtb, const banet_pose_prior_grad_t& out, hipStream_t s);

// ---- prep.hip --------------------------------------------------------------------------
int launch_resample(const float* data, const float* warp, float* out, int B, int N, int C, int H, int W, int mode,
                    hipStream_t s);
int launch_target_map(const float* img, float* out, int B, int H, int W, int C, hipStream_t s);
int launch_depth_output(const float* init, const float* basis, const float* Wc, float* out, int B, int N, int K,
                        hipStream_t s);

// ---- prep_grad.hip ---------------------------------------------------------------------
bool resample_grad_supported(int B, int N, int C, int H, int W);
size_t resample_grad_workspace_bytes(int B, int N, int C, int H, int W);
int launch_resample_grad(const float* data, const float* warp, const float* gout, float* ddata, float* dwarp, int B, int N, int C, int H,
                         int W, int mode, int overwrite, void* ws, hipStream_t s);
size_t depth_output_grad_workspace_bytes(int B, int N, int K);
int launch_depth_output_grad(const float* basis, const float* Wc, const float* gout, float* dinit, float* dbasis, float* dWc, int B,
                             int N, int K, int overwrite, void* ws, hipStream_t s);

// ---- grid_prep.hip: a map resampled onto the pixel grids of up to 8 levels, and the adjoint of all of them (no workspace) ----
// both run every check of their C entry (banet_grid_resample[_grad]_f32) before the one launch
int launch_grid_resample(const float* data, int B, int H, int W, int C, int mode, const banet_grid_level_t* levels, int n_levels,
                         hipStream_t s);
int launch_grid_resample_grad(float* ddata, int B, int H, int W, int C, int mode, const banet_grid_level_t* levels, int n_levels,
                              int overwrite, hipStream_t s);

// ---- eqcon.hip -------------------------------------------------------------------------
void launch_reduce(const float* partials, int B, int G, int pstride, int P, float* AtA, float* Atb, hipStream_t s);
struct EqPlan {
  int Gr, tiles, pstride, nb;
  int fast;            // 1: eqcon_syrk.hip (P <= 144): per-pixel records + W^T W on the bf16 pipe
  size_t off_rec;      // fast: the records [B][N][8] inside the workspace
  size_t partial_bytes;
};
size_t eq_syrk_record_bytes(int B, int N);
int launch_eq_syrk(const float* J, const float* G, const float* d, int B, int N, int C, int P, int nb, int Gr, int pstride,
                   float* partials, float* rec, hipStream_t s);
int plan_eq(int B, int N, int C, int P, EqPlan* pl);
int launch_eq(const float* J, const float* G, const float* d, float* AtA, float* Atb, int B, int N, int C, int P,
              const EqPlan& pl, float* partials, hipStream_t s);
size_t eq_grad_fast_ws_bytes(int B, int N, int P);   // eqcon_grad.hip: 0 = no fast path for this shape
int launch_eq_grad_fast(const float* J, const float* G, const float* d, const float* g0, const float* g1, float* gJ, float* gG,
                        float* gd, int B, int N, int C, int P, void* ws, hipStream_t s);
int launch_eq_grad(const float* J, const float* G, const float* d, const float* g0, const float* g1, float* gJ,
                   float* gG, float* gd, int B, int N, int C, int P, hipStream_t s);

// ---- solve.hip (ba_solve_update_kernel, the control kernels) and spd_solve.hip (spd_solve_kernel); plan: solve_plan.hpp, shared
//      device code: solve_common.hpp ----
struct LmCtl {  // per-window loop state of the legacy early-termination LM (device memory)
  int32_t active;
  int32_t pending;
  float avg_prev;
  float uw, ut;
  float Rprev[9];
  float Tprev[3];
  int32_t pad_[3];
};
static_assert(sizeof(LmCtl) == 80, "LmCtl layout");

struct SolveArgs {
  int B, N, C, K, P, variant, pairs;
  float l2_base;
  int max_iters;  // only used with ctl
  banet_mlp_t mlp;
  int use_mlp;
  const float* AtA;
  const float* Atb;
  const float* absres;
  const float* nvalid;
  banet_state_t st;
  LmCtl* ctl;  // nullptr: fixed-count mode (every call performs one update)
  float* bigA; // pl.big: workspace for the normal matrix, B * pl.big_floats floats; else nullptr
  int* queue;  // LM loop: the next gather's tile-queue heads, zeroed by this kernel (saves a memset per iteration)
  int nqueue;  // words per window
  const float* mlp_y;   // [B] lambda-MLP outputs precomputed by the SYRK launch's role workgroups, or nullptr
  banet_lm_params_t lm;   // run-time LM configuration (legacy/ba.py:5-9)
  SolvePlan pl;           // plan_solve(variant, P, C, lm.solver, the level's flags): method, strides, LDS offsets
};
int launch_solve(const SolveArgs& a, hipStream_t s);   // only launches: a.pl accepted by plan_solve, a.bigA given where a.pl.big
int launch_spd_solve(const float* A, const float* rhs, float* x, int B, int P, hipStream_t s);   // plan_spd_solve's codes, then the launch
void launch_ctl_init(LmCtl* ctl, int32_t* iters, int B, hipStream_t s);
void launch_zero_iters(int32_t* iters, int B, hipStream_t s);

// ---- sstats.hip: per-pixel sampling statistics and their adjoint (differentiable layer support) ----
int sample_stats_blocks(int N);
int launch_sample_stats(const float* conv1, const float* conv2, const float* px, const float* py, int B, int N, int C, int H,
                        int W, float* stats, float* absd_part, hipStream_t s);
int launch_sample_stats_grad(const float* conv1, const float* conv2, const float* px, const float* py, int B, int N, int C,
                             int H, int W, const float* dstats, const float* dabs, float* dconv1, float* dconv2, float* dpos,
                             hipStream_t s);

// ---- adjoint.hip (driver; plan: adjoint_plan.hpp, kernels: adjoint_*.hip): backward of the fused dense bundle assembly;
//      the deterministic sample-stats gradient lives in sstats.hip, the target-map fold in adjoint_map.hip ----
size_t dense_adjoint_workspace_bytes(const banet_level_t* lv, int flags = 0);   // flags: BANET_ADJOINT_FOLD_TARGET changes the layout
int launch_dense_adjoint(const banet_level_t* lv, const float* R, const float* T, const float* Wc, const float* gAtA,
                         const float* gAtb, const float* gabs, float* dsrc, float* dmap3, float* ddepth, float* dbasis,
                         float* dpose, int flags, void* ws, hipStream_t s);
size_t sample_stats_grad_det_workspace_bytes(int B, int N, int C, int H, int W);
int launch_sample_stats_grad_det(const float* conv1, const float* conv2, const float* px, const float* py, int B, int N, int C,
                                 int H, int W, const float* dstats, const float* dabs, float* dconv1, float* dconv2, float* dpos,
                                 void* ws, hipStream_t s);
int launch_target_map_adjoint(const float* dmap3, float* dimg, int B, int H, int W, int C, int overwrite, hipStream_t s);

// ---- smallstep.hip: backward of the small part of an iteration (lambda MLP, damping, solve, SE(3) / W update) ----
bool small_step_supported(int variant, int B, int N, int C, int K, int pairs);
size_t small_step_workspace_bytes(int variant, int B, int N, int C, int K, int pairs);
int launch_small_step_adjoint(int variant, int B, int N, int C, int K, int pairs, float l2_base, const banet_mlp_t* mlp, const float* AtA,
                              const float* Atb, const float* absres, const float* delta, const float* R, const float* T, const float* gR,
                              const float* gT, const float* gW, float* gAtA, float* gAtb, float* gabs, float* dR, float* dT,
                              const banet_mlp_t* gmlp, void* ws, hipStream_t s);

// ---- api.hip: one LM level as "validate + plan" and "enqueue" (banet_lm_level_ex_f32 = both; schedule.hip plans every level
// of a schedule before it enqueues the first) ----
struct LevelWs {  // carve of the level workspace
  float* partials;
  float* AtA;
  float* Atb;
  float* absres;
  float* nvalid;
  LmCtl* ctl;
  float* mlp_y;   // [B] lambda-MLP outputs of the SYRK launch's role workgroups
  float* bigA;
  size_t total;
};
struct LevelRun {   // what lm_level_plan decided; host memory only
  const banet_level_t* lv;
  const banet_mlp_t* mlp;
  AsmPlan pl;
  LevelWs w;
  SolveArgs a;
  int max_iters;
  bool lm;     // device-side loop control (BANET_LEGACY_LM with early termination)
  SyrkRole role;   // role.on: the lambda MLP runs as a role workgroup of the SYRK launch, on role.Gs partial rows per window
  PriorRun prior;  // prior.pl.on: one launch_prior_add between assembly and solve of every iteration (lm_level_prior_plan; off otherwise)
  PosePriorRun pose;  // pose.pl.on: one launch_pose_prior_add next to it (lm_level_pose_prior_plan; off otherwise)
};
// every check of banet_lm_level_ex_f32, in its order and with its return codes; launches nothing
int lm_level_plan(const banet_level_t* lv, const banet_mlp_t* mlp, float l2_base, int max_iters, int early_termination,
                  const banet_lm_params_t* params, const banet_state_t* st, void* ws, size_t ws_bytes, LevelRun* run);
int lm_level_enqueue(const LevelRun& run, hipStream_t s);
// the same for banet_lm_level_prior_f32 (early_termination = 0): the level's checks, then the prior's; the prior's regions lie behind
// the level's carve
int lm_level_prior_plan(const banet_level_t* lv, const banet_mlp_t* mlp, float l2_base, int max_iters, const banet_lm_params_t* params,
                        const banet_prior_t* pr, const banet_state_t* st, void* ws, size_t ws_bytes, LevelRun* run);
size_t lm_level_prior_bytes(const banet_level_t* lv, const banet_prior_t* pr);   // the query: 0 = unsupported / invalid
// the same for banet_lm_level_pose_prior_f32: the pose prior's struct checks, lm_level_prior_plan, then the pose prior's plan (no
// workspace of its own)
int lm_level_pose_prior_plan(const banet_level_t* lv, const banet_mlp_t* mlp, float l2_base, int max_iters, const banet_lm_params_t* params,
                             const banet_prior_t* pr, const banet_pose_prior_t* pp, const banet_state_t* st, void* ws, size_t ws_bytes,
                             LevelRun* run);
size_t lm_level_pose_prior_bytes(const banet_level_t* lv, const banet_prior_t* pr, const banet_pose_prior_t* pp);   // 0 = unsupported / invalid

// ---- schedule.hip --------------------------------------------------------------------------
struct TraceRow {   // one level's row of banet_solve_trace_t (nullptr: not recorded) next to the state it is copied from
  banet_state_t from, to;
  int nR, nT, K, P;   // floats per window: R (9 pairs), T (3 pairs), Wc, delta
};
void launch_lm_trace(const TraceRow& row, int B, hipStream_t s);

}  // namespace banet
