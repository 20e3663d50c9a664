// The depth-basis blocks of the normal equations on gfx950 -- the driver.  Several kernels compute the same sums
//   H_dd = sum_n s_n b_n b_n^T, H_cd = sum_n u_n b_n^T, Atb_d = sum_n r_n b_n
// from the basis [N,K] and the per-pixel records (u, s, r) of the gather:
//   syrk_bf16x6.hip  ba_syrk_bf16x6_kernel  the product path for K = 64 / 128 and <= 4 target frames (+ the lambda-MLP role);
//   syrk_wide.hip    slice / rect jobs      the same scheme for K = 256 and more frames;
//   syrk_mfma32.hip  ba_syrk_direct_kernel  the fp32-MFMA predecessor, kept for A/B (kDevSyrkNoBf16x6);
//   syrk_lds.hip     ba_syrk_kernel<NB>     LDS-tiled fp32 MFMA, any K <= 256 (the remaining basis sizes);
//   syrk_stats.hip   the pre-passes (column / record maxima of the fp16 two-piece form, per-pixel sums over the frames);
//   syrk_reduce.hip  ba_reduce2_kernel      partial rows -> AtA / Atb.
// Which of them a pass runs, in what order, on what grid and with how much LDS is plan_syrk_steps' list (plan.hpp); this file
// fills the argument blocks and walks it.
#include "syrk_common.hpp"

namespace banet {

int launch_syrk(const float* basis, const float* rec, int B, int N, int K, int pairs, const SyrkPlan& pl, const int32_t* active,
                int active_stride, float* partials, hipStream_t s, const SyrkRole& role, const MlpRole* mr, SyrkStats stats) {
  SyrkSteps steps;
  int rc = plan_syrk_steps(pl, B, N, K, pairs, num_cus(), stats, role, &steps);
  if (rc != BANET_OK) return rc;
  // the scales of the fp16 form and the wide jobs' sums lie behind the partial rows (plan_syrk); the kernels of a step that does
  // not use them never look at the pointers
  const char* base = reinterpret_cast<const char*>(partials);
  const float* colmax = reinterpret_cast<const float*>(base + pl.off_colmax);
  const float* recmax = reinterpret_cast<const float*>(base + pl.off_recmax);
  const SyrkArgs a{basis, rec, active, active_stride, partials, N, K, role.Gs, pl.tiles, pl.pstride, pairs, 0,
                   mr != nullptr ? *mr : MlpRole{}, colmax, recmax};
  WideArgs w{basis, rec, nullptr, active, active_stride, partials, N, K, role.Gs, pl.pstride, pairs, 0, 0, 0, 0, colmax, recmax};
  for (int i = 0; i < steps.n && rc == BANET_OK; ++i) {
    const SyrkStep& step = steps.step[i];
    switch (step.kind) {
      case kSyrkStepSrsum:
        w.srsum = reinterpret_cast<const float*>(base + pl.off_aux);   // written now; the jobs then read it, not the only frame's records
        [[fallthrough]];
      case kSyrkStepZero:
      case kSyrkStepColmax:
      case kSyrkStepRecmax: rc = launch_syrk_stats_step(step, w, s); break;
      case kSyrkStepLds: rc = launch_syrk_lds_step(step, a, s); break;
      case kSyrkStepMfma32: rc = launch_syrk_mfma32_step(step, a, s); break;
      case kSyrkStepBf16x6: rc = launch_syrk_bf16x6_step(step, a, s); break;
      case kSyrkStepSlice:
      case kSyrkStepRect: rc = launch_syrk_wide_step(step, w, s); break;
      default: rc = BANET_ERR_UNSUPPORTED;
    }
  }
  if (rc != BANET_OK) return rc;
  return hipGetLastError() == hipSuccess ? BANET_OK : BANET_ERR_LAUNCH;
}

}  // namespace banet
