// The HBM-bound half of one BA assembly pass on gfx950 -- the driver.  Five kernels compute the same per-pixel sums (the arithmetic:
// gather_generic.hip) and leave the same partial rows and per-pixel records:
//   gather_generic.hip  ba_gather_kernel      any C <= 256, K <= 256, sparse points, the [f|gx|gy] target layout;
//   gather128.hip       ba_gather128_kernel   C = 128, direct loads, dynamic tile queue;
//   gather128p.hip      ba_gather128p_kernel  C = 128, wave-private LDS patches (large levels);
//   gather128s.hip      ba_gather128s_kernel  C = 128, strip segments with a rolling LDS window;
//   gather128q.hip      ba_gather128q_kernel  C = 128, 4x4-pixel items (latency-bound launches).
// Which of them a pass runs, on what grid, with how much LDS, and the zeroing / fold launches around it is plan_gather_steps' list
// (plan.hpp); this file fills the argument block and walks it.
#include "gather_common.hpp"

namespace banet {

// sum kFoldRows consecutive partial rows (fixed order) -> one row
__global__ __launch_bounds__(256) void ba_fold_kernel(const float* __restrict__ in, int rows, int stride,
                                                      float* __restrict__ out, int frows, const int32_t* active,
                                                      int active_stride, int pairs) {
  const int b = blockIdx.y, c = blockIdx.x, e = threadIdx.x;   // b = virtual window
  if (active != nullptr && active[(size_t)(b / pairs) * active_stride] == 0) return;
  if (e >= stride) return;
  const int r0 = c * kFoldRows, r1 = min(rows, r0 + kFoldRows);
  const float* p = in + ((size_t)b * rows + r0) * stride + e;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  int i = 0;
  const int n = r1 - r0;
  for (; i + 3 < n; i += 4) {
    s0 += p[(size_t)(i + 0) * stride];
    s1 += p[(size_t)(i + 1) * stride];
    s2 += p[(size_t)(i + 2) * stride];
    s3 += p[(size_t)(i + 3) * stride];
  }
  for (; i < n; ++i) s0 += p[(size_t)i * stride];
  out[((size_t)b * frows + c) * stride + e] = (s0 + s1) + (s2 + s3);
}

// The three seams launch_assemble brackets with its ranges and timer; each enqueues its steps of the one list.

void prepare_gather(const GatherSteps& steps, const GatherPlan& pl, float* partials, hipStream_t s) {
  // zeroed by a kernel, not hipMemsetAsync: a captured HIP graph holding the memset node faulted on its second replay
  // (ROCm 7.2; tests/test_gpu_parity.py::test_solve_is_hip_graph_capturable)
  for (int i = 0; i < steps.n; ++i)
    if (steps.step[i].kind == kGatherStepZero)
      launch_zero_iters(reinterpret_cast<int32_t*>(reinterpret_cast<char*>(partials) + pl.off_queue), steps.step[i].t0, s);
}

int launch_gather(const GatherSteps& steps, const banet_level_t* lv, const GatherPlan& pl, const float* R, const float* T, const float* Wc,
                  const int32_t* active, int active_stride, float* rec, float* partials, hipStream_t s, unsigned char* mask_out) {
  GatherArgs a;
  a.lv = *lv;
  a.R = R;
  a.T = T;
  a.Wc = Wc;
  a.active = active;
  a.active_stride = active_stride;
  a.rec = rec;
  a.partials = partials;
  a.G = pl.G;
  a.tiles = pl.tiles;
  a.tile_pts = pl.tile_pts;
  a.tiles_x = pl.tiles_x;
  a.tiles_y = pl.tiles_y;
  a.groups = pl.groups;
  a.queue = reinterpret_cast<int*>(reinterpret_cast<char*>(partials) + pl.off_queue);
  a.nbands = pl.nbands;
  a.pairs = npairs(lv);
  a.qshift = pl.qshift;
  a.pairloop = pl.pairloop;
  a.seg_h = pl.strip;
  a.strip_fp = pl.strip_fp;
  a.mask_out = mask_out;
  int rc = BANET_OK;
  for (int i = 0; i < steps.n && rc == BANET_OK; ++i) {
    const GatherStep& step = steps.step[i];
    switch (step.kind) {
      case kGatherStepGeneric: rc = launch_gather_generic_step(step, a, s); break;
      case kGatherStepDirect: rc = launch_gather128_step(step, a, s); break;
      case kGatherStepPatch: rc = launch_gather128p_step(step, a, s); break;
      case kGatherStepStrip: rc = launch_gather128s_step(step, a, s); break;
      case kGatherStepQuad: rc = launch_gather128q_step(step, a, s); break;
      default: break;   // the zeroing and the fold: the other two seams
    }
  }
  if (rc != BANET_OK) return rc;
  return hipGetLastError() == hipSuccess ? BANET_OK : BANET_ERR_LAUNCH;
}

const float* finish_gather(const GatherSteps& steps, const banet_level_t* lv, const GatherPlan& pl, const int32_t* active,
                           int active_stride, float* partials, hipStream_t s) {
  const float* red = partials;
  for (int i = 0; i < steps.n; ++i) {
    const GatherStep& step = steps.step[i];
    if (step.kind != kGatherStepFold) continue;
    float* out = reinterpret_cast<float*>(reinterpret_cast<char*>(partials) + pl.off_fold);
    hipLaunchKernelGGL(ba_fold_kernel, dim3(step.gx, step.gy), dim3(step.block), step.lds, s, partials, pl.rows, pl.pstride, out,
                       pl.frows, active, active_stride, npairs(lv));
    red = out;
  }
  return red;
}

}  // namespace banet
