// banet_spd_solve_f32: x = A^-1 b for B symmetric positive definite systems (32 <= P <= ~190), the blocked LDL^T of the
// update kernel (solve_common.hpp) as an op of its own.  Used by the backward of the dense layer (banet_amd/dense_train.py, and
// smallstep.hip): the forward solution of the damped system is recomputed and the implicit-function gradient lam = A^-T g is a
// second call with the same matrix -- torch.linalg.solve costs ~2 ms per iteration there (rocSOLVER getrf + per-item trsv launches).
// Layout and limits: plan_spd_solve (solve_plan.hpp).
#include "solve_common.hpp"

namespace banet {

__global__ __launch_bounds__(kSolveThreads) void spd_solve_kernel(const float* __restrict__ A, const float* __restrict__ rhs,
                                                                  float* __restrict__ x, const SolvePlan pl) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int P = pl.P, ld = pl.ld;
  float* sA = smem;                                   // [P + 4][ld], right-hand side as row P
  float* sX = smem + pl.off_X;                        // [P + 8]
  float* sScr = smem + pl.off_Part;                   // [solve_scratch_floats(P)]
  const float* A_g = A + (size_t)b * P * P;
  for (int e = tid; e < P * P; e += kSolveThreads) {
    const int i = e / P, j = e - i * P;
    sA[i * ld + j] = A_g[e];
  }
  for (int i = tid; i < P; i += kSolveThreads) sA[P * ld + i] = rhs[(size_t)b * P + i];
  __syncthreads();
  ldlt_solve_blocked(smem, ld, pl.ldw, P, sX, sScr);
  for (int k = tid; k < P; k += kSolveThreads) x[(size_t)b * P + k] = sX[k];
}

int launch_spd_solve(const float* A, const float* rhs, float* x, int B, int P, hipStream_t s) {
  SolvePlan pl;
  const int rc = plan_spd_solve(P, &pl);
  if (rc != BANET_OK) return rc;
  if (pl.lds_attr)
    (void)hipFuncSetAttribute((const void*)spd_solve_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds);
  hipLaunchKernelGGL(spd_solve_kernel, dim3(B), dim3(kSolveThreads), pl.lds, s, A, rhs, x, pl);
  return hipGetLastError() == hipSuccess ? BANET_OK : BANET_ERR_LAUNCH;
}

}  // namespace banet
