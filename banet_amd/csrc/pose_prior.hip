// The pose prior inside the LM loop (include/banet_hip.h (5f); plan: pose_prior_plan.hpp).  The update convention is the solve's
// (solve.hip; oracle _se3_update): delta = [w; t], R' = exp(w) R, T' = V(w) t + exp(w) T, i.e. T' = Exp(delta) o T with
// Exp([phi; rho]) = (exp(phi), V(phi) rho) -- a left perturbation, the tangent banet_ba_marginals_f32's pose_cov is expressed in.
// Per window, with prior poses (R0_i, T0_i), i < pairs, and a joint information matrix Lambda [m][m], m = 6 pairs:
//   E_i = T_i o T0_i^-1:  Re = R_i R0_i^T,  te = T_i - Re T0_i         r_i = Log(E_i) = [phi; rho],  rho = V(phi)^-1 te
//   Jr  = blockdiag_i J_l(r_i)^-1,   J_l^-1 = [[J^-1, 0], [-J^-1 Q J^-1, J^-1]],   J = V(phi),   Q: Barfoot's Q(rho, phi)
//   AtA[0:m, 0:m] += scale Jr^T Lambda Jr         Atb[0:m] -= scale Jr^T Lambda r                     (Gauss-Newton; row stride P)
// between launch_assemble and launch_solve of every iteration, before the damping.  No workspace, no once-per-level pass: r and Jr
// change with the state.  One workgroup of four waves per window, whatever the shape:
//   1. all threads stage Lambda in LDS; thread i < pairs computes r_i and the 6 x 6 block Jr_i into LDS
//   2. M = Lambda Jr (6-term fma chains) and u = Lambda r (one m-term chain per row) into LDS
//   3. H = Jr^T M and v = Jr^T u (6-term chains); one lane per element read-modify-writes AtA and Atb (4-byte accesses: a row of
//      AtA has stride P)
// No atomics; every output element is written by exactly one lane; every summation order is a function of pairs alone, never of B:
// a window's bits are the same alone and in any batch.  At R = R0, T = T0 with Re = I exactly: phi = 0, Jr = I and r = 0 exactly,
// so the block gets fl(scale Lambda) and Atb keeps its bits.
#include "kernels.hpp"
#include "pose_prior_common.hpp"   // the forward chain r_i, Jr_i (shared with pose_prior_grad.hip)

namespace banet {

constexpr int kPosePriorM = 6 * kPosePriorPairsMax;
struct PosePriorArgs {
  int pairs, m, P;
  float scale;
  const float* R;        // [B][pairs][3][3] the state's
  const float* T;        // [B][pairs][3]
  const float* R0;       // [B][pairs][3][3] the prior's
  const float* T0;       // [B][pairs][3]
  const float* Lambda;   // [B][m][m]
  float* AtA;            // [B][P][P]
  float* Atb;            // [B][P]
};

__global__ __launch_bounds__(kPosePriorThreads) void ba_pose_prior_add_kernel(const PosePriorArgs a) {
  __shared__ float sL[kPosePriorM * kPosePriorM];   // Lambda [m][m]
  __shared__ float sM[kPosePriorM * kPosePriorM];   // Lambda Jr [m][m]
  __shared__ float sJ[kPosePriorPairsMax * 36];     // Jr_i [6][6]
  __shared__ float sr[kPosePriorM], su[kPosePriorM];
  const int tid = threadIdx.x, m = a.m, mm = m * m, pairs = a.pairs;
  const size_t b = blockIdx.x;
  const float* __restrict__ Lam = a.Lambda + b * mm;
  for (int idx = tid; idx < mm; idx += kPosePriorThreads) sL[idx] = Lam[idx];
  if (tid < pairs) {
    const size_t p = b * pairs + tid;
    pose_log_jr(a.R + 9 * p, a.T + 3 * p, a.R0 + 9 * p, a.T0 + 3 * p, sr + 6 * tid, sJ + 36 * tid);
  }
  __syncthreads();
  // M[k][6 j + q] = sum_e Lambda[k][6 j + e] Jr_j[e][q];   u[k] = sum_l Lambda[k][l] r[l]
  for (int idx = tid; idx < mm + m; idx += kPosePriorThreads) {
    if (idx < mm) {
      const int k = idx / m, col = idx - k * m, j = col / 6, q = col - 6 * j;
      const float* l = sL + k * m + 6 * j;
      const float* jr = sJ + 36 * j + q;
      float acc = 0.f;
#pragma unroll
      for (int e = 0; e < 6; ++e) acc = fmaf(l[e], jr[6 * e], acc);
      sM[idx] = acc;
    } else {
      const int k = idx - mm;
      float acc = 0.f;
      for (int l = 0; l < m; ++l) acc = fmaf(sL[k * m + l], sr[l], acc);
      su[k] = acc;
    }
  }
  __syncthreads();
  // H[6 i + q][col] = sum_e Jr_i[e][q] M[6 i + e][col];   v[6 i + q] = sum_e Jr_i[e][q] u[6 i + e]
  float* __restrict__ A = a.AtA + b * a.P * a.P;
  float* __restrict__ tb = a.Atb + b * a.P;
  for (int idx = tid; idx < mm + m; idx += kPosePriorThreads) {
    const bool mat = idx < mm;
    const int row = mat ? idx / m : idx - mm, col = mat ? idx - row * m : 0;
    const int i = row / 6, q = row - 6 * i;
    const float* jr = sJ + 36 * i + q;
    const float* x = mat ? sM + 6 * i * m + col : su + 6 * i;
    const int xs = mat ? m : 1;
    float acc = 0.f;
#pragma unroll
    for (int e = 0; e < 6; ++e) acc = fmaf(jr[6 * e], x[e * xs], acc);
    const float add = __fmul_rn(a.scale, acc);
    if (mat) A[(size_t)row * a.P + col] = __fadd_rn(A[(size_t)row * a.P + col], add);
    else tb[row] = __fsub_rn(tb[row], add);
  }
}

int launch_pose_prior_add(const PosePriorRun& run, const float* R, const float* T, float* AtA, float* Atb, hipStream_t s) {
  const PosePriorPlan& pl = run.pl;
  if (!pl.on) return BANET_OK;
  PosePriorArgs a;
  a.pairs = pl.pairs;
  a.m = pl.m;
  a.P = pl.P;
  a.scale = run.pp.scale;
  a.R = R;
  a.T = T;
  a.R0 = run.pp.R0;
  a.T0 = run.pp.T0;
  a.Lambda = run.pp.Lambda;
  a.AtA = AtA;
  a.Atb = Atb;
  hipLaunchKernelGGL(ba_pose_prior_add_kernel, dim3(pl.grid), dim3(kPosePriorThreads), 0, s, a);
  if (hipGetLastError() != hipSuccess) return BANET_ERR_LAUNCH;
  return BANET_OK;
}

}  // namespace banet

using namespace banet;

extern "C" {

int banet_pose_prior_apply_f32(const banet_level_t* lv, const banet_pose_prior_t* pp, const float* R, const float* T, float* AtA,
                               float* Atb, banet_stream_t stream) {
  if (!lv || !R || !T || !AtA || !Atb) return BANET_ERR_INVALID_ARG;
  PosePriorRun run{};
  const int rc = plan_pose_prior(lv, pp, &run.pl);
  if (rc != BANET_OK) return rc;
  if (!run.pl.on) return BANET_OK;   // the empty prior: nothing is launched
  run.pp = *pp;
  return launch_pose_prior_add(run, R, T, AtA, Atb, static_cast<hipStream_t>(stream));
}

}  // extern "C"
