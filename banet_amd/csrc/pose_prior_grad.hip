// The backward of the pose prior (include/banet_hip.h (5g); plan: pose_prior_grad_plan.hpp; forward: pose_prior.hip).  With
// G = gAtA'[0:m, 0:m] (raw, row stride P) and g = gAtb'[0:m] the gradients of the post-prior matrices, r, Jr = blockdiag Jr_i,
// Lambda and s = scale the forward's quantities (gAtA' / gAtb' themselves pass through to the dense adjoint, unchanged):
//   y = Jr g     A = Jr G     X = Lambda Jr     Xt = Lambda^T Jr     u = Lambda r
//   gLambda = s (A Jr^T - y r^T)        gscale = <A, X> - <y, u>        gr = -s Lambda^T y
//   gJr_i   = s (X G^T + Xt G)[block i] - s u_i g_i^T
//   (gR_i, gT_i, gR0_i, gT0_i) = (d(r_i, Jr_i) / d(R_i, T_i, R0_i, T0_i))^T (gr_i, gJr_i)
// One launch per iteration, one workgroup of four waves per window whatever pairs and K are, no workspace, no atomics:
//   0. all threads stage Lambda, G and g in LDS; thread i < pairs recomputes r_i and Jr_i with the forward's own function
//      (pose_prior_common.hpp, S = float): the bits the forward added
//   1. A, X, Xt, y (6-term fma chains: Jr is block diagonal) and u (an m-term chain per row)
//   2. gLambda (6-term chains over A Jr^T, then the rank-one term), gr and the 36 pairs entries of gJr (m-term chains) into LDS,
//      gscale (one float64 fma chain per thread, then a fixed tree over the 256 threads)
//   3. forward mode: lane (i, d), d < 24 (R 9, T 3, R0 9, T0 3), runs the forward chain over a value-plus-tangent scalar
//      (S = PoseDual) along its entry, contracts the tangent of (r_i, Jr_i) with (gr_i, gJr_i) in one fixed 42-term chain and owns
//      one output element.  All lanes run one instruction stream; the 24-fold redundant arithmetic sits in lanes that would idle.
// Every output element is written by exactly one lane; every summation order is a function of pairs alone: a window's bits are the
// same alone and in any batch, and an output's bits do not depend on which other outputs are asked for.
#include "kernels.hpp"
#include "pose_prior_common.hpp"

namespace banet {

constexpr int kPoseGradM = 6 * kPosePriorPairsMax;

struct PosePriorGradArgs {
  int pairs, m, P, work, lanes, ow_state, ow_prior;
  float scale;
  const float* R;        // [B][pairs][3][3] the state's
  const float* T;        // [B][pairs][3]
  const float* R0;       // [B][pairs][3][3] the prior's
  const float* T0;       // [B][pairs][3]
  const float* Lambda;   // [B][m][m]
  const float* gAtA;     // [B][P][P]
  const float* gAtb;     // [B][P]
  float* gR;             // [B][pairs][3][3]   (each output or nullptr)
  float* gT;             // [B][pairs][3]
  float* gR0;
  float* gT0;
  float* gLambda;        // [B][m][m]
  float* gscale;         // [B]
};

__global__ __launch_bounds__(kPosePriorGradThreads) void ba_pose_prior_grad_kernel(const PosePriorGradArgs a) {
  __shared__ float sL[kPoseGradM * kPoseGradM];    // Lambda [m][m]
  __shared__ float sG[kPoseGradM * kPoseGradM];    // G [m][m]
  __shared__ float sA[kPoseGradM * kPoseGradM];    // Jr G
  __shared__ float sX[kPoseGradM * kPoseGradM];    // Lambda Jr
  __shared__ float sXt[kPoseGradM * kPoseGradM];   // Lambda^T Jr
  __shared__ float sJ[kPosePriorPairsMax * 36];    // Jr_i [6][6]
  __shared__ float sgJ[kPosePriorPairsMax * 36];   // gJr_i [6][6]
  __shared__ float sr[kPoseGradM], su[kPoseGradM], sy[kPoseGradM], sg[kPoseGradM], sgr[kPoseGradM];
  __shared__ double sred[kPosePriorGradThreads];
  constexpr int NT = kPosePriorGradThreads;
  const int tid = threadIdx.x, m = a.m, mm = m * m, pairs = a.pairs, work = a.work;
  const size_t b = blockIdx.x;
  const float s = a.scale;
  // ---- phase 0
  {
    const float* __restrict__ Lam = a.Lambda + b * mm;
    const float* __restrict__ GA = a.gAtA + b * a.P * a.P;
    const float* __restrict__ gb = a.gAtb + b * a.P;
    for (int idx = tid; idx < mm; idx += NT) {
      const int k = idx / m, l = idx - k * m;
      sL[idx] = Lam[idx];
      sG[idx] = GA[(size_t)k * a.P + l];
    }
    if (tid >= NT - m) sg[tid - (NT - m)] = gb[tid - (NT - m)];   // (the last wave: the first computes the poses)
    if (tid < pairs) {
      const size_t p = b * pairs + tid;
      pose_log_jr<float>(a.R + 9 * p, a.T + 3 * p, a.R0 + 9 * p, a.T0 + 3 * p, sr + 6 * tid, sJ + 36 * tid);
    }
  }
  __syncthreads();
  // ---- phase 1
  //   A[6 i + p][col] = sum_e Jr_i[p][e] G[6 i + e][col]                 y[6 i + p] = sum_e Jr_i[p][e] g[6 i + e]
  //   X[k][6 j + q]   = sum_e Lambda[k][6 j + e] Jr_j[e][q]              u[k]       = sum_l Lambda[k][l] r[l]
  //   Xt[k][6 j + q]  = sum_e Lambda[6 j + e][k] Jr_j[e][q]
  for (int idx = tid; idx < mm; idx += NT) {
    const int k = idx / m, col = idx - k * m, j = col / 6, q = col - 6 * j;
    if (work & kPoseGradA) {
      const int i = k / 6, p = k - 6 * i;
      const float* jr = sJ + 36 * i + 6 * p;
      const float* x = sG + 6 * i * m + col;
      float acc = 0.f;
#pragma unroll
      for (int e = 0; e < 6; ++e) acc = fmaf(jr[e], x[e * m], acc);
      sA[idx] = acc;
    }
    const float* jr = sJ + 36 * j + q;
    if (work & kPoseGradX) {
      const float* l = sL + k * m + 6 * j;
      float acc = 0.f;
#pragma unroll
      for (int e = 0; e < 6; ++e) acc = fmaf(l[e], jr[6 * e], acc);
      sX[idx] = acc;
    }
    if (work & kPoseGradXt) {
      const float* l = sL + 6 * j * m + k;
      float acc = 0.f;
#pragma unroll
      for (int e = 0; e < 6; ++e) acc = fmaf(l[e * m], jr[6 * e], acc);
      sXt[idx] = acc;
    }
  }
  if (tid < m) {
    const int i = tid / 6, p = tid - 6 * i;
    const float* jr = sJ + 36 * i + 6 * p;
    float acc = 0.f;
#pragma unroll
    for (int e = 0; e < 6; ++e) acc = fmaf(jr[e], sg[6 * i + e], acc);
    sy[tid] = acc;
  } else if (tid >= NT - m && (work & kPoseGradX)) {
    const int k = tid - (NT - m);
    float acc = 0.f;
    for (int l = 0; l < m; ++l) acc = fmaf(sL[k * m + l], sr[l], acc);
    su[k] = acc;
  }
  __syncthreads();
  // ---- phase 2
  if (work & kPoseGradLambda) {   // gLambda[k][6 j + q] = s (sum_e A[k][6 j + e] Jr_j[q][e] - y[k] r[6 j + q])
    float* __restrict__ gL = a.gLambda + b * mm;
    for (int idx = tid; idx < mm; idx += NT) {
      const int k = idx / m, l = idx - k * m, j = l / 6, q = l - 6 * j;
      const float* x = sA + k * m + 6 * j;
      const float* jr = sJ + 36 * j + 6 * q;
      float acc = 0.f;
#pragma unroll
      for (int e = 0; e < 6; ++e) acc = fmaf(x[e], jr[e], acc);
      acc = fmaf(-sy[k], sr[l], acc);
      const float v = __fmul_rn(s, acc);
      gL[idx] = a.ow_prior ? v : __fadd_rn(gL[idx], v);
    }
  }
  if (work & kPoseGradPose) {
    // gr[l] = -s sum_k Lambda[k][l] y[k];   gJr_i[p][q] = s (sum_c X[6i+p][c] G[6i+q][c] + sum_c Xt[6i+p][c] G[c][6i+q] - u[6i+p] g[6i+q])
    const int nj = 36 * pairs;
    for (int idx = tid; idx < nj + m; idx += NT) {
      if (idx < nj) {
        const int i = idx / 36, e = idx - 36 * i, p = e / 6, q = e - 6 * p;
        const float* x = sX + (6 * i + p) * m;
        const float* xt = sXt + (6 * i + p) * m;
        const float* gr = sG + (6 * i + q) * m;
        const float* gc = sG + 6 * i + q;
        float acc = 0.f;
        for (int c = 0; c < m; ++c) acc = fmaf(x[c], gr[c], acc);
        for (int c = 0; c < m; ++c) acc = fmaf(xt[c], gc[c * m], acc);
        acc = fmaf(-su[6 * i + p], sg[6 * i + q], acc);
        sgJ[idx] = __fmul_rn(s, acc);
      } else {
        const int l = idx - nj;
        float acc = 0.f;
        for (int k = 0; k < m; ++k) acc = fmaf(sL[k * m + l], sy[k], acc);
        sgr[l] = -__fmul_rn(s, acc);
      }
    }
  }
  if (work & kPoseGradScale) {   // <A, X> - <y, u>: float64 on the float32 values, one chain per thread, then a fixed tree
    double acc = 0.0;
    for (int idx = tid; idx < mm; idx += NT) acc = fma((double)sA[idx], (double)sX[idx], acc);
    if (tid < m) acc = fma(-(double)sy[tid], (double)su[tid], acc);
    sred[tid] = acc;
    __syncthreads();
    for (int off = NT / 2; off > 0; off >>= 1) {
      if (tid < off) sred[tid] += sred[tid + off];
      __syncthreads();
    }
    if (tid == 0) a.gscale[b] = a.ow_prior ? (float)sred[0] : __fadd_rn(a.gscale[b], (float)sred[0]);
  }
  if (!(work & kPoseGradPose)) return;
  __syncthreads();
  // ---- phase 3
  if (tid >= a.lanes) return;
  const int i = tid / kPosePriorGradEntries, d = tid - kPosePriorGradEntries * i;
  const size_t p = b * pairs + i;
  PoseDual in[kPosePriorGradEntries];
#pragma unroll
  for (int e = 0; e < 9; ++e) in[e] = {a.R[9 * p + e], e == d ? 1.f : 0.f};
#pragma unroll
  for (int e = 0; e < 3; ++e) in[9 + e] = {a.T[3 * p + e], 9 + e == d ? 1.f : 0.f};
#pragma unroll
  for (int e = 0; e < 9; ++e) in[12 + e] = {a.R0[9 * p + e], 12 + e == d ? 1.f : 0.f};
#pragma unroll
  for (int e = 0; e < 3; ++e) in[21 + e] = {a.T0[3 * p + e], 21 + e == d ? 1.f : 0.f};
  PoseDual r[6], Jr[36];
  pose_log_jr<PoseDual>(in, in + 9, in + 12, in + 21, r, Jr);
  float acc = 0.f;
#pragma unroll
  for (int e = 0; e < 6; ++e) acc = fmaf(sgr[6 * i + e], r[e].t, acc);
#pragma unroll
  for (int e = 0; e < 36; ++e) acc = fmaf(sgJ[36 * i + e], Jr[e].t, acc);
  float* out;
  bool ow;
  if (d < 9) out = a.gR ? a.gR + 9 * p + d : nullptr, ow = a.ow_state;
  else if (d < 12) out = a.gT ? a.gT + 3 * p + (d - 9) : nullptr, ow = a.ow_state;
  else if (d < 21) out = a.gR0 ? a.gR0 + 9 * p + (d - 12) : nullptr, ow = a.ow_prior;
  else out = a.gT0 ? a.gT0 + 3 * p + (d - 21) : nullptr, ow = a.ow_prior;
  if (out) *out = ow ? acc : __fadd_rn(*out, acc);
}

int launch_pose_prior_grad(const PosePriorGradPlan& pl, const banet_pose_prior_t& pp, const float* R, const float* T, const float* gAtA,
                           const float* gAtb, const banet_pose_prior_grad_t& out, hipStream_t s) {
  if (!pl.on) return BANET_ERR_INVALID_ARG;
  PosePriorGradArgs a;
  a.pairs = pl.pairs;
  a.m = pl.m;
  a.P = pl.P;
  a.work = pl.work;
  a.lanes = pl.lanes;
  a.ow_state = pl.overwrite_state;
  a.ow_prior = pl.overwrite_prior;
  a.scale = pp.scale;
  a.R = R;
  a.T = T;
  a.R0 = pp.R0;
  a.T0 = pp.T0;
  a.Lambda = pp.Lambda;
  a.gAtA = gAtA;
  a.gAtb = gAtb;
  a.gR = out.gR;
  a.gT = out.gT;
  a.gR0 = out.gR0;
  a.gT0 = out.gT0;
  a.gLambda = out.gLambda;
  a.gscale = out.gscale;
  hipLaunchKernelGGL(ba_pose_prior_grad_kernel, dim3(pl.grid), dim3(kPosePriorGradThreads), 0, s, a);
  if (hipGetLastError() != hipSuccess) return BANET_ERR_LAUNCH;
  return BANET_OK;
}

}  // namespace banet
