// Posterior marginals of a level (banet_ba_marginals_f32): from the normal matrix AtA [B,P,P] of a window, damping mu and noise
// level sigma^2,  H = AtA + mu diag(diag(AtA) + 1e-5) = L L^T,  Sigma = sigma^2 H^-1:
//   (a) marg_factor_kernel   one workgroup per window, latency-bound: Cholesky in place, then Y = L^-1 in place (column sweep of
//       the forward substitution L Y = I).  The first 6 pairs columns of Y give pose_cov = sigma^2 Y_p^T Y_p; the trailing K x K
//       block of Y is T = L_WW^-1 (the depth block comes last, so marginalising the poses costs nothing), Sigma_WW = sigma^2 T^T T.
//       The factorisation runs in float64 on the float32 inputs and rounds its outputs once: a float32 Cholesky loses
//       cond(H) 2^-24 of every output (3e-3 on the tests' kappa = 1e6 ladder), where the tests' yardstick -- numpy's Cholesky,
//       which factorises a float32 matrix in double -- stays at 1e-6.  The kernel is a chain of P dependent steps either way.
//   (b) marg_depthvar_kernel the pass over the basis [B,N,K]: depth_var[n] = sigma^2 |T basis[n,:]|^2 on the f32-input MFMA
//       (v_mfma_f32_32x32x2_f32: an exact float32 fma chain), y = T b never leaves the accumulators.
// No atomics; nothing depends on B: a window's bits are the same alone and in any batch.
#include "marginals_common.hpp"   // the factorisation and y = T b, shared with marginals_grad.hip

namespace banet {

int plan_marginals(const banet_level_t* lv, int want_depth_var, MargPlan* pl) {
  if (!lv || lv->B < 1 || lv->K < 0 || lv->pairs < 0) return BANET_ERR_INVALID_ARG;
  const int m = 6 * npairs(lv), K = lv->K;
  const long long P = (long long)m + K;
  if (K > kMargKMax || P > kMargPMax) return BANET_ERR_UNSUPPORTED;
  pl->P = (int)P;
  pl->m = m;
  pl->K = K;
  // the packed lower triangle and two vectors, in doubles: in LDS up to P = 199
  const size_t mat = (size_t)pl->P * (pl->P + 1) / 2 * sizeof(double), vecs = 2 * (size_t)pl->P * sizeof(double);
  pl->big = mat + vecs > kMargLdsMax;
  pl->lds = pl->big ? vecs : mat + vecs;
  Arena ar;
  pl->off_T = ar.take(want_depth_var && K > 0 ? (size_t)lv->B * K * K * sizeof(float) : 0);
  pl->off_big = ar.take(pl->big ? (size_t)lv->B * mat : 0);
  pl->bytes = ar.off < 256 ? 256 : ar.off;      // never 0 for a supported shape: 0 is the query's "unsupported"
  return BANET_OK;
}

struct MargArgs {
  int P, m, K;
  const float* AtA;
  const float* damping;
  const float* sigma2;
  float* pose_cov;
  float* wfactor;
  float* logdet;
  int32_t* status;
  float* T;      // [B][K][K] in the workspace for (b), or nullptr
  double* big;   // [B][P (P + 1) / 2] in the workspace when the matrix does not fit the LDS
};

// ---- (a) ------------------------------------------------------------------------------------------------------------------------
template <bool BIG>
__global__ __launch_bounds__(kMargThreads) void marg_factor_kernel(const MargArgs a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int b = blockIdx.x, tid = threadIdx.x, tx = tid & (kMargCols - 1), ty = tid / kMargCols;
  const int P = a.P, m = a.m, K = a.K;
  const size_t mat = (size_t)P * (P + 1) / 2;
  double* M = BIG ? a.big + (size_t)b * mat : smem;       // packed lower triangle: H, then L (diagonal in `diag`), then Y = L^-1
  double* colbuf = BIG ? smem : smem + mat;               // [P] the current column
  double* diag = colbuf + P;                              // [P] L_jj
  const float* A = a.AtA + (size_t)b * P * P;
  const double mu = a.damping ? (double)a.damping[b] : 0.0;
  const double s2 = a.sigma2 ? (double)a.sigma2[b] : 1.0;
  float* cov = a.pose_cov + (size_t)b * m * m;
  float* wf = a.wfactor ? a.wfactor + (size_t)b * K * K : nullptr;
  float* Tw = a.T ? a.T + (size_t)b * K * K : nullptr;

  const bool ok = marg_cholesky(A, mu, P, M, colbuf, diag);   // H into M, then L in place; uniform

  if (!ok) {
    for (int idx = tid; idx < m * m; idx += kMargThreads) cov[idx] = (idx / m == idx % m) ? __builtin_huge_valf() : 0.f;
    if (wf)
      for (int idx = tid; idx < K * K; idx += kMargThreads) wf[idx] = 0.f;
    if (tid == 0) {
      if (a.logdet) a.logdet[b] = -__builtin_huge_valf();
      a.status[b] = 1;
    }
    return;                                               // (b) reads status and writes +inf; it does not read T
  }

  // log det H = 2 sum log L_jj (first wave, fixed order)
  if (a.logdet && tid < 64) {
    double s = 0.0;
    for (int j = tid; j < P; j += 64) s += log(diag[j]);
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) s += __shfl_xor(s, sh, 64);
    if (tid == 0) a.logdet[b] = (float)(2.0 * s);
  }

  marg_invert_lower(P, M, colbuf, diag);   // Y = L^-1 in place

  // T = the trailing K x K block of Y, strict upper triangle as zeros; rounded to float32 once
  if (wf || Tw)
    for (int r = ty; r < K; r += kMargRows)
      for (int c = tx; c < K; c += kMargCols) {
        const float v = c <= r ? (float)M[tri(m + r) + m + c] : 0.f;
        if (wf) wf[r * K + c] = v;
        if (Tw) Tw[r * K + c] = v;
      }
  // pose_cov = sigma^2 Y_p^T Y_p: entry (i, j), j <= i, sums rows r >= i in ascending order; written to both halves
  for (int i = ty; i < m; i += kMargRows)
    for (int j = tx; j <= i; j += kMargCols) {
      double s = 0.0;
      for (int r = i; r < P; ++r) s = fma(M[tri(r) + i], M[tri(r) + j], s);
      const float v = (float)(s2 * s);
      cov[i * m + j] = v;
      cov[j * m + i] = v;
    }
  if (tid == 0) a.status[b] = 0;
}

// ---- (b) ------------------------------------------------------------------------------------------------------------------------
// T lives in LDS as its lower 32 x 32 blocks (marg_fill_T_image) and a wave computes y = T b for 32 pixels (marg_tile_y; the
// layouts: marginals_common.hpp).  The result has the pixel on the lane and the rows of T in the registers: sum of squares per
// lane, one cross-half add.
template <int NR>
__global__ __launch_bounds__(kDvThreads) void marg_depthvar_kernel(const float* __restrict__ basis, const float* __restrict__ Tws,
                                                                   const float* __restrict__ sigma2, const int32_t* __restrict__ status,
                                                                   float* __restrict__ depth_var, int N, int K, int tiles, int vec4) {
  extern __shared__ __attribute__((aligned(16))) float sT[];
  const int b = blockIdx.y, tid = threadIdx.x;
  float* out = depth_var + (size_t)b * N;
  if (status[b] != 0) {                                   // uniform per workgroup
    for (long long n = (long long)blockIdx.x * kDvThreads + tid; n < N; n += (long long)gridDim.x * kDvThreads) out[n] = __builtin_huge_valf();
    return;
  }
  const float* T = Tws + (size_t)b * K * K;
  marg_fill_T_image<NR>(sT, T, K);
  __syncthreads();

  const int lane = tid & 63, wave = tid >> 6, nl = lane & 31, h = lane >> 5;
  const float s2 = sigma2 ? sigma2[b] : 1.f;
  const float* Bw = basis + (size_t)b * N * K;

  for (int tile = blockIdx.x * kDvWaves + wave; tile < tiles; tile += gridDim.x * kDvWaves) {
    const int n = tile * 32 + nl;
    const bool valid = n < N;
    const float* row = Bw + (size_t)(valid ? n : 0) * K;
    f32x16 acc[NR];
    marg_tile_y<NR>(sT, row, valid, K, vec4, nl, h, acc);
    float ss = 0.f;
#pragma unroll
    for (int R = 0; R < NR; ++R)
#pragma unroll
      for (int i = 0; i < 16; ++i) ss = fmaf(acc[R][i], acc[R][i], ss);
    ss += __shfl_xor(ss, 32, 64);                         // the two row halves of the accumulator layout
    if (valid && h == 0) out[n] = s2 * ss;
  }
}

template <int NR>
static void launch_depthvar(const float* basis, const float* T, const float* sigma2, const int32_t* status, float* depth_var, int B,
                            int N, int K, hipStream_t s) {
  const size_t lds = (size_t)NR * (NR + 1) / 2 * 1024 * sizeof(float);
  if (lds > 64 * 1024)
    (void)hipFuncSetAttribute((const void*)marg_depthvar_kernel<NR>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  const int tiles = (N + 31) / 32;
  // workgroups per window: enough to fill the device twice over, never more than there are 8-tile steps (a pixel's arithmetic does
  // not depend on which workgroup takes it)
  int G = (2 * num_cus() + B - 1) / B;
  const int steps = (tiles + kDvWaves - 1) / kDvWaves;
  if (G > steps) G = steps;
  if (G < 1) G = 1;
  const int vec4 = (K % 4 == 0) && (reinterpret_cast<uintptr_t>(basis) & 15u) == 0;
  hipLaunchKernelGGL(marg_depthvar_kernel<NR>, dim3(G, B), dim3(kDvThreads), lds, s, basis, T, sigma2, status, depth_var, N, K, tiles,
                     vec4);
}

int launch_marginals(const banet_level_t* lv, const MargPlan& pl, const float* AtA, const float* damping, const float* sigma2,
                     const banet_marginals_out_t* out, void* ws, hipStream_t s) {
  char* w = static_cast<char*>(ws);
  const bool want_dv = out->depth_var != nullptr && pl.K > 0;
  MargArgs a;
  a.P = pl.P;
  a.m = pl.m;
  a.K = pl.K;
  a.AtA = AtA;
  a.damping = damping;
  a.sigma2 = sigma2;
  a.pose_cov = out->pose_cov;
  a.wfactor = pl.K > 0 ? out->wfactor : nullptr;
  a.logdet = out->logdet;
  a.status = out->status;
  a.T = want_dv ? reinterpret_cast<float*>(w + pl.off_T) : nullptr;
  a.big = pl.big ? reinterpret_cast<double*>(w + pl.off_big) : nullptr;
  if (pl.big) {
    hipLaunchKernelGGL(marg_factor_kernel<true>, dim3(lv->B), dim3(kMargThreads), pl.lds, s, a);
  } else {
    if (pl.lds > 64 * 1024)
      (void)hipFuncSetAttribute((const void*)marg_factor_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds);
    hipLaunchKernelGGL(marg_factor_kernel<false>, dim3(lv->B), dim3(kMargThreads), pl.lds, s, a);
  }
  if (hipGetLastError() != hipSuccess) return BANET_ERR_LAUNCH;
  if (want_dv) {
    const int NR = (pl.K + 31) / 32;
#define BANET_DV(n) \
  case n: launch_depthvar<n>(lv->basis, a.T, sigma2, out->status, out->depth_var, lv->B, lv->N, pl.K, s); break;
    switch (NR) {
      BANET_DV(1) BANET_DV(2) BANET_DV(3) BANET_DV(4) BANET_DV(5) BANET_DV(6) BANET_DV(7) BANET_DV(8)
      default: return BANET_ERR_UNSUPPORTED;
    }
#undef BANET_DV
    if (hipGetLastError() != hipSuccess) return BANET_ERR_LAUNCH;
  }
  return BANET_OK;
}

}  // namespace banet
