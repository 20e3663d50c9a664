// Weighted, damped least-squares fit of a depth map on a level's basis (banet_basis_fit_f32):
//   r_n = target_n - depth_n,   G = sum_n w_n b_n b_n^T,   g = sum_n w_n r_n b_n,   H = G + mu diag(diag(G) + 1e-5),   Wc = H^-1 g
// over the points with a finite w_n > 0 and a finite target_n (every other point contributes exact zeros, whatever its basis row holds).
//   (a) fit_gram_kernel    one read of the basis on the f32-input MFMA (v_mfma_f32_32x32x2_f32: every product an exact float32 fma).
//       The contraction index is the pixel: a step takes two pixels, lane l holds column 32 blk + (l & 31) of pixel 2 t + (l >> 5)
//       for each 32-column block -- the A operand is w_n times that value, the B operand the value itself, so one set of loads
//       feeds both sides.  Only the NR (NR + 1) / 2 lower 32 x 32 blocks of G are computed (block (R, Cb), Cb <= R, at
//       R (R + 1) / 2 + Cb, as marg_depthvar_kernel stores T).  Columns past K and pixels past the range enter as zeros; nothing
//       past them is read (their lanes read column 0 / the range's first pixel instead, so that every load is unconditional).
//       4-byte loads, 128 contiguous bytes per half wave: one path for every K and every alignment.  g and the two stats ride along
//       on the vector ALU.  A group of waves owns a contiguous pixel range of one window and writes its own partial row; K <= 128:
//       a group is one wave with all <= 10 blocks in its accumulators; K > 128: the four waves of a workgroup share the range and
//       split the <= 36 blocks between them (block p goes to wave p & 3).
//   (b) fit_fold_kernel    adds the partial rows in ascending order; G is written from its lower triangle to both halves: exactly
//       symmetric.  G, g go to the workspace for (c) and to normal / rhs / stats where asked for.
//   (c) fit_solve_kernel   one workgroup per window: Cholesky of H in float64 on the float32 G, forward and back substitution, Wc
//       rounded once; the packed triangle in LDS up to K = 199, in the workspace above.  A pivot <= 0 or not finite: status 1, Wc 0.
// The number of partial rows and every summation order depend on N and K only, never on B; no atomics.
#include <utility>

#include "kernels.hpp"

namespace banet {

constexpr int kFitThreads = 256;          // (a): 4 waves  (kFitRowsMax / kFitRowPixels, the partial rows: prior_plan.hpp)
constexpr int kFitSolveThreads = 1024;    // (c): 16 columns x 64 rows of threads over the trailing blocks
constexpr int kFitCols = 16, kFitRowsT = kFitSolveThreads / kFitCols;
constexpr size_t kFitLdsMax = 160 * 1024;

typedef float fit_f32x16 __attribute__((ext_vector_type(16)));

int plan_basis_fit(const banet_level_t* lv, FitPlan* pl) {
  if (!lv || lv->B < 1) return BANET_ERR_INVALID_ARG;
  if (lv->K < 1 || lv->K > kFitKMax || lv->N < 1) return BANET_ERR_UNSUPPORTED;
  const int K = lv->K, N = lv->N;
  pl->K = K;
  const FitRows fr = fit_rows(N, K);                 // (prior_plan.hpp: the prior's observation half runs the same rows)
  pl->NR = fr.NR;
  pl->NP = fr.NP;
  pl->chunk = fr.chunk;
  pl->rows = fr.rows;
  pl->pstride = fr.pstride;
  const size_t mat = (size_t)K * (K + 1) / 2 * sizeof(double), vecs = 2 * (size_t)K * sizeof(double);
  pl->big = mat + vecs > kFitLdsMax;
  pl->lds = pl->big ? vecs : mat + vecs;
  Arena ar;
  pl->off_part = ar.take((size_t)lv->B * pl->rows * pl->pstride * sizeof(float));
  pl->off_G = ar.take((size_t)lv->B * K * K * sizeof(float));
  pl->off_g = ar.take((size_t)lv->B * K * sizeof(float));
  pl->off_big = ar.take(pl->big ? (size_t)lv->B * mat : 0);
  pl->bytes = ar.off;
  return BANET_OK;
}

struct FitArgs {
  int N, K, chunk, rows, pstride;
  const float* depth;
  const float* basis;
  const float* target;
  const float* weight;   // nullptr: 1
  float* part;           // [B][rows][pstride]
};

__host__ __device__ constexpr int fit_block_row(int p) {
  int R = 0;
  while ((R + 1) * (R + 2) / 2 <= p) ++R;
  return R;
}

// acc[q] += (w b)_R (b)_Cb^T for the wave's blocks p = PART + q S, with (R, Cb) compile-time constants (register indices)
template <int NR, int S, int PART, int... Q>
__device__ __forceinline__ void fit_mfma_blocks(const float (&av)[NR], const float (&v)[NR], fit_f32x16* acc,
                                                std::integer_sequence<int, Q...>) {
  ((acc[Q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[fit_block_row(PART + Q * S)],
                                                  v[PART + Q * S - fit_block_row(PART + Q * S) * (fit_block_row(PART + Q * S) + 1) / 2],
                                                  acc[Q], 0, 0, 0)),
   ...);
}

// One wave over the pixel range [n0, n1) of window b: the blocks p = PART, PART + S, ... of the lower triangle; PART == 0 also g and
// the two stats.  Writes its share of the partial row `prow`.
template <int NR, int S, int PART>
__device__ __forceinline__ void fit_gram_wave(const FitArgs& a, int b, int n0, int n1, float* __restrict__ prow) {
  constexpr int NP = NR * (NR + 1) / 2;
  constexpr int MY = (NP - PART + S - 1) / S;
  const int lane = lane_id(), j = lane & 31, h = lane >> 5;
  const int N = a.N, K = a.K;
  const float* __restrict__ Bw = a.basis + (size_t)b * N * K;
  const float* __restrict__ dep = a.depth + (size_t)b * N;
  const float* __restrict__ tgt = a.target + (size_t)b * N;
  const float* __restrict__ wgt = a.weight ? a.weight + (size_t)b * N : nullptr;

  fit_f32x16 acc[MY];
#pragma unroll
  for (int q = 0; q < MY; ++q)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[q][i] = 0.f;
  float gacc[NR];
#pragma unroll
  for (int blk = 0; blk < NR; ++blk) gacc[blk] = 0.f;
  float sw = 0.f, swr2 = 0.f;

  // A batch = kFitBatch two-pixel steps; a lane's pixel of step u is nb + 2 u + h.  Every load of a batch is unconditional (a pixel
  // past the range reads the range's first pixel, a column past K reads column 0; both are masked at consumption), so the whole
  // batch is in flight at once, and the next batch is loaded before the current one's MFMAs: a load that waited for the pixel's
  // weight cost two memory latencies per step (4 x the bound at K = 128).  Weight, target and depth of the batch's 2 kFitBatch
  // pixels are one load each -- lane l takes pixel nb + (l & 7) -- and reach the steps through the LDS crossbar.
  constexpr int kFitBatch = 4;
  struct Batch {
    float w, t, d, v[kFitBatch][NR];
  };
  int cc[NR];
#pragma unroll
  for (int blk = 0; blk < NR; ++blk) cc[blk] = 32 * blk + j < K ? 32 * blk + j : 0;
  auto load_batch = [&](int nb, Batch& q) {
    const int m = nb + (lane & 7);
    const int mi = m < n1 ? m : n0;
    q.w = wgt ? wgt[mi] : 1.f;
    q.t = tgt[mi];
    q.d = dep[mi];
#pragma unroll
    for (int u = 0; u < kFitBatch; ++u) {
      const int n = nb + 2 * u + h;
      const float* row = Bw + (size_t)(n < n1 ? n : n0) * K;
#pragma unroll
      for (int blk = 0; blk < NR; ++blk) q.v[u][blk] = row[cc[blk]];
    }
  };

  Batch cur, nxt;
  load_batch(n0, cur);
  for (int nb = n0; nb < n1; nb += 2 * kFitBatch) {
    load_batch(nb + 2 * kFitBatch, nxt);   // (past the range on the last round: the clamped pixel again, never consumed)
    // the lane's own pixel of the batch: does it contribute?  (NaN fails each comparison)
    const bool mine = (nb + (lane & 7) < n1) && fit_point_counted(cur.w, cur.t);
    const float wl = mine ? cur.w : 0.f, rl = mine ? cur.t - cur.d : 0.f;
#pragma unroll
    for (int u = 0; u < kFitBatch; ++u) {
      const float w = __shfl(wl, 2 * u + h, 64), r = __shfl(rl, 2 * u + h, 64);
      const bool ok = w > 0.f;
      float v[NR], av[NR];
#pragma unroll
      for (int blk = 0; blk < NR; ++blk) {
        v[blk] = (ok && 32 * blk + j < K) ? cur.v[u][blk] : 0.f;
        av[blk] = w * v[blk];
      }
      fit_mfma_blocks<NR, S, PART>(av, v, acc, std::make_integer_sequence<int, MY>());
      if constexpr (PART == 0) {
        const float wr = w * r;
#pragma unroll
        for (int blk = 0; blk < NR; ++blk) gacc[blk] = fmaf(wr, v[blk], gacc[blk]);
        sw += w;
        swr2 = fmaf(wr, r, swr2);
      }
    }
    cur = nxt;
  }

  // accumulator layout of the 32 x 32 result: register i of lane l is row 8 (i / 4) + 4 (l >> 5) + (i % 4), column l & 31
#pragma unroll
  for (int q = 0; q < MY; ++q) {
    float* blkp = prow + (size_t)(PART + q * S) * 1024;
#pragma unroll
    for (int i = 0; i < 16; ++i) blkp[(8 * (i / 4) + 4 * h + (i % 4)) * 32 + j] = acc[q][i];
  }
  if constexpr (PART == 0) {
    float* gp = prow + (size_t)NP * 1024;
#pragma unroll
    for (int blk = 0; blk < NR; ++blk) {
      const float s = gacc[blk] + __shfl_xor(gacc[blk], 32, 64);   // the two pixel parities
      if (h == 0) gp[32 * blk + j] = s;
    }
    const float s0 = sw + __shfl_xor(sw, 32, 64), s1 = swr2 + __shfl_xor(swr2, 32, 64);
    if (lane == 0) {
      gp[32 * NR + 0] = s0;
      gp[32 * NR + 1] = s1;
    }
  }
}

template <int NR, int S>
__global__ __launch_bounds__(kFitThreads, 2) void fit_gram_kernel(const FitArgs a) {   // two waves per SIMD: <= 256 registers
  const int b = blockIdx.y, wave = wave_id();
  const int row = S == 1 ? blockIdx.x * 4 + wave : blockIdx.x;
  if (row >= a.rows) return;   // wave-uniform
  const int n0 = row * a.chunk, n1 = min(a.N, n0 + a.chunk);
  float* prow = a.part + ((size_t)b * a.rows + row) * a.pstride;
  if constexpr (S == 1) {
    fit_gram_wave<NR, 1, 0>(a, b, n0, n1, prow);
  } else {
    switch (wave) {
      case 0: fit_gram_wave<NR, 4, 0>(a, b, n0, n1, prow); break;
      case 1: fit_gram_wave<NR, 4, 1>(a, b, n0, n1, prow); break;
      case 2: fit_gram_wave<NR, 4, 2>(a, b, n0, n1, prow); break;
      default: fit_gram_wave<NR, 4, 3>(a, b, n0, n1, prow); break;
    }
  }
}

// ---- (b) ------------------------------------------------------------------------------------------------------------------------
struct FoldArgs {
  int K, NR, NP, rows, pstride;
  const float* part;
  float* Gws;      // [B][K][K]
  float* gws;      // [B][K]
  float* normal;   // or nullptr
  float* rhs;      // or nullptr
  float* stats;    // or nullptr
};

__global__ __launch_bounds__(256) void fit_fold_kernel(const FoldArgs a) {
  const int b = blockIdx.y, K = a.K;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int nG = a.NP * 1024, total = nG + a.NR * 32 + 2;
  if (idx >= total) return;
  const float* p = a.part + (size_t)b * a.rows * a.pstride + idx;
  float s = 0.f;
  for (int q = 0; q < a.rows; ++q) s += p[(size_t)q * a.pstride];
  if (idx < nG) {
    const int blk = idx >> 10, i = (idx >> 5) & 31, j = idx & 31;
    const int R = fit_block_row(blk), Cb = blk - R * (R + 1) / 2;
    const int r = 32 * R + i, c = 32 * Cb + j;
    if (r < K && c <= r) {
      const size_t o = (size_t)b * K * K;
      a.Gws[o + (size_t)r * K + c] = s;
      a.Gws[o + (size_t)c * K + r] = s;
      if (a.normal) {
        a.normal[o + (size_t)r * K + c] = s;
        a.normal[o + (size_t)c * K + r] = s;
      }
    }
  } else if (idx < nG + a.NR * 32) {
    const int k = idx - nG;
    if (k < K) {
      a.gws[(size_t)b * K + k] = s;
      if (a.rhs) a.rhs[(size_t)b * K + k] = s;
    }
  } else if (a.stats) {
    a.stats[(size_t)b * 2 + (idx - nG - a.NR * 32)] = s;
  }
}

// ---- (c) ------------------------------------------------------------------------------------------------------------------------
struct FitSolveArgs {
  int K;
  const float* G;
  const float* g;
  const float* damping;
  float* Wc;
  int32_t* status;
  double* big;   // [B][K (K + 1) / 2] in the workspace when the matrix does not fit the LDS
};

__device__ __forceinline__ int fit_tri(int i) { return i * (i + 1) / 2; }   // offset of row i of a packed lower triangle

template <bool BIG>
__global__ __launch_bounds__(kFitSolveThreads) void fit_solve_kernel(const FitSolveArgs a) {
  extern __shared__ __attribute__((aligned(16))) double fit_smem[];
  const int b = blockIdx.x, tid = threadIdx.x, tx = tid & (kFitCols - 1), ty = tid / kFitCols;
  const int K = a.K;
  const size_t mat = (size_t)K * (K + 1) / 2;
  double* M = BIG ? a.big + (size_t)b * mat : fit_smem;    // packed lower triangle: H, then L (its diagonal in `diag`)
  double* y = BIG ? fit_smem : fit_smem + mat;             // [K] the current column, then the right-hand side / solution
  double* diag = y + K;                                    // [K] L_jj
  const float* A = a.G + (size_t)b * K * K;
  const double mu = a.damping ? (double)a.damping[b] : 0.0;
  float* out = a.Wc + (size_t)b * K;

  for (int i = ty; i < K; i += kFitRowsT)
    for (int j = tx; j <= i; j += kFitCols) {
      double v = (double)A[(size_t)i * K + j];
      if (i == j) v = v + mu * (v + 1e-5);                 // every diagonal entry
      M[fit_tri(i) + j] = v;
    }
  __syncthreads();

  // Cholesky, right-looking: column j scaled by 1 / L_jj, then the rank-1 update of the trailing lower triangle
  bool ok = true;
  for (int j = 0; j < K; ++j) {
    const double p = M[fit_tri(j) + j];
    if (!(p > 0.0) || !(p < __builtin_huge_val())) {       // pivot <= 0 or not finite (a NaN / inf elsewhere reaches a later pivot)
      ok = false;
      break;                                               // uniform: every thread read the same pivot
    }
    const double d = sqrt(p);
    for (int i = j + 1 + tid; i < K; i += kFitSolveThreads) {
      const double v = M[fit_tri(i) + j] / d;
      M[fit_tri(i) + j] = v;
      y[i] = v;
    }
    if (tid == 0) diag[j] = d;
    __syncthreads();
    for (int i = j + 1 + ty; i < K; i += kFitRowsT) {
      const double li = y[i];
      double* row = M + fit_tri(i);
      for (int k = j + 1 + tx; k <= i; k += kFitCols) row[k] = fma(-li, y[k], row[k]);
    }
    __syncthreads();
  }
  if (!ok) {
    for (int k = tid; k < K; k += kFitSolveThreads) out[k] = 0.f;
    if (tid == 0) a.status[b] = 1;
    return;
  }

  for (int k = tid; k < K; k += kFitSolveThreads) y[k] = (double)a.g[(size_t)b * K + k];
  __syncthreads();
  // L z = g, column sweep: z_j = y_j / L_jj, then y_i -= L_ij z_j below it (one thread per entry: a fixed order)
  for (int j = 0; j < K; ++j) {
    const double zj = y[j] / diag[j];
    __syncthreads();
    for (int i = j + 1 + tid; i < K; i += kFitSolveThreads) y[i] = fma(-M[fit_tri(i) + j], zj, y[i]);
    if (tid == 0) y[j] = zj;
    __syncthreads();
  }
  // L^T x = z, from the last row up: x_j = y_j / L_jj, then y_i -= L_ji x_j above it
  for (int j = K - 1; j >= 0; --j) {
    const double xj = y[j] / diag[j];
    __syncthreads();
    const double* rj = M + fit_tri(j);
    for (int i = tid; i < j; i += kFitSolveThreads) y[i] = fma(-rj[i], xj, y[i]);
    if (tid == 0) y[j] = xj;
    __syncthreads();
  }
  for (int k = tid; k < K; k += kFitSolveThreads) out[k] = (float)y[k];
  if (tid == 0) a.status[b] = 0;
}

template <int NR, int S>
static void launch_fit_gram(const FitArgs& a, int B, hipStream_t s) {
  const int gx = S == 1 ? (a.rows + 3) / 4 : a.rows;
  hipLaunchKernelGGL((fit_gram_kernel<NR, S>), dim3(gx, B), dim3(kFitThreads), 0, s, a);
}

// (a) + (b): the Gram pass over the rows `fr` and its fold.  G / g go to Gws / gws and to normal / rhs / stats where given.  The
// first two launches of banet_basis_fit_f32, and the observation half of a prior (prior.hip), whose G / g are therefore its bits.
int launch_fit_gram_fold(const banet_level_t* lv, const FitRows& fr, const float* target, const float* weight, float* part, float* Gws,
                         float* gws, float* normal, float* rhs, float* stats, hipStream_t s) {
  FitArgs a;
  a.N = lv->N;
  a.K = lv->K;
  a.chunk = fr.chunk;
  a.rows = fr.rows;
  a.pstride = fr.pstride;
  a.depth = lv->depth;
  a.basis = lv->basis;
  a.target = target;
  a.weight = weight;
  a.part = part;
  switch (fr.NR) {
    case 1: launch_fit_gram<1, 1>(a, lv->B, s); break;
    case 2: launch_fit_gram<2, 1>(a, lv->B, s); break;
    case 3: launch_fit_gram<3, 1>(a, lv->B, s); break;
    case 4: launch_fit_gram<4, 1>(a, lv->B, s); break;
    case 5: launch_fit_gram<5, 4>(a, lv->B, s); break;
    case 6: launch_fit_gram<6, 4>(a, lv->B, s); break;
    case 7: launch_fit_gram<7, 4>(a, lv->B, s); break;
    case 8: launch_fit_gram<8, 4>(a, lv->B, s); break;
    default: return BANET_ERR_UNSUPPORTED;
  }
  if (hipGetLastError() != hipSuccess) return BANET_ERR_LAUNCH;

  FoldArgs f;
  f.K = lv->K;
  f.NR = fr.NR;
  f.NP = fr.NP;
  f.rows = fr.rows;
  f.pstride = fr.pstride;
  f.part = part;
  f.Gws = Gws;
  f.gws = gws;
  f.normal = normal;
  f.rhs = rhs;
  f.stats = stats;
  const int total = fr.NP * 1024 + fr.NR * 32 + 2;
  hipLaunchKernelGGL(fit_fold_kernel, dim3((total + 255) / 256, lv->B), dim3(256), 0, s, f);
  if (hipGetLastError() != hipSuccess) return BANET_ERR_LAUNCH;
  return BANET_OK;
}

int launch_basis_fit(const banet_level_t* lv, const FitPlan& pl, const float* target, const float* weight, const float* damping,
                     const banet_basis_fit_out_t* out, void* ws, hipStream_t s) {
  char* w = static_cast<char*>(ws);
  float* Gws = reinterpret_cast<float*>(w + pl.off_G);
  float* gws = reinterpret_cast<float*>(w + pl.off_g);
  const FitRows fr = {pl.NR, pl.NP, pl.chunk, pl.rows, pl.pstride};
  const int rc = launch_fit_gram_fold(lv, fr, target, weight, reinterpret_cast<float*>(w + pl.off_part), Gws, gws, out->normal, out->rhs,
                                      out->stats, s);
  if (rc != BANET_OK) return rc;

  FitSolveArgs q;
  q.K = pl.K;
  q.G = Gws;
  q.g = gws;
  q.damping = damping;
  q.Wc = out->Wc;
  q.status = out->status;
  q.big = pl.big ? reinterpret_cast<double*>(w + pl.off_big) : nullptr;
  if (pl.big) {
    hipLaunchKernelGGL(fit_solve_kernel<true>, dim3(lv->B), dim3(kFitSolveThreads), pl.lds, s, q);
  } else {
    if (pl.lds > 64 * 1024)
      (void)hipFuncSetAttribute((const void*)fit_solve_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds);
    hipLaunchKernelGGL(fit_solve_kernel<false>, dim3(lv->B), dim3(kFitSolveThreads), pl.lds, s, q);
  }
  if (hipGetLastError() != hipSuccess) return BANET_ERR_LAUNCH;
  return BANET_OK;
}

}  // namespace banet
