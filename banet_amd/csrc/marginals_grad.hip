// The backward of the posterior marginals (banet_ba_marginals_grad_f32): from the upstream gradients g_cov [m,m] of pose_cov,
// g_dv [N] of depth_var and g_ld of logdet (each may be absent = zero) to the gradients of AtA, damping, sigma^2 and the basis.
// With H = AtA + mu diag(diag(AtA) + 1e-5) = L L^T, Y = L^-1, T = Y[m:, m:], Hinv = Y^T Y = H^-1 and s2 = sigma^2:
//     M    = sum_n g_dv[n] b_n b_n^T                 Gbar = blockdiag(1/2 (g_cov + g_cov^T), M)
//     X    = Hinv Gbar                                dH   = g_ld Hinv - s2 X Hinv          (= Y^T (g_ld I - s2 Y Gbar Y^T) Y)
//     gAtA = dH off the diagonal, (1 + mu) dH on it   gdamping = sum_i dH_ii (A_ii + 1e-5)   gsigma2 = trace(X)
//     gbasis[n] = 2 s2 g_dv[n] T^T (T b_n)
//   (a) marg_grad_gram_kernel + marg_grad_fold_kernel   M on the f32-input MFMA, the pixel as the contraction index: fit_gram_kernel's
//       scheme (basisfit.hip) with the weight g_n of EITHER sign and no right-hand side -- lane l holds column 32 blk + (l & 31) of pixel
//       2 t + (l >> 5), the A operand is g_n times that value, the B operand the value itself; only the lower 32 x 32 blocks; one
//       partial row per fixed pixel range, folded in ascending order and written to both halves.  Loads unconditional, a batch ahead.
//   (b) marg_grad_factor_kernel   one workgroup per window, float64 on the float32 inputs, outputs rounded once (the gradient applies
//       H^-1 twice: a float32 route would lose cond(H) 2^-24 twice over).  The factorisation is marg_factor_kernel's own
//       (marginals_common.hpp); then Hinv (packed triangle), X (full) and dH entry by entry, every sum a fixed ascending fma chain.
//       Y's triangle lives where the forward keeps it (LDS up to P = 199, the workspace above); Hinv and X in the workspace.
//   (c) marg_grad_basis_kernel    one read of the basis, one write of [N,K]: y = T b as marg_depthvar_kernel computes it, then
//       z = T^T y without leaving the registers -- a lane's accumulator register 4 j + e holds row 8 j + 4 h + e of y, which is the
//       k-slot order of a second 32x32x2 chain's B operand; its A operand T^T is read column-wise (4-byte reads) from the same
//       swizzled image: row 8 j + 4 h + e, column l & 31 -- the 32 lanes of a half read the 32 banks of one row.
// No atomics; every summation order is a function of N, K and pairs only: a window's bits are the same alone and in any batch, and
// a subset of the outputs gives the same bits.
#include <utility>

#include "marginals_common.hpp"

namespace banet {

constexpr int kMgGramThreads = 256;       // (a): 4 waves
constexpr int kMgRowsMax = 64;            // partial rows per window at most
constexpr int kMgRowPixels = 256;         // ... and never fewer pixels than this per row

int plan_marginals_grad(const banet_level_t* lv, int want_gbasis, MargGradPlan* pl) {
  if (!lv || lv->B < 1 || lv->K < 0 || lv->pairs < 0) return BANET_ERR_INVALID_ARG;
  const int m = 6 * npairs(lv), K = lv->K;
  const long long P = (long long)m + K;
  if (K > kMargKMax || P > kMargPMax) return BANET_ERR_UNSUPPORTED;
  pl->P = (int)P;
  pl->m = m;
  pl->K = K;
  pl->NR = (K + 31) / 32;
  pl->NP = pl->NR * (pl->NR + 1) / 2;
  const int N = lv->N > 0 ? lv->N : 1;               // (K == 0, or a call without g_depth_var / gbasis: N is not read by the kernels)
  int rows = (N + kMgRowPixels - 1) / kMgRowPixels;
  if (rows > kMgRowsMax) rows = kMgRowsMax;
  int chunk = (N + rows - 1) / rows;
  chunk = (chunk + 1) / 2 * 2;                       // whole two-pixel steps
  pl->chunk = chunk;
  pl->rows = (N + chunk - 1) / chunk;
  // Y's packed lower triangle and two vectors, in doubles: where marg_factor_kernel keeps them -- LDS up to P = 199
  // (199 * 200 / 2 * 8 + 2 * 199 * 8 = 162384 <= 163840 < 160800 + 3200 at P = 200)
  const size_t mat = (size_t)pl->P * (pl->P + 1) / 2 * sizeof(double), vecs = 2 * (size_t)pl->P * sizeof(double);
  pl->big = mat + vecs > kMargLdsMax;
  pl->lds = pl->big ? vecs : mat + vecs;
  const size_t B = (size_t)lv->B;
  Arena ar;
  pl->off_part = ar.take(K > 0 ? B * pl->rows * pl->NP * 1024 * sizeof(float) : 0);
  pl->off_M = ar.take(K > 0 ? B * K * K * sizeof(float) : 0);
  pl->off_T = ar.take(want_gbasis && K > 0 ? B * K * K * sizeof(float) : 0);
  pl->off_Hinv = ar.take(B * mat);
  pl->off_X = ar.take(B * (size_t)pl->P * pl->P * sizeof(double));
  pl->off_big = ar.take(pl->big ? B * mat : 0);
  pl->bytes = ar.off;                                // (> 0: Hinv and X exist for every shape)
  return BANET_OK;
}

// ---- (a) ------------------------------------------------------------------------------------------------------------------------
struct MgGramArgs {
  int N, K, chunk, rows, pstride;
  const float* basis;
  const float* g;        // [B][N]
  float* part;           // [B][rows][pstride]
};

// acc[q] += (g b)_R (b)_Cb^T for the wave's blocks p = PART + q S, with (R, Cb) compile-time constants (register indices)
template <int NR, int S, int PART, int... Q>
__device__ __forceinline__ void mg_mfma_blocks(const float (&av)[NR], const float (&v)[NR], f32x16* acc, std::integer_sequence<int, Q...>) {
  ((acc[Q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[marg_block_row(PART + Q * S)],
                                                  v[PART + Q * S - marg_block_row(PART + Q * S) * (marg_block_row(PART + Q * S) + 1) / 2],
                                                  acc[Q], 0, 0, 0)),
   ...);
}

// One wave over the pixel range [n0, n1) of window b: the blocks p = PART, PART + S, ... of the lower triangle -> its share of `prow`
template <int NR, int S, int PART>
__device__ __forceinline__ void mg_gram_wave(const MgGramArgs& a, int b, int n0, int n1, float* __restrict__ prow) {
  constexpr int NP = NR * (NR + 1) / 2;
  constexpr int MY = (NP - PART + S - 1) / S;
  const int lane = lane_id(), j = lane & 31, h = lane >> 5;
  const int N = a.N, K = a.K;
  const float* __restrict__ Bw = a.basis + (size_t)b * N * K;
  const float* __restrict__ gw = a.g + (size_t)b * N;

  f32x16 acc[MY];
#pragma unroll
  for (int q = 0; q < MY; ++q)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[q][i] = 0.f;

  // A batch = kBatch two-pixel steps; a lane's pixel of step u is nb + 2 u + h.  Every load of a batch is unconditional (a pixel past
  // the range reads the range's first pixel, a column past K reads column 0; both are masked at consumption), so the whole batch is
  // in flight at once, and the next batch is loaded before the current one's MFMAs.  The weights of the batch's 2 kBatch pixels are
  // one load -- lane l takes pixel nb + (l & 7) -- and reach the steps through the LDS crossbar.
  constexpr int kBatch = 4;
  struct Batch {
    float w, v[kBatch][NR];
  };
  int cc[NR];
#pragma unroll
  for (int blk = 0; blk < NR; ++blk) cc[blk] = 32 * blk + j < K ? 32 * blk + j : 0;
  auto load_batch = [&](int nb, Batch& q) {
    const int mm = nb + (lane & 7);
    q.w = gw[mm < n1 ? mm : n0];
#pragma unroll
    for (int u = 0; u < kBatch; ++u) {
      const int n = nb + 2 * u + h;
      const float* row = Bw + (size_t)(n < n1 ? n : n0) * K;
#pragma unroll
      for (int blk = 0; blk < NR; ++blk) q.v[u][blk] = row[cc[blk]];
    }
  };

  Batch cur, nxt;
  load_batch(n0, cur);
  for (int nb = n0; nb < n1; nb += 2 * kBatch) {
    load_batch(nb + 2 * kBatch, nxt);   // (past the range on the last round: the clamped pixel again, never consumed)
    const float wl = (nb + (lane & 7) < n1) ? cur.w : 0.f;
#pragma unroll
    for (int u = 0; u < kBatch; ++u) {
      const float w = __shfl(wl, 2 * u + h, 64);
      const bool in = nb + 2 * u + h < n1;
      float v[NR], av[NR];
#pragma unroll
      for (int blk = 0; blk < NR; ++blk) {
        v[blk] = (in && 32 * blk + j < K) ? cur.v[u][blk] : 0.f;
        av[blk] = w * v[blk];
      }
      mg_mfma_blocks<NR, S, PART>(av, v, acc, std::make_integer_sequence<int, MY>());
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
}

template <int NR, int S>
__global__ __launch_bounds__(kMgGramThreads, 2) void marg_grad_gram_kernel(const MgGramArgs a) {   // two waves per SIMD: <= 256 registers
  const int b = blockIdx.y, wave = wave_id();
  const int row = S == 1 ? blockIdx.x * 4 + wave : blockIdx.x;
  if (row >= a.rows) return;   // wave-uniform
  const int n0 = row * a.chunk, n1 = min(a.N, n0 + a.chunk);
  float* prow = a.part + ((size_t)b * a.rows + row) * a.pstride;
  if constexpr (S == 1) {
    mg_gram_wave<NR, 1, 0>(a, b, n0, n1, prow);
  } else {
    switch (wave) {
      case 0: mg_gram_wave<NR, 4, 0>(a, b, n0, n1, prow); break;
      case 1: mg_gram_wave<NR, 4, 1>(a, b, n0, n1, prow); break;
      case 2: mg_gram_wave<NR, 4, 2>(a, b, n0, n1, prow); break;
      default: mg_gram_wave<NR, 4, 3>(a, b, n0, n1, prow); break;
    }
  }
}

// the partial rows added in ascending order; M [B][K][K] written from its lower triangle to both halves: exactly symmetric
__global__ __launch_bounds__(256) void marg_grad_fold_kernel(const float* __restrict__ part, float* __restrict__ Mws, int K, int NP,
                                                             int rows, int pstride) {
  const int b = blockIdx.y;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= NP * 1024) return;
  const float* p = part + (size_t)b * rows * pstride + idx;
  float s = 0.f;
  for (int q = 0; q < rows; ++q) s += p[(size_t)q * pstride];
  const int blk = idx >> 10, i = (idx >> 5) & 31, j = idx & 31;
  const int R = marg_block_row(blk), Cb = blk - R * (R + 1) / 2;
  const int r = 32 * R + i, c = 32 * Cb + j;
  if (r < K && c <= r) {
    const size_t o = (size_t)b * K * K;
    Mws[o + (size_t)r * K + c] = s;
    Mws[o + (size_t)c * K + r] = s;
  }
}

template <int NR, int S>
static void launch_mg_gram(const MgGramArgs& a, int B, hipStream_t s) {
  const int gx = S == 1 ? (a.rows + 3) / 4 : a.rows;
  hipLaunchKernelGGL((marg_grad_gram_kernel<NR, S>), dim3(gx, B), dim3(kMgGramThreads), 0, s, a);
}

// ---- (b) ------------------------------------------------------------------------------------------------------------------------
struct MgFactorArgs {
  int P, m, K;
  const float* AtA;
  const float* damping;
  const float* sigma2;
  const float* g_cov;    // [B][m][m] or nullptr = zeros
  const float* g_ld;     // [B] or nullptr = zeros
  const float* Mws;      // [B][K][K] from (a), or nullptr = zeros (no g_depth_var, or K == 0)
  float* gAtA;           // the outputs: each or nullptr
  float* gdamping;
  float* gsigma2;
  int32_t* status;
  float* T;              // [B][K][K] in the workspace for (c), or nullptr
  double* Hinv;          // [B][P (P + 1) / 2] workspace
  double* X;             // [B][P][P] workspace
  double* big;           // [B][P (P + 1) / 2] in the workspace when Y's triangle does not fit the LDS
};

template <bool BIG>
__global__ __launch_bounds__(kMargThreads) void marg_grad_factor_kernel(const MgFactorArgs a) {
  extern __shared__ __attribute__((aligned(16))) double mg_smem[];
  const int b = blockIdx.x, tid = threadIdx.x, tx = tid & (kMargCols - 1), ty = tid / kMargCols;
  const int P = a.P, m = a.m, K = a.K;
  const size_t mat = (size_t)P * (P + 1) / 2;
  double* M = BIG ? a.big + (size_t)b * mat : mg_smem;    // packed lower triangle: H, then L, then Y = L^-1
  double* colbuf = BIG ? mg_smem : mg_smem + mat;         // [P] the current column; later dH_ii (A_ii + 1e-5)
  double* diag = colbuf + P;                              // [P] L_jj; later X_ii
  const float* A = a.AtA + (size_t)b * P * P;
  const double mu = a.damping ? (double)a.damping[b] : 0.0;
  const double s2 = a.sigma2 ? (double)a.sigma2[b] : 1.0;
  const double gld = a.g_ld ? (double)a.g_ld[b] : 0.0;
  const float* gc = a.g_cov ? a.g_cov + (size_t)b * m * m : nullptr;
  const float* Mg = a.Mws ? a.Mws + (size_t)b * K * K : nullptr;
  float* gA = a.gAtA ? a.gAtA + (size_t)b * P * P : nullptr;

  const bool ok = marg_cholesky(A, mu, P, M, colbuf, diag);   // the forward's failure test; uniform
  if (!ok) {                                              // zeros everywhere; the upstream values are not read
    if (gA)
      for (int idx = tid; idx < P * P; idx += kMargThreads) gA[idx] = 0.f;
    if (tid == 0) {
      if (a.gdamping) a.gdamping[b] = 0.f;
      if (a.gsigma2) a.gsigma2[b] = 0.f;
      a.status[b] = 1;
    }
    return;                                               // (c) reads status and writes zeros; it does not read T
  }
  marg_invert_lower(P, M, colbuf, diag);

  // T for (c): the forward's statement, rounded to float32 once
  if (a.T) {
    float* Tw = a.T + (size_t)b * K * K;
    for (int r = ty; r < K; r += kMargRows)
      for (int c = tx; c < K; c += kMargCols) Tw[r * K + c] = c <= r ? (float)M[tri(m + r) + m + c] : 0.f;
  }
  // Hinv = Y^T Y: entry (i, j), j <= i, sums rows r >= i in ascending order (the forward's pose_cov statement, over all of H^-1)
  double* Hi = a.Hinv + (size_t)b * mat;
  for (int i = ty; i < P; i += kMargRows)
    for (int j = tx; j <= i; j += kMargCols) {
      double s = 0.0;
      for (int r = i; r < P; ++r) s = fma(M[tri(r) + i], M[tri(r) + j], s);
      Hi[tri(i) + j] = s;
    }
  __syncthreads();
  auto hinv = [&](int i, int j) { return i >= j ? Hi[tri(i) + j] : Hi[tri(j) + i]; };

  // X = Hinv Gbar, Gbar = blockdiag(1/2 (g_cov + g_cov^T), M): column c < m sums k over the pose block, c >= m over the depth
  // block, ascending; an absent upstream enters as zeros through the same statements
  double* X = a.X + (size_t)b * P * P;
  for (int i = ty; i < P; i += kMargRows)
    for (int c = tx; c < P; c += kMargCols) {
      double s = 0.0;
      if (c < m) {
        for (int k = 0; k < m; ++k) {
          const double g = gc ? 0.5 * ((double)gc[k * m + c] + (double)gc[c * m + k]) : 0.0;
          s = fma(hinv(i, k), g, s);
        }
      } else {
        for (int k = m; k < P; ++k) {
          const double g = Mg ? (double)Mg[(size_t)(k - m) * K + (c - m)] : 0.0;
          s = fma(hinv(i, k), g, s);
        }
      }
      X[(size_t)i * P + c] = s;
      if (i == c) diag[i] = s;
    }
  __syncthreads();

  // dH = g_ld Hinv - s2 X Hinv, its lower triangle (k ascending), written to both halves: exactly symmetric
  for (int i = ty; i < P; i += kMargRows)
    for (int j = tx; j <= i; j += kMargCols) {
      double s = 0.0;
      const double* xi = X + (size_t)i * P;
      for (int k = 0; k < P; ++k) s = fma(xi[k], hinv(k, j), s);
      const double v = gld * Hi[tri(i) + j] - s2 * s;
      if (i == j) {
        colbuf[i] = v * ((double)A[(size_t)i * P + i] + 1e-5);
        if (gA) gA[(size_t)i * P + i] = (float)((1.0 + mu) * v);
      } else if (gA) {
        const float f = (float)v;
        gA[(size_t)i * P + j] = f;
        gA[(size_t)j * P + i] = f;
      }
    }
  __syncthreads();
  // gdamping = sum_i dH_ii (A_ii + 1e-5), gsigma2 = trace(X): first wave, fixed order
  if (tid < 64) {
    double sd = 0.0, ss = 0.0;
    for (int i = tid; i < P; i += 64) {
      sd += colbuf[i];
      ss += diag[i];
    }
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) {
      sd += __shfl_xor(sd, sh, 64);
      ss += __shfl_xor(ss, sh, 64);
    }
    if (tid == 0) {
      if (a.gdamping) a.gdamping[b] = (float)sd;
      if (a.gsigma2) a.gsigma2[b] = (float)ss;
      a.status[b] = 0;
    }
  }
}

// ---- (c) ------------------------------------------------------------------------------------------------------------------------
// g == nullptr (no upstream) or status != 0: zeros.  Otherwise per 32-pixel tile: y = T b (marg_tile_y), then per 32-column block
// Cb of the output z = sum_{R >= Cb} T[R, Cb]^T y_R, one accumulator, R ascending, the 16 two-row steps of a block in register
// order; the lane's pixel holds columns 32 Cb + 8 j + 4 h + e of its row in register 4 j + e: one 16-byte store per j.
template <int NR>
__global__ __launch_bounds__(kDvThreads) void marg_grad_basis_kernel(const float* __restrict__ basis, const float* __restrict__ Tws,
                                                                     const float* __restrict__ sigma2, const int32_t* __restrict__ status,
                                                                     const float* __restrict__ g, float* __restrict__ gbasis, int N,
                                                                     int K, int tiles, int vec4_in, int vec4_out) {
  extern __shared__ __attribute__((aligned(16))) float mg_sT[];
  const int b = blockIdx.y, tid = threadIdx.x;
  float* out = gbasis + (size_t)b * N * K;
  if (g == nullptr || status[b] != 0) {                   // uniform per workgroup
    const long long total = (long long)N * K;
    for (long long i = (long long)blockIdx.x * kDvThreads + tid; i < total; i += (long long)gridDim.x * kDvThreads) out[i] = 0.f;
    return;
  }
  marg_fill_T_image<NR>(mg_sT, Tws + (size_t)b * K * K, K);
  __syncthreads();

  const int lane = tid & 63, wave = tid >> 6, nl = lane & 31, h = lane >> 5;
  const float s2 = sigma2 ? sigma2[b] : 1.f;
  const float* Bw = basis + (size_t)b * N * K;
  const float* gw = g + (size_t)b * N;

  for (int tile = blockIdx.x * kDvWaves + wave; tile < tiles; tile += gridDim.x * kDvWaves) {
    const int n = tile * 32 + nl;
    const bool valid = n < N;
    const float* row = Bw + (size_t)(valid ? n : 0) * K;
    const float gn = gw[valid ? n : 0];
    f32x16 acc[NR];
    marg_tile_y<NR>(mg_sT, row, valid, K, vec4_in, nl, h, acc);
    const float coef = 2.f * s2 * gn;
    // the lane's read of T^T at step (j, e): row 8 j + 4 h + e of the block, column nl, in the swizzled image; opaque per tile as
    // marg_tile_y's: hoisted out of the loop, the reads would occupy hundreds of registers
    int tcol[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      tcol[e] = (4 * h + e) * 32 + ((((nl >> 2) ^ (4 * h + e))) << 2) + (nl & 3);
      asm volatile("" : "+v"(tcol[e]));
    }
    float* orow = out + (size_t)(valid ? n : 0) * K;
#pragma unroll
    for (int Cb = 0; Cb < NR; ++Cb) {
      f32x16 z;
#pragma unroll
      for (int i = 0; i < 16; ++i) z[i] = 0.f;
#pragma unroll
      for (int R = Cb; R < NR; ++R) {
        const int blk = R * (R + 1) / 2 + Cb;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float t = mg_sT[blk * 1024 + j * 256 + tcol[e]];
            z = __builtin_amdgcn_mfma_f32_32x32x2f32(t, acc[R][4 * j + e], z, 0, 0, 0);
          }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c0 = 32 * Cb + 8 * j + 4 * h;
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = gn == 0.f ? 0.f : coef * z[4 * j + e];
        if (!valid) continue;
        if (vec4_out) {
          if (c0 < K) *reinterpret_cast<f32x4*>(orow + c0) = v;     // K % 4 == 0: the chunk is inside the row
        } else {
          if (c0 + 0 < K) orow[c0 + 0] = v[0];
          if (c0 + 1 < K) orow[c0 + 1] = v[1];
          if (c0 + 2 < K) orow[c0 + 2] = v[2];
          if (c0 + 3 < K) orow[c0 + 3] = v[3];
        }
      }
    }
  }
}

template <int NR>
static void launch_mg_basis(const float* basis, const float* T, const float* sigma2, const int32_t* status, const float* g, float* gbasis,
                            int B, int N, int K, hipStream_t s) {
  const size_t lds = (size_t)NR * (NR + 1) / 2 * 1024 * sizeof(float);
  if (lds > 64 * 1024)
    (void)hipFuncSetAttribute((const void*)marg_grad_basis_kernel<NR>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  const int tiles = (N + 31) / 32;
  // workgroups per window as marg_depthvar_kernel's: a pixel's arithmetic does not depend on which workgroup takes it
  int G = (2 * num_cus() + B - 1) / B;
  const int steps = (tiles + kDvWaves - 1) / kDvWaves;
  if (G > steps) G = steps;
  if (G < 1) G = 1;
  const int vec4_in = (K % 4 == 0) && (reinterpret_cast<uintptr_t>(basis) & 15u) == 0;
  const int vec4_out = (K % 4 == 0) && (reinterpret_cast<uintptr_t>(gbasis) & 15u) == 0;
  hipLaunchKernelGGL(marg_grad_basis_kernel<NR>, dim3(G, B), dim3(kDvThreads), lds, s, basis, T, sigma2, status, g, gbasis, N, K, tiles,
                     vec4_in, vec4_out);
}

int launch_marginals_grad(const banet_level_t* lv, const MargGradPlan& pl, const float* AtA, const float* damping, const float* sigma2,
                          const banet_marginals_grad_in_t* in, const banet_marginals_grad_out_t* out, void* ws, hipStream_t s) {
  char* w = static_cast<char*>(ws);
  const int B = lv->B, K = pl.K;
  const bool want_M = in->g_depth_var != nullptr && K > 0;
  const bool want_gb = out->gbasis != nullptr && K > 0;
  float* Mws = reinterpret_cast<float*>(w + pl.off_M);
  if (want_M) {
    MgGramArgs g;
    g.N = lv->N;
    g.K = K;
    g.chunk = pl.chunk;
    g.rows = pl.rows;
    g.pstride = pl.NP * 1024;
    g.basis = lv->basis;
    g.g = in->g_depth_var;
    g.part = reinterpret_cast<float*>(w + pl.off_part);
    switch (pl.NR) {
      case 1: launch_mg_gram<1, 1>(g, B, s); break;
      case 2: launch_mg_gram<2, 1>(g, B, s); break;
      case 3: launch_mg_gram<3, 1>(g, B, s); break;
      case 4: launch_mg_gram<4, 1>(g, B, s); break;
      case 5: launch_mg_gram<5, 4>(g, B, s); break;
      case 6: launch_mg_gram<6, 4>(g, B, s); break;
      case 7: launch_mg_gram<7, 4>(g, B, s); break;
      case 8: launch_mg_gram<8, 4>(g, B, s); break;
      default: return BANET_ERR_UNSUPPORTED;
    }
    if (hipGetLastError() != hipSuccess) return BANET_ERR_LAUNCH;
    hipLaunchKernelGGL(marg_grad_fold_kernel, dim3((pl.NP * 1024 + 255) / 256, B), dim3(256), 0, s, g.part, Mws, K, pl.NP, pl.rows,
                       g.pstride);
    if (hipGetLastError() != hipSuccess) return BANET_ERR_LAUNCH;
  }

  MgFactorArgs a;
  a.P = pl.P;
  a.m = pl.m;
  a.K = K;
  a.AtA = AtA;
  a.damping = damping;
  a.sigma2 = sigma2;
  a.g_cov = in->g_pose_cov;
  a.g_ld = in->g_logdet;
  a.Mws = want_M ? Mws : nullptr;
  a.gAtA = out->gAtA;
  a.gdamping = out->gdamping;
  a.gsigma2 = out->gsigma2;
  a.status = out->status;
  a.T = want_gb && in->g_depth_var ? reinterpret_cast<float*>(w + pl.off_T) : nullptr;
  a.Hinv = reinterpret_cast<double*>(w + pl.off_Hinv);
  a.X = reinterpret_cast<double*>(w + pl.off_X);
  a.big = pl.big ? reinterpret_cast<double*>(w + pl.off_big) : nullptr;
  if (pl.big) {
    hipLaunchKernelGGL(marg_grad_factor_kernel<true>, dim3(B), dim3(kMargThreads), pl.lds, s, a);
  } else {
    if (pl.lds > 64 * 1024)
      (void)hipFuncSetAttribute((const void*)marg_grad_factor_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds);
    hipLaunchKernelGGL(marg_grad_factor_kernel<false>, dim3(B), dim3(kMargThreads), pl.lds, s, a);
  }
  if (hipGetLastError() != hipSuccess) return BANET_ERR_LAUNCH;

  if (want_gb) {
#define BANET_MGB(n) \
  case n: launch_mg_basis<n>(lv->basis, a.T, sigma2, out->status, in->g_depth_var, out->gbasis, B, lv->N, K, s); break;
    switch (pl.NR) {
      BANET_MGB(1) BANET_MGB(2) BANET_MGB(3) BANET_MGB(4) BANET_MGB(5) BANET_MGB(6) BANET_MGB(7) BANET_MGB(8)
      default: return BANET_ERR_UNSUPPORTED;
    }
#undef BANET_MGB
    if (hipGetLastError() != hipSuccess) return BANET_ERR_LAUNCH;
  }
  return BANET_OK;
}

}  // namespace banet
