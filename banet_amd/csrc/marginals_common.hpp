// Device code shared by marginals.hip (banet_ba_marginals_f32) and marginals_grad.hip (banet_ba_marginals_grad_f32): the float64
// factorisation H = L L^T, Y = L^-1 of a window's damped normal matrix, and y = T b for 32 pixels per wave on the f32-input MFMA
// with T resident in swizzled LDS.  The statements are the forward kernels' own, lifted out unchanged: the backward recomputes
// what the forward computed, bit for bit.
#pragma once
#include "kernels.hpp"

namespace banet {

constexpr int kMargThreads = 1024;       // factor kernels: 16 columns x 64 rows of threads over the trailing blocks
constexpr int kMargCols = 16, kMargRows = kMargThreads / kMargCols;
constexpr int kDvThreads = 512;          // basis passes: 8 waves, 32 pixels each per step
constexpr int kDvWaves = kDvThreads / 64;
constexpr size_t kMargLdsMax = 160 * 1024;

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ int tri(int i) { return i * (i + 1) / 2; }   // offset of row i of a packed lower triangle

__host__ __device__ constexpr int marg_block_row(int p) {   // block p of a packed lower triangle of 32 x 32 blocks: its block row
  int R = 0;
  while ((R + 1) * (R + 2) / 2 <= p) ++R;
  return R;
}

// H = A + mu diag(diag(A) + 1e-5) from the lower triangle of A [P][P] into the packed triangle M, then its Cholesky factor in place
// (the diagonal of L in `diag`).  All kMargThreads threads of the workgroup; -> false (uniform) at a pivot <= 0 or not finite.
__device__ __forceinline__ bool marg_cholesky(const float* A, double mu, int P, double* M, double* colbuf, double* diag) {
  const int tid = threadIdx.x, tx = tid & (kMargCols - 1), ty = tid / kMargCols;
  for (int i = ty; i < P; i += kMargRows)
    for (int j = tx; j <= i; j += kMargCols) {
      double v = (double)A[(size_t)i * P + j];
      if (i == j) v = v + mu * (v + 1e-5);                // every diagonal entry, the last one included
      M[tri(i) + j] = v;
    }
  __syncthreads();

  // right-looking: column j scaled by 1 / L_jj, then the rank-1 update of the trailing lower triangle
  bool ok = true;
  for (int j = 0; j < P; ++j) {
    const double p = M[tri(j) + j];
    if (!(p > 0.0) || !(p < __builtin_huge_val())) {      // pivot <= 0 or not finite (a NaN / inf elsewhere reaches a later pivot)
      ok = false;
      break;                                              // uniform: every thread read the same pivot
    }
    const double d = sqrt(p);
    for (int i = j + 1 + tid; i < P; i += kMargThreads) {
      const double v = M[tri(i) + j] / d;
      M[tri(i) + j] = v;
      colbuf[i] = v;
    }
    if (tid == 0) diag[j] = d;
    __syncthreads();
    for (int i = j + 1 + ty; i < P; i += kMargRows) {
      const double li = colbuf[i];
      double* row = M + tri(i);
      for (int k = j + 1 + tx; k <= i; k += kMargCols) row[k] = fma(-li, colbuf[k], row[k]);
    }
    __syncthreads();
  }
  return ok;
}

// Y = L^-1 in place: column sweep of L Y = I.  Before step k, row i >= k holds the running right-hand side
// R[i,c] = delta_ic - sum_{j<k} L[i,j] Y[j,c] in its columns c < k (1 on the diagonal, implied) and L in its columns >= k.
__device__ __forceinline__ void marg_invert_lower(int P, double* M, double* colbuf, const double* diag) {
  const int tid = threadIdx.x, tx = tid & (kMargCols - 1), ty = tid / kMargCols;
  for (int k = 0; k < P; ++k) {
    const double d = diag[k];
    double* rk = M + tri(k);
    for (int c = tid; c < k; c += kMargThreads) rk[c] = rk[c] / d;
    for (int i = k + 1 + tid; i < P; i += kMargThreads) colbuf[i] = M[tri(i) + k];
    if (tid == 0) rk[k] = 1.0 / d;
    __syncthreads();
    for (int i = k + 1 + ty; i < P; i += kMargRows) {
      const double li = colbuf[i];
      double* row = M + tri(i);
      for (int c = tx; c <= k; c += kMargCols) row[c] = fma(-li, rk[c], c == k ? 0.0 : row[c]);
    }
    __syncthreads();
  }
}

// T [K][K] (lower triangular) into LDS as its NR (NR + 1) / 2 lower 32 x 32 blocks (rows / columns >= K as zeros; the all-zero upper
// blocks do not exist): block (R, Cb) at R (R + 1) / 2 + Cb, rows of 32 floats whose eight 16-byte chunks are XOR-swizzled by the
// row (ds_read_b128 of one chunk column by 32 rows: no bank conflicts, no padding -- K = 256 is 36 blocks = 144 KB).  The caller
// synchronises.
template <int NR>
__device__ __forceinline__ void marg_fill_T_image(float* sT, const float* __restrict__ T, int K) {
  constexpr int NB = NR * (NR + 1) / 2;
  for (int idx = threadIdx.x; idx < NB * 1024; idx += kDvThreads) {
    const int blk = idx >> 10, i = (idx >> 5) & 31, j = idx & 31;
    int R = 0;
    while ((R + 1) * (R + 2) / 2 <= blk) ++R;
    const int Cb = blk - R * (R + 1) / 2;
    const int r = 32 * R + i, c = 32 * Cb + j;
    const float v = (r < K && c <= r) ? T[r * K + c] : 0.f;
    sT[blk * 1024 + i * 32 + ((((j >> 2) ^ (i & 7))) << 2) + (j & 3)] = v;
  }
}

// A wave computes Y^T = T B^T for 32 pixels: A operand = T (lane l: row l & 31 of the block), B operand = the pixel's basis row
// (lane l: pixel l & 31), k slot l >> 5.  Both operands use the same column order inside a 32-column block, chunk 2 q + (l >> 5),
// element e: column 8 q + 4 (l >> 5) + e at MFMA step 4 q + e, so a lane's four steps are one 16-byte load on either side.
// The result has the pixel on the lane and the rows of T in the registers: register 4 j + e of acc[R] is row 32 R + 8 j + 4 h + e.
// `row`: the lane's basis row (any valid row when !valid: it is not read); nl = lane & 31, h = lane >> 5.
template <int NR>
__device__ __forceinline__ void marg_tile_y(const float* sT, const float* __restrict__ row, bool valid, int K, int vec4, int nl, int h,
                                            f32x16 (&acc)[NR]) {
  int trow = nl * 32;                                   // opaque per tile: the reads of T stay inside the loop (hoisted out of
  asm volatile("" : "+v"(trow));                        // it, the blocks of T would occupy up to 576 registers)
  // a lane's 16 floats of column block Cb: columns 32 Cb + 8 q + 4 h + e; zeros past the row's end and for pixels past N
  auto load_block = [&](int Cb, f32x4* dst) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c0 = 32 * Cb + 8 * q + 4 * h;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (vec4) {
        if (valid && c0 < K) v = *reinterpret_cast<const f32x4*>(row + c0);   // K % 4 == 0: the chunk is inside the row
      } else if (valid) {
        if (c0 + 0 < K) v[0] = row[c0 + 0];
        if (c0 + 1 < K) v[1] = row[c0 + 1];
        if (c0 + 2 < K) v[2] = row[c0 + 2];
        if (c0 + 3 < K) v[3] = row[c0 + 3];
      }
      dst[q] = v;
    }
  };
#pragma unroll
  for (int R = 0; R < NR; ++R)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[R][i] = 0.f;
  f32x4 cur[4], nxt[4];
  load_block(0, cur);
#pragma unroll
  for (int Cb = 0; Cb < NR; ++Cb) {
    if (Cb + 1 < NR) load_block(Cb + 1, nxt);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int R = Cb; R < NR; ++R) {                   // the blocks above the diagonal are zero: skipped
        const int blk = R * (R + 1) / 2 + Cb;
        const f32x4 t = *reinterpret_cast<const f32x4*>(&sT[blk * 1024 + trow + (((2 * q + h) ^ (nl & 7)) << 2)]);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[R] = __builtin_amdgcn_mfma_f32_32x32x2f32(t[e], cur[q][e], acc[R], 0, 0, 0);
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) cur[q] = nxt[q];
  }
}

}  // namespace banet
