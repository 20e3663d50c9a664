// What the two solve translation units share (solve.hip: ba_solve_update_kernel; spd_solve.hip: spd_solve_kernel): the wave
// reductions on DPP + permlane swaps, block_sum_n, rdlane, the cycle-counter macro of the -DBANET_TIMING build and the blocked LDL^T.
// Workgroups of kSolveThreads threads; strides and scratch offsets come from the SolvePlan (solve_plan.hpp).
#pragma once
#include <type_traits>

#include "kernels.hpp"

namespace banet {

#ifdef BANET_TIMING
__device__ __forceinline__ unsigned long long stick() {
  unsigned long long t;
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  return t;
}
#define STICK(v) const unsigned long long v = stick()
#else
#define STICK(v)
#endif

// sum over the 64 lanes without the LDS crossbar; every lane gets the total
__device__ __forceinline__ float wave_sum_fast(float v) {
  v = row16_sum(v);
  v = bfly_merge(v, v, 16);
  return bfly_merge(v, v, 32);
}

// max / min over the 64 lanes on DPP + permlane swaps (every lane gets the result)
__device__ __forceinline__ float wave_max_fast(float v) {
  v = fmaxf(v, dpp_mov<kDppRor8>(v));
  v = fmaxf(v, dpp_mov<kDppHalfMirror>(v));
  v = fmaxf(v, dpp_mov<kDppXor2>(v));
  v = fmaxf(v, dpp_mov<kDppXor1>(v));
  float a = v, b = v;
  asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
  v = fmaxf(a, b);
  a = v;
  b = v;
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
  return fmaxf(a, b);
}
__device__ __forceinline__ int wave_min_fast(int v) {
  auto dpp = [](int x, auto ctrl) { return __builtin_amdgcn_update_dpp(0x7fffffff, x, decltype(ctrl)::value, 0xF, 0xF, false); };
  v = min(v, dpp(v, std::integral_constant<int, kDppRor8>{}));
  v = min(v, dpp(v, std::integral_constant<int, kDppHalfMirror>{}));
  v = min(v, dpp(v, std::integral_constant<int, kDppXor2>{}));
  v = min(v, dpp(v, std::integral_constant<int, kDppXor1>{}));
  int a = v, b = v;
  asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
  v = min(a, b);
  a = v;
  b = v;
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
  return min(a, b);
}

// block-wide sums of NV values per thread (fixed order); sr: 16 * NV floats, a different buffer than the previous call's
template <int NV>
__device__ __forceinline__ void block_sum_n(float (&v)[NV], float* sr) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const float t = wave_sum_fast(v[k]);
    if (lane == 0) sr[wv * NV + k] = t;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < kSolveWaves; ++i) t += sr[i * NV + k];
    v[k] = t;
  }
}

__device__ __forceinline__ float rdlane(float v, int l) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}

// --------------------------------------------------------------------------------------
// Blocked LDL^T for the bundle variants (32 <= n): the damped normal matrix is symmetric positive
// definite (PSD Gram matrix + positive damping), so the pivoted LU of tf.matrix_solve
// (bundlenet.py:267) reduces to elimination in natural order; same solution up to rounding
// (checked at 1e-4 by the parity tests).  Storage: lower triangle of A in rows 0..n-1, the right-hand
// side as ROW n -- eliminating it like any other row leaves w = D^-1 L^-1 b there, the right-hand
// side of the back substitution L^T x = w.  Right-looking, 16 columns per panel:
//   A  wave 0 factors the 16x16 diagonal block in registers (lane = row, pivot rows broadcast with
//      v_readlane) and publishes U11 and the reciprocal pivots;
//   B  one thread per remaining row eliminates its 16 panel entries against U11 (broadcast LDS
//      reads), keeps the multipliers in place and the unscaled entries d_j l_ij as W^T;
//   C  trailing update A22 -= L21 W (lower triangle + rhs row), one 4x4 register tile per thread.
// 3 barriers per panel instead of one per column, and no redundant upper-triangle work.
// --------------------------------------------------------------------------------------
// ld, ldw: SolvePlan's strides for n unknowns; scratch: kPanel * ldw + kLdltFixedFloats floats
__device__ __attribute__((always_inline)) void ldlt_solve_blocked(float* A, int ld, int ldw, int n, float* x, float* scratch) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int m = n + 1;                 // rows including the right-hand side
  float* sWT = scratch;                // [16][ldw]
  float* sU = sWT + kPanel * ldw;      // [16][16]  upper part of the factored diagonal block
  float* sDinv = sU + kPanel * kPanel; // [16]
#ifdef BANET_TIMING
  __shared__ float sDbg[4];
  float dA = 0.f, dB = 0.f, dC = 0.f;
#endif
  for (int k0 = 0; k0 < n; k0 += kPanel) {
    const int nb = min(kPanel, n - k0);
    STICK(pa);
    // ---- A: diagonal block (wave 0) ------------------------------------------------------
    if (tid < 64) {
      const int row = lane & 15;
      float a[kPanel];
#pragma unroll
      for (int c = 0; c < kPanel; ++c) {
        const bool in = row < nb && c < nb;
        const int r = k0 + row, cc = k0 + c;
        const int idx = in ? (c <= row ? r * ld + cc : cc * ld + r) : 0;   // symmetric read from the lower triangle
        const float v = A[idx];
        a[c] = in ? v : (c == row ? 1.f : 0.f);                          // identity padding of a partial panel
      }
      float myinv = 1.f;
#pragma unroll
      for (int j = 0; j < kPanel; ++j) {
        // pivot row j: all broadcasts first, then the arithmetic (a v_readlane feeding the very next VALU instruction costs
        // wait states; batched, the 16 - j reads pipeline)
        float pr[kPanel];
#pragma unroll
        for (int c = j; c < kPanel; ++c) pr[c] = rdlane(a[c], j);
        __builtin_amdgcn_sched_barrier(0);
        const float inv = __builtin_amdgcn_rcpf(pr[j]);                  // v_rcp_f32: <= 1 ulp
        if (row == j) myinv = inv;
        const float l = row > j ? a[j] * inv : 0.f;
#pragma unroll
        for (int c = j + 1; c < kPanel; ++c) a[c] = fmaf(-l, pr[c], a[c]);
        a[j] = row > j ? l : a[j];
        __builtin_amdgcn_sched_barrier(0);
      }
      if (lane < kPanel) {
        sDinv[row] = myinv;
#pragma unroll
        for (int c = 0; c < kPanel; ++c) {
          if (c <= row) {
            if (row < nb && c < nb) A[(k0 + row) * ld + k0 + c] = a[c];
          } else {
            sU[row * kPanel + c] = a[c];
          }
        }
      }
    }
    __syncthreads();
    STICK(pb);
    // ---- B: panel rows below the block ---------------------------------------------------
    const int base = k0 + nb, mrem = m - base;
    for (int t = tid; t < mrem; t += kSolveThreads) {
      float* rowp = A + (base + t) * ld + k0;
      float a[kPanel];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 v = *reinterpret_cast<const float4*>(rowp + 4 * q);
        a[4 * q + 0] = (4 * q + 0 < nb) ? v.x : 0.f;
        a[4 * q + 1] = (4 * q + 1 < nb) ? v.y : 0.f;
        a[4 * q + 2] = (4 * q + 2 < nb) ? v.z : 0.f;
        a[4 * q + 3] = (4 * q + 3 < nb) ? v.w : 0.f;
      }
#pragma unroll
      for (int j = 0; j < kPanel; ++j) {
        sWT[j * ldw + t] = a[j];                        // d_j l_ij
        const float l = a[j] * sDinv[j];
        a[j] = l;
#pragma unroll
        for (int c = j + 1; c < kPanel; ++c) a[c] = fmaf(-l, sU[j * kPanel + c], a[c]);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q)
        *reinterpret_cast<float4*>(rowp + 4 * q) = make_float4(a[4 * q], a[4 * q + 1], a[4 * q + 2], a[4 * q + 3]);
    }
    __syncthreads();
    STICK(pc);
    // ---- C: trailing update, 4x4 tiles of the lower triangle ---------------------------------
    const int mt = (mrem + 3) >> 2, ntiles = mt * (mt + 1) / 2;
    for (int t = tid; t < ntiles; t += kSolveThreads) {
      int I4 = (int)((sqrtf(8.f * (float)t + 1.f) - 1.f) * 0.5f);
      while ((I4 + 1) * (I4 + 2) / 2 <= t) ++I4;
      while (I4 * (I4 + 1) / 2 > t) --I4;
      const int C4 = t - I4 * (I4 + 1) / 2;
      float acc[4][4];
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = 0.f;
      const float* Lp = A + (base + 4 * I4) * ld + k0;
      const float* Wp = sWT + 4 * C4;
#pragma unroll
      for (int j4 = 0; j4 < 4; ++j4) {
        float4 Lr[4], Wj[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) Lr[r] = *reinterpret_cast<const float4*>(Lp + r * ld + 4 * j4);
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) Wj[jj] = *reinterpret_cast<const float4*>(Wp + (4 * j4 + jj) * ldw);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float lr[4] = {Lr[r].x, Lr[r].y, Lr[r].z, Lr[r].w};
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) {
            acc[r][0] = fmaf(lr[jj], Wj[jj].x, acc[r][0]);
            acc[r][1] = fmaf(lr[jj], Wj[jj].y, acc[r][1]);
            acc[r][2] = fmaf(lr[jj], Wj[jj].z, acc[r][2]);
            acc[r][3] = fmaf(lr[jj], Wj[jj].w, acc[r][3]);
          }
        }
      }
      float* Cp = A + (base + 4 * I4) * ld + base + 4 * C4;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float4 cv = *reinterpret_cast<float4*>(Cp + r * ld);
        cv.x -= acc[r][0];
        cv.y -= acc[r][1];
        cv.z -= acc[r][2];
        cv.w -= acc[r][3];
        *reinterpret_cast<float4*>(Cp + r * ld) = cv;
      }
    }
    __syncthreads();
#ifdef BANET_TIMING
    {
      STICK(pd);
      dA += (float)(pb - pa);
      dB += (float)(pc - pb);
      dC += (float)(pd - pc);
    }
#endif
  }
  STICK(pe);
  // ---- back substitution L^T x = w (wave 0), panels from the last to the first ---------------
  if (tid < 64) {
    const int li = lane & 15, part = lane >> 4;
    const int npan = (n + kPanel - 1) / kPanel;
    for (int p = npan - 1; p >= 0; --p) {
      const int k0 = p * kPanel, nb = min(kPanel, n - k0), base = k0 + nb;
      // t_l = w_l - sum_{j >= base} L[j][k0 + l] x_j : 4 interleaved slices of j, one per 16-lane row
      float tsum = 0.f;
      {
        const float* Lc = A + k0 + (li < nb ? li : 0);
        float t0 = 0.f, t1 = 0.f, t2 = 0.f, t3 = 0.f;
        int j = base + part;
        for (; j + 12 < n; j += 16) {   // 4 independent loads in flight per lane
          const float l0 = Lc[j * ld], l1 = Lc[(j + 4) * ld], l2 = Lc[(j + 8) * ld], l3 = Lc[(j + 12) * ld];
          t0 = fmaf(l0, x[j], t0);
          t1 = fmaf(l1, x[j + 4], t1);
          t2 = fmaf(l2, x[j + 8], t2);
          t3 = fmaf(l3, x[j + 12], t3);
        }
        for (; j < n; j += 4) t0 = fmaf(Lc[j * ld], x[j], t0);
        tsum = li < nb ? (t0 + t1) + (t2 + t3) : 0.f;
      }
      tsum += __shfl_xor(tsum, 16, 64);
      tsum += __shfl_xor(tsum, 32, 64);
      float tl = (li < nb ? A[n * ld + k0 + li] : 0.f) - tsum;
      float col[kPanel];   // column l of the block's unit lower triangle: L[k0 + i][k0 + l], i > l
#pragma unroll
      for (int i = 0; i < kPanel; ++i) col[i] = (i > li && i < nb) ? A[(k0 + i) * ld + k0 + li] : 0.f;
#pragma unroll
      for (int i = kPanel - 1; i >= 1; --i) {
        const float xi = rdlane(tl, i);      // final once rows > i have been applied
        tl = fmaf(-col[i], xi, tl);
      }
      if (lane < nb) x[k0 + lane] = tl;
    }
  }
  __syncthreads();
#ifdef BANET_TIMING
  {
    STICK(pf);
    if (tid == 0) {
      sDbg[0] = dA;
      sDbg[1] = dB;
      sDbg[2] = dC;
      sDbg[3] = (float)(pf - pe);
      x[n + 0] = dA; x[n + 1] = dB; x[n + 2] = dC; x[n + 3] = (float)(pf - pe);
    }
    __syncthreads();
  }
#endif
}

}  // namespace banet
