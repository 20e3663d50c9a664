// Dense adjoint (driver, derivation and the kernel list in launch order: adjoint.hip): the symmetrised seed and the one
// GEMM-shaped piece -- adj_sym_kernel, adj_basis_kernel, adj_basis6_kernel, adj_basis_wide_kernel.
#include "adjoint_common.hpp"
#include "syrk_split.hpp"

namespace banet {
namespace adj {

namespace {

typedef __bf16 bf16x8a __attribute__((ext_vector_type(8)));

__global__ void adj_sym_kernel(const float* __restrict__ g, float* __restrict__ S, int P, size_t total) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const size_t b = e / ((size_t)P * P);
  const int r = (int)(e - b * P * P);
  const int i = r / P, j = r - i * P;
  S[e] = 0.5f * (g[e] + g[b * P * P + (size_t)j * P + i]);
}

// ---- the GEMM-shaped piece --------------------------------------------------------------------------------------------
template <int NK>   // KP = 16 NK >= K
__global__ __launch_bounds__(kBlock, 2) void adj_basis_kernel(const AdjArgs a) {
  extern __shared__ float Wl[];
  constexpr int KP = 16 * NK, LS = KP + 20, NB = NK + 1;   // LS: 4 kq groups 4 LS floats apart -> 16 banks apart
  const int b = blockIdx.y, K = a.lv.K, N = a.lv.N, P = 6 + K;
  {
    const float* __restrict__ S = a.S + (size_t)b * P * P;
    const float* __restrict__ gb = a.gb + (size_t)b * P;
    for (int idx = threadIdx.x; idx < KP * LS; idx += kBlock) {
      const int k = idx / LS, j = idx - k * LS;
      float v = 0.f;
      if (k < K) {
        if (j < K)
          v = S[(size_t)(6 + k) * P + 6 + j];
        else if (j >= KP && j < KP + 6)
          v = S[(size_t)(j - KP) * P + 6 + k];
        else if (j == KP + 6)
          v = gb[6 + k];
      }
      Wl[idx] = v;
    }
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, w = wave_id(), i = lane & 15, kq = lane >> 4;
  const float* __restrict__ bas = a.lv.basis + (size_t)b * N * K;
  float* __restrict__ z2 = a.z2 + (size_t)b * N * K;
  float* __restrict__ arec = a.arec + (size_t)b * N * 8;
  const int nrb = (N + 15) >> 4;
  for (int rb = blockIdx.x * kNumWaves + w; rb < nrb; rb += gridDim.x * kNumWaves) {
    const int n = rb * 16 + i;
    const bool okn = n < N;
    const float* __restrict__ row = bas + (size_t)(okn ? n : 0) * K;
    float av[NK][4];
#pragma unroll
    for (int kk = 0; kk < NK; ++kk)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int k = 16 * kk + 4 * kq + e;
        const float v = row[k < K ? k : 0];
        av[kk][e] = (okn && k < K) ? v : 0.f;
      }
    f32x4 acc[NB];
#pragma unroll
    for (int jb = 0; jb < NB; ++jb) acc[jb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < NK; ++kk) {
      asm volatile("" ::: "memory");   // keeps the LDS operand reads inside the row-block loop (LICM would hoist all 36 NK of them)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float* wl = Wl + (16 * kk + 4 * kq + e) * LS + i;
#pragma unroll
        for (int jb = 0; jb < NB; ++jb) acc[jb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[kk][e], wl[16 * jb], acc[jb], 0, 0, 0);
      }
    }
    // accumulator layout: lane (j = lane & 15, rq = lane >> 4) holds rows 4 rq + v, column 16 jb + j
    float zeta[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int nn = rb * 16 + 4 * kq + v;
      const bool ok = nn < N;
#pragma unroll
      for (int jb = 0; jb < NK; ++jb) {
        const int j = 16 * jb + i;
        if (ok && j < K) {
          zeta[v] = fmaf(acc[jb][v], bas[(size_t)nn * K + j], zeta[v]);
          z2[(size_t)nn * K + j] = 2.f * acc[jb][v];
        }
      }
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const float zt = row16_sum(zeta[v]);
      const int nn = rb * 16 + 4 * kq + v;
      if (nn < N) {
        if (i < 6) arec[(size_t)nn * 8 + i] = acc[NK][v];
        if (i == 6) arec[(size_t)nn * 8 + 7] = acc[NK][v];
        if (i == 7) arec[(size_t)nn * 8 + 6] = zt;
      }
    }
  }
}

// The same GEMM on the bf16 matrix pipe at fp32 accuracy (K <= 128): both operands are split exactly into three bf16 pieces and
// each 16 x 16 x 32 block takes six v_mfma_f32_16x16x32_bf16 (products exact in fp32, fp32 accumulate, the three terms below
// fp32 rounding dropped -- the scheme of syrk.hip / eqcon_grad.hip): 6 x 17 cycles against 8 x 32 for v_mfma_f32_16x16x4_f32.
// The seed block is split ONCE per workgroup into LDS as MFMA B operands ([k step][column block][piece][lane], 3 KB per block and
// k step: 108 KB at K = 128); a wave takes 16 pixels at a time: lane (m, kq) loads the 8 coefficients 32 ks + 8 kq .. + 7 of pixel
// m (32 contiguous bytes; the four kq lanes of a pixel read 128), splits them (registers) and accumulates.  512 threads: two
// waves per SIMD.  Epilogue as adj_basis_kernel (same accumulator layout).  kDevAdjFp32Mfma keeps the fp32-MFMA kernel (A/B).
constexpr int kAdjB6Waves = kAdjB6Threads / 64;
// REUSE (BANET_ADJOINT_REUSE_DEPTH_SEED; the later target frames of a multi-frame window): S_dd, gAtb_d and the basis are those of the
// previous call on this workspace, so z2 = 2 S_dd b, zeta and e are already there -- only the frame's own q = S_cd b is computed:
// one column block of MFMAs instead of NK + 1, no z2 traffic.
template <int NK, bool REUSE>   // KP = 16 NK >= K, NK <= 8
__global__ __launch_bounds__(kAdjB6Threads) void adj_basis6_kernel(const AdjArgs a) {
  constexpr int KS = (NK + 1) / 2, NB = NK + 1, KP = 16 * NK, JB0 = REUSE ? NK : 0;      // column blocks JB0 .. NK
  extern __shared__ __attribute__((aligned(16))) unsigned sB6[];   // [KS][NB][3][64] quads
  const int b = blockIdx.y, K = a.lv.K, N = a.lv.N, P = 6 + K;
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m = lane & 15, kq = lane >> 4;
  {
    const float* __restrict__ S = a.S + (size_t)b * P * P;
    const float* __restrict__ gb = a.gb + (size_t)b * P;
    for (int task = w; task < KS * NB; task += kAdjB6Waves) {
      const int ks = task / NB, jb = task - ks * NB;
      if (jb < JB0) continue;
      float vv[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int k = 32 * ks + 8 * kq + e, j = 16 * jb + m;     // seed[k][j], the layout of adj_basis_kernel's Wl
        float v = 0.f;
        if (k < K) {
          if (j < K)
            v = S[(size_t)(6 + k) * P + 6 + j];
          else if (j >= KP && j < KP + 6)
            v = S[(size_t)(j - KP) * P + 6 + k];
          else if (j == KP + 6)
            v = gb[6 + k];
        }
        vv[e] = v;
      }
      u32x4_t pc[3];
      split8_bf16x3(vv, pc);
#pragma unroll
      for (int t = 0; t < 3; ++t) *reinterpret_cast<u32x4_t*>(&sB6[(((ks * NB + jb) * 3 + t) * 64 + lane) * 4]) = pc[t];
    }
  }
  __syncthreads();
  const float* __restrict__ bas = a.lv.basis + (size_t)b * N * K;
  float* __restrict__ z2 = a.z2 + (size_t)b * N * K;
  float* __restrict__ arec = a.arec + (size_t)b * N * 8;
  const int nrb = (N + 15) >> 4;
  const bool k8 = (K & 7) == 0;
  auto load_a = [&](int rb, int ks, float (&v)[8]) __attribute__((always_inline)) {
    const int n = min(rb * 16 + m, N - 1), c0 = 32 * ks + 8 * kq;
    const float* p = bas + (size_t)n * K + c0;
    if (k8 && c0 + 8 <= K) {
      const f32x4 t0 = *reinterpret_cast<const f32x4*>(p), t1 = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[e] = t0[e];
        v[4 + e] = t1[e];
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = (c0 + e < K) ? p[e] : 0.f;
    }
    if (rb * 16 + m >= N) {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = 0.f;
    }
  };
  for (int rb = blockIdx.x * kAdjB6Waves + w; rb < nrb; rb += gridDim.x * kAdjB6Waves) {
    f32x4 acc[NB];
#pragma unroll
    for (int jb = 0; jb < NB; ++jb) acc[jb] = f32x4{0.f, 0.f, 0.f, 0.f};
    float av[8], an[8];
    load_a(rb, 0, av);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      asm volatile("" ::: "memory");   // the B operands are re-read from LDS every row block (hoisting all of them spills)
      u32x4_t pa[3];
      split8_bf16x3(av, pa);
      if (ks + 1 < KS) load_a(rb, ks + 1, an);
      constexpr int kTa[6] = {2, 0, 1, 1, 0, 0}, kTb[6] = {0, 2, 1, 0, 1, 0};   // smallest terms first
      u32x4_t pb[NB][3];
#pragma unroll
      for (int jb = JB0; jb < NB; ++jb)
#pragma unroll
        for (int t = 0; t < 3; ++t) pb[jb][t] = *reinterpret_cast<const u32x4_t*>(&sB6[(((ks * NB + jb) * 3 + t) * 64 + lane) * 4]);
      // round 6: the SEED block is the A operand and the basis rows the B operand -- S_dd is symmetric and the extra block is kept
      // transposed, so the LDS image serves either way -- which transposes the product: lane (m, rq) then holds coefficients
      // 16 jb + 4 rq .. + 3 of pixel m, four CONSECUTIVE floats: z2 and the basis re-read of zeta are 16-byte accesses (the old layout
      // -- lane = column, four rows -- needed 32 scattered 4-byte loads and stores per block: 56 % of the kernel's time by ablation)
#pragma unroll
      for (int t = 0; t < 6; ++t)       // term-major: consecutive MFMAs write different accumulators
#pragma unroll
        for (int jb = JB0; jb < NB; ++jb)
          acc[jb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8a, pb[jb][kTb[t]]), __builtin_bit_cast(bf16x8a, pa[kTa[t]]),
                                                            acc[jb], 0, 0, 0);
      if (ks + 1 < KS) {
#pragma unroll
        for (int e = 0; e < 8; ++e) av[e] = an[e];
      }
    }
    // accumulator layout: lane (m = pixel, rq = kq) holds z[pixel m][16 jb + 4 rq + v], v = 0..3
    const int nn = rb * 16 + m;
    const bool ok = nn < N;
    const size_t ro = (size_t)(ok ? nn : 0) * K;
    float zeta = 0.f;
    if constexpr (REUSE) {
      if (ok) {                            // the frame's q; (zeta, e) stay as the first frame's call left them
        float* __restrict__ ar = arec + (size_t)nn * 8;
        if (kq == 0) *reinterpret_cast<f32x4*>(ar) = acc[NK];
        if (kq == 1) {
          ar[4] = acc[NK][0];
          ar[5] = acc[NK][1];
        }
      }
      continue;
    }
    if ((K & 3) == 0) {
#pragma unroll
      for (int jb = 0; jb < NK; ++jb) {
        const int j = 16 * jb + 4 * kq;
        if (ok && j < K) {
          const f32x4 bq = *reinterpret_cast<const f32x4*>(bas + ro + j);
          zeta += acc[jb][0] * bq[0] + acc[jb][1] * bq[1] + acc[jb][2] * bq[2] + acc[jb][3] * bq[3];
          *reinterpret_cast<f32x4*>(z2 + ro + j) = 2.f * acc[jb];
        }
      }
    } else {
#pragma unroll
      for (int jb = 0; jb < NK; ++jb)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int j = 16 * jb + 4 * kq + v;
          if (ok && j < K) {
            zeta = fmaf(acc[jb][v], bas[ro + j], zeta);
            z2[ro + j] = 2.f * acc[jb][v];
          }
        }
    }
    zeta += __shfl_xor(zeta, 16, 64);      // the pixel's four coefficient quarters (lanes m, m + 16, m + 32, m + 48)
    zeta += __shfl_xor(zeta, 32, 64);
    if (ok) {                              // the extra block: rows 0..5 = q = S_cd b, row 6 = e = gAtb_d . b  (row 4 rq + v)
      float* __restrict__ ar = arec + (size_t)nn * 8;
      if (kq == 0) *reinterpret_cast<f32x4*>(ar) = acc[NK];
      if (kq == 1) {
        ar[4] = acc[NK][0];
        ar[5] = acc[NK][1];
        ar[7] = acc[NK][2];
        ar[6] = zeta;
      }
    }
  }
}

// K > 128: the seed block [K x (K+16)] no longer fits the LDS (K = 256: 282 KB), so its COLUMN blocks are taken in chunks of NBC
// (K = 256: 3 chunks of 6 / 6 / 5 blocks, 116 KB each) and the row blocks are walked once per chunk -- the basis is read NCH
// times (the backward of a K = 256 level is not the hot path; the forward reads it twice per iteration anyway).  A wave meets the
// same row blocks in every chunk, so zeta = b.S_dd b is accumulated in the pixel's record by the lane that owns it: first chunk
// writes, later chunks add, in chunk order -- deterministic.
template <int NK, int NBC>
__global__ __launch_bounds__(kBlock, 1) void adj_basis_wide_kernel(const AdjArgs a) {
  extern __shared__ float Wl[];
  constexpr int KP = 16 * NK, LSC = 16 * NBC + 20, NB = NK + 1, NCH = (NB + NBC - 1) / NBC;   // LSC mod 32 = 20 as in adj_basis_kernel
  static_assert((NBC & 1) == 0, "bank spreading of the kq groups needs 16 NBC = 0 mod 32");
  const int b = blockIdx.y, K = a.lv.K, N = a.lv.N, P = 6 + K;
  const float* __restrict__ S = a.S + (size_t)b * P * P;
  const float* __restrict__ gb = a.gb + (size_t)b * P;
  const int lane = threadIdx.x & 63, w = wave_id(), i = lane & 15, kq = lane >> 4;
  const float* __restrict__ bas = a.lv.basis + (size_t)b * N * K;
  float* __restrict__ z2 = a.z2 + (size_t)b * N * K;
  float* __restrict__ arec = a.arec + (size_t)b * N * 8;
  const int nrb = (N + 15) >> 4;
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    __syncthreads();   // the previous chunk's readers are done
    for (int idx = threadIdx.x; idx < KP * LSC; idx += kBlock) {
      const int k = idx / LSC, jj = idx - k * LSC, j = 16 * NBC * ch + jj;
      float v = 0.f;
      if (k < K && jj < 16 * NBC) {
        if (j < K)
          v = S[(size_t)(6 + k) * P + 6 + j];
        else if (j >= KP && j < KP + 6)
          v = S[(size_t)(j - KP) * P + 6 + k];
        else if (j == KP + 6)
          v = gb[6 + k];
      }
      Wl[idx] = v;
    }
    __syncthreads();
    for (int rb = blockIdx.x * kNumWaves + w; rb < nrb; rb += gridDim.x * kNumWaves) {
      const int n = rb * 16 + i;
      const bool okn = n < N;
      const float* __restrict__ row = bas + (size_t)(okn ? n : 0) * K;
      float av[NK][4];
#pragma unroll
      for (int kk = 0; kk < NK; ++kk)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int k = 16 * kk + 4 * kq + e;
          const float v = row[k < K ? k : 0];
          av[kk][e] = (okn && k < K) ? v : 0.f;
        }
      f32x4 acc[NBC];
#pragma unroll
      for (int jb = 0; jb < NBC; ++jb) acc[jb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < NK; ++kk) {
        asm volatile("" ::: "memory");   // as in adj_basis_kernel: keep the LDS operand reads inside the loop
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float* wl = Wl + (16 * kk + 4 * kq + e) * LSC + i;
#pragma unroll
          for (int jb = 0; jb < NBC; ++jb)
            if (NBC * ch + jb < NB) acc[jb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[kk][e], wl[16 * jb], acc[jb], 0, 0, 0);
        }
      }
      float zeta[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int nn = rb * 16 + 4 * kq + v;
        const bool ok = nn < N;
#pragma unroll
        for (int jb = 0; jb < NBC; ++jb) {
          const int j = 16 * (NBC * ch + jb) + i;
          if (NBC * ch + jb < NK && ok && j < K) {
            zeta[v] = fmaf(acc[jb][v], bas[(size_t)nn * K + j], zeta[v]);
            z2[(size_t)nn * K + j] = 2.f * acc[jb][v];
          }
        }
      }
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const float zt = row16_sum(zeta[v]);
        const int nn = rb * 16 + 4 * kq + v;
        if (nn < N) {
          if (i == 7) {
            if (ch == 0)
              arec[(size_t)nn * 8 + 6] = zt;
            else
              arec[(size_t)nn * 8 + 6] += zt;
          }
          if (NBC * ch <= NK && NK < NBC * (ch + 1)) {   // the chunk that holds the extra block [S_cd^T | gb]
            constexpr int je = NK % NBC;
            if (i < 6) arec[(size_t)nn * 8 + i] = acc[je][v];
            if (i == 6) arec[(size_t)nn * 8 + 7] = acc[je][v];
          }
        }
      }
    }
  }
}

}  // namespace

// > 64 KB of dynamic LDS needs the attribute; it belongs to the CURRENT device's function object, so it is set on every
// launch (like launch_spd_solve / launch_syrk_nb) rather than once per process behind a flag
template <typename Kernel>
void launch_seed_kernel(Kernel* k, int threads, const AdjArgs& a, const AdjPlan& pl, hipStream_t s) {
  if (pl.seed_lds > 64 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.seed_lds);
  hipLaunchKernelGGL(k, dim3(pl.seed_grid, a.lv.B), dim3(threads), pl.seed_lds, s, a);
}

void launch_adj_sym(const float* gAtA, float* S, int B, int P, hipStream_t s) {
  const size_t tot = (size_t)B * P * P;
  hipLaunchKernelGGL(adj_sym_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, gAtA, S, P, tot);
}

// (assert: a plan that returned BANET_OK names an instantiation of the lists below -- plan_detail::choose_adj_seed looked it up
//  in the same lists -- so BANET_ERR_UNSUPPORTED cannot be returned for it)
int launch_adj_seed(const AdjArgs& a, const AdjPlan& pl, hipStream_t s) {
  switch (pl.seed) {
    case kAdjSeedNone: return BANET_OK;
    case kAdjSeedF32:
      switch (pl.seed_nk) {
#define BANET_X(nk) \
  case nk: launch_seed_kernel(&adj_basis_kernel<nk>, kBlock, a, pl, s); return BANET_OK;
        BANET_ADJ_SEED_F32_LIST(BANET_X)
#undef BANET_X
      }
      break;
    case kAdjSeedB6:
      switch (pl.seed_nk) {
#define BANET_X(nk)                                                                        \
  case nk:                                                                                 \
    if (pl.reuse_z)                                                                        \
      launch_seed_kernel(&adj_basis6_kernel<nk, true>, kAdjB6Threads, a, pl, s);           \
    else                                                                                   \
      launch_seed_kernel(&adj_basis6_kernel<nk, false>, kAdjB6Threads, a, pl, s);          \
    return BANET_OK;
        BANET_ADJ_SEED_B6_LIST(BANET_X)
#undef BANET_X
      }
      break;
    case kAdjSeedWide:
      switch (pl.seed_nk) {
#define BANET_X(nk)                                                                                                                      \
  case nk:                                                                                                                               \
    static_assert((size_t)(16 * nk) * (16 * kAdjWideNBC + 20) * sizeof(float) <= 160 * 1024, "seed chunk exceeds the LDS");              \
    launch_seed_kernel(&adj_basis_wide_kernel<nk, kAdjWideNBC>, kBlock, a, pl, s);                                                       \
    return BANET_OK;
        BANET_ADJ_SEED_WIDE_LIST(BANET_X)
#undef BANET_X
      }
      break;
  }
  return BANET_ERR_UNSUPPORTED;
}

}  // namespace adj
}  // namespace banet
