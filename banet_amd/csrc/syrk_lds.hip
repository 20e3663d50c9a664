// ba_syrk_kernel<NB> -- LDS-tiled fp32 MFMA, any K <= 256 (the basis sizes the register kernels do not take): the depth-basis
// blocks of the normal equations on gfx950:
//   H_dd = sum_n s_n b_n b_n^T   (K x K, fp32 MFMA v_mfma_f32_16x16x4_f32, upper 16x16 blocks)
//   H_cd = sum_n u_n b_n^T       (6 x K, VALU rank-1 updates)
//   Atb_d = sum_n r_n b_n        (K)
// from the basis [N,K] (streamed once, 64-pixel tiles = 32 KB contiguous at K=128) and the
// per-pixel records (u,s,r) written by ba_gather_kernel.  This is the part of
// EquationConstruction (utils.cu:331-414) that involves J's depth columns jd (x) b_n
// (bundlenet.py:260-261), never materialised here.
// Pipeline: registers <- tile t+1 (global loads issued before the MFMA phase of tile t),
// LDS double buffer, one barrier per tile.  Wave w owns block rows w and NB-1-w of the upper
// triangle (NB+1 blocks: balanced); accumulators stay in registers for the whole kernel.
#include "syrk_common.hpp"

namespace banet {

template <int NB>
__global__ __launch_bounds__(kBlock, NB > 8 ? 1 : 2) void ba_syrk_kernel(const SyrkArgs a) {
  constexpr int PW = NB > 8 ? 2 : 1;    // block-row pairs per wave (NB = 16, K <= 256: rows {w, 15-w} and {w+4, 11-w})
  constexpr int KPAD = NB * 16;
  constexpr int KP = KPAD + 16;         // row stride: bank shift 16 per row -> conflict-free MFMA operand reads
  constexpr int KV = KPAD >= 64 ? KPAD / 64 : 1;
  constexpr int QPR = KPAD / 4;         // float4 per row
  constexpr int QT = (kTilePix * QPR + kBlock - 1) / kBlock;  // float4 per thread per tile
  constexpr int NSLOT = NB + 1;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* sB0 = smem;                          // [2][64][KP]
  float* sU0 = smem + 2 * kTilePix * KP;      // [2][64][8]
  const int b = blockIdx.y, g = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  if (a.active != nullptr && a.active[(size_t)b * a.active_stride] == 0) return;
  const int w = wave_id();
  const int N = a.N, K = a.K;
  const float* __restrict__ bas_b = a.basis + (size_t)b * N * K;
  const float* __restrict__ rec_b = a.rec + ((size_t)b * a.pairs + a.pass) * N * 8;   // this pass's pair
  const bool k4 = (K & 3) == 0;

  float hcd[7][KV];
#pragma unroll
  for (int i = 0; i < 7; ++i)
#pragma unroll
    for (int e = 0; e < KV; ++e) hcd[i][e] = 0.f;
  f32x4 acc[PW][NSLOT];
#pragma unroll
  for (int p = 0; p < PW; ++p)
#pragma unroll
    for (int q = 0; q < NSLOT; ++q) acc[p][q] = f32x4{0.f, 0.f, 0.f, 0.f};
  constexpr int npairs = (NB + 1) / 2;
  const bool mf_on = w < npairs && a.pass == 0;

  float4 pre[QT];
  float4 preu = make_float4(0.f, 0.f, 0.f, 0.f);
  auto load_tile = [&](int t) {
    const int pt0 = t * kTilePix;
    if (k4) {  // uniform; kept OUTSIDE the unrolled loop and branch-free inside it, so that all row
               // loads of the tile are in flight together (an `if` per load serialises them on vmcnt(0))
#pragma unroll
      for (int i = 0; i < QT; ++i) {
        const int idx = tid + i * kBlock;
        const int n = idx / QPR, q = idx - n * QPR;
        const bool ok = idx < kTilePix * QPR && pt0 + n < N && 4 * q < K;
        const float4 v = *reinterpret_cast<const float4*>(bas_b + (ok ? (size_t)(pt0 + n) * K + 4 * q : 0));
        pre[i] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    } else {
#pragma unroll
      for (int i = 0; i < QT; ++i) {
        const int idx = tid + i * kBlock;
        const int n = idx / QPR, q = idx - n * QPR;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (idx < kTilePix * QPR && pt0 + n < N) {
          const float* p = bas_b + (size_t)(pt0 + n) * K + 4 * q;
          if (4 * q + 0 < K) v.x = p[0];
          if (4 * q + 1 < K) v.y = p[1];
          if (4 * q + 2 < K) v.z = p[2];
          if (4 * q + 3 < K) v.w = p[3];
        }
        pre[i] = v;
      }
    }
    {
      const int n = tid >> 1;
      const bool ok = tid < 2 * kTilePix && pt0 + n < N;
      float4 v = *reinterpret_cast<const float4*>(rec_b + (ok ? (size_t)(pt0 + n) * 8 + 4 * (tid & 1) : 0));
      if (a.pass > 0) {   // H_cd of this pair only: no s (MFMA phase is off), no r
        if (tid & 1) v.w = 0.f;
      } else if ((tid & 1) && ok) {   // pass 0 of a multi-frame window: s and r summed over the pairs
        for (int i = 1; i < a.pairs; ++i) {
          const float4 o = *reinterpret_cast<const float4*>(rec_b + ((size_t)i * N + pt0 + n) * 8 + 4);
          v.z += o.z;
          v.w += o.w;
        }
      }
      preu = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto store_tile = [&](int buf) {
    float* sB = sB0 + buf * kTilePix * KP;
    float* sU = sU0 + buf * kTilePix * kUStrideS;
#pragma unroll
    for (int i = 0; i < QT; ++i) {
      const int idx = tid + i * kBlock;
      const int n = idx / QPR, q = idx - n * QPR;
      if (idx < kTilePix * QPR) *reinterpret_cast<float4*>(sB + n * KP + 4 * q) = pre[i];
    }
    if (tid < 2 * kTilePix) *reinterpret_cast<float4*>(sU + (tid >> 1) * kUStrideS + 4 * (tid & 1)) = preu;
  };

  int t = g;
  int cur = 0;
  if (t < a.tiles) {
    load_tile(t);
    store_tile(0);
  }
  __syncthreads();
  for (; t < a.tiles; t += a.Gs) {
    const bool more = t + a.Gs < a.tiles;
    if (more) load_tile(t + a.Gs);          // global loads in flight during the compute below
    const float* sB = sB0 + cur * kTilePix * KP;
    const float* sU = sU0 + cur * kTilePix * kUStrideS;
    // ---- H_cd += u_n b_n^T, Atb_d += r_n b_n ;  lane = coefficient(s), wave w pixels 16w.. ----
    {
      const int kb = lane * KV;
      if (kb < KPAD) {
#pragma unroll 4
        for (int i = 0; i < 16; ++i) {
          const int n = 16 * w + i;
          const float4 ua = *reinterpret_cast<const float4*>(sU + n * kUStrideS);
          const float4 ub = *reinterpret_cast<const float4*>(sU + n * kUStrideS + 4);
#pragma unroll
          for (int e = 0; e < KV; ++e) {
            const float bv = sB[n * KP + kb + e];
            hcd[0][e] = fmaf(ua.x, bv, hcd[0][e]);
            hcd[1][e] = fmaf(ua.y, bv, hcd[1][e]);
            hcd[2][e] = fmaf(ua.z, bv, hcd[2][e]);
            hcd[3][e] = fmaf(ua.w, bv, hcd[3][e]);
            hcd[4][e] = fmaf(ub.x, bv, hcd[4][e]);
            hcd[5][e] = fmaf(ub.y, bv, hcd[5][e]);
            hcd[6][e] = fmaf(ub.w, bv, hcd[6][e]);
          }
        }
      }
    }
    // ---- H_dd += sum_n s_n b_n b_n^T on the matrix cores ---------------------------------
    if (mf_on) {
      const int col = lane & 15, kq = lane >> 4;
#pragma unroll 2
      for (int kk = 0; kk < kTilePix / 4; ++kk) {
        const int pix = 4 * kk + kq;
        const float* row = sB + pix * KP + col;
        const float sv = sU[pix * kUStrideS + 6];
#pragma unroll
        for (int p = 0; p < PW; ++p) {
          const int i1 = w + 4 * p, i2 = NB - 1 - i1;
          if (i1 > i2) continue;  // wave-uniform (odd NB / fewer pairs than waves)
          const int n1 = NB - i1;
          const int nslots = (i2 != i1) ? NB + 1 : n1;
          const float a1 = sv * row[16 * i1];
          const float a2 = sv * row[16 * i2];
#pragma unroll
          for (int q = 0; q < NSLOT; ++q) {
            if (q < nslots) {  // wave-uniform
              const bool first = q < n1;
              const float bj = row[16 * (first ? i1 + q : i2 + q - n1)];
              acc[p][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(first ? a1 : a2, bj, acc[p][q], 0, 0, 0);
            }
          }
        }
      }
    }
    if (more) store_tile(cur ^ 1);
    __syncthreads();
    cur ^= 1;
  }

  // ---- epilogue ------------------------------------------------------------------------
  float* __restrict__ part = a.partials + ((size_t)b * a.Gs + g) * a.pstride;
  float* sH = smem;  // [4][8][KPAD] overlays the tile buffers (all waves are past the last barrier)
  {
    const int kb = lane * KV;
    if (kb < KPAD) {
#pragma unroll
      for (int i = 0; i < 7; ++i)
#pragma unroll
        for (int e = 0; e < KV; ++e) sH[(w * 8 + i) * KPAD + kb + e] = hcd[i][e];
    }
  }
  __syncthreads();
  for (int e = tid; e < 7 * K; e += kBlock) {
    const int i = e / K, k = e - i * K;
    if (i == 6 && a.pass > 0) continue;   // Atb_d comes from pass 0
    const int row = i < 6 ? 6 * a.pass + i : 6 * a.pairs;
    part[row * K + k] = (sH[(0 * 8 + i) * KPAD + k] + sH[(1 * 8 + i) * KPAD + k]) +
                        (sH[(2 * 8 + i) * KPAD + k] + sH[(3 * 8 + i) * KPAD + k]);
  }
  if (mf_on) {
    float* pd = part + (6 * a.pairs + 1) * K;
    const int col = lane & 15, rq = (lane >> 4) * 4;
#pragma unroll
    for (int p = 0; p < PW; ++p) {
      const int i1 = w + 4 * p, i2 = NB - 1 - i1;
      if (i1 > i2) continue;
      const int n1 = NB - i1;
      const int nslots = (i2 != i1) ? NB + 1 : n1;
#pragma unroll
      for (int q = 0; q < NSLOT; ++q) {
        if (q < nslots) {
          const bool first = q < n1;
          const int bi = first ? i1 : i2, bj = first ? i1 + q : i2 + q - n1;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int rr = 16 * bi + rq + r, cc = 16 * bj + col;
            if (rr < K && cc < K && (bj > bi || rr <= cc)) {
              pd[rr * K + cc] = acc[p][q][r];
              pd[cc * K + rr] = acc[p][q][r];
            }
          }
        }
      }
    }
  }
}

template <int NB>
static void launch_syrk_nb(const SyrkStep& st, const SyrkArgs& a, hipStream_t s) {
  auto k = ba_syrk_kernel<NB>;
  if (st.lds_attr) (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, st.lds);
  hipLaunchKernelGGL(k, dim3(st.gx, st.gy), dim3(st.block), st.lds, s, a);
}

int launch_syrk_lds_step(const SyrkStep& st, SyrkArgs a, hipStream_t s) {
  a.pass = st.j0;
  switch (st.t0) {
#define BANET_X(nb) \
  case nb: launch_syrk_nb<nb>(st, a, s); return BANET_OK;
    BANET_SYRK_LDS_LIST(BANET_X)
#undef BANET_X
  }
  return BANET_ERR_UNSUPPORTED;
}

}  // namespace banet
