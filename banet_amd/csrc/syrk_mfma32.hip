// ba_syrk_direct_kernel -- the fp32-MFMA predecessor of ba_syrk_bf16x6_kernel (syrk_bf16x6.hip), kept for A/B (kDevSyrkNoBf16x6).
#include "syrk_common.hpp"

namespace banet {

// --------------------------------------------------------------------------------------
// ba_syrk_direct_kernel -- K = 64 KH (the reference's K = 128 is KH = 2): the same sums without LDS
// and without workgroup barriers.  A wave owns a contiguous run of pixel quads and ALL 16x16
// blocks of the upper triangle (36 for K = 128: 144 accumulator registers).  Lane (m, kq) of a
// quad loads pixel 4q + kq's coefficients {4m..4m+3} + 64h as 16-byte loads (a wave instruction =
// 4 x 256 contiguous bytes) and uses every loaded value as the A operand (scaled by s_n) of one
// "virtual" block row and the B operand of one virtual block column: virtual block i' holds the
// coefficients 64 (i' >> 2) + 4 m + (i' & 3), m = 0..15 -- a permutation that is undone when the
// partial is written.  Loads run one batch of quads ahead of the matrix cores (register double
// buffer); H_cd / Atb_d are packed-fp32 FMAs issued in the shadow of the MFMAs.
// --------------------------------------------------------------------------------------
constexpr int kSyrkBatch = 4;

template <int KH, int PAIRS>
__global__ __launch_bounds__(kBlock, 1) void ba_syrk_direct_kernel(const SyrkArgs a) {
  constexpr int NBV = 4 * KH, NPAIR = NBV * (NBV + 1) / 2, K = 64 * KH, NV = 4 * KH;
  constexpr int NU = (PAIRS + 1) / 2;   // record block rows: rows 0..5 / 6..11 = u of pairs 2j / 2j+1; block row 0 rows 12+i = r_i
  __shared__ float sAcc[NPAIR + NU * NBV][4][64];
  const int b = blockIdx.y, g = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  if (a.active != nullptr && a.active[(size_t)b * a.active_stride] == 0) return;
  const int w = wave_id();
  const int N = a.N;
  const int m = lane & 15, kq = lane >> 4;
  const float* __restrict__ bas_b = a.basis + (size_t)b * N * K;
  const float* __restrict__ rec_b = a.rec + (size_t)b * PAIRS * N * 8;
  // record word this lane feeds to block row j: (pair, word) or none
  size_t uoff[NU];
  bool uon[NU];
#pragma unroll
  for (int j = 0; j < NU; ++j) {
    int pair = -1, word = 0;
    if (m < 12) {
      pair = 2 * j + m / 6;
      word = m % 6;
    } else if (j == 0) {
      pair = m - 12;
      word = 7;
    }
    uon[j] = pair >= 0 && pair < PAIRS;
    uoff[j] = uon[j] ? (size_t)pair * N * 8 + word : 0;
  }

  f32x4 acc[NPAIR];      // H_dd, upper triangle of virtual blocks
  f32x4 acu[NU][NBV];    // record block rows against every virtual block column
#pragma unroll
  for (int q = 0; q < NPAIR; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < NU; ++j)
#pragma unroll
    for (int q = 0; q < NBV; ++q) acu[j][q] = f32x4{0.f, 0.f, 0.f, 0.f};

  // this wave's run of quads
  const int nq = (N + 3) >> 2, nwaves = a.Gs * kNumWaves, gw = g * kNumWaves + w;
  const int q0 = (int)(((long long)nq * gw) / nwaves), q1 = (int)(((long long)nq * (gw + 1)) / nwaves);

  // register double buffer, kSyrkBatch quads per batch: the loads of batch t+1 are issued (and pinned
  // with a scheduling barrier) before batch t is multiplied, so they have a whole batch of MFMAs
  // (kSyrkBatch x 44 x 32 cycles) to arrive
  struct Batch {
    f32x4 pb[kSyrkBatch][KH];
    float ps[kSyrkBatch][PAIRS], pu[kSyrkBatch][NU];
  };
  auto issue = [&](Batch& B_, int q) __attribute__((always_inline)) {
#pragma unroll
    for (int d = 0; d < kSyrkBatch; ++d) {
      const int pix = 4 * (q + d) + kq;
      const size_t p = (q + d < q1 && pix < N) ? (size_t)pix : 0;
#pragma unroll
      for (int h = 0; h < KH; ++h)
        B_.pb[d][h] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(bas_b + p * K + 64 * h + 4 * m));
#pragma unroll
      for (int i = 0; i < PAIRS; ++i) B_.ps[d][i] = rec_b[((size_t)i * N + p) * 8 + 6];
#pragma unroll
      for (int j = 0; j < NU; ++j) B_.pu[d][j] = rec_b[p * 8 + uoff[j]];
    }
  };
  auto consume = [&](const Batch& B_, int q) __attribute__((always_inline)) {
#pragma unroll
    for (int d = 0; d < kSyrkBatch; ++d) {
      const bool ok = q + d < q1 && 4 * (q + d) + kq < N;
      float ssum = B_.ps[d][0];
#pragma unroll
      for (int i = 1; i < PAIRS; ++i) ssum += B_.ps[d][i];
      const float sv = ok ? ssum : 0.f;                     // zero records switch the pixel off
      float bv[NV], av[NV];
#pragma unroll
      for (int h = 0; h < KH; ++h)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          bv[4 * h + e] = B_.pb[d][h][e];
          av[4 * h + e] = sv * B_.pb[d][h][e];
        }
      int idx = 0;
#pragma unroll
      for (int bi = 0; bi < NBV; ++bi)
#pragma unroll
        for (int bj = bi; bj < NBV; ++bj) {
          acc[idx] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[bi], bv[bj], acc[idx], 0, 0, 0);
          ++idx;
        }
#pragma unroll
      for (int j = 0; j < NU; ++j) {
        const float uv = (ok && uon[j]) ? B_.pu[d][j] : 0.f;
#pragma unroll
        for (int bj = 0; bj < NBV; ++bj) acu[j][bj] = __builtin_amdgcn_mfma_f32_16x16x4f32(uv, bv[bj], acu[j][bj], 0, 0, 0);
      }
    }
  };
#ifdef BANET_TIMING
  unsigned long long tm0, tr0;
  asm volatile("s_memtime %0\n\ts_memrealtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(tm0), "=s"(tr0)::"memory");
#endif
  Batch R0, R1;
  issue(R0, q0);
  for (int q = q0; q < q1; q += 2 * kSyrkBatch) {
    issue(R1, q + kSyrkBatch);
    __builtin_amdgcn_sched_barrier(0);   // the scheduler would otherwise sink the loads next to their use
    consume(R0, q);
    __builtin_amdgcn_sched_barrier(0);
    issue(R0, q + 2 * kSyrkBatch);
    __builtin_amdgcn_sched_barrier(0);
    consume(R1, q + kSyrkBatch);
    __builtin_amdgcn_sched_barrier(0);
  }
#ifdef BANET_TIMING
  unsigned long long tm1, tr1;
  asm volatile("s_memtime %0\n\ts_memrealtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(tm1), "=s"(tr1)::"memory");
#endif

  // ---- epilogue: add the 4 waves in fixed order through LDS, un-permute, publish ---------------
  for (int ww = 0; ww < kNumWaves; ++ww) {
    if (w == ww) {
#pragma unroll
      for (int q = 0; q < NPAIR; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r) sAcc[q][r][lane] = (ww == 0 ? 0.f : sAcc[q][r][lane]) + acc[q][r];
#pragma unroll
      for (int j = 0; j < NU; ++j)
#pragma unroll
        for (int q = 0; q < NBV; ++q)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float* c = &sAcc[NPAIR + j * NBV + q][r][lane];
            *c = (ww == 0 ? 0.f : *c) + acu[j][q][r];
          }
    }
    __syncthreads();
  }
  float* __restrict__ part = a.partials + ((size_t)b * a.Gs + g) * a.pstride;
  // thread (w, lane) publishes accumulator register r = w of every block: row 4 kq + r, column m
  const int r = w, brow = 4 * kq + r;
#pragma unroll
  for (int j = 0; j < NU; ++j) {
    const int pair = 2 * j + brow / 6;
    if (brow < 12 && pair < PAIRS) {
#pragma unroll
      for (int bj = 0; bj < NBV; ++bj)
        part[(6 * pair + brow % 6) * K + 64 * (bj >> 2) + 4 * m + (bj & 3)] = sAcc[NPAIR + j * NBV + bj][r][lane];
    }
  }
  if (brow == 12) {   // Atb_d: rows 12 + i of block row 0 hold r_i; add the pairs in order (kq = 3, register i)
#pragma unroll
    for (int bj = 0; bj < NBV; ++bj) {
      float v = sAcc[NPAIR + bj][0][lane];
#pragma unroll
      for (int i = 1; i < PAIRS; ++i) v += sAcc[NPAIR + bj][i][lane];
      part[6 * PAIRS * K + 64 * (bj >> 2) + 4 * m + (bj & 3)] = v;
    }
  }
#ifdef BANET_TIMING
  __syncthreads();
  if (tid == 0) {   // development aid (tools/time_syrk.py): overwrites 3 words of the partial
    part[0] = (float)(tm1 - tm0);
    part[1] = (float)(tr1 - tr0);
    part[2] = (float)(q1 - q0);
  }
  return;
#endif
  float* pd = part + (6 * PAIRS + 1) * K;
  {
    int idx = 0;
    for (int bi = 0; bi < NBV; ++bi)
      for (int bj = bi; bj < NBV; ++bj) {
        const int rr = 64 * (bi >> 2) + 4 * brow + (bi & 3), cc = 64 * (bj >> 2) + 4 * m + (bj & 3);
        const float v = sAcc[idx][r][lane];
        if (bj > bi || rr <= cc) {
          pd[rr * K + cc] = v;
          pd[cc * K + rr] = v;
        }
        ++idx;
      }
  }
}

template <int KH>
static int launch_direct(const SyrkStep& st, const SyrkArgs& a, hipStream_t s) {
  const dim3 grid(st.gx, st.gy), block(st.block);
  switch (st.t1) {
#define BANET_X(p) \
  case p: hipLaunchKernelGGL((ba_syrk_direct_kernel<KH, p>), grid, block, 0, s, a); return BANET_OK;
    BANET_SYRK_FRAMES_LIST(BANET_X)
#undef BANET_X
  }
  return BANET_ERR_UNSUPPORTED;
}

int launch_syrk_mfma32_step(const SyrkStep& st, const SyrkArgs& a, hipStream_t s) {
  switch (st.t0) {
#define BANET_X(kh) \
  case kh: return launch_direct<kh>(st, a, s);
    BANET_SYRK_MFMA32_LIST(BANET_X)
#undef BANET_X
  }
  return BANET_ERR_UNSUPPORTED;
}

}  // namespace banet
