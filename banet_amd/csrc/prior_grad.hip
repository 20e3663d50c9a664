// The backward of the prior term (include/banet_hip.h (5e); plan: prior_grad_plan.hpp; forward: prior.hip).
//   every iteration (banet_prior_add_grad_f32)   prior_add_grad_kernel, one wave per row i of Le: row i of gLe, gee[i], and the
//                   column sum gWc[i] -= sum_r Le[r,i] gAtb'[m+r] -- lane l owns the four-row chunks c = l, l + 64, ..., ONE fma
//                   chain over its rows ascending, the 64 chains joined by wave_sum (ba_prior_add_kernel's scheme, transposed).
//   once per level  (banet_prior_terms_grad_f32)
//     prior_grad_prep_kernel    one workgroup per window: Gh = fl(scale fl(1/2 fl(gLe + gLe^T))) (exactly symmetric) and
//                   gh = fl(scale gee) into the workspace; gLambda, geta; gscale in float64 on the float32 inputs, one fma chain per
//                   thread over its elements ascending, then a fixed tree over the threads.
//     prior_grad_pixel_kernel   y = Gh b_n for 32 pixels per wave on v_mfma_f32_32x32x2_f32, the operand layout of marg_tile_y /
//                   marg_grad_basis_kernel (marginals_common.hpp, marginals_grad.hip): the pixel on the lane, rows of y in the
//                   accumulator registers.  Gh is symmetric: only its NR (NR + 1) / 2 lower 32 x 32 blocks live in LDS (the swizzled
//                   image of marg_fill_T_image, diagonal blocks whole; 144 KB + gh at K = 256).  For the column block Cb of the basis
//                   row, loaded once, y_R += Gh[R,Cb] b_Cb reads block (R, Cb) row-wise (16-byte reads) for R >= Cb and block (Cb, R)
//                   column-wise (4-byte reads) for R < Cb: one accumulator chain per R, Cb ascending -- first the blocks left of
//                   the diagonal and the diagonal one, then the transposed ones below it.  A loaded block's registers are the
//                   B operand of both reads.  p = b . gh rides along per lane; q = b . y runs over the finished accumulators
//                   (K <= 128: the basis row kept in registers, loaded once; above, a second read of the row the wave has just
//                   read, only when gweight is asked for).  The two half-waves of a pixel are added last.  The gbasis row is
//                   read (accumulate mode) and written once, 16 bytes per lane and step.  K <= 128 with 16-byte accesses
//                   compiles without scratch (190 registers at K = 128); the K > 160 and the 4-byte instantiations of K > 96
//                   still spill (76 .. 992 bytes per lane), which costs them time, not bits -- profiles/prior_grad.txt.
// No atomics; every output element is written by exactly one lane; a pixel's arithmetic does not depend on which workgroup takes
// it, nor on B, nor on which outputs are asked for.
#include "marginals_common.hpp"

namespace banet {

// ---- every iteration ----------------------------------------------------------------------------------------------------------------
struct PriorAddGradArgs {
  int K, m, P;
  int rows;          // B K
  int overwrite;     // gLe / gee written, not accumulated
  const float* Le;   // [B][K][K]
  const float* Wc;   // [B][K]
  const float* gAtA; // [B][P][P]
  const float* gAtb; // [B][P]
  float* gLe;        // [B][K][K]
  float* gee;        // [B][K]
  float* gWc;        // [B][K]
};

// V4: Wc and the row of gLe by 16-byte accesses (K % 4 == 0, both 16-byte aligned); otherwise 4-byte accesses of the same elements
// -- the arithmetic per element is the same statement.  gAtA's depth block starts (m + i) P + m floats into the window: 4-byte reads.
template <bool V4>
__global__ __launch_bounds__(kPriorThreads) void prior_add_grad_kernel(const PriorAddGradArgs a) {
  const int row = blockIdx.x * (kPriorThreads / kWave) + wave_id();
  if (row >= a.rows) return;   // wave-uniform
  const int K = a.K, lane = lane_id();
  const int b = row / K, i = row - b * K;
  const float* __restrict__ gb = a.gAtb + (size_t)b * a.P + a.m;
  const float* __restrict__ gA = a.gAtA + ((size_t)b * a.P + a.m + i) * a.P + a.m;
  const float* __restrict__ w = a.Wc + (size_t)b * K;
  float* __restrict__ gL = a.gLe + (size_t)row * K;
  const float gbi = gb[i];
  for (int j = 4 * lane; j < K; j += 4 * kWave) {
    float x[4], prev[4] = {0.f, 0.f, 0.f, 0.f}, o[4];
    if constexpr (V4) {
      const float4 wv = *reinterpret_cast<const float4*>(w + j);
      x[0] = wv.x, x[1] = wv.y, x[2] = wv.z, x[3] = wv.w;
      if (!a.overwrite) {
        const float4 pv = *reinterpret_cast<const float4*>(gL + j);
        prev[0] = pv.x, prev[1] = pv.y, prev[2] = pv.z, prev[3] = pv.w;
      }
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        x[q] = j + q < K ? w[j + q] : 0.f;
        prev[q] = (!a.overwrite && j + q < K) ? gL[j + q] : 0.f;
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float t = fmaf(-gbi, x[q], j + q < K ? gA[j + q] : 0.f);
      o[q] = a.overwrite ? t : prev[q] + t;
    }
    if constexpr (V4) {
      *reinterpret_cast<float4*>(gL + j) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (j + q < K) gL[j + q] = o[q];
    }
  }
  // column i of Le against gAtb'
  const float* __restrict__ Lc = a.Le + (size_t)b * K * K + i;
  float acc = 0.f;
  for (int r0 = 4 * lane; r0 < K; r0 += 4 * kWave) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (r0 + q < K) acc = fmaf(Lc[(size_t)(r0 + q) * K], gb[r0 + q], acc);
  }
  acc = wave_sum(acc);
  if (lane == 0) {
    float* t = a.gWc + (size_t)b * K + i;
    *t = *t - acc;
    a.gee[row] = a.overwrite ? gbi : a.gee[row] + gbi;
  }
}

// ---- once per level: Gh, gh, gLambda, geta, gscale ----------------------------------------------------------------------------------
struct PriorPrepArgs {
  int K;
  float scale;
  const float* gLe;
  const float* gee;
  const float* Le;      // gscale only
  const float* ee;
  float* Gh;            // workspace
  float* gh;
  float* gLambda;       // the outputs: each or nullptr
  float* geta;
  float* gscale;
};

__global__ __launch_bounds__(kPriorPrepThreads) void prior_grad_prep_kernel(const PriorPrepArgs a) {
  __shared__ double red[kPriorPrepThreads];
  const int b = blockIdx.x, tid = threadIdx.x, K = a.K, KK = K * K;
  const size_t o = (size_t)b * KK, ov = (size_t)b * K;
  double s = 0.0;
  for (int idx = tid; idx < KK; idx += kPriorPrepThreads) {
    const int i = idx / K, j = idx - i * K;
    const float g = a.gLe[o + idx], gt = a.gLe[o + (size_t)j * K + i];
    a.Gh[o + idx] = __fmul_rn(a.scale, __fmul_rn(0.5f, __fadd_rn(g, gt)));   // (the sum commutes: exactly symmetric)
    if (a.gLambda) a.gLambda[o + idx] = __fmul_rn(a.scale, g);
    if (a.gscale) s = fma((double)g, (double)a.Le[o + idx], s);
  }
  for (int k = tid; k < K; k += kPriorPrepThreads) {
    const float g = a.gee[ov + k];
    const float v = __fmul_rn(a.scale, g);
    a.gh[ov + k] = v;
    if (a.geta) a.geta[ov + k] = v;
    if (a.gscale) s = fma((double)g, (double)a.ee[ov + k], s);
  }
  if (a.gscale) {   // uniform
    red[tid] = s;
    __syncthreads();
    for (int st = kPriorPrepThreads / 2; st >= 1; st >>= 1) {
      if (tid < st) red[tid] += red[tid + st];
      __syncthreads();
    }
    if (tid == 0) a.gscale[b] = (float)(red[0] / (double)a.scale);
  }
}

// ---- once per level: the per-pixel outputs -----------------------------------------------------------------------------------------
struct PriorPixelArgs {
  int N, K, tiles;
  int accumulate;        // gdepth / gbasis read-modify-write, no store at a point that is not counted
  const float* depth;
  const float* basis;
  const float* obs;
  const float* weight;   // nullptr: 1
  const float* Gh;       // [B][K][K] symmetric
  const float* gh;       // [B][K]
  float* gobs;           // the outputs: each or nullptr
  float* gweight;
  float* gdepth;
  float* gbasis;
};

// V4: 16-byte accesses of the basis and gbasis rows (K % 4 == 0, both 16-byte aligned); otherwise 4-byte accesses of the same
// elements.  K <= 128: 8 waves, two per SIMD, 256 registers each -- accumulators and the kept row fit; above, 4 waves with 512
// registers (the image leaves room for one workgroup per CU anyway, and 16 NR MFMAs per LDS read keep one wave per SIMD busy).
template <int NR, bool V4>
__global__ __launch_bounds__(prior_grad_threads(NR)) void prior_grad_pixel_kernel(const PriorPixelArgs a) {
  constexpr int kThreads = prior_grad_threads(NR), kWaves = kThreads / kWave;
  extern __shared__ __attribute__((aligned(16))) float pg_smem[];
  constexpr int NB = NR * (NR + 1) / 2;
  constexpr bool KEEP = NR <= 4;                          // the basis row stays in registers for q = b . y
  float* sG = pg_smem;                                    // the lower blocks of Gh, marg_fill_T_image's layout
  float* sg = pg_smem + NB * 1024;                        // gh, zeros past K
  const int b = blockIdx.y, tid = threadIdx.x, K = a.K, N = a.N;
  {
    const float* __restrict__ Gw = a.Gh + (size_t)b * K * K;
    for (int idx = tid; idx < NB * 1024; idx += kThreads) {
      const int blk = idx >> 10, i = (idx >> 5) & 31, j = idx & 31;
      const int R = marg_block_row(blk), Cb = blk - R * (R + 1) / 2;
      const int r = 32 * R + i, c = 32 * Cb + j;
      const float v = (r < K && c < K) ? Gw[r * K + c] : 0.f;      // (diagonal blocks whole: Gh is symmetric, not triangular)
      sG[blk * 1024 + i * 32 + ((((j >> 2) ^ (i & 7))) << 2) + (j & 3)] = v;
    }
    for (int k = tid; k < NR * 32; k += kThreads) sg[k] = k < K ? a.gh[(size_t)b * K + k] : 0.f;
  }
  __syncthreads();

  const int lane = tid & 63, wave = tid >> 6, nl = lane & 31, h = lane >> 5;
  const float* __restrict__ Bw = a.basis + (size_t)b * N * K;
  const float* __restrict__ dep = a.depth + (size_t)b * N;
  const float* __restrict__ ob = a.obs + (size_t)b * N;
  const float* __restrict__ wg = a.weight ? a.weight + (size_t)b * N : nullptr;

  for (int tile = blockIdx.x * kWaves + wave; tile < a.tiles; tile += gridDim.x * kWaves) {
    const int n = tile * 32 + nl;
    const bool valid = n < N;
    const int ni = valid ? n : 0;
    const float wn = wg ? wg[ni] : 1.f, tn = ob[ni], dn = dep[ni];
    const bool cnt = valid && fit_point_counted(wn, tn);  // basisfit.hip's decision
    const float w = cnt ? wn : 0.f, r = cnt ? tn - dn : 0.f;
    const float* row = Bw + (size_t)ni * K;

    // a lane's 16 floats of column block Cb: columns 32 Cb + 8 q + 4 h + e; zeros past the row's end and for points not counted
    auto load_block = [&](int Cb, f32x4* dst) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c0 = 32 * Cb + 8 * q + 4 * h;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if constexpr (V4) {
          if (cnt && c0 < K) v = *reinterpret_cast<const f32x4*>(row + c0);   // K % 4 == 0: the chunk is inside the row
        } else if (cnt) {
          if (c0 + 0 < K) v[0] = row[c0 + 0];
          if (c0 + 1 < K) v[1] = row[c0 + 1];
          if (c0 + 2 < K) v[2] = row[c0 + 2];
          if (c0 + 3 < K) v[3] = row[c0 + 3];
        }
        dst[q] = v;
      }
    };

    if (__ballot(cnt) == 0ull) {                          // wave-uniform: no counted point in the tile -- zeros, or nothing
      if (valid && h == 0) {
        if (a.gobs) a.gobs[(size_t)b * N + n] = 0.f;
        if (a.gweight) a.gweight[(size_t)b * N + n] = 0.f;
        if (a.gdepth && !a.accumulate) a.gdepth[(size_t)b * N + n] = 0.f;
      }
      if (a.gbasis && valid && !a.accumulate) {
        float* __restrict__ orow = a.gbasis + ((size_t)b * N + n) * K;
        for (int c = 4 * h; c < K; c += 8) {              // the lane's chunks of the row, as below
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (c + e < K) orow[c + e] = 0.f;
        }
      }
      continue;
    }

    f32x16 acc[NR];
#pragma unroll
    for (int R = 0; R < NR; ++R)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[R][i] = 0.f;
    f32x4 bk[KEEP ? NR : 1][4];                           // KEEP: the whole row, every load in flight at once
    float p = 0.f, qv = 0.f;
    int goff = 4 * h;                                     // the lane's reads of gh: opaque per tile too (16 NR registers otherwise)
    asm volatile("" : "+v"(goff));

    {
      // the lane's reads of the image, opaque per tile as marg_tile_y's (hoisted out of the loops, the blocks would occupy
      // hundreds of registers): row nl of a block, and -- transposed -- row 8 q + 4 h + e, column nl
      int trow = nl * 32;
      asm volatile("" : "+v"(trow));
      int tcol[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        tcol[e] = (4 * h + e) * 32 + ((((nl >> 2) ^ (4 * h + e))) << 2) + (nl & 3);
        asm volatile("" : "+v"(tcol[e]));
      }
      // block Cb of the row against column block Cb of Gh: every accumulator one step further
      auto step = [&](int Cb, const f32x4* cb) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const f32x4 gq = *reinterpret_cast<const f32x4*>(&sg[32 * Cb + 8 * q + goff]);
#pragma unroll
          for (int e = 0; e < 4; ++e) p = fmaf(cb[q][e], gq[e], p);
#pragma unroll
          for (int R = 0; R < NR; ++R) {
            if (R >= Cb) {                                // Gh[R, Cb]: row-wise
              const int blk = R * (R + 1) / 2 + Cb;
              const f32x4 t = *reinterpret_cast<const f32x4*>(&sG[blk * 1024 + trow + (((2 * q + h) ^ (nl & 7)) << 2)]);
#pragma unroll
              for (int e = 0; e < 4; ++e) acc[R] = __builtin_amdgcn_mfma_f32_32x32x2f32(t[e], cb[q][e], acc[R], 0, 0, 0);
            } else {                                      // Gh[R, Cb] = Gh[Cb, R]^T: the stored block column-wise
              const int blk = Cb * (Cb + 1) / 2 + R;
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                const float t = sG[blk * 1024 + q * 256 + tcol[e]];
                acc[R] = __builtin_amdgcn_mfma_f32_32x32x2f32(t, cb[q][e], acc[R], 0, 0, 0);
              }
            }
          }
          // one step's image reads in flight at a time: left to itself the scheduler front-loads the reads of the whole unrolled
          // tile (16 NR^2 registers) and spills
          __builtin_amdgcn_sched_barrier(0);
        }
      };
      // q = b . y: register 4 j + e of acc[R] is row 32 R + 8 j + 4 h + e of y, the column a loaded block holds in [j][e]
      if constexpr (KEEP) {
#pragma unroll
        for (int Cb = 0; Cb < NR; ++Cb) load_block(Cb, bk[Cb]);
#pragma unroll
        for (int Cb = 0; Cb < NR; ++Cb) step(Cb, bk[Cb]);
#pragma unroll
        for (int R = 0; R < NR; ++R)
#pragma unroll
          for (int i = 0; i < 16; ++i) qv = fmaf(bk[R][i >> 2][i & 3], acc[R][i], qv);
      } else {
        f32x4 cur[4], nxt[4];
        load_block(0, cur);
#pragma unroll
        for (int Cb = 0; Cb < NR; ++Cb) {
          if (Cb + 1 < NR) load_block(Cb + 1, nxt);
          step(Cb, cur);
#pragma unroll
          for (int q = 0; q < 4; ++q) cur[q] = nxt[q];
        }
        if (a.gweight) {                                  // uniform: the row again, one block in flight at a time
#pragma unroll
          for (int R = 0; R < NR; ++R) {
            load_block(R, cur);
#pragma unroll
            for (int i = 0; i < 16; ++i) qv = fmaf(cur[i >> 2][i & 3], acc[R][i], qv);
            asm volatile("" : "+v"(row) : "v"(qv));       // the next block's address waits for this one's chain: one block in flight
          }
        }
      }
      p = p + __shfl_xor(p, 32, 64);                      // the two column halves of the pixel
      qv = qv + __shfl_xor(qv, 32, 64);
    }

    const float wp = w * p;
    if (valid && h == 0) {
      if (a.gobs) a.gobs[(size_t)b * N + n] = cnt ? wp : 0.f;
      if (a.gweight) a.gweight[(size_t)b * N + n] = cnt ? fmaf(r, p, qv) : 0.f;
      if (a.gdepth) {
        float* gd = a.gdepth + (size_t)b * N + n;
        if (!a.accumulate) *gd = cnt ? -wp : 0.f;
        else if (cnt) *gd = *gd - wp;
      }
    }
    if (a.gbasis && valid && (cnt || !a.accumulate)) {
      float* orow = a.gbasis + ((size_t)b * N + n) * K;
#pragma unroll
      for (int R = 0; R < NR; ++R) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int c0 = 32 * R + 8 * j + 4 * h;
          const f32x4 gq = *reinterpret_cast<const f32x4*>(&sg[32 * R + 8 * j + goff]);
          f32x4 v;
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = cnt ? w * fmaf(r, gq[e], 2.f * acc[R][4 * j + e]) : 0.f;
          if constexpr (V4) {
            if (c0 < K) {                                 // K % 4 == 0: the chunk is inside the row
              if (a.accumulate) v += *reinterpret_cast<const f32x4*>(orow + c0);
              *reinterpret_cast<f32x4*>(orow + c0) = v;
            }
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (c0 + e < K) orow[c0 + e] = a.accumulate ? orow[c0 + e] + v[e] : v[e];
          }
          // the next block's address waits for this one's values: 16 loads in flight, not 16 NR (which spills)
          if (j == 3) asm volatile("" : "+v"(orow) : "v"(v[3]));
        }
      }
    }
  }
}

template <int NR, bool V4>
static void launch_prior_pixel_v(const PriorPixelArgs& a, const PriorGradPlan& pl, int B, hipStream_t s) {
  if (pl.lds > 64 * 1024)
    (void)hipFuncSetAttribute((const void*)prior_grad_pixel_kernel<NR, V4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds);
  hipLaunchKernelGGL((prior_grad_pixel_kernel<NR, V4>), dim3(pl.grid, B), dim3(prior_grad_threads(NR)), pl.lds, s, a);
}

template <int NR>
static void launch_prior_pixel(const PriorPixelArgs& a, const PriorGradPlan& pl, int B, hipStream_t s) {
  const bool v4 = (pl.K % 4 == 0) && ((reinterpret_cast<uintptr_t>(a.basis) | reinterpret_cast<uintptr_t>(a.gbasis)) & 15u) == 0;
  if (v4) launch_prior_pixel_v<NR, true>(a, pl, B, s);
  else launch_prior_pixel_v<NR, false>(a, pl, B, s);
}

static int launch_prior_terms_grad(const banet_level_t* lv, const banet_prior_t* pr, const PriorGradPlan& pl,
                                   const banet_prior_grad_in_t* in, const banet_prior_grad_out_t* out, void* ws, hipStream_t s) {
  char* w = static_cast<char*>(ws);
  PriorPrepArgs p;
  p.K = pl.K;
  p.scale = pr->scale;
  p.gLe = in->gLe;
  p.gee = in->gee;
  p.Le = in->Le;
  p.ee = in->ee;
  p.Gh = reinterpret_cast<float*>(w + pl.off_Gh);
  p.gh = reinterpret_cast<float*>(w + pl.off_gh);
  p.gLambda = out->gLambda;
  p.geta = out->geta;
  p.gscale = out->gscale;
  hipLaunchKernelGGL(prior_grad_prep_kernel, dim3(lv->B), dim3(kPriorPrepThreads), 0, s, p);
  if (hipGetLastError() != hipSuccess) return BANET_ERR_LAUNCH;
  if (!pl.pixel) return BANET_OK;

  PriorPixelArgs a;
  a.N = lv->N;
  a.K = pl.K;
  a.tiles = pl.tiles;
  a.accumulate = (in->flags & BANET_PRIOR_GRAD_ACCUMULATE) != 0;
  a.depth = lv->depth;
  a.basis = lv->basis;
  a.obs = pr->obs_depth;
  a.weight = pr->obs_weight;
  a.Gh = p.Gh;
  a.gh = p.gh;
  a.gobs = out->gobs;
  a.gweight = out->gweight;
  a.gdepth = out->gdepth;
  a.gbasis = out->gbasis;
#define BANET_PGP(n) \
  case n: launch_prior_pixel<n>(a, pl, lv->B, s); break;
  switch (pl.NR) {
    BANET_PGP(1) BANET_PGP(2) BANET_PGP(3) BANET_PGP(4) BANET_PGP(5) BANET_PGP(6) BANET_PGP(7) BANET_PGP(8)
    default: return BANET_ERR_UNSUPPORTED;
  }
#undef BANET_PGP
  if (hipGetLastError() != hipSuccess) return BANET_ERR_LAUNCH;
  return BANET_OK;
}

}  // namespace banet

using namespace banet;

extern "C" {

int banet_prior_terms_f32(const banet_level_t* lv, const banet_prior_t* pr, float* Le, float* ee, void* ws, size_t workspace_bytes,
                          banet_stream_t stream) {
  if (!lv || !Le || !ee) return BANET_ERR_INVALID_ARG;
  PriorPlan pl;
  const int rc = plan_prior(lv, pr, 0, &pl);
  if (rc != BANET_OK) return rc;
  if (!pl.on) return BANET_OK;   // the empty prior: nothing is launched, nothing written
  if (pl.obs && (!lv->depth || !lv->basis)) return BANET_ERR_INVALID_ARG;
  if (!ws || workspace_bytes < pl.bytes || (reinterpret_cast<uintptr_t>(ws) & 255u) != 0) return BANET_ERR_WORKSPACE;
  PriorRun run = make_prior_run(lv, pr, pl, ws);
  run.Le = Le;                   // the combine launch writes the caller's memory (4-byte stores: any alignment)
  run.ee = ee;
  return launch_prior_setup(lv, run, static_cast<hipStream_t>(stream));
}

int banet_prior_add_grad_f32(const banet_level_t* lv, const float* Le, const float* Wc, const float* gAtA, const float* gAtb, float* gLe,
                             float* gee, float* gWc, int flags, banet_stream_t stream) {
  if (!lv || !Le || !Wc || !gAtA || !gAtb || !gLe || !gee || !gWc) return BANET_ERR_INVALID_ARG;
  PriorGradPlan pl;
  const int rc = plan_prior_add_grad(lv, flags, &pl);
  if (rc != BANET_OK) return rc;
  PriorAddGradArgs a;
  a.K = pl.K;
  a.m = pl.m;
  a.P = pl.P;
  a.rows = lv->B * pl.K;
  a.overwrite = (flags & BANET_PRIOR_GRAD_OVERWRITE) != 0;
  a.Le = Le;
  a.Wc = Wc;
  a.gAtA = gAtA;
  a.gAtb = gAtb;
  a.gLe = gLe;
  a.gee = gee;
  a.gWc = gWc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool v4 = (pl.K & 3) == 0 && ((reinterpret_cast<uintptr_t>(Wc) | reinterpret_cast<uintptr_t>(gLe)) & 15u) == 0;
  if (v4) hipLaunchKernelGGL(prior_add_grad_kernel<true>, dim3(pl.add_grid), dim3(kPriorThreads), 0, s, a);
  else hipLaunchKernelGGL(prior_add_grad_kernel<false>, dim3(pl.add_grid), dim3(kPriorThreads), 0, s, a);
  if (hipGetLastError() != hipSuccess) return BANET_ERR_LAUNCH;
  return BANET_OK;
}

size_t banet_prior_terms_grad_workspace_bytes(const banet_level_t* lv, const banet_prior_t* pr) {
  PriorGradPlan pl;
  if (plan_prior_grad_layout(lv, pr, num_cus(), &pl) != BANET_OK) return 0;
  return pl.bytes;
}

int banet_prior_terms_grad_f32(const banet_level_t* lv, const banet_prior_t* pr, const banet_prior_grad_in_t* in,
                               const banet_prior_grad_out_t* out, void* ws, size_t workspace_bytes, banet_stream_t stream) {
  PriorGradPlan pl;
  const int rc = plan_prior_terms_grad(lv, pr, in, out, num_cus(), &pl);
  if (rc != BANET_OK) return rc;
  if (!ws || workspace_bytes < pl.bytes || (reinterpret_cast<uintptr_t>(ws) & 255u) != 0) return BANET_ERR_WORKSPACE;
  return launch_prior_terms_grad(lv, pr, pl, in, out, ws, static_cast<hipStream_t>(stream));
}

}  // extern "C"
