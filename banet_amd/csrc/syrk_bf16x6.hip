// ba_syrk_bf16x6_kernel -- the product path for K = 64 / 128 and <= 4 target frames: the bf16 matrix pipe at fp32 accuracy, operands
// straight from registers; one extra workgroup per window carries the lambda-MLP role (mlp.hpp).  K = 256 and more frames: the same
// scheme cut into jobs, syrk_wide.hip.
#include "mlp.hpp"
#include "syrk_common.hpp"

namespace banet {

// --------------------------------------------------------------------------------------
// ba_syrk_bf16x6_kernel -- same sums as ba_syrk_direct_kernel, H_dd on the bf16 matrix pipe at fp32
// accuracy.  s_n = jd^T M jd >= 0 (M is a Gram matrix), so H_dd = sum (sqrt(s_n) b_n)(sqrt(s_n) b_n)^T:
// A and B operands are the SAME values v = sqrt(s) b.  Each fp32 v is split EXACTLY into three bf16
// pieces (v = hi + mid + lo: 8 + 8 + 8 significand bits, v_cvt_pk_bf16_f32 and exact subtractions), and
//   v w  =  hi hi' + (hi mid' + mid hi') + (hi lo' + lo hi' + mid mid')  + O(2^-24 |v w|)
// -- six v_mfma_f32_16x16x32_bf16 (products exact in fp32, fp32 accumulate) per 32 pixels and block,
// 6 x 17 cycles against 8 x 32 cycles for v_mfma_f32_16x16x4_f32: 2.5x less matrix-pipe time, the
// dropped terms are below fp32 rounding.  Lane (m, kq) loads, for the 8 pixels 8 kq .. 8 kq + 7 of a
// 32-pixel step, the coefficients {4m..4m+3} + 64h (16-byte loads, 256 contiguous bytes per pixel and
// 16 lanes); one register quad per virtual block and piece is then directly an MFMA operand (k = pixel).
// H_cd / Atb_d stay on v_mfma_f32_16x16x4_f32 with the raw fp32 values (u is not non-negative).
// --------------------------------------------------------------------------------------

// T0 = 0: six bf16 products (fp32-exact); 1: the same + this launch also leaves max_n |b_nk| per column in a.colmax (the first
// iteration of a level in the LM loop: the later ones run T0 = 16 with it, no extra pass over the basis); 3: the three largest
// bf16 products only (opt-in, see plan_syrk); 16: two fp16 pieces, three products, scaled (below)
template <int KH, int PAIRS, int T0>
__global__ __launch_bounds__(kBlock, 1) void ba_syrk_bf16x6_kernel(const SyrkArgs a) {
  constexpr int NBV = 4 * KH, NPAIR = NBV * (NBV + 1) / 2, K = 64 * KH;
  constexpr int NU = (PAIRS + 1) / 2;
  __shared__ float sAcc[NPAIR + NU * NBV][4][64];
  __shared__ float sMlp[kMlpRoleFloats];
  const int b = blockIdx.y, g = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  if (a.active != nullptr && a.active[(size_t)b * a.active_stride] == 0) return;
  if (g == a.Gs) {   // the MLP role workgroup (launched only when a.mr.y != nullptr): hidden behind the SYRK workgroups
    mlp_role_block(a.mr, b, sMlp);
    return;
  }
  const int w = wave_id();
  const int N = a.N;
  const int m = lane & 15, kq = lane >> 4;
  const float* __restrict__ bas_b = a.basis + (size_t)b * N * K;
  const float* __restrict__ rec_b = a.rec + (size_t)b * PAIRS * N * 8;
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

  f32x4 acc[NPAIR];
  f32x4 acu[NU][NBV];
#pragma unroll
  for (int q = 0; q < NPAIR; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < NU; ++j)
#pragma unroll
    for (int q = 0; q < NBV; ++q) acu[j][q] = f32x4{0.f, 0.f, 0.f, 0.f};

  // ---- T0 = 16: the fp16 two-piece split needs every operand inside fp16's range.  v = sqrt(s_n) b_nk is scaled per COLUMN by
  // a power of two from max_n |b_nk| (ba_colmax_kernel, once per level: the basis does not change) and max_n s_n (ba_recmax_kernel,
  // per pass), so that |v| < 2^14 and a column's largest entries keep 22 significand bits while its small ones carry an absolute
  // error of 2^-25 of the scaled unit, i.e. <= 2^-39 of the column's bound; the record rows u / sqrt(s), r / sqrt(s) by one power
  // of two from max word^2 / s.  Powers of two: the scaling and its inverse (epilogue) are exact.  Inputs that are not finite, or
  // exponents beyond what the inverse can undo, fall back to the exact bf16 form below (use16 = false, wave-uniform per window).
  [[maybe_unused]] float csc[4 * KH];       // this lane's columns 64 h + 4 m + e
  [[maybe_unused]] unsigned cmx[4 * KH];    // T0 = 1: running max |b| of those columns over this wave's pixels, as float bits
  if constexpr (T0 == 1) {
#pragma unroll
    for (int c = 0; c < 4 * KH; ++c) cmx[c] = 0u;
  }
  [[maybe_unused]] float usc = 1.f, uinv = 1.f;
  [[maybe_unused]] bool use16 = false;
  [[maybe_unused]] __shared__ float sInv[K];
  if constexpr (T0 == 16) {
    float smx = 0.f, wmx = 0.f;
    if (lane < kRecMaxBlocks) {
      smx = a.recmax[((size_t)b * kRecMaxBlocks + lane) * 2];
      wmx = a.recmax[((size_t)b * kRecMaxBlocks + lane) * 2 + 1];
    }
#pragma unroll
    for (int sh = 1; sh < 64; sh <<= 1) {
      smx = fmaxf(smx, __shfl_xor(smx, sh, 64));
      wmx = fmaxf(wmx, __shfl_xor(wmx, sh, 64));
    }
    int es = 0, eu = 0;
    (void)frexpf(sqrtf(smx), &es);          // sqrt(s) < 2^es
    (void)frexpf(sqrtf(wmx), &eu);
    bool ok = (smx < __builtin_inff()) && (wmx < __builtin_inff()) && !(smx != smx) && !(wmx != wmx);
    usc = ldexpf(1.f, 14 - eu);
    uinv = ldexpf(1.f, eu - 14);
#pragma unroll
    for (int h = 0; h < KH; ++h)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int col = 64 * h + 4 * m + e;
        const float cm = a.colmax[(size_t)b * K + col];
        int ek = 0;
        (void)frexpf(cm, &ek);
        const int sh = 14 - ek - es;          // |sqrt(s) b| 2^sh < 2^14
        ok = ok && (cm < __builtin_inff()) && !(cm != cm) && sh > -100 && sh < 100;
        csc[4 * h + e] = ldexpf(1.f, sh);
        if (w == 0 && kq == 0) sInv[col] = ldexpf(1.f, -sh);
      }
    use16 = __ballot(!ok) == 0ull;           // the same decision in every wave of the window's workgroups (same inputs)
    __syncthreads();
  }

  // this wave's run of 32-pixel steps
  const int ns = (N + 31) >> 5, nwaves = a.Gs * kNumWaves, gw = g * kNumWaves + w;
  const int s0 = (int)(((long long)ns * gw) / nwaves), s1 = (int)(((long long)ns * (gw + 1)) / nwaves);

  // raw registers of one 32-pixel step: basis rows, s and record words as loaded
  struct Raw {
    f32x4 pb[8][KH];
    float ps[8][PAIRS], pu[8][NU];
  };
  Raw ra;
  auto issue = [&](Raw& R, int st) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int pix = 32 * st + 8 * kq + i;
      const size_t p = (st < s1 && pix < N) ? (size_t)pix : 0;
#pragma unroll
      for (int h = 0; h < KH; ++h)
        R.pb[i][h] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(bas_b + p * K + 64 * h + 4 * m));
#pragma unroll
      for (int pr = 0; pr < PAIRS; ++pr) R.ps[i][pr] = rec_b[((size_t)pr * N + p) * 8 + 6];
#pragma unroll
      for (int j = 0; j < NU; ++j) R.pu[i][j] = rec_b[p * 8 + uoff[j]];
    }
  };
#ifdef BANET_TIMING
  unsigned long long tm0, tr0;
  asm volatile("s_memtime %0\n\ts_memrealtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(tm0), "=s"(tr0)::"memory");
#endif
  if constexpr (T0 == 16) {
    if (use16) {
      // ---- the fp16 loop.  One wave per SIMD issues its vector and matrix instructions one after the other, so a step costs what
      // its instructions cost, and a good quarter of a step's vector instructions used to be sqrt(s) and usc / sqrt(s) of the lane's 8
      // pixels -- the same 8 values in all 16 lanes of a pixel group.  Now lane l computes them for ONE pixel, 32 st + (l & 31),
      // from one load of s per target frame, and the lanes fetch their 8 pixels' values across the wave: the same operations on
      // the same operands, one instead of 8 square roots and divisions per lane and step.
      // The loads are kept ahead of the split that consumes them, per instantiation:
      //  * kTwoSets (K = 64): TWO sets of raw registers -- step st splits set st & 1 and issues step st + 2 into it before its MFMA
      //    block, so a batch has a whole step plus an MFMA block to land.  (At K = 128 a second set does not fit: with one target
      //    frame every formulation tried left 56-372 bytes of scratch per lane)
      //  * kStagger (K = 128, one target frame): one set, refilled piecewise as the split frees it -- the records once the record
      //    rows are split, the basis quads of column half h after half h -- so every piece has about half a split more to land and
      //    some 8 KB per wave stay in flight throughout the split.  No extra registers.
      //  * otherwise the refill follows the whole split, as in the exact loop.
      // -DBANET_SYRK_SINGLE_BUFFER: the last form everywhere (A/B builds).
#ifdef BANET_SYRK_SINGLE_BUFFER
      constexpr bool kTwoSets = false, kStagger = false;
#else
      constexpr bool kTwoSets = KH == 1, kStagger = KH == 2 && PAIRS == 1;
#endif
      struct Raw16 {
        f32x4 pb[8][KH];
        float ps1[PAIRS], pu[8][NU];
      };
      Raw16 r0;
      [[maybe_unused]] Raw16 r1;
      const int l32 = lane & 31;
      // A refill's step index is made to depend on the split results that free its registers (an empty asm: no instruction), and
      // a scheduling barrier follows it: the compiler may then neither hoist the loads above the split (it did, and spilled the
      // values they would overwrite) nor sink them towards the MFMA block.  The waits stay the compiler's counted vmcnt.
      auto after = [](int st_, const u32x4_t& x) __attribute__((always_inline)) {
        asm volatile("" : "+s"(st_) : "v"(x));
        return st_;
      };
      // the pieces of a refill; pixels past the run or the window repeat row 0, as in issue()
      auto row_of = [&](int st_, int o) __attribute__((always_inline)) {
        const int lim = st_ < s1 ? N : 0;      // (one scalar select: as a condition of its own the compiler branches on it per load)
        const unsigned pix = 32 * st_ + o;
        return (size_t)((int)pix < lim ? pix : 0u);
      };
      auto issue_rec = [&](Raw16& R, int st_) __attribute__((always_inline)) {
        const size_t p1 = row_of(st_, l32);
#pragma unroll
        for (int pr = 0; pr < PAIRS; ++pr) R.ps1[pr] = rec_b[((size_t)pr * N + p1) * 8 + 6];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const size_t p = row_of(st_, 8 * kq + i);
#pragma unroll
          for (int j = 0; j < NU; ++j) R.pu[i][j] = rec_b[p * 8 + uoff[j]];
        }
      };
      auto issue_rows = [&](Raw16& R, int st_, int h) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 8; ++i)
          R.pb[i][h] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(bas_b + row_of(st_, 8 * kq + i) * K + 64 * h + 4 * m));
      };
      auto issue16 = [&](Raw16& R, int st_) __attribute__((always_inline)) {   // always in this order: the counted waits at the loop
        issue_rec(R, st_);                                                      // head are merged over the prologue and the back edge
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int h = 0; h < KH; ++h) {
          issue_rows(R, st_, h);
          __builtin_amdgcn_sched_barrier(0);
        }
      };
      // one step: split set R (step st), refill it, multiply
      auto step16 = [&](Raw16& R, int st) __attribute__((always_inline)) {
        float sq[8];
        u32x4_t opu[NU][2];
        {
          float ssum = R.ps1[0];
#pragma unroll
          for (int pr = 1; pr < PAIRS; ++pr) ssum += R.ps1[pr];
          const float sq1 = 32 * st + l32 < N ? sqrtf(fmaxf(ssum, 0.f)) : 0.f;          // zero switches the pixel off
          const float inv1 = sq1 > 0.f ? usc / sq1 : 0.f;
          float ut[NU][8];
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            sq[i] = __shfl(sq1, 8 * kq + i, 64);
            const float inv = __shfl(inv1, 8 * kq + i, 64);
#pragma unroll
            for (int j = 0; j < NU; ++j) ut[j][i] = uon[j] ? R.pu[i][j] * inv : 0.f;
          }
#pragma unroll
          for (int j = 0; j < NU; ++j) split8_f16x2(ut[j], opu[j]);
        }
        [[maybe_unused]] int stn = st + (kTwoSets ? 2 : 1);
        if constexpr (kTwoSets || kStagger) {
#pragma unroll
          for (int j = 0; j < NU; ++j) stn = after(stn, opu[j][1]);
        }
        if constexpr (kStagger) {
          issue_rec(R, stn);                                    // s and the record words are free
          __builtin_amdgcn_sched_barrier(0);
        }
        u32x4_t op[NBV][2];
#pragma unroll
        for (int h = 0; h < KH; ++h) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float vv[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) vv[i] = (sq[i] * R.pb[i][h][e]) * csc[4 * h + e];
            split8_f16x2(vv, op[4 * h + e]);
          }
          if constexpr (kTwoSets || kStagger) {
#pragma unroll
            for (int e = 0; e < 4; ++e) stn = after(stn, op[4 * h + e][1]);
          }
          if constexpr (kStagger) {
            issue_rows(R, stn, h);                              // the quads of column half h are free
            __builtin_amdgcn_sched_barrier(0);
          }
        }
        if constexpr (!kStagger) issue16(R, stn);               // the set is free again (two sets: for the step after the next)
        __builtin_amdgcn_sched_barrier(0);
        // three products, smallest first, term-major (consecutive MFMAs write different accumulators): lo hi' + hi lo' + hi hi'
        constexpr int kFa[3] = {1, 0, 0}, kFb[3] = {0, 1, 0};
#pragma unroll
        for (int t3 = 0; t3 < 3; ++t3) {
#pragma unroll
          for (int j = 0; j < NU; ++j)
#pragma unroll
            for (int bj = 0; bj < NBV; ++bj)
              acu[j][bj] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, opu[j][kFa[t3]]),
                                                                  __builtin_bit_cast(f16x8, op[bj][kFb[t3]]), acu[j][bj], 0, 0, 0);
          int idx = 0;
#pragma unroll
          for (int bi = 0; bi < NBV; ++bi)
#pragma unroll
            for (int bj = bi; bj < NBV; ++bj) {
              acc[idx] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, op[bi][kFa[t3]]),
                                                                __builtin_bit_cast(f16x8, op[bj][kFb[t3]]), acc[idx], 0, 0, 0);
              ++idx;
            }
        }
        __builtin_amdgcn_sched_barrier(0);
      };
      issue16(r0, s0);
      if constexpr (kTwoSets) {
        issue16(r1, s0 + 1);
        int st = s0;
        for (; st + 1 < s1; st += 2) {   // unrolled by two: the set of a step is a compile-time choice, both stay in registers
          step16(r0, st);
          step16(r1, st + 1);
        }
        if (st < s1) step16(r0, st);
      } else {
        for (int st = s0; st < s1; ++st) step16(r0, st);
      }
    }
  }
  // the exact loop: T0 = 0 / 1 / 3, and the window-wide fallback of T0 = 16 (from step s0, with loads of its own)
  const bool exact_loop = !(T0 == 16 && use16);
  if (exact_loop) issue(ra, s0);
  for (int st = (T0 == 16 && use16) ? s1 : s0; st < s1; ++st) {
    // ---- H_cd / Atb_d on the bf16 pipe too: sum u b = sum (u / sqrt(s)) (sqrt(s) b) = sum u~ v with the SAME split v
    // as H_dd (|u| <= sqrt(Jc^T M Jc) sqrt(s): u~ is bounded, and s = 0 implies M jd = 0, i.e. u = r = 0 exactly).
    // 6 NBV bf16 MFMAs (16 cycles) per record block row instead of 8 NBV fp32 MFMAs (32 cycles).
    float sq[8];
    u32x4_t opu[NU][3];
    {
      float ut[NU][8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const bool ok = 32 * st + 8 * kq + i < N;
        float ssum = ra.ps[i][0];
#pragma unroll
        for (int pr = 1; pr < PAIRS; ++pr) ssum += ra.ps[i][pr];
        sq[i] = ok ? sqrtf(fmaxf(ssum, 0.f)) : 0.f;          // zero switches the pixel off
        const float inv = sq[i] > 0.f ? 1.f / sq[i] : 0.f;
#pragma unroll
        for (int j = 0; j < NU; ++j) ut[j][i] = uon[j] ? ra.pu[i][j] * inv : 0.f;
      }
#pragma unroll
      for (int j = 0; j < NU; ++j) split8_bf16x3(ut[j], opu[j]);
    }
    // ---- exact 3-way bf16 split of v = sqrt(s) b; one register quad per (virtual block, piece)
    u32x4_t op[NBV][3];
#pragma unroll
    for (int h = 0; h < KH; ++h)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float vv[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) vv[i] = sq[i] * ra.pb[i][h][e];
        split8_bf16x3(vv, op[4 * h + e]);
        if constexpr (T0 == 1) {
#pragma unroll
          for (int i = 0; i < 8; i += 2) {   // (rows past N repeat row 0)  On the bit patterns of |b|: they order like unsigned integers
            const unsigned a0 = __float_as_uint(ra.pb[i][h][e]) & 0x7fffffffu;       // and a NaN lies above every finite value, so it
            const unsigned a1 = __float_as_uint(ra.pb[i + 1][h][e]) & 0x7fffffffu;   // sticks as in ba_colmax_kernel (fmaxf would drop it).
            cmx[4 * h + e] = max(cmx[4 * h + e], max(a0, a1));                       // One three-input unsigned max per two values.
          }
        }
      }
    issue(ra, st + 1);                                      // the raw registers are free again
    __builtin_amdgcn_sched_barrier(0);                      // keep the prefetch ahead of the MFMA block
    // Term-major order: consecutive MFMAs write DIFFERENT accumulators.  Block-major (six dependent MFMAs in a row on
    // one accumulator) measured 19 cycles per MFMA instead of 16 and kept the wave stalled at issue behind each one.
    // Per accumulator the order of the terms is unchanged (smallest first): bit-identical sums.
    constexpr int kTa[6] = {2, 0, 1, 1, 0, 0}, kTb[6] = {0, 2, 1, 0, 1, 0};
#if defined(BANET_SYRK_ABL) && BANET_SYRK_ABL >= 1   // development ablation (tools/time_syrk.py): one product instead of six
    constexpr int kT0 = 5;
#else
    constexpr int kT0 = (T0 == 16 || T0 == 1) ? 0 : T0;   // 3: mid hi' + hi mid' + hi hi' -- the third piece of the split is then dead code
#endif
#pragma unroll
    for (int t6 = kT0; t6 < 6; ++t6) {
#pragma unroll
      for (int j = 0; j < NU; ++j)
#pragma unroll
        for (int bj = 0; bj < NBV; ++bj)
          acu[j][bj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, opu[j][kTa[t6]]),
                                                               __builtin_bit_cast(bf16x8, op[bj][kTb[t6]]), acu[j][bj], 0, 0, 0);
      int idx = 0;
#pragma unroll
      for (int bi = 0; bi < NBV; ++bi)
#pragma unroll
        for (int bj = bi; bj < NBV; ++bj) {
          acc[idx] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, op[bi][kTa[t6]]),
                                                             __builtin_bit_cast(bf16x8, op[bj][kTb[t6]]), acc[idx], 0, 0, 0);
          ++idx;
        }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
#ifdef BANET_TIMING
  unsigned long long tm1, tr1;
  asm volatile("s_memtime %0\n\ts_memrealtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(tm1), "=s"(tr1)::"memory");
#endif

  if constexpr (T0 == 1) {   // column maxima: over the 4 pixel groups of the wave, then every wave of the window by atomic max
    unsigned* cm = reinterpret_cast<unsigned*>(const_cast<float*>(a.colmax)) + (size_t)b * K;     // (non-negative floats order like
#pragma unroll                                                                                   //  unsigned integers; zeroed before)
    for (int c = 0; c < 4 * KH; ++c) {
      unsigned v = cmx[c];                       // bit patterns: |x| orders like an unsigned integer and a NaN stays the maximum
      v = max(v, (unsigned)__shfl_xor((int)v, 16, 64));
      v = max(v, (unsigned)__shfl_xor((int)v, 32, 64));
      if (kq == 0 && s1 > s0) atomicMax(&cm[64 * (c >> 2) + 4 * m + (c & 3)], v);
    }
  }
  // ---- epilogue (as ba_syrk_direct_kernel) ------------------------------------------------------
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
  const int r = w, brow = 4 * kq + r;
#pragma unroll
  for (int j = 0; j < NU; ++j) {
    const int pair = 2 * j + brow / 6;
    if (brow < 12 && pair < PAIRS) {
#pragma unroll
      for (int bj = 0; bj < NBV; ++bj) {
        const int cc = 64 * (bj >> 2) + 4 * m + (bj & 3);
        float v = sAcc[NPAIR + j * NBV + bj][r][lane];
        if constexpr (T0 == 16) {
          if (use16) v = (v * uinv) * sInv[cc];          // undo the power-of-two scales: exact
        }
        part[(6 * pair + brow % 6) * K + cc] = v;
      }
    }
  }
  if (brow == 12) {
#pragma unroll
    for (int bj = 0; bj < NBV; ++bj) {
      const int cc = 64 * (bj >> 2) + 4 * m + (bj & 3);
      float v = sAcc[NPAIR + bj][0][lane];
#pragma unroll
      for (int i = 1; i < PAIRS; ++i) v += sAcc[NPAIR + bj][i][lane];
      if constexpr (T0 == 16) {
        if (use16) v = (v * uinv) * sInv[cc];
      }
      part[6 * PAIRS * K + cc] = v;
    }
  }
#ifdef BANET_TIMING
  __syncthreads();
  if (tid == 0) {   // development aid (tools/time_syrk.py): overwrites 3 words of the partial
    part[0] = (float)(tm1 - tm0);
    part[1] = (float)(tr1 - tr0);
    part[2] = (float)(s1 - s0);
  }
  return;
#endif
  float* pd = part + (6 * PAIRS + 1) * K;
  {
    int idx = 0;
    for (int bi = 0; bi < NBV; ++bi)
      for (int bj = bi; bj < NBV; ++bj) {
        const int rr = 64 * (bi >> 2) + 4 * brow + (bi & 3), cc = 64 * (bj >> 2) + 4 * m + (bj & 3);
        float v = sAcc[idx][r][lane];
        if constexpr (T0 == 16) {
          if (use16) v = (v * sInv[rr]) * sInv[cc];
        }
        if (bj > bi || rr <= cc) {
          pd[rr * K + cc] = v;
          pd[cc * K + rr] = v;
        }
        ++idx;
      }
  }
}

template <int KH, int T0>
static int launch_bf16x6(const SyrkStep& st, const SyrkArgs& a, hipStream_t s) {
  const dim3 grid(st.gx, st.gy), block(st.block);
  switch (st.t1) {
#define BANET_X(p) \
  case p: hipLaunchKernelGGL((ba_syrk_bf16x6_kernel<KH, p, T0>), grid, block, 0, s, a); return BANET_OK;
    BANET_SYRK_FRAMES_LIST(BANET_X)
#undef BANET_X
  }
  return BANET_ERR_UNSUPPORTED;
}

int launch_syrk_bf16x6_step(const SyrkStep& st, const SyrkArgs& a, hipStream_t s) {
#define BANET_X(kh, t) \
  if (st.t0 == kh && st.t2 == t) return launch_bf16x6<kh, t>(st, a, s);
  BANET_SYRK_BF16X6_LIST(BANET_X)
#undef BANET_X
  return BANET_ERR_UNSUPPORTED;
}

}  // namespace banet
