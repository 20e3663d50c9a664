// What the translation units of the forward SYRK share (syrk.hip, the driver, and syrk_lds / _mfma32 / _bf16x6 / _wide / _stats.hip):
// the kernels' argument blocks, the vector types of the MFMA operands, the scales of the fp16 two-piece form and the internal
// launchers.  Every launcher takes one step of plan_syrk_steps (plan.hpp) and enqueues the instantiation it names on the step's grid;
// a step without a compiled instantiation is BANET_ERR_UNSUPPORTED.  The launchers only enqueue: the driver asks hipGetLastError()
// once at the end.
#pragma once
#include "kernels.hpp"
#include "syrk_split.hpp"

namespace banet {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

struct SyrkArgs {
  const float* basis;  // [B][N][K]
  const float* rec;    // [B][pairs][N][8]
  const int32_t* active;
  int active_stride;
  float* partials;     // [B][Gs][(6 pairs + 1) K + K*K]: H_cd rows (pair, c), the Atb_d row, H_dd
  int N, K, Gs, tiles, pstride;
  int pairs;           // target frames per window (records of pair i: rec + ((b pairs + i) N) 8)
  int pass;            // LDS-tiled kernel only: pass p adds H_cd of pair p; pass 0 also H_dd / Atb_d with s, r summed over pairs
  MlpRole mr;          // ba_syrk_bf16x6_kernel: workgroup Gs of every window evaluates the lambda MLP (mr.y != nullptr)
  const float* colmax; // T0 = 16 (fp16 two-piece split): [B][K] max_n |b_nk| (ba_colmax_kernel)
  const float* recmax; // T0 = 16: [B][kRecMaxBlocks][2] per-block max_n s_n and max_n,word word^2 / s_n (ba_recmax_kernel)
};

struct WideArgs {
  const float* basis;  // [B][N][K]
  const float* rec;    // [B][pairs][N][8]
  const float* srsum;  // [B][N][2] (s, r summed over the frames) or nullptr when pairs == 1 (then rec words 6, 7)
  const int32_t* active;
  int active_stride;
  float* partials;
  int N, K, Gs, pstride, pairs;
  int koff, p0;        // slice job
  int r0, c0;          // rect job
  const float* colmax; // F16 (the fp16 two-piece form, see syrk_bf16x6.hip): [B][K] max_n |b_nk|
  const float* recmax; // F16: [B][kRecMaxBlocks][2] per-block max s_n, max word^2 / s_n (ba_recmax_kernel)
};

// the window's record maxima -> (2^es > sqrt(max s), 2^eu > sqrt(max word^2 / s)); false if they are not finite
__device__ __forceinline__ bool f16_rec_exponents(const float* recmax, int b, int lane, int& es, int& eu) {
  float smx = 0.f, wmx = 0.f;
  if (lane < kRecMaxBlocks) {
    smx = recmax[((size_t)b * kRecMaxBlocks + lane) * 2];
    wmx = recmax[((size_t)b * kRecMaxBlocks + lane) * 2 + 1];
  }
#pragma unroll
  for (int sh = 1; sh < 64; sh <<= 1) {
    smx = fmaxf(smx, __shfl_xor(smx, sh, 64));
    wmx = fmaxf(wmx, __shfl_xor(wmx, sh, 64));
  }
  (void)frexpf(sqrtf(smx), &es);
  (void)frexpf(sqrtf(wmx), &eu);
  return (smx < __builtin_inff()) && (wmx < __builtin_inff()) && !(smx != smx) && !(wmx != wmx);
}
// column scale 2^(14 - ek - es) for max |b| = cm < 2^ek; ok &= representable
__device__ __forceinline__ float f16_col_scale(float cm, int es, bool& ok, float& inv) {
  int ek = 0;
  (void)frexpf(cm, &ek);
  const int sh = 14 - ek - es;
  ok = ok && (cm < __builtin_inff()) && !(cm != cm) && sh > -100 && sh < 100;
  inv = ldexpf(1.f, -sh);
  return ldexpf(1.f, sh);
}

int launch_syrk_stats_step(const SyrkStep& st, const WideArgs& a, hipStream_t s);         // syrk_stats.hip: zero / colmax / recmax / srsum (all of a's buffers)
int launch_syrk_lds_step(const SyrkStep& st, SyrkArgs a, hipStream_t s);                  // syrk_lds.hip
int launch_syrk_mfma32_step(const SyrkStep& st, const SyrkArgs& a, hipStream_t s);        // syrk_mfma32.hip
int launch_syrk_bf16x6_step(const SyrkStep& st, const SyrkArgs& a, hipStream_t s);        // syrk_bf16x6.hip
int launch_syrk_wide_step(const SyrkStep& st, WideArgs a, hipStream_t s);                 // syrk_wide.hip: slice / rect jobs

}  // namespace banet
