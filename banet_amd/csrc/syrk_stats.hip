// The small pre-passes of the SYRK forms: the scales of the fp16 two-piece form (ba_colmax_kernel once per level, ba_recmax_kernel
// per pass) and the wide jobs' per-pixel (s, r) sums over a window's frames (ba_srsum_kernel).
#include "syrk_common.hpp"

namespace banet {

// per window and basis column: max_n |b_nk| as float bits (non-negative floats order like unsigned integers; a NaN ends up
// above every finite value and is caught by the consumer).  colmax zeroed before the launch.  Streams the basis once.
__global__ __launch_bounds__(256) void ba_colmax_kernel(const float* __restrict__ basis, int N, int K, const int32_t* active,
                                                        int active_stride, unsigned* __restrict__ colmax) {
  __shared__ unsigned sMax[256][4];
  const int b = blockIdx.y, tid = threadIdx.x;
  if (active != nullptr && active[(size_t)b * active_stride] == 0) return;
  const int QK = K >> 2;                    // 16-byte column quads per row (K % 4 == 0)
  const int cq = tid % QK, r0 = tid / QK, rstep = 256 / QK;      // QK divides 256 for K = 64 / 128
  const float* bas_b = basis + (size_t)b * N * K;
  f32x4 mx = {0.f, 0.f, 0.f, 0.f};
  const int rows_per_block = (N + gridDim.x - 1) / gridDim.x;
  const int n0 = blockIdx.x * rows_per_block, n1 = min(N, n0 + rows_per_block);
  for (int n = n0 + r0; n < n1; n += rstep) {
    const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(bas_b + (size_t)n * K + 4 * cq));
#pragma unroll
    for (int e = 0; e < 4; ++e) mx[e] = (fabsf(v[e]) > mx[e] || v[e] != v[e]) ? fabsf(v[e]) : mx[e];   // NaN sticks
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) sMax[tid][e] = __float_as_uint(mx[e]);
  __syncthreads();
  if (tid < QK) {
    unsigned m[4] = {0u, 0u, 0u, 0u};
    for (int r = 0; r < rstep; ++r)
#pragma unroll
      for (int e = 0; e < 4; ++e) m[e] = max(m[e], sMax[r * QK + tid][e]);
#pragma unroll
    for (int e = 0; e < 4; ++e) atomicMax(&colmax[(size_t)b * K + 4 * tid + e], m[e]);
  }
}

// per window and block: max_n s_n (s summed over the window's target frames, as the SYRK uses it) and max over pixels and
// record words (u_0..u_5 of every frame, r of every frame) of word^2 / s_n.  No atomics: [B][kRecMaxBlocks][2].
__global__ __launch_bounds__(256) void ba_recmax_kernel(const float* __restrict__ rec, int N, int pairs, const int32_t* active,
                                                        int active_stride, float* __restrict__ out) {
  __shared__ float sRed[4][2];
  const int b = blockIdx.y, tid = threadIdx.x;
  if (active != nullptr && active[(size_t)b * active_stride] == 0) return;
  const float* rec_b = rec + (size_t)b * pairs * N * 8;
  float smx = 0.f, wmx = 0.f;
  for (int n = blockIdx.x * 256 + tid; n < N; n += gridDim.x * 256) {
    float ssum = 0.f, w2 = 0.f;
    for (int p = 0; p < pairs; ++p) {
      const float4 ua = *reinterpret_cast<const float4*>(rec_b + ((size_t)p * N + n) * 8);
      const float4 ub = *reinterpret_cast<const float4*>(rec_b + ((size_t)p * N + n) * 8 + 4);
      ssum += ub.z;
      w2 = fmaxf(w2, fmaxf(fmaxf(ua.x * ua.x, ua.y * ua.y), fmaxf(ua.z * ua.z, ua.w * ua.w)));
      w2 = fmaxf(w2, fmaxf(fmaxf(ub.x * ub.x, ub.y * ub.y), ub.w * ub.w));
      if (ua.x != ua.x || ua.y != ua.y || ua.z != ua.z || ua.w != ua.w || ub.x != ub.x || ub.y != ub.y || ub.z != ub.z || ub.w != ub.w)
        w2 = __builtin_nanf("");                                       // not finite: the consumer falls back
    }
    const float q = ssum > 0.f ? w2 / ssum : (w2 != w2 ? w2 : 0.f);   // s = 0 implies u = r = 0 exactly
    smx = (ssum > smx || ssum != ssum) ? ssum : smx;
    wmx = (q > wmx || q != q) ? q : wmx;
  }
  auto nanmax = [](float a_, float b_) { return (a_ != a_) ? a_ : (b_ != b_) ? b_ : fmaxf(a_, b_); };
#pragma unroll
  for (int sh = 1; sh < 64; sh <<= 1) {
    smx = nanmax(smx, __shfl_xor(smx, sh, 64));
    wmx = nanmax(wmx, __shfl_xor(wmx, sh, 64));
  }
  if ((tid & 63) == 0) {
    sRed[tid >> 6][0] = smx;
    sRed[tid >> 6][1] = wmx;
  }
  __syncthreads();
  if (tid == 0) {
    out[((size_t)b * kRecMaxBlocks + blockIdx.x) * 2] = nanmax(nanmax(sRed[0][0], sRed[1][0]), nanmax(sRed[2][0], sRed[3][0]));
    out[((size_t)b * kRecMaxBlocks + blockIdx.x) * 2 + 1] = nanmax(nanmax(sRed[0][1], sRed[1][1]), nanmax(sRed[2][1], sRed[3][1]));
  }
}

// s and r summed over the window's target frames (8 bytes per pixel), so that the wide jobs do not depend on the number of frames
__global__ __launch_bounds__(256) void ba_srsum_kernel(const float* __restrict__ rec, int N, int pairs,
                                                       const int32_t* active, int active_stride, float* __restrict__ out) {
  const int b = blockIdx.y, n = blockIdx.x * blockDim.x + threadIdx.x;
  if (active != nullptr && active[(size_t)b * active_stride] == 0) return;
  if (n >= N) return;
  float s = 0.f, r = 0.f;
  for (int p = 0; p < pairs; ++p) {   // fixed order
    const float2 v = *reinterpret_cast<const float2*>(rec + (((size_t)b * pairs + p) * N + n) * 8 + 6);
    s += v.x;
    r += v.y;
  }
  *reinterpret_cast<float2*>(out + ((size_t)b * N + n) * 2) = make_float2(s, r);
}

// (the pre-passes write what the SYRK kernels only read: the one place where the argument block's const goes)
int launch_syrk_stats_step(const SyrkStep& st, const WideArgs& a, hipStream_t s) {
  const dim3 grid(st.gx, st.gy), block(st.block);
  unsigned* colmax = reinterpret_cast<unsigned*>(const_cast<float*>(a.colmax));
  switch (st.kind) {
    case kSyrkStepZero: launch_zero_iters(reinterpret_cast<int32_t*>(colmax), st.j0, s); break;
    case kSyrkStepColmax: hipLaunchKernelGGL(ba_colmax_kernel, grid, block, 0, s, a.basis, a.N, a.K, a.active, a.active_stride, colmax); break;
    case kSyrkStepRecmax: hipLaunchKernelGGL(ba_recmax_kernel, grid, block, 0, s, a.rec, a.N, a.pairs, a.active, a.active_stride, const_cast<float*>(a.recmax)); break;
    case kSyrkStepSrsum: hipLaunchKernelGGL(ba_srsum_kernel, grid, block, 0, s, a.rec, a.N, a.pairs, a.active, a.active_stride, const_cast<float*>(a.srsum)); break;
    default: return BANET_ERR_UNSUPPORTED;
  }
  return BANET_OK;
}

}  // namespace banet
