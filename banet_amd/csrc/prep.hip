// Per-level preparation kernels -- the step immediately before the LM loop:
//   ba_resample_kernel     tf.contrib.resampler.resampler (bundlenet.py:290,320,343-344,385) and
//                          interpolate2d2 (legacy/utils_python.py:177-232; legacy/ba.py:115)
//   ba_target_map_kernel   conv2 = [f | gx | gy], grad_fixed with REFLECT padding
//                          (bundlenet.py:92-100,323-324 ; legacy/ba.py:17-25,116-118)
//   ba_depth_output_kernel depth = init + basis . W   (bundlenet.py:397)
// All three are pure streaming kernels (HBM-bound): channel-contiguous rows, lane = channel(s),
// so every tap / row is a coalesced load.  Same operation order as the reference expressions
// (the oracle restates them), fp32.
#include "kernels.hpp"
#include "resample_taps.hpp"

namespace banet {

// the footprint (floor, weights, in-image tests) and the sum order of both modes: resample_taps.hpp, shared with grid_prep.hip
__global__ __launch_bounds__(256) void ba_resample_kernel(const float* __restrict__ data, const float* __restrict__ warp,
                                                          float* __restrict__ out, int N, int C, int H, int W, int mode) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int wv = blockIdx.x * 4 + (threadIdx.x >> 6), nw = gridDim.x * 4;
  const float* __restrict__ img = data + (size_t)b * H * W * C;
  for (int n = wv; n < N; n += nw) {   // one wave per point, lanes over channels
    const float x = warp[((size_t)b * N + n) * 2], y = warp[((size_t)b * N + n) * 2 + 1];
    float* o = out + ((size_t)b * N + n) * C;
    const ResampleTaps t = resample_taps(x, y, H, W, mode);
    const float* p0 = img + ((size_t)t.ty[0] * W + t.tx[0]) * C;
    const float* p1 = img + ((size_t)t.ty[1] * W + t.tx[1]) * C;
    const float* p2 = img + ((size_t)t.ty[2] * W + t.tx[2]) * C;
    const float* p3 = img + ((size_t)t.ty[3] * W + t.tx[3]) * C;
    for (int c = lane; c < C; c += 64) o[c] = resample_sum(t, mode, p0[c], p1[c], p2[c], p3[c]);
  }
}

// [B,H,W,C] -> [B,H,W,3C] = [f | gx | gy]; thread = (pixel, channel), channels fastest
__global__ __launch_bounds__(256) void ba_target_map_kernel(const float* __restrict__ img, float* __restrict__ out, int H,
                                                            int W, int C) {
  const int b = blockIdx.y;
  const size_t total = (size_t)H * W * C;
  const float* __restrict__ im = img + (size_t)b * total;
  float* __restrict__ o = out + (size_t)b * total * 3;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(e % C);
    const size_t pix = e / C;
    const int x = (int)(pix % W), y = (int)(pix / W);
    const float f = im[e];
    const float gx = 0.5f * (im[((size_t)y * W + refl_p(x, W)) * C + c] - im[((size_t)y * W + refl_m(x)) * C + c]);
    const float gy = 0.5f * (im[((size_t)refl_p(y, H) * W + x) * C + c] - im[((size_t)refl_m(y) * W + x) * C + c]);
    float* op = o + pix * 3 * C;
    op[c] = f;
    op[C + c] = gx;
    op[2 * C + c] = gy;
  }
}

// out[b,n] = init[b,n] + sum_k basis[b,n,k] W[b,k]: one wave per row, fixed-order lane reduction
__global__ __launch_bounds__(256) void ba_depth_output_kernel(const float* __restrict__ init, const float* __restrict__ basis,
                                                              const float* __restrict__ Wc, float* __restrict__ out, int N,
                                                              int K) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int wv = blockIdx.x * 4 + (threadIdx.x >> 6), nw = gridDim.x * 4;
  const float* __restrict__ wb = Wc + (size_t)b * K;
  for (int n = wv; n < N; n += nw) {
    const float* row = basis + ((size_t)b * N + n) * K;
    float acc = 0.f;
    for (int k = lane; k < K; k += 64) acc = fmaf(row[k], wb[k], acc);
    acc = wave_sum(acc);
    if (lane == 0) out[(size_t)b * N + n] = init[(size_t)b * N + n] + acc;
  }
}

int launch_resample(const float* data, const float* warp, float* out, int B, int N, int C, int H, int W, int mode,
                    hipStream_t s) {
  if (B <= 0 || N <= 0 || C <= 0 || H <= 0 || W <= 0 || (mode != 0 && mode != 1)) return BANET_ERR_INVALID_ARG;
  int gx = (N + 3) / 4;
  if (gx > 4096) gx = 4096;
  hipLaunchKernelGGL(ba_resample_kernel, dim3(gx, B), dim3(256), 0, s, data, warp, out, N, C, H, W, mode);
  return hipGetLastError() == hipSuccess ? BANET_OK : BANET_ERR_LAUNCH;
}

int launch_target_map(const float* img, float* out, int B, int H, int W, int C, hipStream_t s) {
  if (B <= 0 || C <= 0 || H < 2 || W < 2) return BANET_ERR_INVALID_ARG;
  size_t blocks = ((size_t)H * W * C + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(ba_target_map_kernel, dim3((unsigned)blocks, B), dim3(256), 0, s, img, out, H, W, C);
  return hipGetLastError() == hipSuccess ? BANET_OK : BANET_ERR_LAUNCH;
}

int launch_depth_output(const float* init, const float* basis, const float* Wc, float* out, int B, int N, int K,
                        hipStream_t s) {
  if (B <= 0 || N <= 0 || K <= 0) return BANET_ERR_INVALID_ARG;
  int gx = (N + 3) / 4;
  if (gx > 4096) gx = 4096;
  hipLaunchKernelGGL(ba_depth_output_kernel, dim3(gx, B), dim3(256), 0, s, init, basis, Wc, out, N, K);
  return hipGetLastError() == hipSuccess ? BANET_OK : BANET_ERR_LAUNCH;
}

}  // namespace banet
