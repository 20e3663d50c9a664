// Dense adjoint (driver, derivation and the kernel list in launch order: adjoint.hip): the round-5 per-texel gather of the
// [f|gx|gy] map adjoint -- adj_map_kernel, adj_map2_kernel -- and, once per level, target_map_adjoint_kernel /
// target_map_adjoint4_kernel.  The deterministic sample-stats gradient (sstats.hip) gathers with the same map kernels.
#include "adjoint_common.hpp"

namespace banet {
namespace adj {

namespace {

__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v = min(v, __shfl_xor(v, s, 64));
  return v;
}

// One wave per target texel: the adjoint of the bilinear sampling as a GATHER over the source pixels whose footprint
// covers the texel, in a fixed order (cells row-major, ascending pixel index inside a cell).  Common case (every cell
// holds at most one pixel, e.g. near-unit local scale): straight-line code, 4 + 4 + 4 independent loads, then the rows.
template <int J3>   // 3C <= 64 J3; one texel, the whole wave
__device__ __forceinline__ void adj_map_texel(const AdjArgs& a, int b, int t, int lane) {
  const int N = a.lv.N, C = a.lv.C, H = a.lv.H, W = a.lv.W, HW = H * W, C3 = 3 * C;
  const int2* __restrict__ cs = reinterpret_cast<const int2*>(a.start) + (size_t)b * HW;
  const int* __restrict__ list = a.list + (size_t)b * N;
  const float* __restrict__ frac = a.frac + (size_t)b * N * kFrac;
  const float* __restrict__ arow = a.arow + (size_t)b * N * C3;
  bool cok[J3];
#pragma unroll
  for (int j = 0; j < J3; ++j) cok[j] = lane + 64 * j < C3;
  {
    const int ty = t / W, tx = t - ty * W;
    int L[4], s0[4];
#pragma unroll
    for (int cell = 0; cell < 4; ++cell) {
      const int cy = ty - 1 + (cell >> 1), cx = tx - 1 + (cell & 1);
      const bool okc = cy >= 0 && cx >= 0;
      const int2 v = cs[okc ? cy * W + cx : 0];
      L[cell] = okc ? v.y : 0;
      s0[cell] = v.x;
    }
    const int Lmax = max(max(L[0], L[1]), max(L[2], L[3]));
    if (Lmax == 0) {         // wave-uniform: nothing lands on this texel
      if (a.overwrite_map) {
        float* __restrict__ o = a.dmap3 + ((size_t)b * HW + t) * C3;
#pragma unroll
        for (int j = 0; j < J3; ++j)
          if (cok[j]) o[lane + 64 * j] = 0.f;
      }
      return;
    }
    float acc[J3];
#pragma unroll
    for (int j = 0; j < J3; ++j) acc[j] = 0.f;
    bool any = false;
    if (Lmax == 1) {
      int n1[4];
#pragma unroll
      for (int cell = 0; cell < 4; ++cell) n1[cell] = list[L[cell] ? s0[cell] : 0];
      float wt[4];
#pragma unroll
      for (int cell = 0; cell < 4; ++cell) {
        const float fax = frac[(size_t)n1[cell] * kFrac + 1], fay = frac[(size_t)n1[cell] * kFrac + 2];
        const float v = ((cell & 1) ? 1.f - fax : fax) * ((cell >> 1) ? 1.f - fay : fay);   // cell = texel - (1,1) ... texel
        wt[cell] = L[cell] ? v : 0.f;
        any = any || wt[cell] != 0.f;
      }
      float val[4][J3];
#pragma unroll
      for (int cell = 0; cell < 4; ++cell)
#pragma unroll
        for (int j = 0; j < J3; ++j) val[cell][j] = arow[(size_t)n1[cell] * C3 + (cok[j] ? lane + 64 * j : 0)];
#pragma unroll
      for (int cell = 0; cell < 4; ++cell)
#pragma unroll
        for (int j = 0; j < J3; ++j) acc[j] = fmaf(wt[cell], wt[cell] != 0.f ? val[cell][j] : 0.f, acc[j]);
    } else {
#pragma unroll 1
      for (int cell = 0; cell < 4; ++cell) {
        int last = -1;
        for (int it = 0; it < L[cell]; ++it) {
          int mn = 0x7fffffff;
          for (int e = lane; e < L[cell]; e += 64) {
            const int v = list[s0[cell] + e];
            if (v > last) mn = min(mn, v);
          }
          const int n = wave_min_i(mn);
          last = n;
          const float ax = frac[(size_t)n * kFrac + 1], ay = frac[(size_t)n * kFrac + 2];
          const float wt = ((cell & 1) ? 1.f - ax : ax) * ((cell >> 1) ? 1.f - ay : ay);
          if (wt != 0.f) {
            any = true;
#pragma unroll
            for (int j = 0; j < J3; ++j) acc[j] = fmaf(wt, arow[(size_t)n * C3 + (cok[j] ? lane + 64 * j : 0)], acc[j]);
          }
        }
      }
    }
    if (any || a.overwrite_map) {   // (acc is all zeros when nothing contributed)
      float* __restrict__ o = a.dmap3 + ((size_t)b * HW + t) * C3;
#pragma unroll
      for (int j = 0; j < J3; ++j)
        if (cok[j]) o[lane + 64 * j] = a.overwrite_map ? acc[j] : o[lane + 64 * j] + acc[j];
    }
  }
}

template <int J3>
__global__ __launch_bounds__(kBlock) void adj_map_kernel(const AdjArgs a) {
  const int b = blockIdx.y, lane = threadIdx.x & 63, w = wave_id();
  const int HW = a.lv.H * a.lv.W;
  for (int t = blockIdx.x * kNumWaves + w; t < HW; t += gridDim.x * kNumWaves) adj_map_texel<J3>(a, b, t, lane);
}

// Two texels per wave (a half wave each, 16-byte accesses) for the common case that every cell involved holds at most one
// pixel; a pair with a fuller cell goes through adj_map_texel, one texel after the other.  Same fma sequence per element as
// adj_map_kernel: identical bits.  3C % 4 == 0, 3C <= 128 J4.
template <int J4, int J3>
__global__ __launch_bounds__(kBlock) void adj_map2_kernel(const AdjArgs a) {
  const int b = blockIdx.y, lane = threadIdx.x & 63, w = wave_id(), hl = lane & 31, hi = lane >> 5;
  const int N = a.lv.N, C = a.lv.C, H = a.lv.H, W = a.lv.W, HW = H * W, C3 = 3 * C;
  const int2* __restrict__ cs = reinterpret_cast<const int2*>(a.start) + (size_t)b * HW;
  const int* __restrict__ list = a.list + (size_t)b * N;
  const float* __restrict__ frac = a.frac + (size_t)b * N * kFrac;
  const float* __restrict__ arow = a.arow + (size_t)b * N * C3;
  bool cok[J4];
#pragma unroll
  for (int j = 0; j < J4; ++j) cok[j] = 4 * hl + 128 * j < C3;
  for (int t2 = 2 * (blockIdx.x * kNumWaves + w); t2 < HW; t2 += 2 * gridDim.x * kNumWaves) {
    const int t = t2 + hi;
    const bool live = t < HW;
    const int tt = live ? t : HW - 1;
    const int ty = tt / W, tx = tt - ty * W;
    int L[4], s0[4];
#pragma unroll
    for (int cell = 0; cell < 4; ++cell) {
      const int cy = ty - 1 + (cell >> 1), cx = tx - 1 + (cell & 1);
      const bool okc = live && cy >= 0 && cx >= 0;
      const int2 v = cs[okc ? cy * W + cx : 0];
      L[cell] = okc ? v.y : 0;
      s0[cell] = v.x;
    }
    const int Lmax = max(max(L[0], L[1]), max(L[2], L[3]));
    if (__any(Lmax > 1)) {                       // wave-uniform: a fuller cell somewhere in the pair
      adj_map_texel<J3>(a, b, t2, lane);
      if (t2 + 1 < HW) adj_map_texel<J3>(a, b, t2 + 1, lane);
      continue;
    }
    if (!__any(Lmax == 1)) {                     // nothing lands on either texel
      if (a.overwrite_map && live) {
        float* __restrict__ o = a.dmap3 + ((size_t)b * HW + t) * C3 + 4 * hl;
#pragma unroll
        for (int j = 0; j < J4; ++j)
          if (cok[j]) *reinterpret_cast<f32x4*>(o + 128 * j) = f32x4{0.f, 0.f, 0.f, 0.f};
      }
      continue;
    }
    int n1[4];
#pragma unroll
    for (int cell = 0; cell < 4; ++cell) n1[cell] = list[L[cell] ? s0[cell] : 0];
    float wt[4];
    bool any = false;
#pragma unroll
    for (int cell = 0; cell < 4; ++cell) {
      const float fax = frac[(size_t)n1[cell] * kFrac + 1], fay = frac[(size_t)n1[cell] * kFrac + 2];
      const float v = ((cell & 1) ? 1.f - fax : fax) * ((cell >> 1) ? 1.f - fay : fay);
      wt[cell] = L[cell] ? v : 0.f;
      any = any || wt[cell] != 0.f;
    }
    f32x4 val[4][J4];
#pragma unroll
    for (int cell = 0; cell < 4; ++cell)
#pragma unroll
      for (int j = 0; j < J4; ++j) val[cell][j] = *reinterpret_cast<const f32x4*>(arow + (size_t)n1[cell] * C3 + (cok[j] ? 4 * hl + 128 * j : 0));
    f32x4 acc[J4];
#pragma unroll
    for (int j = 0; j < J4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int cell = 0; cell < 4; ++cell)
#pragma unroll
      for (int j = 0; j < J4; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[j][e] = fmaf(wt[cell], wt[cell] != 0.f ? val[cell][j][e] : 0.f, acc[j][e]);
    if (any || (a.overwrite_map && live)) {           // (acc is all zeros when nothing contributed)
      float* __restrict__ o = a.dmap3 + ((size_t)b * HW + t) * C3 + 4 * hl;
#pragma unroll
      for (int j = 0; j < J4; ++j)
        if (cok[j]) {
          f32x4* op = reinterpret_cast<f32x4*>(o + 128 * j);
          *op = a.overwrite_map ? acc[j] : *op + acc[j];
        }
    }
  }
}

// d img += dmap_f + grad_fixed^T (dmap_gx, dmap_gy): gx[x] = 0.5 (img[x+1] - img[x-1]) for 1 <= x <= W-2, 0 on the rim
__global__ void target_map_adjoint_kernel(const float* __restrict__ dmap3, float* __restrict__ dimg, int H, int W, int C,
                                          size_t total, int overwrite) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int c = (int)(e % C);
  const size_t tix = e / C;
  const int x = (int)(tix % W);
  const size_t r = tix / W;
  const int y = (int)(r % H);
  const size_t C3 = 3 * (size_t)C;
  const float* m = dmap3 + tix * C3;
  float v = m[c];
  if (x - 1 >= 1 && x - 1 <= W - 2) v += 0.5f * (m - C3)[C + c];
  if (x + 1 >= 1 && x + 1 <= W - 2) v -= 0.5f * (m + C3)[C + c];
  if (y - 1 >= 1 && y - 1 <= H - 2) v += 0.5f * (m - (size_t)W * C3)[2 * C + c];
  if (y + 1 >= 1 && y + 1 <= H - 2) v -= 0.5f * (m + (size_t)W * C3)[2 * C + c];
  dimg[e] = overwrite ? v : dimg[e] + v;
}

// C % 4 == 0: four channels per thread, 16-byte accesses; per element the same operations in the same order (identical bits)
__global__ void target_map_adjoint4_kernel(const float* __restrict__ dmap3, float* __restrict__ dimg, int H, int W, int C4,
                                           size_t total4, int overwrite) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total4) return;
  const int c = (int)(e % C4);
  const size_t tix = e / C4;
  const int x = (int)(tix % W);
  const size_t r = tix / W;
  const int y = (int)(r % H);
  const size_t Q3 = 3 * (size_t)C4;                      // float4 per texel of the [f|gx|gy] map
  const float4* m = reinterpret_cast<const float4*>(dmap3) + tix * Q3;
  float4 v = m[c];
  auto axpy = [&](float a, const float4 t) {
    v.x += a * t.x;
    v.y += a * t.y;
    v.z += a * t.z;
    v.w += a * t.w;
  };
  if (x - 1 >= 1 && x - 1 <= W - 2) axpy(0.5f, (m - Q3)[C4 + c]);
  if (x + 1 >= 1 && x + 1 <= W - 2) axpy(-0.5f, (m + Q3)[C4 + c]);
  if (y - 1 >= 1 && y - 1 <= H - 2) axpy(0.5f, (m - (size_t)W * Q3)[2 * C4 + c]);
  if (y + 1 >= 1 && y + 1 <= H - 2) axpy(-0.5f, (m + (size_t)W * Q3)[2 * C4 + c]);
  float4* o = reinterpret_cast<float4*>(dimg) + e;
  if (overwrite) {
    *o = v;
    return;
  }
  float4 d = *o;
  d.x += v.x;
  d.y += v.y;
  d.z += v.z;
  d.w += v.w;
  *o = d;
}

}  // namespace

// (assert: plan_adj_cells takes map_j3 from the list below, so BANET_ERR_UNSUPPORTED cannot be returned for a plan that
//  returned BANET_OK)
int launch_adj_map(const AdjArgs& a, const AdjCellPlan& c, hipStream_t s) {
  const dim3 grid(c.Gm, a.lv.B), block(kBlock);
  switch (c.map_j3) {
#define BANET_X(j4, j3)                                                        \
  case j3:                                                                     \
    if (c.map_half)                                                            \
      hipLaunchKernelGGL((adj_map2_kernel<j4, j3>), grid, block, 0, s, a);     \
    else                                                                       \
      hipLaunchKernelGGL((adj_map_kernel<j3>), grid, block, 0, s, a);          \
    return BANET_OK;
    BANET_ADJ_MAP_LIST(BANET_X)
#undef BANET_X
  }
  return BANET_ERR_UNSUPPORTED;
}

}  // namespace adj

int launch_target_map_adjoint(const float* dmap3, float* dimg, int B, int H, int W, int C, int overwrite, hipStream_t s) {
  using namespace adj;
  const size_t total = (size_t)B * H * W * C;
  if (total == 0) return BANET_OK;
  if ((C & 3) == 0 && ((reinterpret_cast<uintptr_t>(dmap3) | reinterpret_cast<uintptr_t>(dimg)) & 15) == 0) {
    const size_t total4 = total / 4;
    hipLaunchKernelGGL(target_map_adjoint4_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, s, dmap3, dimg, H, W, C / 4,
                       total4, overwrite);
    return hipGetLastError() == hipSuccess ? BANET_OK : BANET_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(target_map_adjoint_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, dmap3, dimg, H, W, C, total, overwrite);
  return hipGetLastError() == hipSuccess ? BANET_OK : BANET_ERR_LAUNCH;
}
}  // namespace banet
