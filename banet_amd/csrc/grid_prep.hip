// Dense level preparation: the decoder's depth / basis map resampled onto the pixel grids of up to 8 pyramid levels, and the
// adjoint of all of them (what tf.gradients derives for bundlenet.py:343-344 when every pixel of a level is a point).
//   ba_grid_resample_kernel          out_l[b,i,j,:] = resample(data[b], x = j sx_l + ox_l, y = i sy_l + oy_l), every level in ONE
//                                    launch, no warp tensor; lanes cover (pixel, channel group) pairs, 16-byte accesses where
//                                    C % 4 == 0, so a C = 1 depth map puts 64 pixels on a wave
//   ba_grid_resample_adjoint_kernel  ddata[b,y,x,:] (= or +=) the taps of every level that land on the texel, ONE launch over the
//                                    texels: a texel inverts the affine map to the candidate pixels (grid_plan.hpp), re-evaluates
//                                    each with the forward's own footprint (resample_taps.hpp) and adds the hits in a fixed order
//                                    -- levels ascending, then i, then j, then the forward's tap order.  No sort, no workspace, no
//                                    memset, no float atomics: every texel is written once, bit-reproducibly.
// Both are streaming kernels.  The footprint, the weights and the tap sum are those of ba_resample_kernel (one definition).
#include "kernels.hpp"
#include "resample_taps.hpp"

namespace banet {

struct GridTable {   // kernel argument: the caller's host array, copied
  int n;
  int pad_;
  unsigned long long start[kGridMaxLevels + 1];   // forward: first work item of each level (items = pixels x channel groups)
  banet_grid_level_t lv[kGridMaxLevels];
};

template <int V>
struct Vec;
template <>
struct Vec<1> {
  float v[1];
  __device__ __forceinline__ void load(const float* p) { v[0] = p[0]; }
  __device__ __forceinline__ void store(float* p) const { p[0] = v[0]; }
};
template <>
struct Vec<4> {
  float v[4];
  __device__ __forceinline__ void load(const float* p) {
    const f32x4 q = *reinterpret_cast<const f32x4*>(p);
    v[0] = q[0], v[1] = q[1], v[2] = q[2], v[3] = q[3];
  }
  __device__ __forceinline__ void store(float* p) const {
    f32x4 q;
    q[0] = v[0], q[1] = v[1], q[2] = v[2], q[3] = v[3];
    *reinterpret_cast<f32x4*>(p) = q;
  }
};

// V channels per lane, G = C / V lanes per pixel; grid (blocks, B), grid-stride over the items of all levels
template <int V>
__global__ __launch_bounds__(256) void ba_grid_resample_kernel(const float* __restrict__ data, const GridTable tb, int H, int W, int C,
                                                               int G, int mode) {
  const int b = blockIdx.y;
  const float* __restrict__ img = data + (size_t)b * H * W * C;
  const unsigned long long total = tb.start[tb.n], stride = (unsigned long long)gridDim.x * 256;
  for (unsigned long long e = (unsigned long long)blockIdx.x * 256 + threadIdx.x; e < total; e += stride) {
    int l = 0;
    while (l + 1 < tb.n && e >= tb.start[l + 1]) ++l;
    const banet_grid_level_t& L = tb.lv[l];
    const int Ho = L.Ho, Wo = L.Wo;
    const unsigned r = (unsigned)(e - tb.start[l]);
    const unsigned pix = r / (unsigned)G;
    const int c = (int)(r - pix * (unsigned)G) * V;
    const int i = (int)(pix / (unsigned)Wo), j = (int)(pix - (unsigned)i * (unsigned)Wo);
    const ResampleTaps t = resample_taps(grid_coord(j, L.sx, L.ox), grid_coord(i, L.sy, L.oy), H, W, mode);
    Vec<V> a[4], o;
#pragma unroll
    for (int q = 0; q < 4; ++q) a[q].load(img + ((size_t)t.ty[q] * W + t.tx[q]) * C + c);
#pragma unroll
    for (int k = 0; k < V; ++k) o.v[k] = resample_sum(t, mode, a[0].v[k], a[1].v[k], a[2].v[k], a[3].v[k]);
    o.store(L.out + ((size_t)b * Ho * Wo + pix) * C + c);
  }
}

// lanes cover (texel, channel group) pairs like the forward; grid (blocks, B), grid-stride over H W G items
template <int V>
__global__ __launch_bounds__(256) void ba_grid_resample_adjoint_kernel(float* __restrict__ ddata, const GridTable tb, int H, int W,
                                                                       int C, int G, int mode, int overwrite) {
  const int b = blockIdx.y;
  const unsigned total = (unsigned)H * (unsigned)W * (unsigned)G, stride = gridDim.x * 256u;
  for (unsigned e = blockIdx.x * 256u + threadIdx.x; e < total; e += stride) {
    const unsigned tex = e / (unsigned)G;
    const int c = (int)(e - tex * (unsigned)G) * V;
    const int Y = (int)(tex / (unsigned)W), X = (int)(tex - (unsigned)Y * (unsigned)W);
    float* __restrict__ o = ddata + ((size_t)b * H * W + tex) * C + c;
    Vec<V> acc;
    if (overwrite) {
#pragma unroll
      for (int k = 0; k < V; ++k) acc.v[k] = 0.f;
    } else {
      acc.load(o);
    }
    for (int l = 0; l < tb.n; ++l) {
      const banet_grid_level_t& L = tb.lv[l];
      const int Ho = L.Ho, Wo = L.Wo;
      int i0, i1, j0, j1;
      grid_candidates(Y, Ho, L.sy, L.oy, &i0, &i1);
      grid_candidates(X, Wo, L.sx, L.ox, &j0, &j1);
      const float* __restrict__ g = L.out + (size_t)b * Ho * Wo * C + c;
      for (int i = i0; i <= i1; ++i) {
        const float y = grid_coord(i, L.sy, L.oy);
        for (int j = j0; j <= j1; ++j) {
          const ResampleTaps t = resample_taps(grid_coord(j, L.sx, L.ox), y, H, W, mode);
          bool hit[4];
          bool any = false;
#pragma unroll
          for (int q = 0; q < 4; ++q) {   // (a clamped texel is always in the image, so m = 0 never equals a hit by accident)
            hit[q] = t.ok && t.m[q] != 0.f && t.tx[q] == X && t.ty[q] == Y;
            any = any || hit[q];
          }
          if (!any) continue;
          Vec<V> gv;
          gv.load(g + ((size_t)i * Wo + j) * C);
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (hit[q]) {
#pragma unroll
              for (int k = 0; k < V; ++k) acc.v[k] = fmaf(t.w[q], gv.v[k], acc.v[k]);
            }
        }
      }
    }
    acc.store(o);
  }
}

namespace {

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// the checks of both entries, in one order; fills the table
int grid_table(const void* data, int B, int H, int W, int C, int mode, const banet_grid_level_t* levels, int n_levels, GridTable* tb,
               int* V) {
  if (!data || !levels) return BANET_ERR_INVALID_ARG;
  if (mode != BANET_RESAMPLE_ZERO_PAD && mode != BANET_RESAMPLE_CLAMP) return BANET_ERR_INVALID_ARG;
  int rc = grid_check_shape(B, H, W, C, n_levels);
  if (rc) return rc;
  bool wide = (C & 3) == 0 && aligned16(data);
  for (int l = 0; l < n_levels; ++l) {
    const banet_grid_level_t& L = levels[l];
    if (!L.out) return BANET_ERR_INVALID_ARG;
    rc = grid_check_level(H, W, C, L.Ho, L.Wo, L.sx, L.sy, L.ox, L.oy);
    if (rc) return rc;
    wide = wide && aligned16(L.out);
  }
  *V = wide ? 4 : 1;
  tb->n = n_levels;
  tb->pad_ = 0;
  tb->start[0] = 0;
  for (int l = 0; l < kGridMaxLevels; ++l) {
    tb->lv[l] = levels[l < n_levels ? l : 0];
    tb->start[l + 1] = tb->start[l] + (l < n_levels ? (unsigned long long)levels[l].Ho * levels[l].Wo * (C / *V) : 0ull);
  }
  return BANET_OK;
}

unsigned grid_blocks(unsigned long long items, int B) {
  const unsigned long long want = (items + 255) / 256, cap = (unsigned long long)std::max(1, (4096 + B - 1) / B);
  return (unsigned)std::max<unsigned long long>(1, std::min(want, cap));
}

}  // namespace

int launch_grid_resample(const float* data, int B, int H, int W, int C, int mode, const banet_grid_level_t* levels, int n_levels,
                         hipStream_t s) {
  GridTable tb;
  int V;
  const int rc = grid_table(data, B, H, W, C, mode, levels, n_levels, &tb, &V);
  if (rc != BANET_OK) return rc;
  const dim3 grid(grid_blocks(tb.start[tb.n], B), B), block(256);
  if (V == 4)
    hipLaunchKernelGGL(ba_grid_resample_kernel<4>, grid, block, 0, s, data, tb, H, W, C, C / 4, mode);
  else
    hipLaunchKernelGGL(ba_grid_resample_kernel<1>, grid, block, 0, s, data, tb, H, W, C, C, mode);
  return hipGetLastError() == hipSuccess ? BANET_OK : BANET_ERR_LAUNCH;
}

int launch_grid_resample_grad(float* ddata, int B, int H, int W, int C, int mode, const banet_grid_level_t* levels, int n_levels,
                              int overwrite, hipStream_t s) {
  GridTable tb;
  int V;
  const int rc = grid_table(ddata, B, H, W, C, mode, levels, n_levels, &tb, &V);
  if (rc != BANET_OK) return rc;
  const dim3 grid(grid_blocks((unsigned long long)H * W * (C / V), B), B), block(256);
  if (V == 4)
    hipLaunchKernelGGL(ba_grid_resample_adjoint_kernel<4>, grid, block, 0, s, ddata, tb, H, W, C, C / 4, mode, overwrite);
  else
    hipLaunchKernelGGL(ba_grid_resample_adjoint_kernel<1>, grid, block, 0, s, ddata, tb, H, W, C, C, mode, overwrite);
  return hipGetLastError() == hipSuccess ? BANET_OK : BANET_ERR_LAUNCH;
}

}  // namespace banet
