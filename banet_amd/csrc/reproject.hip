// Depth reprojection with a z-buffer (banet_depth_reproject_f32): the key frame's depth map D = depth + basis . Wc carried into
// the pixel grid of every target frame f of a dense level at the poses (R_f, T_f).
//   (a) reproj_init_kernel    keys[b,f,texel] = all ones (the workspace holds arbitrary bytes on entry)
//   (b) reproj_splat_kernel   per source pixel n: D (once per pixel, reused for every frame), then per frame the float32 geometry
//       statements of the assembly / residual pass (strip_geometry, quad_common.hpp): ray from the pixel index, the level scale
//       and intr; X = R_f (p D) + T_f; (px, py) with the level intrinsics intr / scale; d' = |X| (normalize_rays: range along the
//       ray) or X_z.  A point with (px, py) inside [0, W-1] x [0, H-1] (NaN fails the comparison), X_z > 0 and a finite d' > 0
//       lands on texel (floor(px + 0.5), floor(py + 0.5)) with the key (bits of d' << 32) | n through an unsigned 64-bit atomic min:
//       d' > 0, so its bit pattern orders like its value and the smallest (d', n) wins whatever the arrival order.
//   (c) reproj_decode_kernel  every element of both outputs: depth = the key's high word as a float, index = its low word; 0 / -1
//       where the key is still all ones (a finite d' never has that high word).
// Integer atomics only.  The kernel's bytes are the basis rows: 16 lanes per pixel, lane l takes the 4-column chunks l, l + 16, ...
// of the row, as one 16-byte load each where K % 4 == 0 and the basis is 16-byte aligned, else as up to four 4-byte loads -- the
// same fma chain in the same order either way, then the 16-lane row sum.  Nothing depends on B or on the grid.
#include "kernels.hpp"

namespace banet {

constexpr int kRpStepPts = 4;   // pixels per wave instruction (16 lanes each)

struct ReprojArgs {
  int B, N, K, H, W, F, normalize;
  float scale;
  const float* depth;
  const float* basis;
  const float* intr;
  const float* R;
  const float* T;
  const float* Wc;   // nullptr: D = depth
  unsigned long long* keys;
  int units;         // 4-pixel units per window
};

__global__ __launch_bounds__(256) void reproj_init_kernel(unsigned long long* __restrict__ keys, size_t count) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (size_t)gridDim.x * 256) keys[i] = ~0ull;
}

template <bool VEC4>
__global__ __launch_bounds__(kBlock) void reproj_splat_kernel(const ReprojArgs a) {
  const int b = blockIdx.y;
  const int lane = lane_id(), row = lane >> 4, l = lane & 15;
  const int N = a.N, K = a.K, H = a.H, W = a.W, F = a.F;
  const float* __restrict__ dep_b = a.depth + (size_t)b * N;
  const float* __restrict__ bas_b = a.Wc ? a.basis + (size_t)b * N * K : nullptr;
  const float* __restrict__ wc_b = a.Wc ? a.Wc + (size_t)b * K : nullptr;
  const float fx0 = rfl(a.intr[b * 4 + 0]), fy0 = rfl(a.intr[b * 4 + 1]), ox0 = rfl(a.intr[b * 4 + 2]), oy0 = rfl(a.intr[b * 4 + 3]);
  const float fx = fx0 / a.scale, fy = fy0 / a.scale, ox = ox0 / a.scale, oy = oy0 / a.scale;

  const int gw = blockIdx.x * kNumWaves + wave_id(), nw = gridDim.x * kNumWaves;
  for (int u = gw; u < a.units; u += nw) {   // wave-uniform
    const int n = u * kRpStepPts + row;
    const bool valid = n < N;
    const int pt = valid ? n : 0;            // rows past the end read pixel 0 (always there) and land nowhere
    float D = dep_b[pt];
    if (wc_b != nullptr) {
      const float* brow = bas_b + (size_t)pt * K;
      float acc = 0.f;
      for (int c = 4 * l; c < K; c += 64) {
        if constexpr (VEC4) {
          const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(brow + c));   // K % 4 == 0: inside the row
          acc = fmaf(v.x, wc_b[c + 0], acc);
          acc = fmaf(v.y, wc_b[c + 1], acc);
          acc = fmaf(v.z, wc_b[c + 2], acc);
          acc = fmaf(v.w, wc_b[c + 3], acc);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (c + e < K) acc = fmaf(brow[c + e], wc_b[c + e], acc);
        }
      }
      D += row16_sum(acc);
    }
    const int py = pt / W, px = pt - py * W;
    float p0 = ((float)px * a.scale - ox0) / fx0;
    float p1 = ((float)py * a.scale - oy0) / fy0;
    float p2 = 1.f;
    if (a.normalize) {
      const float ss = p0 * p0 + p1 * p1 + p2 * p2;
      const float inv = 1.f / sqrtf(fmaxf(ss, 1e-12f));
      p0 *= inv;
      p1 *= inv;
      p2 *= inv;
    }
    for (int f = 0; f < F; ++f) {
      const size_t vb = (size_t)b * F + f;
      const float* __restrict__ Rm = a.R + vb * 9;
      const float* __restrict__ Tv = a.T + vb * 3;
      const float rx = Rm[0] * p0 + Rm[1] * p1 + Rm[2] * p2;
      const float ry = Rm[3] * p0 + Rm[4] * p1 + Rm[5] * p2;
      const float rz = Rm[6] * p0 + Rm[7] * p1 + Rm[8] * p2;
      const float X = rx * D + Tv[0], Y = ry * D + Tv[1], Z = rz * D + Tv[2];
      const float x = X / Z, y = Y / Z;
      const float pxl = fx * x + ox, pyl = fy * y + oy;
      const float dp = a.normalize ? sqrtf(X * X + Y * Y + Z * Z) : Z;
      const bool in = (pxl >= 0.f) && (pxl <= (float)(W - 1)) && (pyl >= 0.f) && (pyl <= (float)(H - 1));   // false for NaN
      const bool ok = valid && in && (Z > 0.f) && (dp > 0.f) && (dp < __builtin_huge_valf());
      if (ok && l == 0) {
        int tx = (int)floorf(pxl + 0.5f), ty = (int)floorf(pyl + 0.5f);
        tx = min(max(tx, 0), W - 1);   // (already inside: 0 <= pxl <= W - 1)
        ty = min(max(ty, 0), H - 1);
        const unsigned long long key = ((unsigned long long)__float_as_uint(dp) << 32) | (unsigned)n;
        atomicMin(a.keys + vb * (size_t)N + (size_t)ty * W + tx, key);
      }
    }
  }
}

__global__ __launch_bounds__(256) void reproj_decode_kernel(const unsigned long long* __restrict__ keys, float* __restrict__ depth,
                                                            int32_t* __restrict__ index, size_t count) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (size_t)gridDim.x * 256) {
    const unsigned long long k = keys[i];
    const bool hit = k != ~0ull;
    depth[i] = hit ? __uint_as_float((unsigned)(k >> 32)) : 0.f;
    index[i] = hit ? (int32_t)(unsigned)(k & 0xffffffffull) : -1;
  }
}

int plan_reproject(const banet_level_t* lv, size_t* bytes) {
  if (!lv || lv->B < 1 || lv->N < 1 || lv->K < 0 || lv->H < 1 || lv->W < 1 || lv->pairs < 0) return BANET_ERR_INVALID_ARG;
  if (!lv->dense) return BANET_ERR_UNSUPPORTED;
  if ((long long)lv->H * lv->W != (long long)lv->N || !(lv->scale > 0.f)) return BANET_ERR_INVALID_ARG;
  *bytes = align_up((size_t)lv->B * npairs(lv) * lv->N * sizeof(unsigned long long), 256);
  return BANET_OK;
}

int launch_reproject(const banet_level_t* lv, const float* R, const float* T, const float* Wc, const banet_reproject_out_t* out,
                     void* ws, hipStream_t s) {
  ReprojArgs a;
  a.B = lv->B;
  a.N = lv->N;
  a.K = lv->K;
  a.H = lv->H;
  a.W = lv->W;
  a.F = npairs(lv);
  a.normalize = lv->normalize_rays;
  a.scale = lv->scale;
  a.depth = lv->depth;
  a.basis = lv->basis;
  a.intr = lv->intr;
  a.R = R;
  a.T = T;
  a.Wc = lv->K > 0 ? Wc : nullptr;
  a.keys = static_cast<unsigned long long*>(ws);
  a.units = (lv->N + kRpStepPts - 1) / kRpStepPts;
  const size_t count = (size_t)a.B * a.F * a.N;
  const int fill = (int)std::min<size_t>((count + 255) / 256, (size_t)num_cus() * 16);
  hipLaunchKernelGGL(reproj_init_kernel, dim3(fill), dim3(256), 0, s, a.keys, count);
  if (hipGetLastError() != hipSuccess) return BANET_ERR_LAUNCH;
  const int want = (a.units + kNumWaves - 1) / kNumWaves;
  int G = (num_cus() * 8 + a.B - 1) / a.B;   // the grid enters no result
  if (G > want) G = want;
  if (G < 1) G = 1;
  const bool vec4 = a.Wc != nullptr && (a.K % 4 == 0) && (reinterpret_cast<uintptr_t>(a.basis) & 15u) == 0;
  if (vec4) hipLaunchKernelGGL(reproj_splat_kernel<true>, dim3(G, a.B), dim3(kBlock), 0, s, a);
  else hipLaunchKernelGGL(reproj_splat_kernel<false>, dim3(G, a.B), dim3(kBlock), 0, s, a);
  if (hipGetLastError() != hipSuccess) return BANET_ERR_LAUNCH;
  hipLaunchKernelGGL(reproj_decode_kernel, dim3(fill), dim3(256), 0, s, a.keys, out->depth, out->index, count);
  if (hipGetLastError() != hipSuccess) return BANET_ERR_LAUNCH;
  return BANET_OK;
}

}  // namespace banet
