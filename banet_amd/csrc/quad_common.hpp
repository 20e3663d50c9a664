// Device helpers shared by the quad-lane C = 128 gather kernels (gather128s.hip: strip segments with a rolling LDS window;
// gather128q.hip: 16-pixel items with direct taps): 4 lanes per pixel, 8 channels per lane and 32-channel slice.
#pragma once
#include "gather_common.hpp"

namespace banet {

// per-chunk state of a segment (one register per chunk of 64 pixels) is held in groups of four chunks: inside a group the
// chunk index is a run-time loop counter (4-way select chains, ~3 instructions per access), across groups a compile-time
// one (the group loop is unrolled) -- an 8-wide register vector with a run-time index costs 7-8 v_cndmask per access, which
// made 32-row segments slower than 16-row ones although they fetch less (profiles/r03_run11_*)
typedef float fvec4 __attribute__((ext_vector_type(4)));
typedef int ivec4 __attribute__((ext_vector_type(4)));

// sum over the 4 lanes of a quad; every lane of the quad gets the total, fixed order
__device__ __forceinline__ float quad_sum(float v) {
  v += dpp_mov<kDppXor1>(v);
  v += dpp_mov<kDppXor2>(v);
  return v;
}
// lane k of every quad -> all four lanes of the quad
template <int K4>
__device__ __forceinline__ int quad_bcast(int v) {
  return __builtin_amdgcn_update_dpp(0, v, K4 * 0x55, 0xF, 0xF, true);   // quad_perm:[k,k,k,k]
}
template <int K4>
__device__ __forceinline__ float quad_bcast(float v) {
  return __builtin_bit_cast(float, quad_bcast<K4>(__builtin_bit_cast(int, v)));
}

// ---- reductions of the lane = pixel phases on DPP + the half / row swaps: no ds_bpermute (__shfl_xor), no s_waitcnt lgkmcnt ----
constexpr int kDppShl4 = 0x104;        // lane i <- lane i + 4 of its 16-lane row (lanes 12..15 read nothing: 0 with bound_ctrl)
constexpr int kDppRor4 = 0x124;        // lane i <- the lane 4 away around its 16-lane row
template <int CTRL>
__device__ __forceinline__ int dpp_movi(int v) {
  return __builtin_amdgcn_update_dpp(v, v, CTRL, 0xF, 0xF, false);
}
// min (MAX = false) / max over the wave; COLS: over the 16 lanes that agree in lane & 3 only (one pixel row of a chunk: lane = 4 x
// column + row).  Every lane gets the result; exact, so the order does not matter.
template <bool MAX, bool COLS>
__device__ __forceinline__ int wave_minmax(int v) {
  auto op = [](int a, int b) { return MAX ? max(a, b) : min(a, b); };
  if constexpr (COLS) {
    v = op(v, dpp_movi<kDppRor4>(v));
    v = op(v, dpp_movi<kDppRor8>(v));
  } else {
    v = op(v, dpp_movi<kDppRor8>(v));
    v = op(v, dpp_movi<kDppHalfMirror>(v));
    v = op(v, dpp_movi<kDppXor2>(v));
    v = op(v, dpp_movi<kDppXor1>(v));
  }
  int a = v, b = v;
  asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));   // (s_nop: VALU write -> permlane read, cf. bfly_merge)
  v = op(a, b);
  a = v;
  b = v;
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
  return op(a, b);
}
// sum over the 16 lanes that agree in lane & 3, valid on LANES 0..3 only, in the pairing of the xor butterfly over the lane
// distances 4, 8, 16, 32 ((v[l] + v[l+4]) + (v[l+8] + v[l+12]) per row, rows 0 + 1 and 2 + 3, then the halves): the same bits
__device__ __forceinline__ float cols16_sum_lanes03(float v) {
  v += dpp_mov<kDppShl4>(v);
  v += dpp_mov<kDppRor8>(v);
  v = bfly_merge(v, v, 16);
  return bfly_merge(v, v, 32);
}

struct SGeo {
  float dx, dy, jd0, jd1;
  float jc[12];
  int x0, y0, flags;   // kPix* bits (gather_common.hpp)
};

// the pixel's projection, tap fractions and Jacobian rows from (pixel, D, R, T): statement for statement the geometry
// phase of ba_gather128_kernel (gather128.hip)
// The pose and the window's full-resolution intrinsics as 16 wave-uniform scalars, read ONCE per (window, target frame) by the caller.
// Read inside strip_geometry they were vector loads (the compiler cannot prove that the kernel's own stores do not alias R / T / intr,
// so it neither hoists them nor uses scalar loads): five loads and three s_waitcnt vmcnt(0) round trips per chunk and phase, 24 per
// segment, each of which also drains whatever the wave has in flight (round 5).
struct PoseIntr {
  float R[9], T[3], fx0, fy0, ox0, oy0;
};
__device__ __forceinline__ PoseIntr load_pose_intr(const banet_level_t& lv, int b, const float* __restrict__ Rm, const float* __restrict__ Tv) {
  auto u = [](float v) { return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v))); };   // -> SGPRs
  PoseIntr q;
#pragma unroll
  for (int i = 0; i < 9; ++i) q.R[i] = u(Rm[i]);
#pragma unroll
  for (int i = 0; i < 3; ++i) q.T[i] = u(Tv[i]);
  q.fx0 = u(lv.intr[b * 4 + 0]);
  q.fy0 = u(lv.intr[b * 4 + 1]);
  q.ox0 = u(lv.intr[b * 4 + 2]);
  q.oy0 = u(lv.intr[b * 4 + 3]);
  return q;
}
__device__ __forceinline__ void strip_geometry(const banet_level_t& lv, const PoseIntr& pq, bool valid, int px, int py, float D, SGeo& o) {
  const int W = lv.W, H = lv.H;
  const float* Rm = pq.R;
  const float* Tv = pq.T;
  o.dx = o.dy = o.jd0 = o.jd1 = 0.f;
  float p0 = 0.f, p1 = 0.f, p2 = 1.f, fx = 1.f, fy = 1.f, ox = 0.f, oy = 0.f;
  if (valid) {
    const float fx0 = pq.fx0, fy0 = pq.fy0, ox0 = pq.ox0, oy0 = pq.oy0;
    p0 = ((float)px * lv.scale - ox0) / fx0;
    p1 = ((float)py * lv.scale - oy0) / fy0;
    p2 = 1.f;
    if (lv.normalize_rays) {
      const float ss = p0 * p0 + p1 * p1 + p2 * p2;
      const float inv = 1.f / sqrtf(fmaxf(ss, 1e-12f));
      p0 *= inv;
      p1 *= inv;
      p2 *= inv;
    }
    fx = fx0 / lv.scale;
    fy = fy0 / lv.scale;
    ox = ox0 / lv.scale;
    oy = oy0 / lv.scale;
  }
  const float rx = Rm[0] * p0 + Rm[1] * p1 + Rm[2] * p2;
  const float ry = Rm[3] * p0 + Rm[4] * p1 + Rm[5] * p2;
  const float rz = Rm[6] * p0 + Rm[7] * p1 + Rm[8] * p2;
  const float X = rx * D + Tv[0], Y = ry * D + Tv[1], Z = rz * D + Tv[2];
  const float x = X / Z, y = Y / Z;
  const float pxl = fx * x + ox, pyl = fy * y + oy;
  const bool m = valid && (pxl >= 0.f) && (pxl <= (float)(W - 1)) && (pyl >= 0.f) && (pyl <= (float)(H - 1));
#pragma unroll
  for (int i = 0; i < 12; ++i) o.jc[i] = 0.f;
  int x0 = 0, y0 = 0;
  if (m) {
    const float xf = floorf(pxl), yf = floorf(pyl);
    o.dx = pxl - xf;
    o.dy = pyl - yf;
    x0 = (int)xf;
    y0 = (int)yf;
    const float iz = 1.f / Z;
    o.jc[0] = fx * (x * y);
    o.jc[1] = fx * (-1.f - x * x);
    o.jc[2] = fx * y;
    o.jc[3] = fx * (-iz);
    o.jc[4] = 0.f;
    o.jc[5] = fx * (x / Z);
    o.jc[6] = fy * (1.f + y * y);
    o.jc[7] = fy * (-(x * y));
    o.jc[8] = fy * (-x);
    o.jc[9] = 0.f;
    o.jc[10] = fy * (-iz);
    o.jc[11] = fy * (y / Z);
    o.jd0 = fx * ((rx - rz * x) / Z);
    o.jd1 = fy * ((ry - rz * y) / Z);
  }
  const bool interior = (x0 >= 1) && (x0 + 2 <= W - 1) && (y0 >= 1) && (y0 + 2 <= H - 1);
  const bool fast = m && interior;
  o.flags = (m ? kPixInMask : 0) | (fast ? kPixFast : 0) | ((m && !fast) ? kPixRim : 0);
  o.x0 = x0;
  o.y0 = y0;
}

}  // namespace banet
