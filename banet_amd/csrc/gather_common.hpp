// Shared device helpers of the gather kernels (gather_generic.hip: generic C / 3C-map layout;
// gather128*.hip: C = 128 fast paths) and the per-family step launchers gather.hip walks.
#pragma once
#include "kernels.hpp"

namespace banet {

struct GatherArgs {
  banet_level_t lv;
  const float* R;
  const float* T;
  const float* Wc;
  const int32_t* active;
  int active_stride;
  float* rec;       // [B][N][8]  u0..u5, s, r   (bundle only)
  float* partials;  // [B][G][kGHdr + C]
  int G, tiles, tiles_x, tiles_y, groups;
  int* queue;       // [B][8] tile-queue heads (ba_gather128_kernel), zero at launch
  int nbands;
  int pairs;        // target frames per window: blockIdx.y = window * pairs + pair
  int pairloop;     // ba_gather128p_kernel: 1 = grid y = window, the window's target frames are looped over inside a tile
  int qshift;       // ba_gather128_kernel: 0 = a work item is a tile, 2 = a quarter tile (small levels)
  int seg_h;        // ba_gather128s_kernel: pixel rows per strip segment (32 or 16)
  unsigned char* mask_out;   // optional (parity diagnostics): [B * pairs][N] the in-image mask bit of every pixel, or nullptr
  int strip_fp;     // ba_gather128s_kernel: 1 = frame-parallel workgroups (`pairs` waves per segment, one per target frame)
  int tile_pts;     // ba_gather_kernel, sparse points: points per wave item (64 or 16)
};

// per-pixel geometry bits of the gather kernels (`gflags`, QuadGeo::flags)
enum : int {
  kPixInMask = 1,   // the projection falls inside the target image
  kPixFast = 2,     // ... and its whole stencil does (3C map: always): the main loop's taps
  kPixRim = 4,      // in the mask but on the rim: patched by the slow path
};

template <int VEC>
struct Vec {
  float v[VEC];
};

// Branch-free row load: lanes beyond the row length read element 0 (always valid) and are
// zeroed by a select afterwards.  No exec-mask branch => the compiler can keep every row load
// of a pixel pair in flight together (an `if (ok) load` splits them into wait-separated blocks).
template <int VEC>
__device__ __forceinline__ Vec<VEC> ldv(const float* __restrict__ row, int c, bool ok) {
  Vec<VEC> r;
  const float* p = row + (ok ? c : 0);
  if constexpr (VEC == 2) {
    const float2 t = *reinterpret_cast<const float2*>(p);
    r.v[0] = ok ? t.x : 0.f;
    r.v[1] = ok ? t.y : 0.f;
  } else {
    const float t = *p;
    r.v[0] = ok ? t : 0.f;
  }
  return r;
}

// same, with the non-temporal hint: for rows that are streamed exactly once (basis, source)
template <int VEC>
__device__ __forceinline__ Vec<VEC> ldv_nt(const float* __restrict__ row, int c, bool ok) {
  Vec<VEC> r;
  const float* p = row + (ok ? c : 0);
  if constexpr (VEC == 2) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    const f32x2 t = __builtin_nontemporal_load(reinterpret_cast<const f32x2*>(p));
    r.v[0] = ok ? t.x : 0.f;
    r.v[1] = ok ? t.y : 0.f;
  } else {
    const float t = __builtin_nontemporal_load(p);
    r.v[0] = ok ? t : 0.f;
  }
  return r;
}

// dense tile order: vertical strips 8 tiles wide, row-major inside a strip, so that tiles that
// are processed at the same time share target rows in L1/L2.
__device__ __forceinline__ void tile_coords(int t, int tiles_x, int tiles_y, int& tx, int& ty) {
  const int full = tiles_x >> 3;
  const int per_strip = tiles_y << 3;
  if (t < full * per_strip) {
    const int s = t / per_strip;
    const int r = t - s * per_strip;
    ty = r >> 3;
    tx = (s << 3) + (r & 7);
  } else {
    const int r = t - full * per_strip;
    const int wl = tiles_x - (full << 3);
    ty = r / wl;
    tx = (full << 3) + (r - ty * wl);
  }
}

__device__ __forceinline__ float rdl(float v, int l) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}
__device__ __forceinline__ int rdl(int v, int l) { return __builtin_amdgcn_readlane(v, l); }

// binary-counter carry chain of the transposing butterfly: leaf t (0..63) in, result out after
// leaf 63; level L merges with lane distance 32>>L, so leaf t ends on lane bitrev6(t).
__device__ __forceinline__ float merge(float a, float b, int s) { return bfly_merge(a, b, s); }
__device__ __forceinline__ Q5 merge(const Q5& a, const Q5& b, int s) { return q5_merge(a, b, s); }

template <typename TT>
__device__ __forceinline__ void carry_push(TT (&pend)[6], TT v, int t, TT& out) {
  bool done = false;
#pragma unroll
  for (int L = 0; L < 6; ++L) {
    if (!done) {
      if (((t >> L) & 1) == 0) {
        pend[L] = v;
        done = true;
      } else {
        v = merge(pend[L], v, 32 >> L);
      }
    }
  }
  if (!done) out = v;
}

__device__ __forceinline__ int brev6(int t) { return (int)(__brev((unsigned)t) >> 26); }

#ifdef BANET_TIMING  // development aid: per-segment cycle counts of the gather loop (tools/prof_assemble.py)
__device__ __forceinline__ unsigned long long tick() {
  unsigned long long t;
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  return t;
}
__device__ __forceinline__ unsigned long long realtime() {  // 100 MHz, synchronised across the chip
  unsigned long long t;
  asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  return t;
}
#define BANET_TICK(var) const unsigned long long var = tick()
#define BANET_TACC(acc, a, b) acc += (float)((b) - (a))
#else
#define BANET_TICK(var)
#define BANET_TACC(acc, a, b)
#endif

// Pixel id n (= the lane that owns the pixel) -> position inside the 8x8 patch.  The butterfly
// visits pixel ids in the order brev6(0), brev6(1), ...; mapping id n to the Z-order (Morton)
// position of brev6(n) makes consecutive visits spatial neighbours (they share 8 of their 12
// target texel rows while those are still in L1/L2).
__device__ __forceinline__ void patch_pos(int n, int& px, int& py) {
  const int z = brev6(n);  // visit order of this pixel id
  px = (z & 1) | ((z >> 1) & 2) | ((z >> 2) & 4);
  py = ((z >> 1) & 1) | ((z >> 2) & 2) | ((z >> 3) & 4);
}

// Slow generic path for pixels whose gradient stencil touches the image rim: clamped taps
// (utils_python.py:96-99) and reflect-padded central differences (bundlenet.py:97-99).
template <int VEC, int CH>
__device__ __noinline__ Q5 border_pixel_q5(int x0, int y0, float w00, float w01, float w10, float w11,
                                           const float* __restrict__ srow, const float* __restrict__ tgt_b, int C,
                                           int H, int W, int lane, float (&absd)[CH][VEC]) {
  Q5 q{0.f, 0.f, 0.f, 0.f, 0.f};
  const float wt[4] = {w00, w01, w10, w11};
  const int xs[2] = {min(max(x0, 0), W - 1), min(max(x0 + 1, 0), W - 1)};
  const int ys[2] = {min(max(y0, 0), H - 1), min(max(y0 + 1, 0), H - 1)};
#pragma unroll
  for (int ch = 0; ch < CH; ++ch) {
    const int c = (ch * 64 + lane) * VEC;
    const bool ok = c < C;
    const Vec<VEC> f1 = ldv<VEC>(srow, c, ok);
    Vec<VEC> f, gx, gy;
#pragma unroll
    for (int e = 0; e < VEC; ++e) f.v[e] = gx.v[e] = gy.v[e] = 0.f;
#pragma unroll
    for (int iy = 0; iy < 2; ++iy)
#pragma unroll
      for (int ix = 0; ix < 2; ++ix) {
        const int xc = xs[ix], yc = ys[iy];
        const Vec<VEC> cc = ldv<VEC>(tgt_b + (size_t)(yc * W + xc) * C, c, ok);
        const Vec<VEC> xl = ldv<VEC>(tgt_b + (size_t)(yc * W + refl_m(xc)) * C, c, ok);
        const Vec<VEC> xr = ldv<VEC>(tgt_b + (size_t)(yc * W + refl_p(xc, W)) * C, c, ok);
        const Vec<VEC> yu = ldv<VEC>(tgt_b + (size_t)(refl_m(yc) * W + xc) * C, c, ok);
        const Vec<VEC> yd = ldv<VEC>(tgt_b + (size_t)(refl_p(yc, H) * W + xc) * C, c, ok);
        const float wq = wt[iy * 2 + ix];
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          f.v[e] += cc.v[e] * wq;
          gx.v[e] += (0.5f * (xr.v[e] - xl.v[e])) * wq;
          gy.v[e] += (0.5f * (yd.v[e] - yu.v[e])) * wq;
        }
      }
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const float d = f.v[e] - f1.v[e];
      q.m11 = fmaf(gx.v[e], gx.v[e], q.m11);
      q.m12 = fmaf(gx.v[e], gy.v[e], q.m12);
      q.m22 = fmaf(gy.v[e], gy.v[e], q.m22);
      q.g1 = fmaf(gx.v[e], d, q.g1);
      q.g2 = fmaf(gy.v[e], d, q.g2);
      absd[ch][e] += fabsf(d);
    }
  }
  return q;
}

// (BANET_G128_WAVES / BANET_G128P_WAVES, the workgroups per CU of the launch bounds: plan.hpp)

// ---- helpers of the C = 128 kernels (gather128 / 128p / 128s / 128q.hip) ---------------------------------------------------------------
constexpr int kC128 = 128;
constexpr int kParStride = 8;  // tile kernels' per-pixel tap parameters in LDS: src offset, texel offset, w00,w01,w10,w11 (pre-masked), mask, -
typedef float v2f __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void morton8(int n, int& px, int& py) {  // pixel id -> position in the 8x8 patch
  px = (n & 1) | ((n >> 1) & 2) | ((n >> 2) & 4);
  py = ((n >> 1) & 1) | ((n >> 2) & 2) | ((n >> 3) & 4);
}

__device__ __forceinline__ int brev5(int t) { return (int)(__brev((unsigned)t) >> 27); }

// carry chain of the transposing butterfly over NL levels, first lane distance S0 (cf. carry_push)
template <int NL, int S0>
__device__ __forceinline__ void carry_push_n(float (&pend)[NL + 1], float v, int t) {
  bool done = false;
#pragma unroll
  for (int L = 0; L < NL; ++L) {
    if (!done) {
      if (((t >> L) & 1) == 0) {
        pend[L] = v;
        done = true;
      } else {
        v = bfly_merge(pend[L], v, S0 >> L);
      }
    }
  }
  if (!done) pend[NL] = v;
}

// channel maths of one pixel's 4-channel slice (packed fp32), accumulated into q[5] / absd[4]
__device__ __forceinline__ void tap_math(const float4& f1, const float4& a0, const float4& a1, const float4& a2,
                                         const float4& a3, const float4& b0, const float4& b1, const float4& b2,
                                         const float4& b3, const float4& m1, const float4& m2, const float4& p1,
                                         const float4& p2, float w00, float w01, float w10, float w11, float mk,
                                         float (&q)[5], float (&absd)[4]) {
  const float h00 = 0.5f * w00, h01 = 0.5f * w01, h10 = 0.5f * w10, h11 = 0.5f * w11;
#ifdef BANET_TAP_SCALAR   // development A/B (build with -fno-slp-vectorize): the same arithmetic, same order, one channel per instruction
  {
    const float F1[4] = {f1.x, f1.y, f1.z, f1.w}, A0[4] = {a0.x, a0.y, a0.z, a0.w}, A1[4] = {a1.x, a1.y, a1.z, a1.w},
                A2[4] = {a2.x, a2.y, a2.z, a2.w}, A3[4] = {a3.x, a3.y, a3.z, a3.w}, B0[4] = {b0.x, b0.y, b0.z, b0.w},
                B1[4] = {b1.x, b1.y, b1.z, b1.w}, B2[4] = {b2.x, b2.y, b2.z, b2.w}, B3[4] = {b3.x, b3.y, b3.z, b3.w},
                M1[4] = {m1.x, m1.y, m1.z, m1.w}, M2[4] = {m2.x, m2.y, m2.z, m2.w}, P1[4] = {p1.x, p1.y, p1.z, p1.w},
                P2[4] = {p2.x, p2.y, p2.z, p2.w};
    float s11[4], s12[4], s22[4], sg1[4], sg2[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float f = ((A1[c] * w00 + A2[c] * w01) + B1[c] * w10) + B2[c] * w11;
      const float gx = (((A2[c] - A0[c]) * h00 + (A3[c] - A1[c]) * h01) + (B2[c] - B0[c]) * h10) + (B3[c] - B1[c]) * h11;
      const float gy = (((B1[c] - M1[c]) * h00 + (B2[c] - M2[c]) * h01) + (P1[c] - A1[c]) * h10) + (P2[c] - A2[c]) * h11;
      const float d = f - F1[c] * mk;
      s11[c] = gx * gx, s12[c] = gx * gy, s22[c] = gy * gy, sg1[c] = gx * d, sg2[c] = gy * d;
      absd[c] += fabsf(d);
    }
    // the packed form's order: lanes {x, z} and {y, w} accumulate separately, then x + y
    q[0] += (s11[0] + s11[2]) + (s11[1] + s11[3]);
    q[1] += (s12[0] + s12[2]) + (s12[1] + s12[3]);
    q[2] += (s22[0] + s22[2]) + (s22[1] + s22[3]);
    q[3] += (sg1[0] + sg1[2]) + (sg1[1] + sg1[3]);
    q[4] += (sg2[0] + sg2[2]) + (sg2[1] + sg2[3]);
    return;
  }
#endif
  v2f qm11 = {0.f, 0.f}, qm12 = {0.f, 0.f}, qm22 = {0.f, 0.f}, qg1 = {0.f, 0.f}, qg2 = {0.f, 0.f};
#define BANET_V2F(v, k) (v2f){(k) ? (v).z : (v).x, (k) ? (v).w : (v).y}
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const v2f F1 = BANET_V2F(f1, k);
    const v2f A0 = BANET_V2F(a0, k), A1 = BANET_V2F(a1, k), A2 = BANET_V2F(a2, k), A3 = BANET_V2F(a3, k);
    const v2f B0 = BANET_V2F(b0, k), B1 = BANET_V2F(b1, k), B2 = BANET_V2F(b2, k), B3 = BANET_V2F(b3, k);
    const v2f M1 = BANET_V2F(m1, k), M2 = BANET_V2F(m2, k), P1 = BANET_V2F(p1, k), P2 = BANET_V2F(p2, k);
    const v2f f = ((A1 * w00 + A2 * w01) + B1 * w10) + B2 * w11;
    const v2f gx = (((A2 - A0) * h00 + (A3 - A1) * h01) + (B2 - B0) * h10) + (B3 - B1) * h11;
    const v2f gy = (((B1 - M1) * h00 + (B2 - M2) * h01) + (P1 - A1) * h10) + (P2 - A2) * h11;
    const v2f d = f - F1 * mk;
    qm11 += gx * gx;
    qm12 += gx * gy;
    qm22 += gy * gy;
    qg1 += gx * d;
    qg2 += gy * d;
    absd[2 * k] += fabsf(d.x);
    absd[2 * k + 1] += fabsf(d.y);
  }
#undef BANET_V2F
  q[0] += qm11.x + qm11.y;
  q[1] += qm12.x + qm12.y;
  q[2] += qm22.x + qm22.y;
  q[3] += qg1.x + qg1.y;
  q[4] += qg2.x + qg2.y;
}

// one step of plan_gather_steps' list (plan.hpp), one function per kernel family: the instantiation the step names on the step's
// grid, block and LDS; BANET_ERR_UNSUPPORTED for one outside the family's BANET_GATHER_*_LIST
int launch_gather_generic_step(const GatherStep& st, const GatherArgs& a, hipStream_t s);   // gather_generic.hip
int launch_gather128_step(const GatherStep& st, const GatherArgs& a, hipStream_t s);        // gather128.hip: direct loads
int launch_gather128p_step(const GatherStep& st, const GatherArgs& a, hipStream_t s);       // gather128p.hip: wave-private LDS patches
int launch_gather128s_step(const GatherStep& st, const GatherArgs& a, hipStream_t s);       // gather128s.hip: strip segments, rolling LDS window
int launch_gather128q_step(const GatherStep& st, const GatherArgs& a, hipStream_t s);       // gather128q.hip: 4x4-pixel items, one step per item (latency-bound launches)

}  // namespace banet
