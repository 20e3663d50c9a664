// Dense adjoint (driver, derivation and the kernel list in launch order: adjoint.hip): the per-pixel and per-point kernels --
// adj_pixel_kernel, adj_pixel2_kernel -- and adj_fold_kernel, which sums their per-wave partials into dpose.
#include <type_traits>

#include "adjoint_common.hpp"

namespace banet {
namespace adj {

namespace {

// ---- per-pixel adjoint ------------------------------------------------------------------------------------------------
// sum over the wave, every lane gets it: DPP row sums + 4 v_readlane (the ds_bpermute butterfly of wave_sum costs ~6 LDS
// round trips per value; this kernel needs 8 sums per pixel).  Fixed order -> deterministic.
__device__ __forceinline__ float wsum(float v) {
  v = row16_sum(v);
  const float a0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 0));
  const float a1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 16));
  const float a2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 32));
  const float a3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 48));
  return (a0 + a1) + (a2 + a3);
}

// SP (round 5): SPARSE points in the reference's own layout -- what bundlenet.py:332-399 trains on: conv1 [B,N,C] sampled at N points,
// rays p [B,3,N] and per-point level intrinsics supplied (bundlenet.py:115-119), the target map precomputed as [f|gx|gy]
// [B,H,W,3C] (bundlenet.py:92-100) and sampled with plain bilinear taps, clamped one by one like the forward's generic kernel
// (gather_generic.hip, GRAD = true).  Same per-pixel algebra; dmap3 is then the gradient of that 3C map itself.
template <int CJ, int KJ, bool SP = false>   // C <= 64 CJ, K <= 64 KJ (K > 128: 2 waves per SIMD -- the per-coefficient state would spill at 3)
__global__ __launch_bounds__(kBlock, (KJ >= 3 ? 2 : 3)) void adj_pixel_kernel(const AdjArgs a) {
  const banet_level_t& lv = a.lv;
  const int b = blockIdx.y, g = blockIdx.x, lane = threadIdx.x & 63, w = wave_id();
  const int N = lv.N, C = lv.C, K = lv.K, H = lv.H, W = lv.W, P = 6 + K;
  const float* __restrict__ src_b = lv.src + (size_t)b * N * C;
  const float* __restrict__ tgt_b = lv.tgt + (size_t)b * H * W * (SP ? 3 * C : C);
  const float* __restrict__ bas_b = lv.basis + (size_t)b * N * K;
  const float* __restrict__ S = a.S + (size_t)b * P * P;
  const float* __restrict__ gb = a.gb + (size_t)b * P;
  float Scc[6][6], gbc[6], Rm[9], Tv[3];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    gbc[i] = gb[i];
#pragma unroll
    for (int j = 0; j < 6; ++j) Scc[i][j] = S[i * P + j];
  }
#pragma unroll
  for (int i = 0; i < 9; ++i) Rm[i] = a.R[b * 9 + i];
#pragma unroll
  for (int i = 0; i < 3; ++i) Tv[i] = a.T[b * 3 + i];
  float fx0 = 1.f, fy0 = 1.f, ox0 = 0.f, oy0 = 0.f;
  if constexpr (!SP) fx0 = lv.intr[b * 4 + 0], fy0 = lv.intr[b * 4 + 1], ox0 = lv.intr[b * 4 + 2], oy0 = lv.intr[b * 4 + 3];
  float fx = fx0 / lv.scale, fy = fy0 / lv.scale, ox = ox0 / lv.scale, oy = oy0 / lv.scale;     // SP: per point, below
  float wc[KJ], scd[KJ][6], gbd[KJ], dwc[KJ];
  bool kok[KJ], cok[CJ];
#pragma unroll
  for (int j = 0; j < KJ; ++j) {
    const int k = lane + 64 * j;
    kok[j] = k < K;
    wc[j] = kok[j] ? a.Wc[(size_t)b * K + k] : 0.f;
    gbd[j] = kok[j] ? gb[6 + k] : 0.f;
    dwc[j] = 0.f;
#pragma unroll
    for (int i = 0; i < 6; ++i) scd[j][i] = kok[j] ? S[i * P + 6 + k] : 0.f;
  }
  float ga[CJ];
#pragma unroll
  for (int j = 0; j < CJ; ++j) {
    const int c = lane + 64 * j;
    cok[j] = c < C;
    ga[j] = cok[j] ? a.gabs[(size_t)b * C + c] : 0.f;
  }
  float accR[9], accT[3];
#pragma unroll
  for (int i = 0; i < 9; ++i) accR[i] = 0.f;
#pragma unroll
  for (int i = 0; i < 3; ++i) accT[i] = 0.f;

  const int nw = a.G * kNumWaves, chunk = (N + nw - 1) / nw;
  const int n_lo = (g * kNumWaves + w) * chunk, n_hi = min(N, n_lo + chunk);
  for (int n = n_lo; n < n_hi; ++n) {
    // ---- depth and warp (bundlenet.py:206-224), every lane the same values
    float p0, p1, p2;
    if constexpr (SP) {
      const size_t o = (size_t)b * 3 * N, qn = (size_t)b * N + n;
      p0 = lv.rays[o + n], p1 = lv.rays[o + N + n], p2 = lv.rays[o + 2 * (size_t)N + n];
      fx = lv.fx[qn], fy = lv.fy[qn], ox = lv.ox[qn], oy = lv.oy[qn];
    } else {
      const int qy = n / W, qx = n - qy * W;
      p0 = ((float)qx * lv.scale - ox0) / fx0, p1 = ((float)qy * lv.scale - oy0) / fy0, p2 = 1.f;
      if (lv.normalize_rays) {
        const float inv = 1.f / sqrtf(fmaxf(p0 * p0 + p1 * p1 + p2 * p2, 1e-12f));
        p0 *= inv;
        p1 *= inv;
        p2 *= inv;
      }
    }
    float bv[KJ], z2v[KJ], f1v[CJ], bsum = 0.f;
#pragma unroll
    for (int j = 0; j < KJ; ++j) {
      const int k = kok[j] ? lane + 64 * j : 0;
      bv[j] = bas_b[(size_t)n * K + k];
      z2v[j] = a.z2[((size_t)b * N + n) * K + k];
      bv[j] = kok[j] ? bv[j] : 0.f;
      bsum = fmaf(bv[j], wc[j], bsum);
    }
#pragma unroll
    for (int j = 0; j < CJ; ++j) f1v[j] = src_b[(size_t)n * C + (cok[j] ? lane + 64 * j : 0)];
    const float* __restrict__ ar = a.arec + ((size_t)b * N + n) * 8;
    float q[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) q[i] = ar[i];
    const float zeta = ar[6], ee = ar[7];
    const float D = lv.depth[(size_t)b * N + n] + wsum(bsum);
    const float rx = Rm[0] * p0 + Rm[1] * p1 + Rm[2] * p2;
    const float ry = Rm[3] * p0 + Rm[4] * p1 + Rm[5] * p2;
    const float rz = Rm[6] * p0 + Rm[7] * p1 + Rm[8] * p2;
    const float X = rx * D + Tv[0], Y = ry * D + Tv[1], Z = rz * D + Tv[2];
    const float x = X / Z, y = Y / Z;
    const float px = fx * x + ox, py = fy * y + oy;
    const bool m = (px >= 0.f) && (px <= (float)(W - 1)) && (py >= 0.f) && (py <= (float)(H - 1));
    float* __restrict__ fr = a.frac + ((size_t)b * N + n) * kFrac;
    if (!m) {   // wave-uniform: no contribution to anything (M = g = 0)
      if (lane == 0) fr[0] = __int_as_float(-1);
      if (a.overwrite) {   // nothing was zero-filled: this pixel's rows are written here
#pragma unroll
        for (int j = 0; j < CJ; ++j)
          if (cok[j]) a.dsrc[((size_t)b * N + n) * C + lane + 64 * j] = 0.f;
#pragma unroll
        for (int j = 0; j < KJ; ++j)
          if (kok[j]) a.dbasis[((size_t)b * N + n) * K + lane + 64 * j] = 0.f;
        if (lane == 0) a.ddepth[(size_t)b * N + n] = 0.f;
      }
      continue;
    }
    const float xf = floorf(px), yf = floorf(py);
    const int x0 = (int)xf, y0 = (int)yf;
    const float ax = px - xf, ay = py - yf;
    // ---- the 4x4 neighbourhood (minus corners) of the target map, clamped to the image: 12 coalesced row loads per
    // channel chunk; [f|gx|gy] at the 4 bilinear taps from it (grad_fixed on the fly, REFLECT rim -> 0, outside -> 0)
    float tex[CJ][4][4];       // SP: tex[j][t][e] = channel e (f, gx, gy) of the 3C map at bilinear tap t, taps clamped one by one
    if constexpr (SP) {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int yy = min(max(y0 + (t >> 1), 0), H - 1), xx = min(max(x0 + (t & 1), 0), W - 1);
        const float* __restrict__ row = tgt_b + (size_t)(yy * W + xx) * 3 * C;
#pragma unroll
        for (int e = 0; e < 3; ++e)
#pragma unroll
          for (int j = 0; j < CJ; ++j) tex[j][t][e] = row[e * C + (cok[j] ? lane + 64 * j : 0)];
      }
    } else {
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int cc = 0; cc < 4; ++cc) {
        if ((r == 0 || r == 3) && (cc == 0 || cc == 3)) continue;
        const int yy = min(max(y0 - 1 + r, 0), H - 1), xx = min(max(x0 - 1 + cc, 0), W - 1);
        const float* __restrict__ row = tgt_b + (size_t)(yy * W + xx) * C;
#pragma unroll
        for (int j = 0; j < CJ; ++j) tex[j][r][cc] = row[cok[j] ? lane + 64 * j : 0];
      }
    }
    float Sf[CJ], Sgx[CJ], Sgy[CJ], Ax[CJ][3], Ay[CJ][3], dif[CJ];
#pragma unroll
    for (int j = 0; j < CJ; ++j) {
      Sf[j] = Sgx[j] = Sgy[j] = 0.f;
#pragma unroll
      for (int e = 0; e < 3; ++e) Ax[j][e] = Ay[j][e] = 0.f;
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int ix = t & 1, iy = t >> 1;
      const int tx = x0 + ix, ty = y0 + iy;
      const bool in = tx <= W - 1 && ty <= H - 1;
      const float hx = (in && tx > 0 && tx < W - 1) ? 0.5f : 0.f, hy = (in && ty > 0 && ty < H - 1) ? 0.5f : 0.f;
      const float fin = in ? 1.f : 0.f;
      const float wx = ix ? ax : 1.f - ax, wy = iy ? ay : 1.f - ay;
      const float wt = wx * wy, sx = (ix ? 1.f : -1.f) * wy, sy = (iy ? 1.f : -1.f) * wx;
#pragma unroll
      for (int j = 0; j < CJ; ++j) {
        const float F = SP ? tex[j][t][0] : fin * tex[j][1 + iy][1 + ix];
        const float GX = SP ? tex[j][t][1] : hx * (tex[j][1 + iy][2 + ix] - tex[j][1 + iy][ix]);
        const float GY = SP ? tex[j][t][2] : hy * (tex[j][2 + iy][1 + ix] - tex[j][iy][1 + ix]);
        Sf[j] = fmaf(wt, F, Sf[j]);
        Sgx[j] = fmaf(wt, GX, Sgx[j]);
        Sgy[j] = fmaf(wt, GY, Sgy[j]);
        Ax[j][0] = fmaf(sx, F, Ax[j][0]);
        Ax[j][1] = fmaf(sx, GX, Ax[j][1]);
        Ax[j][2] = fmaf(sx, GY, Ax[j][2]);
        Ay[j][0] = fmaf(sy, F, Ay[j][0]);
        Ay[j][1] = fmaf(sy, GX, Ay[j][1]);
        Ay[j][2] = fmaf(sy, GY, Ay[j][2]);
      }
    }
    float M11 = 0.f, M12 = 0.f, M22 = 0.f, g1 = 0.f, g2 = 0.f;
#pragma unroll
    for (int j = 0; j < CJ; ++j) {
      if (!cok[j]) Sf[j] = Sgx[j] = Sgy[j] = f1v[j] = 0.f;
      dif[j] = f1v[j] - Sf[j];       // bundlenet.py:234
      M11 = fmaf(Sgx[j], Sgx[j], M11);
      M12 = fmaf(Sgx[j], Sgy[j], M12);
      M22 = fmaf(Sgy[j], Sgy[j], M22);
      g1 = fmaf(Sgx[j], dif[j], g1);
      g2 = fmaf(Sgy[j], dif[j], g2);
    }
    M11 = wsum(M11);
    M12 = wsum(M12);
    M22 = wsum(M22);
    g1 = wsum(g1);
    g2 = wsum(g2);
    // ---- per-pixel algebra (bundlenet.py:49-74 Jacobians with the bundle sign, J = [-Jc | jd b])
    const float iz = 1.f / Z;
    float J0[6], J1[6];
    J0[0] = fx * (-(x * y));
    J0[1] = fx * (1.f + x * x);
    J0[2] = fx * (-y);
    J0[3] = fx * iz;
    J0[4] = 0.f;
    J0[5] = fx * (-(x * iz));
    J1[0] = fy * (-1.f - y * y);
    J1[1] = fy * (x * y);
    J1[2] = fy * x;
    J1[3] = 0.f;
    J1[4] = fy * iz;
    J1[5] = fy * (-(y * iz));
    const float jd0 = fx * ((rx - rz * x) * iz), jd1 = fy * ((ry - rz * y) * iz);
    float JS0[6], JS1[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      float s0 = jd0 * q[j], s1 = jd1 * q[j];
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        s0 = fmaf(J0[i], Scc[i][j], s0);
        s1 = fmaf(J1[i], Scc[i][j], s1);
      }
      JS0[j] = s0;
      JS1[j] = s1;
    }
    float t0 = jd0 * zeta, t1 = jd1 * zeta, dM11 = 0.f, dM12 = 0.f, dM22 = 0.f, dg1 = jd0 * ee, dg2 = jd1 * ee;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      t0 = fmaf(J0[i], q[i], t0);
      t1 = fmaf(J1[i], q[i], t1);
      dM11 = fmaf(JS0[i], J0[i], dM11);
      dM12 = fmaf(JS0[i], J1[i], dM12);
      dM22 = fmaf(JS1[i], J1[i], dM22);
      dg1 = fmaf(J0[i], gbc[i], dg1);
      dg2 = fmaf(J1[i], gbc[i], dg2);
    }
    dM11 = fmaf(t0, jd0, dM11);
    dM12 = fmaf(t0, jd1, dM12);
    dM22 = fmaf(t1, jd1, dM22);
    float dJ0[6], dJ1[6], u[6];
    const float Mjd0 = M11 * jd0 + M12 * jd1, Mjd1 = M12 * jd0 + M22 * jd1;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      dJ0[i] = 2.f * (M11 * JS0[i] + M12 * JS1[i]) + g1 * gbc[i];
      dJ1[i] = 2.f * (M12 * JS0[i] + M22 * JS1[i]) + g2 * gbc[i];
      u[i] = J0[i] * Mjd0 + J1[i] * Mjd1;
    }
    const float djd0 = 2.f * (M11 * t0 + M12 * t1) + g1 * ee, djd1 = 2.f * (M12 * t0 + M22 * t1) + g2 * ee;
    const float s_n = jd0 * Mjd0 + jd1 * Mjd1, r_n = jd0 * g1 + jd1 * g2;
    // ---- channel adjoints: dsrc, the 3C adjoint row, d(px, py)
    float dpx = 0.f, dpy = 0.f;
    float* __restrict__ dsrc_n = a.dsrc + ((size_t)b * N + n) * C;
    float* __restrict__ arow_n = a.arow + ((size_t)b * N + n) * 3 * C;
#pragma unroll
    for (int j = 0; j < CJ; ++j) {
      const int c = lane + 64 * j;
      if (cok[j]) {
        const float d = dif[j], gx = Sgx[j], gy = Sgy[j];
        const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
        const float dd = dg1 * gx + dg2 * gy + sgn * ga[j];
        const float dgx = 2.f * (dM11 * gx + dM12 * gy) + dg1 * d;
        const float dgy = 2.f * (dM12 * gx + dM22 * gy) + dg2 * d;
        dsrc_n[c] = a.overwrite ? dd : dsrc_n[c] + dd;
        if (a.arow) {
          arow_n[c] = -dd;
          arow_n[C + c] = dgx;
          arow_n[2 * C + c] = dgy;
        }
        dpx += -dd * Ax[j][0] + dgx * Ax[j][1] + dgy * Ax[j][2];
        dpy += -dd * Ay[j][0] + dgx * Ay[j][1] + dgy * Ay[j][2];
      }
    }
    dpx = wsum(dpx);
    dpy = wsum(dpy);
    // ---- geometry adjoint
    float dx_ = fx * dpx + fx * (-y * dJ0[0] + 2.f * x * dJ0[1] - dJ0[5] * iz) + fy * (y * dJ1[1] + dJ1[2]);
    float dy_ = fy * dpy + fx * (-x * dJ0[0] - dJ0[2]) + fy * (-2.f * y * dJ1[0] + x * dJ1[1] - dJ1[5] * iz);
    float dZ_ = (fx * (-dJ0[3] + x * dJ0[5]) + fy * (-dJ1[4] + y * dJ1[5])) * iz * iz;
    float drx = fx * djd0 * iz, dry = fy * djd1 * iz, drz = -(fx * x * djd0 + fy * y * djd1) * iz;
    dx_ -= fx * rz * djd0 * iz;
    dy_ -= fy * rz * djd1 * iz;
    dZ_ -= (jd0 * djd0 + jd1 * djd1) * iz;
    const float dX = dx_ * iz, dY = dy_ * iz, dZt = dZ_ - (x * dx_ + y * dy_) * iz;
    drx = fmaf(dX, D, drx);
    dry = fmaf(dY, D, dry);
    drz = fmaf(dZt, D, drz);
    const float dD = dX * rx + dY * ry + dZt * rz;
    accT[0] += dX;
    accT[1] += dY;
    accT[2] += dZt;
    accR[0] = fmaf(drx, p0, accR[0]);
    accR[1] = fmaf(drx, p1, accR[1]);
    accR[2] = fmaf(drx, p2, accR[2]);
    accR[3] = fmaf(dry, p0, accR[3]);
    accR[4] = fmaf(dry, p1, accR[4]);
    accR[5] = fmaf(dry, p2, accR[5]);
    accR[6] = fmaf(drz, p0, accR[6]);
    accR[7] = fmaf(drz, p1, accR[7]);
    accR[8] = fmaf(drz, p2, accR[8]);
    // ---- depth, basis, coefficients
    float* __restrict__ dbas_n = a.dbasis + ((size_t)b * N + n) * K;
#pragma unroll
    for (int j = 0; j < KJ; ++j) {
      const int k = lane + 64 * j;
      if (kok[j]) {
        float v = s_n * z2v[j] + r_n * gbd[j] + dD * wc[j];
        float su = 0.f;
#pragma unroll
        for (int i = 0; i < 6; ++i) su = fmaf(u[i], scd[j][i], su);
        v = fmaf(2.f, su, v);
        dbas_n[k] = a.overwrite ? v : dbas_n[k] + v;
        dwc[j] = fmaf(dD, bv[j], dwc[j]);
      }
    }
    if (lane == 0) {
      a.ddepth[(size_t)b * N + n] = a.overwrite ? dD : a.ddepth[(size_t)b * N + n] + dD;
      const int key = y0 * W + x0;
      fr[0] = __int_as_float(key);
      fr[1] = ax;
      fr[2] = ay;
      fr[3] = dg1;
      fr[4] = dg2;
      fr[5] = dM11;
      fr[6] = dM12;
      fr[7] = dM22;
      atomicAdd(&a.cnt[(size_t)b * H * W + key], 1);
    }
  }
  float* __restrict__ prow = a.part + ((size_t)b * a.G * kNumWaves + g * kNumWaves + w) * (kAdjHdr + K);
#pragma unroll
  for (int i = 0; i < 9; ++i)
    if (lane == i) prow[i] = accR[i];
#pragma unroll
  for (int i = 0; i < 3; ++i)
    if (lane == 9 + i) prow[9 + i] = accT[i];
#pragma unroll
  for (int j = 0; j < KJ; ++j) {
    const int k = lane + 64 * j;
    if (k < K) prow[kAdjHdr + k] = dwc[j];
  }
}

// ---- per-pixel adjoint, two pixels per wave -------------------------------------------------------------------------------
// Same arithmetic as adj_pixel_kernel with a HALF wave per pixel (lanes 0-31: pixel n, lanes 32-63: pixel n + 1) and 4
// channels / coefficients per lane: every row access is one 16-byte load or store per lane, the per-pixel algebra is done once
// per pair of pixels instead of once per pixel, and the eight reductions per pixel run over 32 lanes (DPP row sum + one
// permlane swap).  C % 4 == 0, C <= 128 CJ4, K % 4 == 0, K <= 128.  Pixels outside the image take safe coordinates and skip
// their stores (the two halves of a wave diverge, so there is no early exit).
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 fma2(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f32x2 splat2(float v) { return f32x2{v, v}; }
__device__ __forceinline__ f32x4 fma4(f32x4 a, f32x4 b, f32x4 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ float hsum(float v) {   // sum over the 32 lanes of each half wave, every lane gets its half's total
  v = row16_sum(v);
  return bfly_merge(v, v, 16);
}

template <int CJ4, bool OW>     // OW: dsrc / ddepth / dbasis are written (BANET_ADJOINT_OVERWRITE), else read (early, with the texels) and added to
__global__ __launch_bounds__(kBlock, 2) void adj_pixel2_kernel(const AdjArgs a) {
  const banet_level_t& lv = a.lv;
  const int b = blockIdx.y, g = blockIdx.x, lane = threadIdx.x & 63, w = wave_id();
  const int N = lv.N, C = lv.C, K = lv.K, H = lv.H, W = lv.W, P = 6 + K;
  const int hl = lane & 31, hi = lane >> 5;
  const float* __restrict__ src_b = lv.src + (size_t)b * N * C;
  const float* __restrict__ tgt_b = lv.tgt + (size_t)b * N * C;
  const float* __restrict__ bas_b = lv.basis + (size_t)b * N * K;
  // every row of the loop = a per-window base (wave-uniform: scalar registers) + an unsigned 32-bit BYTE offset (launch_dense_adjoint
  // takes this kernel only while a window's largest array, N x 3C floats, stays below 4 GB): no 64-bit address arithmetic per access
  const char* const src_c = reinterpret_cast<const char*>(src_b);
  const char* const tgt_c = reinterpret_cast<const char*>(tgt_b);
  const char* const bas_c = reinterpret_cast<const char*>(bas_b);
  const char* const arec_c = reinterpret_cast<const char*>(a.arec + (size_t)b * N * 8);
  const char* const dep_c = reinterpret_cast<const char*>(lv.depth + (size_t)b * N);
  const char* const z2_c = reinterpret_cast<const char*>(a.z2 + (size_t)b * N * K);
  char* const dsrc_c = reinterpret_cast<char*>(a.dsrc + (size_t)b * N * C);
  char* const dbas_c = reinterpret_cast<char*>(a.dbasis + (size_t)b * N * K);
  char* const ddep_c = reinterpret_cast<char*>(a.ddepth + (size_t)b * N);
  char* const frac_c = reinterpret_cast<char*>(a.frac + (size_t)b * N * kFrac);
  char* const cnt_c = reinterpret_cast<char*>(a.cnt + (size_t)b * H * W);
  char* const arow_c = a.arow ? reinterpret_cast<char*>(a.arow + (size_t)b * N * 3 * C) : nullptr;
  const unsigned rowC = (unsigned)C * 4u, rowK = (unsigned)K * 4u;
  // (pixel index x row bytes with the full-rate 24-bit multiply: N < 2^24 and the product < 2^32 are launch conditions; the 32-bit
  // v_mul_lo / v_mad_u64 the compiler takes otherwise run at a quarter of the rate, 26 of them per pixel pair)
  auto offC = [&](unsigned pix, unsigned add) { return __umul24(pix, rowC) + add; };
  auto offK = [&](unsigned pix, unsigned add) { return __umul24(pix, rowK) + add; };
  const float* __restrict__ S = a.S + (size_t)b * P * P;
  const float* __restrict__ gb = a.gb + (size_t)b * P;
  float Scc[6][6], gbc[6], Rm[9], Tv[3];      // S is symmetric (adj_sym_kernel): 21 distinct uniform values, not 36 -- the scalar registers are short
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    gbc[i] = gb[i];
#pragma unroll
    for (int j = i; j < 6; ++j) Scc[i][j] = Scc[j][i] = S[i * P + j];
  }
#pragma unroll
  for (int i = 0; i < 9; ++i) Rm[i] = a.R[b * 9 + i];
#pragma unroll
  for (int i = 0; i < 3; ++i) Tv[i] = a.T[b * 3 + i];
  const float fx0 = lv.intr[b * 4 + 0], fy0 = lv.intr[b * 4 + 1], ox0 = lv.intr[b * 4 + 2], oy0 = lv.intr[b * 4 + 3];
  const float fx = fx0 / lv.scale, fy = fy0 / lv.scale, ox = ox0 / lv.scale, oy = oy0 / lv.scale;
  // this lane's 4 depth coefficients (k = 4 hl .. 4 hl + 3) and channel quads (c = 4 hl + 128 j)
  const int k0 = 4 * hl;
  const bool kok = k0 < K;
  f32x4 wc = {0.f, 0.f, 0.f, 0.f}, gbd = {0.f, 0.f, 0.f, 0.f}, dwc = {0.f, 0.f, 0.f, 0.f};
  f32x4 scd[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) scd[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (kok) {
    wc = *reinterpret_cast<const f32x4*>(a.Wc + (size_t)b * K + k0);
#pragma unroll
    for (int e = 0; e < 4; ++e) gbd[e] = gb[6 + k0 + e];
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) scd[i][e] = S[i * P + 6 + k0 + e];
  }
  bool cok[CJ4];
  unsigned chb[CJ4];      // this lane's channel quad of chunk j as a byte offset into a row (clamped: a lane without channels reads quad 0)
  f32x4 ga[CJ4];
#pragma unroll
  for (int j = 0; j < CJ4; ++j) {
    const int c = 4 * hl + 128 * j;
    cok[j] = c < C;
    chb[j] = cok[j] ? (unsigned)c * 4u : 0u;
    ga[j] = cok[j] ? *reinterpret_cast<const f32x4*>(a.gabs + (size_t)b * C + c) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
  float accR[9], accT[3];
#pragma unroll
  for (int i = 0; i < 9; ++i) accR[i] = 0.f;
#pragma unroll
  for (int i = 0; i < 3; ++i) accT[i] = 0.f;

  const int nw = a.G * kNumWaves, chunk = ((N + nw - 1) / nw + 1) & ~1;   // even: the pairs of a wave never straddle two waves
  const int n_lo = (g * kNumWaves + w) * chunk, n_hi = min(N, n_lo + chunk);
  // Software pipeline (round 6; by ablation the kernel was bound by two exposed memory round trips per pixel pair, not by its
  // bytes): the rows a pair's geometry needs -- basis, depth, the (q, zeta, e) record -- are requested one pair ahead; the 12 target
  // texel loads go out as soon as the projection is known and the part of the per-pixel algebra that does not depend on the texels
  // (Jacobians, J S_cc + jd q^T, t, dM, dg) runs while they travel.
  auto pix_of = [&](int n2) { const int n = n2 + hi; return n < n_hi ? n : n_hi - 1; };     // a dead upper half recomputes the lower pixel
  const int kc = kok ? k0 : 0;      // loads are unconditional at clamped offsets (a conditional load is merged with its default by
                                    // copies that wait for it on the spot); what a lane without coefficients / channels reads is masked where it is used
  f32x4 bv_n, ar0_n, ar1_n;
  float dep_n;
  const unsigned kcb = (unsigned)kc * 4u;
  {
    const unsigned q0 = (unsigned)pix_of(n_lo < n_hi ? n_lo : 0);
    bv_n = *reinterpret_cast<const f32x4*>(bas_c + offK(q0, kcb));
    ar0_n = *reinterpret_cast<const f32x4*>(arec_c + q0 * 32u);
    ar1_n = *reinterpret_cast<const f32x4*>(arec_c + (q0 * 32u + 16u));
    dep_n = *reinterpret_cast<const float*>(dep_c + q0 * 4u);
  }
  int by = n_lo / W, bx = n_lo - by * W;               // (column, row) of the pair's first pixel, stepped along with n2 (uniform)
  for (int n2 = n_lo; n2 < n_hi; n2 += 2) {
    const int n = n2 + hi;
    const bool live = n < n_hi;
    const int nn = live ? n : n_hi - 1;                 // a dead upper half recomputes the lower pixel (n_hi - 1 = n2: chunks are even) and stores nothing
    int qx = bx + (live ? hi : 0), qy = by;
    if (qx >= W) {
      qx = 0;
      ++qy;
    }
    float p0 = ((float)qx * lv.scale - ox0) / fx0, p1 = ((float)qy * lv.scale - oy0) / fy0, p2 = 1.f;
    if (lv.normalize_rays) {
      const float inv = 1.f / sqrtf(fmaxf(p0 * p0 + p1 * p1 + p2 * p2, 1e-12f));
      p0 *= inv;
      p1 *= inv;
      p2 *= inv;
    }
    const unsigned qn0 = (unsigned)nn;
    const f32x4 bv = bv_n, ar0 = ar0_n, ar1 = ar1_n;
    const float qv[6] = {ar0[0], ar0[1], ar0[2], ar0[3], ar1[0], ar1[1]};
    const float zeta = ar1[2], ee = ar1[3];
    const float D = dep_n + hsum(bv[0] * wc[0] + bv[1] * wc[1] + bv[2] * wc[2] + bv[3] * wc[3]);
    const float rx = Rm[0] * p0 + Rm[1] * p1 + Rm[2] * p2;
    const float ry = Rm[3] * p0 + Rm[4] * p1 + Rm[5] * p2;
    const float rz = Rm[6] * p0 + Rm[7] * p1 + Rm[8] * p2;
    const float X = rx * D + Tv[0], Y = ry * D + Tv[1], Z0 = rz * D + Tv[2];
    float x = X / Z0, y = Y / Z0, Z = Z0;
    float px = fx * x + ox, py = fy * y + oy;
    const bool m = live && (px >= 0.f) && (px <= (float)(W - 1)) && (py >= 0.f) && (py <= (float)(H - 1));
    if (!m) {            // safe stand-ins: everything below stays finite, nothing of it is stored
      x = 0.f;
      y = 0.f;
      Z = 1.f;
      px = 1.5f;
      py = 1.5f;
    }
    const float xf = floorf(px), yf = floorf(py);
    const int x0 = (int)xf, y0 = (int)yf;
    const float ax = px - xf, ay = py - yf;
    // ---- the 4x4 neighbourhood (minus corners), clamped: 12 row loads of 16 bytes per lane and channel chunk
    f32x4 tex[CJ4][4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int cc = 0; cc < 4; ++cc) {
        if ((r == 0 || r == 3) && (cc == 0 || cc == 3)) continue;
        const int yy = min(max(y0 - 1 + r, 0), H - 1), xx = min(max(x0 - 1 + cc, 0), W - 1);
        const unsigned row = offC((unsigned)(__mul24(yy, W) + xx), 0u);
#pragma unroll
        for (int j = 0; j < CJ4; ++j) tex[j][r][cc] = *reinterpret_cast<const f32x4*>(tgt_c + (row + chb[j]));
      }
    // this pair's source row and z2 row (needed after the taps / at the very end), the next pair's geometry rows
    const f32x4 z2v = *reinterpret_cast<const f32x4*>(z2_c + offK(qn0, kcb));
    f32x4 f1v[CJ4];
#pragma unroll
    for (int j = 0; j < CJ4; ++j) f1v[j] = *reinterpret_cast<const f32x4*>(src_c + offC(qn0, chb[j]));
    f32x4 ds_old[CJ4], db_old;      // accumulate mode: the old contents travel with the texels
    float dd_old = 0.f;
    if constexpr (!OW) {
#pragma unroll
      for (int j = 0; j < CJ4; ++j) ds_old[j] = *reinterpret_cast<const f32x4*>(dsrc_c + offC(qn0, chb[j]));
      db_old = *reinterpret_cast<const f32x4*>(dbas_c + offK(qn0, kcb));
      dd_old = *reinterpret_cast<const float*>(ddep_c + qn0 * 4u);
    }
    {
      const unsigned nx = (unsigned)pix_of(n2 + 2 < n_hi ? n2 + 2 : n2);      // (the last pair requests itself again: no branch around the loads)
      bv_n = *reinterpret_cast<const f32x4*>(bas_c + offK(nx, kcb));
      ar0_n = *reinterpret_cast<const f32x4*>(arec_c + nx * 32u);
      ar1_n = *reinterpret_cast<const f32x4*>(arec_c + (nx * 32u + 16u));
      dep_n = *reinterpret_cast<const float*>(dep_c + nx * 4u);
    }
    // ---- per-pixel algebra, the part without M and g (as adj_pixel_kernel), under the texel loads
    // (written on PAIRS (row 0, row 1) of the 2 x 6 Jacobian: one packed operation per pair, element by element the same chain of
    // fused multiply-adds as adj_pixel_kernel -- left to itself the compiler packs across the column index instead and spends
    // ~130 register copies per pixel pair on building its operands)
    const float iz = 1.f / Z;
    const f32x2 fxy = {fx, fy};
    f32x2 Jp[6];
    Jp[0] = fxy * f32x2{-(x * y), -1.f - y * y};
    Jp[1] = fxy * f32x2{1.f + x * x, x * y};
    Jp[2] = fxy * f32x2{-y, x};
    Jp[3] = f32x2{fx * iz, 0.f};
    Jp[4] = f32x2{0.f, fy * iz};
    Jp[5] = fxy * f32x2{-(x * iz), -(y * iz)};
    const f32x2 jdp = fxy * f32x2{(rx - rz * x) * iz, (ry - rz * y) * iz};
    const float jd0 = jdp[0], jd1 = jdp[1];
    f32x2 JSp[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      f32x2 sp = jdp * qv[j];
#pragma unroll
      for (int i = 0; i < 6; ++i) sp = fma2(Jp[i], splat2(Scc[i][j]), sp);
      JSp[j] = sp;
    }
    f32x2 tp = jdp * zeta, dgp = jdp * ee, dMd = {0.f, 0.f};
    float dM12 = 0.f;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      tp = fma2(Jp[i], splat2(qv[i]), tp);
      dMd = fma2(JSp[i], Jp[i], dMd);
      dM12 = fmaf(JSp[i][0], Jp[i][1], dM12);
      dgp = fma2(Jp[i], splat2(gbc[i]), dgp);
    }
    dMd = fma2(tp, jdp, dMd);
    dM12 = fmaf(tp[0], jd1, dM12);
    const float t0 = tp[0], t1 = tp[1], dg1 = dgp[0], dg2 = dgp[1], dM11 = dMd[0], dM22 = dMd[1];
    asm volatile("" ::: "memory");      // (keeps the block above ahead of the first use of a texel)
    f32x4 Sf[CJ4], Sgx[CJ4], Sgy[CJ4], Ax[CJ4][3], Ay[CJ4][3];
#pragma unroll
    for (int j = 0; j < CJ4; ++j) {
      Sf[j] = Sgx[j] = Sgy[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int e = 0; e < 3; ++e) Ax[j][e] = Ay[j][e] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    // the four taps.  `inner` (every footprint of the wave off the image rim: nearly always) knows fin = 1, hx = hy = 0.5 at compile
    // time -- ~75 instructions less per pair; same values, and explicit fused multiply-adds so that the two paths (and the two
    // instantiations of this kernel) round alike
    auto taps = [&](auto innerc) __attribute__((always_inline)) {
      constexpr bool IN = decltype(innerc)::value;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int ix = t & 1, iy = t >> 1;
        const int tx = x0 + ix, ty = y0 + iy;
        const bool in = IN || (tx <= W - 1 && ty <= H - 1);
        const float hx = (IN || (in && tx > 0 && tx < W - 1)) ? 0.5f : 0.f, hy = (IN || (in && ty > 0 && ty < H - 1)) ? 0.5f : 0.f;
        const float wx = ix ? ax : 1.f - ax, wy = iy ? ay : 1.f - ay;
        const float wt = wx * wy, sx = (ix ? 1.f : -1.f) * wy, sy = (iy ? 1.f : -1.f) * wx;
        const f32x4 wt4 = {wt, wt, wt, wt}, sx4 = {sx, sx, sx, sx}, sy4 = {sy, sy, sy, sy};
#pragma unroll
        for (int j = 0; j < CJ4; ++j) {
          f32x4 F = tex[j][1 + iy][1 + ix];
          if (!IN && !in) F = f32x4{0.f, 0.f, 0.f, 0.f};
          const f32x4 GX = hx * (tex[j][1 + iy][2 + ix] - tex[j][1 + iy][ix]);
          const f32x4 GY = hy * (tex[j][2 + iy][1 + ix] - tex[j][iy][1 + ix]);
          Sf[j] = fma4(wt4, F, Sf[j]);
          Sgx[j] = fma4(wt4, GX, Sgx[j]);
          Sgy[j] = fma4(wt4, GY, Sgy[j]);
          Ax[j][0] = fma4(sx4, F, Ax[j][0]);
          Ax[j][1] = fma4(sx4, GX, Ax[j][1]);
          Ax[j][2] = fma4(sx4, GY, Ax[j][2]);
          Ay[j][0] = fma4(sy4, F, Ay[j][0]);
          Ay[j][1] = fma4(sy4, GX, Ay[j][1]);
          Ay[j][2] = fma4(sy4, GY, Ay[j][2]);
        }
      }
    };
    if (__builtin_expect(__all(x0 >= 1 && y0 >= 1 && x0 + 2 <= W - 1 && y0 + 2 <= H - 1) != 0, 1)) {
      taps(std::true_type{});
    } else {
      asm volatile("" ::: "memory");
      taps(std::false_type{});
      asm volatile("" ::: "memory");
    }
    f32x4 dif[CJ4];
    float M11 = 0.f, M12 = 0.f, M22 = 0.f, g1 = 0.f, g2 = 0.f;
#pragma unroll
    for (int j = 0; j < CJ4; ++j) {
      if (!cok[j]) Sf[j] = Sgx[j] = Sgy[j] = f1v[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      dif[j] = f1v[j] - Sf[j];       // bundlenet.py:234
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        M11 = fmaf(Sgx[j][e], Sgx[j][e], M11);
        M12 = fmaf(Sgx[j][e], Sgy[j][e], M12);
        M22 = fmaf(Sgy[j][e], Sgy[j][e], M22);
        g1 = fmaf(Sgx[j][e], dif[j][e], g1);
        g2 = fmaf(Sgy[j][e], dif[j][e], g2);
      }
    }
    M11 = hsum(M11);
    M12 = hsum(M12);
    M22 = hsum(M22);
    g1 = hsum(g1);
    g2 = hsum(g2);
    // ---- per-pixel algebra, the part with M and g
    f32x2 dJp[6];
    float u[6];
    const f32x2 Mr0 = {M11, M12}, Mr1 = {M12, M22}, gp = {g1, g2};
    const float Mjd0 = fmaf(M11, jd0, M12 * jd1), Mjd1 = fmaf(M12, jd0, M22 * jd1);
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      dJp[i] = fma2(splat2(2.f), fma2(Mr0, splat2(JSp[i][0]), Mr1 * JSp[i][1]), gp * gbc[i]);
      u[i] = fmaf(Jp[i][0], Mjd0, Jp[i][1] * Mjd1);
    }
    const f32x2 djdp = fma2(splat2(2.f), fma2(Mr0, splat2(t0), Mr1 * t1), gp * ee);
    const float djd0 = djdp[0], djd1 = djdp[1];
    const float s_n = fmaf(jd0, Mjd0, jd1 * Mjd1), r_n = fmaf(jd0, g1, jd1 * g2);
    float dJ0[6], dJ1[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      dJ0[i] = dJp[i][0];
      dJ1[i] = dJp[i][1];
    }
    // ---- channel adjoints
    float dpx = 0.f, dpy = 0.f;
    const unsigned dsrc_o = offC(qn0, (unsigned)hl * 16u), arow_o = 3u * offC(qn0, 0u) + (unsigned)hl * 16u;     // (base + 32-bit offset at every store)
#pragma unroll
    for (int j = 0; j < CJ4; ++j) {
      if (cok[j]) {
        f32x4 dd, dgx, dgy;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float d = dif[j][e], gx = Sgx[j][e], gy = Sgy[j][e];
          const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
          // (explicit fused operations: the two instantiations of this kernel -- write / accumulate -- must round alike, and the
          // compiler's own contraction of a * b + c * d + e * f is free to differ between them)
          dd[e] = fmaf(sgn, ga[j][e], fmaf(dg2, gy, dg1 * gx));
          dgx[e] = fmaf(dg1, d, 2.f * fmaf(dM12, gy, dM11 * gx));
          dgy[e] = fmaf(dg2, d, 2.f * fmaf(dM22, gy, dM12 * gx));
          dpx += -dd[e] * Ax[j][0][e] + dgx[e] * Ax[j][1][e] + dgy[e] * Ax[j][2][e];
          dpy += -dd[e] * Ay[j][0][e] + dgx[e] * Ay[j][1][e] + dgy[e] * Ay[j][2][e];
        }
        if (OW && live && !m) *reinterpret_cast<f32x4*>(dsrc_c + (dsrc_o + 512u * j)) = f32x4{0.f, 0.f, 0.f, 0.f};
        if (m) {
          f32x4* ds = reinterpret_cast<f32x4*>(dsrc_c + (dsrc_o + 512u * j));
          if constexpr (OW)
            *ds = dd;
          else
            *ds = ds_old[j] + dd;
          if (arow_c) {
            *reinterpret_cast<f32x4*>(arow_c + (arow_o + 512u * j)) = -dd;
            *reinterpret_cast<f32x4*>(arow_c + (arow_o + rowC + 512u * j)) = dgx;
            *reinterpret_cast<f32x4*>(arow_c + (arow_o + 2u * rowC + 512u * j)) = dgy;
          }
        }
      }
    }
    dpx = hsum(dpx);
    dpy = hsum(dpy);
    // ---- geometry adjoint
    float dx_ = fx * dpx + fx * (-y * dJ0[0] + 2.f * x * dJ0[1] - dJ0[5] * iz) + fy * (y * dJ1[1] + dJ1[2]);
    float dy_ = fy * dpy + fx * (-x * dJ0[0] - dJ0[2]) + fy * (-2.f * y * dJ1[0] + x * dJ1[1] - dJ1[5] * iz);
    float dZ_ = (fx * (-dJ0[3] + x * dJ0[5]) + fy * (-dJ1[4] + y * dJ1[5])) * iz * iz;
    float drx = fx * djd0 * iz, dry = fy * djd1 * iz, drz = -(fx * x * djd0 + fy * y * djd1) * iz;
    dx_ -= fx * rz * djd0 * iz;
    dy_ -= fy * rz * djd1 * iz;
    dZ_ -= (jd0 * djd0 + jd1 * djd1) * iz;
    const float ms = m ? 1.f : 0.f;
    const float dX = ms * dx_ * iz, dY = ms * dy_ * iz, dZt = ms * (dZ_ - (x * dx_ + y * dy_) * iz);
    drx = fmaf(dX, D, ms * drx);
    dry = fmaf(dY, D, ms * dry);
    drz = fmaf(dZt, D, ms * drz);
    const float dD = dX * rx + dY * ry + dZt * rz;
    accT[0] += dX;
    accT[1] += dY;
    accT[2] += dZt;
    accR[0] = fmaf(drx, p0, accR[0]);
    accR[1] = fmaf(drx, p1, accR[1]);
    accR[2] = fmaf(drx, p2, accR[2]);
    accR[3] = fmaf(dry, p0, accR[3]);
    accR[4] = fmaf(dry, p1, accR[4]);
    accR[5] = fmaf(dry, p2, accR[5]);
    accR[6] = fmaf(drz, p0, accR[6]);
    accR[7] = fmaf(drz, p1, accR[7]);
    accR[8] = fmaf(drz, p2, accR[8]);
    // ---- depth, basis, coefficients
    if (m && kok) {
      f32x4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float su = 0.f;
#pragma unroll
        for (int i = 0; i < 6; ++i) su = fmaf(u[i], scd[i][e], su);
        v[e] = fmaf(2.f, su, fmaf(dD, wc[e], fmaf(r_n, gbd[e], s_n * z2v[e])));
        dwc[e] = fmaf(dD, bv[e], dwc[e]);
      }
      f32x4* db = reinterpret_cast<f32x4*>(dbas_c + offK(qn0, kcb));
      if constexpr (OW)
        *db = v;
      else
        *db = db_old + v;
    } else if (OW && live && kok) {
      *reinterpret_cast<f32x4*>(dbas_c + offK(qn0, kcb)) = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (hl == 0 && live) {
      const unsigned fro = qn0 * (unsigned)(kFrac * 4), ddo = qn0 * 4u;
      if (OW && !m) *reinterpret_cast<float*>(ddep_c + ddo) = 0.f;
      if (m) {
        *reinterpret_cast<float*>(ddep_c + ddo) = OW ? dD : dd_old + dD;
        const int key = y0 * W + x0;
        *reinterpret_cast<f32x4*>(frac_c + fro) = f32x4{__int_as_float(key), ax, ay, dg1};
        *reinterpret_cast<f32x4*>(frac_c + (fro + 16u)) = f32x4{dg2, dM11, dM12, dM22};
        atomicAdd(reinterpret_cast<int*>(cnt_c + (unsigned)key * 4u), 1);
      } else {
        *reinterpret_cast<float*>(frac_c + fro) = __int_as_float(-1);
      }
    }
    bx += 2;
    while (bx >= W) {
      bx -= W;
      ++by;
    }
  }
  // the wave's partial row: lower half + upper half, fixed order
  float* __restrict__ prow = a.part + ((size_t)b * a.G * kNumWaves + g * kNumWaves + w) * (kAdjHdr + K);
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    const float v = bfly_merge(accR[i], accR[i], 32);
    if (lane == i) prow[i] = v;
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float v = bfly_merge(accT[i], accT[i], 32);
    if (lane == 9 + i) prow[9 + i] = v;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float v = bfly_merge(dwc[e], dwc[e], 32);
    if (hi == 0 && kok) prow[kAdjHdr + k0 + e] = v;
  }
}

__global__ void adj_fold_kernel(const float* __restrict__ part, int rows, int K, float* __restrict__ dpose) {
  const int b = blockIdx.y, e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= 12 + K) return;
  const int off = e < 12 ? e : kAdjHdr + (e - 12);
  const float* p = part + (size_t)b * rows * (kAdjHdr + K) + off;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  int i = 0;
  for (; i + 3 < rows; i += 4) {
    s0 += p[(size_t)(i + 0) * (kAdjHdr + K)];
    s1 += p[(size_t)(i + 1) * (kAdjHdr + K)];
    s2 += p[(size_t)(i + 2) * (kAdjHdr + K)];
    s3 += p[(size_t)(i + 3) * (kAdjHdr + K)];
  }
  for (; i < rows; ++i) s0 += p[(size_t)i * (kAdjHdr + K)];
  dpose[(size_t)b * (12 + K) + e] = (s0 + s1) + (s2 + s3);
}

}  // namespace

// (assert: a plan that returned BANET_OK names an instantiation of the lists below -- plan_detail::choose_adj_pixel looked it up
//  in the same lists -- so BANET_ERR_UNSUPPORTED cannot be returned for it)
int launch_adj_pixel(const AdjArgs& a, const AdjPlan& pl, hipStream_t s) {
  const dim3 grid(pl.G, a.lv.B), block(kBlock);
  switch (pl.pixel) {
    case kAdjPixelPoint:
      switch (pl.pixel_cj * 8 + pl.pixel_kj) {
#define BANET_X(cj, kj) \
  case cj * 8 + kj: hipLaunchKernelGGL((adj_pixel_kernel<cj, kj, true>), grid, block, 0, s, a); return BANET_OK;
        BANET_ADJ_POINT_LIST(BANET_X)
#undef BANET_X
      }
      break;
    case kAdjPixelOne:
      switch (pl.pixel_cj * 8 + pl.pixel_kj) {
#define BANET_X(cj, kj) \
  case cj * 8 + kj: hipLaunchKernelGGL((adj_pixel_kernel<cj, kj>), grid, block, 0, s, a); return BANET_OK;
        BANET_ADJ_PIXEL_LIST(BANET_X)
#undef BANET_X
      }
      break;
    case kAdjPixelTwo:
      switch (pl.pixel_cj * 8 + pl.pixel_ow) {
#define BANET_X(cj4, ow) \
  case cj4 * 8 + (ow ? 1 : 0): hipLaunchKernelGGL((adj_pixel2_kernel<cj4, ow>), grid, block, 0, s, a); return BANET_OK;
        BANET_ADJ_PIXEL2_LIST(BANET_X)
#undef BANET_X
      }
      break;
  }
  return BANET_ERR_UNSUPPORTED;
}

void launch_adj_fold(const float* part, int rows, int B, int K, float* dpose, hipStream_t s) {
  hipLaunchKernelGGL(adj_fold_kernel, dim3((12 + K + 127) / 128, B), dim3(128), 0, s, part, rows, K, dpose);
}

}  // namespace adj
}  // namespace banet
