// ba_residual_grad_kernel / ba_residual_grad_fold_kernel -- banet_ba_residual_grad_f32: the backward of banet_ba_residual_f32.
//
// L = sum_{b,f,n} gsq sq + gab ab + gproj . proj with sq = sum_c d^2, ab = sum_c |d|, d_c = F2w_c - F1_c, the forward's mask and the
// forward's floor held fixed (the one-sided derivative at an integer coordinate, as banet_resample_grad_f32).  Per window b, target
// frame f and point n, in this order:
//   1. D = D0 + Bs.W, the ray, the projection, the mask and the four taps: the float32 statements of ba_residual_kernel
//      (residual.hip) -- strip_geometry's (quad_common.hpp) on a dense level, gather_generic.hip's on sparse points -- restated here
//      because the backward needs their intermediates (ray, R p, X / Z, Z);
//   2. e_c = mask (2 gsq d_c + gab sgn d_c),  sgn 0 = 0;
//   3. (dpx, dpy) = sum_c e_c dF2w_c / d(px, py) + mask gproj,  dF2w/dpx = (I01 - I00)(1 - dy) + (I11 - I10) dy, dF2w/dpy alike;
//   4. geometry backward: px = fx X/Z + ox, py = fy Y/Z + oy, (X, Y, Z) = (R p) D + T:
//        gX = fx dpx / Z, gY = fy dpy / Z, gZ = -(fx dpx x + fy dpy y) / Z, dT_f += (gX, gY, gZ), dR_f[i][j] += g_i D p_j,
//        dD_n += gX rx + gY ry + gZ rz = (fx dpx (rx Tz - rz Tx) + fy dpy (ry Tz - rz Ty)) / Z^2   (rays and intrinsics get no gradient).
// Per point: dsrc = -sum_f e (the row stays in registers over the frames), ddepth = dD, dbasis = dD Wc.  A point outside the image (or
// with a NaN projection) reads no tap and contributes exact zeros everywhere; gproj is ignored there.
//
// Lanes: the forward's -- 16 per point, four points per wave instruction (one such step in flight per wave: the double chain below
// takes the registers of the forward's second step); C = 128 /
// K = 128 as two 16-byte pieces per lane, any other C, K <= 256 with lanes striding over the channels / coefficients, 16 apart.
// Channel sums: row16_sum's order (DPP inside the 16-lane row), on doubles.
//
// Precision: the forward's float32 statements fix WHERE the derivative is taken (mask, floor, dx, dy).  From there on -- the sample, d,
// e, the channel sums, the geometry backward, the pose slots, dD and the fold -- the arithmetic is double: d is a difference of nearly
// equal features and the sums over channels and points cancel again, so float32 there lost 20 x what the float32 projection itself
// costs (bundle_camera 5x7: dT 1.2e-5 of its largest entry against 5e-7).  e, dD and the partial rows are rounded to float32 once.
//
// Sums over points (dWc, and 12 pose numbers per frame): no atomics.  A workgroup owns kRgWgUnits x 4 = 512 CONSECUTIVE points (a constant), its
// wave w the 4-point units w, w + 4, ... of them in sequence:
//   pose  -- lane l < 12 of a point's row owns number l (dR 0..8, dT 9..11) and adds the row's point of the unit to ITS slot
//            [wave][row][frame][l] (a double; LDS; in the workspace for windows of more than kResGradLdsFrames frames): a plain read-modify-write
//            by the one lane that owns the address.  After a barrier the 16 slots are added in slot order;
//   dWc   -- per-lane registers (a lane's 8 or 16 coefficients) over the wave's points, then rows 0..3 by two shuffles, then waves
//            0..3 through LDS in wave order.
// One partial row [12 pairs + K] per workgroup goes to the workspace; the fold launch adds a window's rows in ascending order.  So
// every summation order depends on N and pairs alone, never on B or the grid: a window's bits are the same alone and in any batch.
//
// dtgt: the kernel stores the e rows [B pairs][N][C] and the projections [B pairs][N][2] ((0, 0) and a zero row for a masked point)
// in the workspace; prep_grad.hip's resampler gradient (clamp mode, batch = B pairs) sums them per texel in ascending (point, tap)
// order.  Its footprint recomputes floor / fractions / weights from the stored projection px = x0 + dx with the forward's own
// expressions and clamps the +1 taps as the forward does, so the weights are the forward's bits.
#include "kernels.hpp"

namespace banet {

namespace {

constexpr int kRgStepPts = 4;                    // points per wave instruction (16 lanes each)
constexpr int kRgSteps = 1;                      // steps in flight per wave (the double chain needs the registers of a second one)
constexpr int kRgUnitPts = kRgStepPts * kRgSteps;
constexpr int kRgWgUnits = 128;                  // 4-point units per workgroup (512 points): 32 per wave
constexpr int kRgChunks = 16;                    // plain path: channels / coefficients l, l + 16, ... (<= 256)
constexpr int kRgSlots = kNumWaves * kRgStepPts; // pose accumulators per workgroup: one per (wave, row)
constexpr int kRgPoseLds = 16;                   // target frames whose pose is staged in LDS (more: read from memory per frame)

struct ResGradArgs {
  banet_level_t lv;
  const float* R;
  const float* T;
  const float* Wc;
  const float* gsq;      // [B][pairs][N] or nullptr (zeros)
  const float* gab;      // [B][pairs][N] or nullptr
  const float* gproj;    // [B][pairs][N][2] or nullptr
  float* dsrc;           // [B][N][C] or nullptr
  float* ddepth;         // [B][N] or nullptr
  float* dbasis;         // [B][N][K] or nullptr
  float* part;           // workspace: [B][G][cols] partial rows (pose numbers of every frame, then dWc)
  double* slots;         // workspace: [B][G][kRgSlots][pairs][12] doubles when the pose slots do not fit the LDS, else nullptr
  float* erow;           // workspace: [B pairs][N][C] or nullptr (no dtgt)
  float* eproj;          // workspace: [B pairs][N][2] or nullptr
  int pairs, units, G, cols, overwrite, want_dwc;
};

struct RgRay {
  float p0, p1, p2, fx, fy, ox, oy;
  float pj;   // component cj of the ray (the lane's column of dR)
};
struct RgGeo {
  float dx, dy, rx, ry, rz, x, y, Z;
  int x0, y0;
  bool m;
};

// the ray and the level intrinsics of a dense level's pixel: strip_geometry's statements (quad_common.hpp)
__device__ __forceinline__ RgRay dense_ray(const banet_level_t& lv, float fx0, float fy0, float ox0, float oy0, bool valid, int px, int py, int cj) {
  RgRay r;
  float p0 = 0.f, p1 = 0.f, p2 = 1.f, fx = 1.f, fy = 1.f, ox = 0.f, oy = 0.f;
  if (valid) {
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
  r.p0 = p0, r.p1 = p1, r.p2 = p2, r.fx = fx, r.fy = fy, r.ox = ox, r.oy = oy;
  r.pj = cj == 0 ? p0 : cj == 1 ? p1 : p2;
  return r;
}

// sparse points: the loads of ba_gather_kernel's geometry phase (gather_generic.hip)
__device__ __forceinline__ RgRay sparse_ray(const banet_level_t& lv, int b, bool valid, int pt, int cj) {
  const int N = lv.N;
  RgRay r;
  float p0 = 0.f, p1 = 0.f, p2 = 1.f;
  r.fx = 1.f, r.fy = 1.f, r.ox = 0.f, r.oy = 0.f;
  if (valid) {
    const size_t o = (size_t)b * 3 * N;
    p0 = lv.rays[o + pt];
    p1 = lv.rays[o + N + pt];
    p2 = lv.rays[o + 2 * (size_t)N + pt];
    const size_t q = (size_t)b * N + pt;
    r.fx = lv.fx[q];
    r.fy = lv.fy[q];
    r.ox = lv.ox[q];
    r.oy = lv.oy[q];
  }
  r.p0 = p0, r.p1 = p1, r.p2 = p2;
  r.pj = cj == 0 ? p0 : cj == 1 ? p1 : p2;
  return r;
}

// the same ray and intrinsics in double, from the same float32 inputs (what the derivative is evaluated with; the float32 ones above
// decide the mask and the floor)
struct RgRayD {
  double p0, p1, p2, fx, fy, ox, oy, pj;
};
__device__ __forceinline__ RgRayD dense_ray_d(const banet_level_t& lv, float fx0, float fy0, float ox0, float oy0, bool valid, int px, int py,
                                              int cj) {
  RgRayD r;
  double p0 = 0.0, p1 = 0.0, p2 = 1.0, fx = 1.0, fy = 1.0, ox = 0.0, oy = 0.0;
  if (valid) {
    const double sc = (double)lv.scale;
    p0 = ((double)px * sc - (double)ox0) / (double)fx0;
    p1 = ((double)py * sc - (double)oy0) / (double)fy0;
    if (lv.normalize_rays) {
      const double inv = 1.0 / sqrt(fmax(p0 * p0 + p1 * p1 + 1.0, 1e-12));
      p0 *= inv;
      p1 *= inv;
      p2 = inv;
    }
    fx = (double)fx0 / sc;
    fy = (double)fy0 / sc;
    ox = (double)ox0 / sc;
    oy = (double)oy0 / sc;
  }
  r.p0 = p0, r.p1 = p1, r.p2 = p2, r.fx = fx, r.fy = fy, r.ox = ox, r.oy = oy;
  r.pj = cj == 0 ? p0 : cj == 1 ? p1 : p2;
  return r;
}
__device__ __forceinline__ RgRayD widen_ray(const RgRay& f) {   // sparse points: the rays and intrinsics are inputs
  RgRayD r;
  r.p0 = f.p0, r.p1 = f.p1, r.p2 = f.p2, r.fx = f.fx, r.fy = f.fy, r.ox = f.ox, r.oy = f.oy, r.pj = f.pj;
  return r;
}

// projection, mask, floor and fractions: the statements both geometry functions of the forward share
__device__ __forceinline__ RgGeo project(const RgRay& r, const float (&Rm)[9], const float (&Tv)[3], bool valid, float D, int W, int H) {
  RgGeo g;
  const float p0 = r.p0, p1 = r.p1, p2 = r.p2;
  const float rx = Rm[0] * p0 + Rm[1] * p1 + Rm[2] * p2;
  const float ry = Rm[3] * p0 + Rm[4] * p1 + Rm[5] * p2;
  const float rz = Rm[6] * p0 + Rm[7] * p1 + Rm[8] * p2;
  const float X = rx * D + Tv[0], Y = ry * D + Tv[1], Z = rz * D + Tv[2];
  const float x = X / Z, y = Y / Z;
  const float pxl = r.fx * x + r.ox, pyl = r.fy * y + r.oy;
  g.m = valid && (pxl >= 0.f) && (pxl <= (float)(W - 1)) && (pyl >= 0.f) && (pyl <= (float)(H - 1));
  g.dx = g.dy = 0.f;
  g.x0 = g.y0 = 0;
  if (g.m) {
    const float xf = floorf(pxl), yf = floorf(pyl);
    g.dx = pxl - xf;
    g.dy = pyl - yf;
    g.x0 = (int)xf;
    g.y0 = (int)yf;
  }
  g.rx = rx, g.ry = ry, g.rz = rz, g.x = x, g.y = y, g.Z = Z;
  return g;
}

__device__ __forceinline__ float4 ld16_stream(const float* p) {   // a row piece that is read exactly once: non-temporal
  const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
  return make_float4(v.x, v.y, v.z, v.w);
}

__device__ __forceinline__ double sgn0(double d) { return d > 0.0 ? 1.0 : d < 0.0 ? -1.0 : 0.0; }

// sum over the 16 lanes of a DPP row in double (row16_sum's order, the two halves of the value moved separately)
template <int CTRL>
__device__ __forceinline__ double dpp_mov_d(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double row16_sum_d(double v) {
  v += dpp_mov_d<kDppRor8>(v);
  v += dpp_mov_d<kDppHalfMirror>(v);
  v += dpp_mov_d<kDppXor2>(v);
  v += dpp_mov_d<kDppXor1>(v);
  return v;
}

// one channel: the sample, d, e (m: the point is in the image), the two projection-gradient terms and the running -sum e.
// Everything after the forward's float32 (dx, dy) is DOUBLE: d = F2w - F1 is a difference of nearly equal features near a solution and
// the sums over channels and points cancel again, so float32 arithmetic here cost 20 x the error the float32 projection itself causes
// (measured); the kernel is bound by memory, not by these operations.  e is rounded to float32 once, for dsrc and the e rows.
__device__ __forceinline__ float chan(float i00, float i01, float i10, float i11, float f1, double ex, double ey, double g2, double ga, bool m,
                                      double& spx, double& spy, float& acc) {
  const double ux = 1.0 - ex, uy = 1.0 - ey;
  const double f = (((double)i00 * (ux * uy) + (double)i01 * (ex * uy)) + (double)i10 * (ux * ey)) + (double)i11 * (ex * ey);
  const double d = f - (double)f1;
  const double e = m ? g2 * d + ga * sgn0(d) : 0.0;
  const double gxc = ((double)i01 - (double)i00) * uy + ((double)i11 - (double)i10) * ey;
  const double gyc = ((double)i10 - (double)i00) * ux + ((double)i11 - (double)i01) * ex;
  spx += e * gxc;
  spy += e * gyc;
  const float ef = (float)e;
  acc -= ef;
  return ef;
}

__device__ __forceinline__ float4 chan4(const float4& i00, const float4& i01, const float4& i10, const float4& i11, const float4& f1,
                                        double dx, double dy, double g2, double ga, bool m, double& spx, double& spy, float4& acc) {
  float4 e;
  e.x = chan(i00.x, i01.x, i10.x, i11.x, f1.x, dx, dy, g2, ga, m, spx, spy, acc.x);
  e.y = chan(i00.y, i01.y, i10.y, i11.y, f1.y, dx, dy, g2, ga, m, spx, spy, acc.y);
  e.z = chan(i00.z, i01.z, i10.z, i11.z, f1.z, dx, dy, g2, ga, m, spx, spy, acc.z);
  e.w = chan(i00.w, i01.w, i10.w, i11.w, f1.w, dx, dy, g2, ga, m, spx, spy, acc.w);
  return e;
}

// out = (overwrite ? +0 : old) + v: one statement for both modes, so that overwriting has the bits of accumulating into zeros (a -0 too)
__device__ __forceinline__ void st16(float* p, const float4& v, bool overwrite) {
  float4* q = reinterpret_cast<float4*>(p);
  const float4 o = overwrite ? make_float4(0.f, 0.f, 0.f, 0.f) : *q;
  *q = make_float4(o.x + v.x, o.y + v.y, o.z + v.z, o.w + v.w);
}
// out = (overwrite ? +0 : old) + s w, fused
__device__ __forceinline__ void st16_scaled(float* p, float s, float w0, float w1, float w2, float w3, bool overwrite) {
  float4* q = reinterpret_cast<float4*>(p);
  const float4 o = overwrite ? make_float4(0.f, 0.f, 0.f, 0.f) : *q;
  *q = make_float4(fmaf(s, w0, o.x), fmaf(s, w1, o.y), fmaf(s, w2, o.z), fmaf(s, w3, o.w));
}

// C128: C == 128, 16-byte accesses; KM: 0 = no basis, 1 = K == 128 with 16-byte accesses, 2 = any K, lanes stride over the coefficients
#ifndef BANET_RG_MIN_WAVES
#define BANET_RG_MIN_WAVES 2   // waves per SIMD the register allocation aims at (development A/B: 1 = no limit below 512 registers)
#endif
template <bool C128, int KM>
__global__ __launch_bounds__(kBlock, BANET_RG_MIN_WAVES) void ba_residual_grad_kernel(const ResGradArgs a) {
  const banet_level_t& lv = a.lv;
  const int b = blockIdx.y, g = blockIdx.x;
  const int lane = lane_id(), row = lane >> 4, l = lane & 15, wv = wave_id();
  const int N = lv.N, C = lv.C, K = lv.K, H = lv.H, W = lv.W, pairs = a.pairs;
  const int Ct = lv.tgt_has_grad ? 3 * C : C;
  const bool dense = lv.dense != 0, ow = a.overwrite != 0;
  const float* __restrict__ src_b = lv.src + (size_t)b * N * C;
  const float* __restrict__ dep_b = lv.depth + (size_t)b * N;
  const float* __restrict__ bas_b = KM ? lv.basis + (size_t)b * N * K : nullptr;
  const float* __restrict__ wc_b = KM ? a.Wc + (size_t)b * K : nullptr;

  extern __shared__ double s_dyn[];                 // the pose slots (when they fit)
  __shared__ float s_pose[kRgPoseLds][12];
  __shared__ float s_w[KM ? kNumWaves : 1][KM ? 256 : 1];
  double* slots = a.slots != nullptr ? a.slots + ((size_t)b * a.G + g) * kRgSlots * pairs * 12 : s_dyn;
  for (int i = threadIdx.x; i < kRgSlots * pairs * 12; i += kBlock) slots[i] = 0.0;
  if ((int)threadIdx.x < min(pairs, kRgPoseLds) * 12) {
    const int f = threadIdx.x / 12, i = threadIdx.x - f * 12;
    const size_t vb = (size_t)b * pairs + f;
    s_pose[f][i] = i < 9 ? a.R[vb * 9 + i] : a.T[vb * 3 + (i - 9)];
  }
  float fx0 = 1.f, fy0 = 1.f, ox0 = 0.f, oy0 = 0.f;   // dense: the window's full-resolution intrinsics
  if (dense) {
    fx0 = rfl(lv.intr[b * 4 + 0]);
    fy0 = rfl(lv.intr[b * 4 + 1]);
    ox0 = rfl(lv.intr[b * 4 + 2]);
    oy0 = rfl(lv.intr[b * 4 + 3]);
  }
  __syncthreads();

  // this lane's pose number (l < 12): component ci of (gX, gY, gZ), times D p_cj for the rotation entries
  const int ci = l < 9 ? l / 3 : l < 12 ? l - 9 : 0, cj = l % 3;
  double* my_slot = slots + (size_t)(wv * kRgStepPts + row) * pairs * 12 + l;

  float wreg[8];               // KM == 1: this lane's coefficients 4l .. 4l+3, 64+4l .. 64+4l+3
  float wacc[KM == 2 ? kRgChunks : 8];   // dWc over this wave's points: KM == 1 the same 8 coefficients, KM == 2 l, l + 16, ...
#pragma unroll
  for (int i = 0; i < (KM == 2 ? kRgChunks : 8); ++i) wacc[i] = 0.f;
  if constexpr (KM == 1) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      wreg[e] = wc_b[4 * l + e];
      wreg[4 + e] = wc_b[64 + 4 * l + e];
    }
  }

  for (int j = 0; j < kRgWgUnits / kNumWaves; ++j) {
    const int u = g * kRgWgUnits + j * kNumWaves + wv;   // wave-uniform
    if (u >= a.units) break;
    int pt[kRgSteps];
    bool valid[kRgSteps];
    float D[kRgSteps];
    double dDt[kRgSteps], pm[kRgSteps], Dd[kRgSteps];
    RgRay ray[kRgSteps];
    RgRayD rd[kRgSteps];
    float4 f1a[kRgSteps], f1b[kRgSteps], aca[kRgSteps], acb[kRgSteps];   // C128: the source row and -sum_f e
    float4 ba[kRgSteps], bb[kRgSteps];                                   // KM == 1: the basis row
    float f1[C128 ? 1 : kRgSteps][C128 ? 1 : kRgChunks], ac[C128 ? 1 : kRgSteps][C128 ? 1 : kRgChunks];
#pragma unroll
    for (int s = 0; s < kRgSteps; ++s) {
      const int n = u * kRgUnitPts + s * kRgStepPts + row;
      valid[s] = n < N;
      pt[s] = valid[s] ? n : 0;              // rows past the end read point 0 (always there) and store nothing
    }
    // ---- depth and the source row, once per point -------------------------------------------
    float dot[kRgSteps];
    double dotd[kRgSteps];
#pragma unroll
    for (int s = 0; s < kRgSteps; ++s) {
      dot[s] = 0.f;
      dotd[s] = 0.0;
      if constexpr (KM == 1) {
        const float* brow = bas_b + (size_t)pt[s] * 128;
        const float4 b0 = ld16_stream(brow + 4 * l);
        const float4 b1 = ld16_stream(brow + 64 + 4 * l);
        float acc = b0.x * wreg[0];
        acc = fmaf(b0.y, wreg[1], acc);
        acc = fmaf(b0.z, wreg[2], acc);
        acc = fmaf(b0.w, wreg[3], acc);
        acc = fmaf(b1.x, wreg[4], acc);
        acc = fmaf(b1.y, wreg[5], acc);
        acc = fmaf(b1.z, wreg[6], acc);
        acc = fmaf(b1.w, wreg[7], acc);
        dot[s] = acc;
        dotd[s] = ((((double)b0.x * wreg[0] + (double)b0.y * wreg[1]) + ((double)b0.z * wreg[2] + (double)b0.w * wreg[3])) +
                   (((double)b1.x * wreg[4] + (double)b1.y * wreg[5]) + ((double)b1.z * wreg[6] + (double)b1.w * wreg[7])));
        ba[s] = b0;
        bb[s] = b1;
      } else if constexpr (KM == 2) {
        const float* brow = bas_b + (size_t)pt[s] * K;
        float acc = 0.f;
        double accd = 0.0;
        for (int k = l; k < K; k += 16) {
          acc = fmaf(brow[k], wc_b[k], acc);
          accd += (double)brow[k] * (double)wc_b[k];
        }
        dot[s] = acc;
        dotd[s] = accd;
      }
      if constexpr (C128) {
        const float* srow = src_b + (size_t)pt[s] * 128;
        f1a[s] = ld16_stream(srow + 4 * l);
        f1b[s] = ld16_stream(srow + 64 + 4 * l);
        aca[s] = acb[s] = make_float4(0.f, 0.f, 0.f, 0.f);
      } else {
#pragma unroll
        for (int i = 0; i < kRgChunks; ++i) {
          const int c = i * 16 + l;
          f1[s][i] = c < C ? src_b[(size_t)pt[s] * C + c] : 0.f;
          ac[s][i] = 0.f;
        }
      }
    }
#pragma unroll
    for (int s = 0; s < kRgSteps; ++s) {
      D[s] = dep_b[pt[s]];
      if constexpr (KM != 0) D[s] += row16_sum(dot[s]);
      Dd[s] = (double)dep_b[pt[s]];
      if constexpr (KM != 0) Dd[s] += row16_sum_d(dotd[s]);
      dDt[s] = 0.0;
      if (dense) {
        const int py = pt[s] / W, px = pt[s] - py * W;
        ray[s] = dense_ray(lv, fx0, fy0, ox0, oy0, valid[s], px, py, cj);
        rd[s] = dense_ray_d(lv, fx0, fy0, ox0, oy0, valid[s], px, py, cj);
      } else {
        ray[s] = sparse_ray(lv, b, valid[s], pt[s], cj);
        rd[s] = widen_ray(ray[s]);
      }
      pm[s] = l < 9 ? Dd[s] * rd[s].pj : 1.0;
    }

    // ---- the window's target frames ------------------------------------------------------------
    for (int f = 0; f < pairs; ++f) {
      const int vb = b * pairs + f;
      const float* __restrict__ tgt_f = lv.tgt + (size_t)vb * H * W * Ct;
      float Rm[9], Tv[3];
#pragma unroll
      for (int i = 0; i < 9; ++i) Rm[i] = rfl(f < kRgPoseLds ? s_pose[f][i] : a.R[(size_t)vb * 9 + i]);
#pragma unroll
      for (int i = 0; i < 3; ++i) Tv[i] = rfl(f < kRgPoseLds ? s_pose[f][9 + i] : a.T[(size_t)vb * 3 + i]);
      RgGeo q[kRgSteps];
      const float* r00[kRgSteps];
      int sx[kRgSteps], sy[kRgSteps];
      double g2[kRgSteps], ga[kRgSteps];
      double ex[kRgSteps], ey[kRgSteps], grx[kRgSteps], gry[kRgSteps], grz[kRgSteps], gx[kRgSteps], gy[kRgSteps], giz[kRgSteps];
      float gpx[kRgSteps], gpy[kRgSteps];
#pragma unroll
      for (int s = 0; s < kRgSteps; ++s) {
        q[s] = project(ray[s], Rm, Tv, valid[s], D[s], W, H);
        // in the mask: 0 <= x0 <= W-1, 0 <= y0 <= H-1; the +1 neighbours are clamped (stride 0; their weight is 0 there)
        const int x0 = q[s].x0, y0 = q[s].y0;
        r00[s] = tgt_f + ((size_t)y0 * W + x0) * Ct;
        sx[s] = x0 + 1 <= W - 1 ? Ct : 0;
        sy[s] = y0 + 1 <= H - 1 ? W * Ct : 0;
        // the projection again in double: the fractions the sample and its derivative are evaluated at, relative to the FORWARD's floor
        ex[s] = ey[s] = grx[s] = gry[s] = grz[s] = gx[s] = gy[s] = giz[s] = 0.0;
        if (q[s].m) {
          const double p0 = rd[s].p0, p1 = rd[s].p1, p2 = rd[s].p2;
          grx[s] = (double)Rm[0] * p0 + (double)Rm[1] * p1 + (double)Rm[2] * p2;
          gry[s] = (double)Rm[3] * p0 + (double)Rm[4] * p1 + (double)Rm[5] * p2;
          grz[s] = (double)Rm[6] * p0 + (double)Rm[7] * p1 + (double)Rm[8] * p2;
          giz[s] = 1.0 / (grz[s] * Dd[s] + (double)Tv[2]);
          gx[s] = (grx[s] * Dd[s] + (double)Tv[0]) * giz[s];
          gy[s] = (gry[s] * Dd[s] + (double)Tv[1]) * giz[s];
          ex[s] = (rd[s].fx * gx[s] + rd[s].ox) - (double)x0;
          ey[s] = (rd[s].fy * gy[s] + rd[s].oy) - (double)y0;
        }
        const size_t o = (size_t)vb * N + pt[s];
        g2[s] = (q[s].m && a.gsq != nullptr) ? 2.0 * (double)a.gsq[o] : 0.0;
        ga[s] = (q[s].m && a.gab != nullptr) ? (double)a.gab[o] : 0.0;
        gpx[s] = (q[s].m && a.gproj != nullptr) ? a.gproj[2 * o] : 0.f;
        gpy[s] = (q[s].m && a.gproj != nullptr) ? a.gproj[2 * o + 1] : 0.f;
      }

      double spx[kRgSteps], spy[kRgSteps];
#pragma unroll
      for (int s = 0; s < kRgSteps; ++s) spx[s] = spy[s] = 0.0;
      if constexpr (C128) {
        float4 t[kRgSteps][8];
#pragma unroll
        for (int s = 0; s < kRgSteps; ++s) {
#pragma unroll
          for (int i = 0; i < 8; ++i) t[s][i] = make_float4(0.f, 0.f, 0.f, 0.f);
          if (q[s].m) {   // a masked point reads no tap
            t[s][0] = *reinterpret_cast<const float4*>(r00[s] + 4 * l);
            t[s][1] = *reinterpret_cast<const float4*>(r00[s] + sx[s] + 4 * l);
            t[s][2] = *reinterpret_cast<const float4*>(r00[s] + sy[s] + 4 * l);
            t[s][3] = *reinterpret_cast<const float4*>(r00[s] + sy[s] + sx[s] + 4 * l);
            t[s][4] = *reinterpret_cast<const float4*>(r00[s] + 64 + 4 * l);
            t[s][5] = *reinterpret_cast<const float4*>(r00[s] + sx[s] + 64 + 4 * l);
            t[s][6] = *reinterpret_cast<const float4*>(r00[s] + sy[s] + 64 + 4 * l);
            t[s][7] = *reinterpret_cast<const float4*>(r00[s] + sy[s] + sx[s] + 64 + 4 * l);
          }
        }
#pragma unroll
        for (int s = 0; s < kRgSteps; ++s) {
          const float4 ea = chan4(t[s][0], t[s][1], t[s][2], t[s][3], f1a[s], ex[s], ey[s], g2[s],
                                  ga[s], q[s].m, spx[s], spy[s], aca[s]);
          const float4 eb = chan4(t[s][4], t[s][5], t[s][6], t[s][7], f1b[s], ex[s], ey[s], g2[s],
                                  ga[s], q[s].m, spx[s], spy[s], acb[s]);
          if (a.erow != nullptr && valid[s]) {
            float* er = a.erow + ((size_t)vb * N + pt[s]) * 128;
            *reinterpret_cast<float4*>(er + 4 * l) = ea;
            *reinterpret_cast<float4*>(er + 64 + 4 * l) = eb;
          }
        }
      } else {
#pragma unroll
        for (int i = 0; i < kRgChunks; ++i) {
          if (i * 16 < C) {   // wave-uniform
            const int c = i * 16 + l;
            const bool ok = c < C;
            const int cc = ok ? c : 0;
#pragma unroll
            for (int s = 0; s < kRgSteps; ++s) {
              float t0 = 0.f, t1 = 0.f, t2 = 0.f, t3 = 0.f;
              if (q[s].m) {
                t0 = r00[s][cc];
                t1 = r00[s][sx[s] + cc];
                t2 = r00[s][sy[s] + cc];
                t3 = r00[s][sy[s] + sx[s] + cc];
              }
              const float e = chan(t0, t1, t2, t3, f1[s][i], ex[s], ey[s], g2[s], ga[s],
                                   ok && q[s].m, spx[s], spy[s], ac[s][i]);
              if (a.erow != nullptr && valid[s] && ok) a.erow[((size_t)vb * N + pt[s]) * C + c] = e;
            }
          }
        }
      }

      // ---- projection gradient, geometry backward, the frame's pose numbers ----------------------
      double pv = 0.0;
#pragma unroll
      for (int s = 0; s < kRgSteps; ++s) {
        const double dpx = row16_sum_d(spx[s]) + (double)gpx[s], dpy = row16_sum_d(spy[s]) + (double)gpy[s];
        double gX = 0.0, gY = 0.0, gZ = 0.0;
        if (q[s].m) {
          const double rx = grx[s], ry = gry[s], rz = grz[s], iz = giz[s], x = gx[s], y = gy[s];
          const double hx = rd[s].fx * dpx, hy = rd[s].fy * dpy;
          gX = hx * iz;
          gY = hy * iz;
          gZ = -(hx * x + hy * y) * iz;
          // gX rx + gY ry + gZ rz with rx - rz x = (rx Tz - rz Tx) / Z: the same number without the cancellation of rx against rz x
          const double ax = rx * (double)Tv[2] - rz * (double)Tv[0], ay = ry * (double)Tv[2] - rz * (double)Tv[1];
          dDt[s] += ((hx * ax + hy * ay) * iz) * iz;
        }
        const double gi = ci == 0 ? gX : ci == 1 ? gY : gZ;
        pv += q[s].m ? gi * pm[s] : 0.0;
        if (a.eproj != nullptr && l == 0 && valid[s]) {
          const size_t o = (size_t)vb * N + pt[s];
          a.eproj[2 * o] = (float)q[s].x0 + q[s].dx;       // (0, 0) for a masked point: its zero row lands on texel (0, 0) as +0
          a.eproj[2 * o + 1] = (float)q[s].y0 + q[s].dy;
        }
      }
      if (l < 12) my_slot[(size_t)f * 12] += pv;
    }

    // ---- per point: dsrc, ddepth, dbasis; dWc into the lane's registers ----------------------------
#pragma unroll
    for (int s = 0; s < kRgSteps; ++s) {
      const float dd = valid[s] ? (float)dDt[s] : 0.f;
      const bool nz = dd != 0.f;   // a point that contributes nothing: not even 0 x a non-finite basis entry
      if (valid[s]) {
        if (a.dsrc != nullptr) {
          if constexpr (C128) {
            float* o = a.dsrc + ((size_t)b * N + pt[s]) * 128;
            st16(o + 4 * l, aca[s], ow);
            st16(o + 64 + 4 * l, acb[s], ow);
          } else {
            float* o = a.dsrc + ((size_t)b * N + pt[s]) * C;
#pragma unroll
            for (int i = 0; i < kRgChunks; ++i) {
              const int c = i * 16 + l;
              if (c < C) o[c] = (ow ? 0.f : o[c]) + ac[s][i];
            }
          }
        }
        if (a.ddepth != nullptr && l == 0) {
          float* o = a.ddepth + (size_t)b * N + pt[s];
          *o = (ow ? 0.f : *o) + dd;
        }
      }
      if constexpr (KM == 1) {
        if (a.dbasis != nullptr && valid[s]) {
          float* o = a.dbasis + ((size_t)b * N + pt[s]) * 128;
          st16_scaled(o + 4 * l, dd, wreg[0], wreg[1], wreg[2], wreg[3], ow);
          st16_scaled(o + 64 + 4 * l, dd, wreg[4], wreg[5], wreg[6], wreg[7], ow);
        }
        wacc[0] = nz ? fmaf(dd, ba[s].x, wacc[0]) : wacc[0];
        wacc[1] = nz ? fmaf(dd, ba[s].y, wacc[1]) : wacc[1];
        wacc[2] = nz ? fmaf(dd, ba[s].z, wacc[2]) : wacc[2];
        wacc[3] = nz ? fmaf(dd, ba[s].w, wacc[3]) : wacc[3];
        wacc[4] = nz ? fmaf(dd, bb[s].x, wacc[4]) : wacc[4];
        wacc[5] = nz ? fmaf(dd, bb[s].y, wacc[5]) : wacc[5];
        wacc[6] = nz ? fmaf(dd, bb[s].z, wacc[6]) : wacc[6];
        wacc[7] = nz ? fmaf(dd, bb[s].w, wacc[7]) : wacc[7];
      } else if constexpr (KM == 2) {
        if (a.dbasis != nullptr && valid[s]) {
          float* o = a.dbasis + ((size_t)b * N + pt[s]) * K;
          for (int k = l; k < K; k += 16) o[k] = fmaf(dd, wc_b[k], ow ? 0.f : o[k]);
        }
        if (a.want_dwc) {
          const float* brow = bas_b + (size_t)pt[s] * K;
#pragma unroll
          for (int i = 0; i < kRgChunks; ++i) {
            const int k = i * 16 + l;
            if (k < K && nz) wacc[i] = fmaf(dd, brow[k], wacc[i]);
          }
        }
      }
    }
  }

  // ---- the workgroup's partial row: rows 0..3 of a wave by two shuffles, waves through LDS in wave order ------------
  if constexpr (KM != 0) {
#pragma unroll
    for (int i = 0; i < (KM == 2 ? kRgChunks : 8); ++i) {
      float v = wacc[i];
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      if (row == 0) {
        const int k = KM == 1 ? (i < 4 ? 4 * l + i : 64 + 4 * l + (i - 4)) : i * 16 + l;
        s_w[wv][k] = v;
      }
    }
  }
  __syncthreads();
  float* prow = a.part + ((size_t)b * a.G + g) * a.cols;
  for (int t = threadIdx.x; t < pairs * 12; t += kBlock) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < kRgSlots; ++k) s += slots[(size_t)k * pairs * 12 + t];
    prow[t] = (float)s;
  }
  if constexpr (KM != 0) {
    for (int k = threadIdx.x; k < K; k += kBlock) prow[pairs * 12 + k] = ((s_w[0][k] + s_w[1][k]) + s_w[2][k]) + s_w[3][k];
  }
}

// a window's partial rows added in ascending order: one thread per column (pose numbers of every frame, then dWc)
__global__ __launch_bounds__(256) void ba_residual_grad_fold_kernel(const float* __restrict__ part, float* __restrict__ dR, float* __restrict__ dT,
                                                                    float* __restrict__ dWc, int G, int cols, int pairs, int K) {
  const int b = blockIdx.y, col = blockIdx.x * 256 + threadIdx.x;
  if (col >= cols) return;
  const float* __restrict__ p = part + (size_t)b * G * cols + col;
  double s = 0.0;   // the rows are float32; their sum is kept in double until the one rounding of the result
#pragma unroll 8
  for (int g = 0; g < G; ++g) s += (double)p[(size_t)g * cols];
  if (col < pairs * 12) {
    const int f = col / 12, i = col - f * 12;
    const size_t vb = (size_t)b * pairs + f;
    if (i < 9) {
      if (dR != nullptr) dR[vb * 9 + i] = (float)s;
    } else if (dT != nullptr) {
      dT[vb * 3 + (i - 9)] = (float)s;
    }
  } else if (dWc != nullptr) {
    dWc[(size_t)b * K + (col - pairs * 12)] = (float)s;
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

bool residual_grad_dtgt_supported(const banet_level_t* lv) {
  return !lv->tgt_has_grad && resample_grad_supported(lv->B * npairs(lv), lv->N, lv->C, lv->H, lv->W);
}

void plan_residual_grad(const banet_level_t* lv, int want_dtgt, ResGradPlan* pl) {
  const int pairs = npairs(lv);
  pl->pairs = pairs;
  pl->units = (lv->N + kRgUnitPts - 1) / kRgUnitPts;
  pl->G = (pl->units + kRgWgUnits - 1) / kRgWgUnits;
  pl->cols = 12 * pairs + lv->K;
  pl->slots_in_ws = pairs > kResGradLdsFrames ? 1 : 0;
  const size_t VB = (size_t)lv->B * pairs;
  Arena ar;
  pl->off_part = ar.take((size_t)lv->B * pl->G * pl->cols * 4);
  pl->off_slots = pl->slots_in_ws ? ar.take((size_t)lv->B * pl->G * kRgSlots * pairs * 12 * 8) : 0;
  pl->off_erow = pl->off_eproj = pl->off_rg = 0;
  if (want_dtgt) {
    pl->off_erow = ar.take(VB * lv->N * lv->C * 4);
    pl->off_eproj = ar.take(VB * lv->N * 2 * 4);
    pl->off_rg = ar.take(resample_grad_workspace_bytes((int)VB, lv->N, lv->C, lv->H, lv->W));
  }
  pl->bytes = ar.off;
}

int launch_residual_grad(const banet_level_t* lv, const float* R, const float* T, const float* Wc, const banet_residual_grad_in_t* gin,
                         const banet_residual_grad_out_t* out, int flags, void* ws, hipStream_t s) {
  ResGradPlan pl;
  plan_residual_grad(lv, out->dtgt != nullptr, &pl);
  char* base = static_cast<char*>(ws);
  ResGradArgs a;
  a.lv = *lv;
  a.R = R;
  a.T = T;
  a.Wc = Wc;
  a.gsq = gin->gsq;
  a.gab = gin->gab;
  a.gproj = gin->gproj;
  a.dsrc = out->dsrc;
  a.ddepth = out->ddepth;
  a.dbasis = lv->K > 0 ? out->dbasis : nullptr;
  a.part = reinterpret_cast<float*>(base + pl.off_part);
  a.slots = pl.slots_in_ws ? reinterpret_cast<double*>(base + pl.off_slots) : nullptr;
  a.erow = out->dtgt ? reinterpret_cast<float*>(base + pl.off_erow) : nullptr;
  a.eproj = out->dtgt ? reinterpret_cast<float*>(base + pl.off_eproj) : nullptr;
  a.pairs = pl.pairs;
  a.units = pl.units;
  a.G = pl.G;
  a.cols = pl.cols;
  a.overwrite = (flags & BANET_ADJOINT_OVERWRITE) ? 1 : 0;
  float* dWc = lv->K > 0 ? out->dWc : nullptr;
  a.want_dwc = dWc != nullptr;
  const dim3 grid(pl.G, lv->B), block(kBlock);
  const size_t lds = pl.slots_in_ws ? 0 : (size_t)kRgSlots * pl.pairs * 12 * 8;
  // 16-byte accesses need 16-byte aligned rows (C = 128: every row of a 16-byte aligned tensor is); anything else takes the plain path
  const bool c128 = lv->C == 128 && aligned16(lv->src) && aligned16(lv->tgt) && aligned16(out->dsrc) && aligned16(a.erow);
  const int km = lv->K == 0 ? 0 : (c128 && lv->K == 128 && aligned16(lv->basis) && aligned16(out->dbasis)) ? 1 : 2;
  if (c128 && km == 0) hipLaunchKernelGGL((ba_residual_grad_kernel<true, 0>), grid, block, lds, s, a);
  else if (c128 && km == 1) hipLaunchKernelGGL((ba_residual_grad_kernel<true, 1>), grid, block, lds, s, a);
  else if (c128) hipLaunchKernelGGL((ba_residual_grad_kernel<true, 2>), grid, block, lds, s, a);
  else if (km == 0) hipLaunchKernelGGL((ba_residual_grad_kernel<false, 0>), grid, block, lds, s, a);
  else hipLaunchKernelGGL((ba_residual_grad_kernel<false, 2>), grid, block, lds, s, a);
  if (hipGetLastError() != hipSuccess) return BANET_ERR_LAUNCH;
  if (out->dR != nullptr || out->dT != nullptr || dWc != nullptr) {
    hipLaunchKernelGGL(ba_residual_grad_fold_kernel, dim3((pl.cols + 255) / 256, lv->B), dim3(256), 0, s, a.part, out->dR, out->dT, dWc,
                       pl.G, pl.cols, pl.pairs, lv->K);
    if (hipGetLastError() != hipSuccess) return BANET_ERR_LAUNCH;
  }
  if (out->dtgt != nullptr)
    return launch_resample_grad(nullptr, a.eproj, a.erow, out->dtgt, nullptr, lv->B * pl.pairs, lv->N, lv->C, lv->H, lv->W,
                                BANET_RESAMPLE_CLAMP, (flags & BANET_ADJOINT_OVERWRITE_MAP) ? 1 : 0, base + pl.off_rg, s);
  return BANET_OK;
}

}  // namespace banet
