// The bilinear footprint and tap sum of the resampler, ONE definition for ba_resample_kernel (prep.hip, arbitrary points) and
// the grid kernels (grid_prep.hip, a level's pixel grid and its adjoint), so the kernels cannot drift apart: the same floor,
// weights, in-image tests and sum order give the same bits.
//   mode 0: tf.contrib.resampler -- zero padding, a point is sampled iff x > -1, y > -1, x < W, y < H;
//           weights from the CEIL side (dx = cx - x), sum order a*f(fx,fy) + b*f(cx,cy) + c*f(fx,cy) + d*f(cx,fy)
//   mode 1: interpolate2d2 -- weights from the unclamped floor, indices clamped, ((a+b)+c)+d
#pragma once
#include <hip/hip_runtime.h>

namespace banet {

struct ResampleTaps {   // taps in the forward's sum order
  bool ok;              // mode 0: the point is sampled (else the output is 0); mode 1: always
  int tx[4], ty[4];     // texel of each tap, clamped into the image (always addressable)
  float m[4];           // mode 0: 1 where the unclamped tap lies in the image, else 0; mode 1: 1
  float w[4];
};

__device__ __forceinline__ ResampleTaps resample_taps(float x, float y, int H, int W, int mode) {
  ResampleTaps t;
  if (mode == 0) {
    const bool ok = (x > -1.f) && (y > -1.f) && (x < (float)W) && (y < (float)H);
    const float xs = ok ? x : 0.f, ys = ok ? y : 0.f;
    const float fxf = floorf(xs), fyf = floorf(ys), cxf = fxf + 1.f, cyf = fyf + 1.f;
    const float dx = cxf - xs, dy = cyf - ys;
    const int fx = (int)fxf, fy = (int)fyf, cx = (int)cxf, cy = (int)cyf;
    auto in = [&](int xi, int yi) { return xi >= 0 && yi >= 0 && xi <= W - 1 && yi <= H - 1; };
    const int ux[4] = {fx, cx, fx, cx}, uy[4] = {fy, cy, cy, fy};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      t.tx[q] = min(max(ux[q], 0), W - 1);
      t.ty[q] = min(max(uy[q], 0), H - 1);
      t.m[q] = in(ux[q], uy[q]) ? 1.f : 0.f;
    }
    t.ok = ok;
    t.w[0] = dx * dy, t.w[1] = (1.f - dx) * (1.f - dy), t.w[2] = dx * (1.f - dy), t.w[3] = (1.f - dx) * dy;
  } else {
    const float x0f = floorf(x), y0f = floorf(y);
    const float dx = x - x0f, dy = y - y0f;
    t.w[0] = (1.f - dx) * (1.f - dy), t.w[1] = dx * (1.f - dy), t.w[2] = (1.f - dx) * dy, t.w[3] = dx * dy;
    // NaN / inf coordinates: index 0 / saturated, like the oracle's nan_to_num before the clamp
    const float xc = (x0f == x0f) ? fminf(fmaxf(x0f, -1e9f), 1e9f) : 0.f, yc = (y0f == y0f) ? fminf(fmaxf(y0f, -1e9f), 1e9f) : 0.f;
    const int x0 = (int)xc, y0 = (int)yc;
    const int xa = min(max(x0, 0), W - 1), xb = min(max(x0 + 1, 0), W - 1);
    const int ya = min(max(y0, 0), H - 1), yb = min(max(y0 + 1, 0), H - 1);
    t.ok = true;
    t.tx[0] = xa, t.ty[0] = ya, t.tx[1] = xb, t.ty[1] = ya, t.tx[2] = xa, t.ty[2] = yb, t.tx[3] = xb, t.ty[3] = yb;
#pragma unroll
    for (int q = 0; q < 4; ++q) t.m[q] = 1.f;
  }
  return t;
}

// One channel of the output from its four tap values (v[q] = the map at (tx[q], ty[q])): ((t0 + t1) + t2) + t3 with the roundings
// spelled out -- t1 is a rounded product and every other term joins through one fused multiply-add.  Left to the compiler's
// contraction (the `a * b + c` spelling), ba_resample_kernel rounded a channel differently depending on whether the unrolled
// channel loop or its remainder processed it (mode 1), and two kernels sharing the spelling would not have shared the bits;
// this is the form the compiler had chosen for mode 0 everywhere and for mode 1 in the unrolled loop.
__device__ __forceinline__ float resample_sum(const ResampleTaps& t, int mode, float v0, float v1, float v2, float v3) {
  if (mode == 0) {
    const float v = fmaf(t.w[3], t.m[3] * v3, fmaf(t.w[2], t.m[2] * v2, fmaf(t.w[0], t.m[0] * v0, t.w[1] * (t.m[1] * v1))));
    return t.ok ? v : 0.f;
  }
  return fmaf(t.w[3], v3, fmaf(t.w[2], v2, fmaf(t.w[0], v0, t.w[1] * v1)));
}

}  // namespace banet
