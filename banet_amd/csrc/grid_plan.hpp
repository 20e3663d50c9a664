// Geometry of the grid resampler (grid_prep.hip): a level's pixel (i, j) samples the map at x = j sx + ox, y = i sy + oy.
// Plain C++17 with no HIP include -- the kernels and the host share it, and tests/test_dense_prep_cpu.py builds it with g++
// (tests/native/grid_plan_host.cpp) to sweep the candidate ranges against a brute-forced forward.
//
//   grid_coord       the coordinate, two separately rounded float32 operations (never an fma): numpy float32 j * s + o
//   grid_candidates  the output indices along one axis whose taps can touch texel X: the affine map inverted, widened, then
//                    corrected with grid_coord itself
//   grid_check       the supported geometry, decided on the host before a launch
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define BANET_HD __host__ __device__ __forceinline__
#else
#define BANET_HD inline
#endif

namespace banet {

constexpr int kGridMaxLevels = 8;
constexpr float kGridMinStep = 0.25f, kGridMaxStep = 64.f;

BANET_HD float grid_coord(int j, float s, float o) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fadd_rn(__fmul_rn((float)j, s), o);
#else
  volatile float p = (float)j * s;   // (volatile: the host compiler must not contract the two operations either)
  return p + o;
#endif
}

// Output indices j in [0, n) along one axis whose sample coordinate lies in [X - 1, X + 1]: every index whose two taps along the
// axis (floor and floor + 1; CLAMP mode: each clamped into the image, coordinates in [-1, W]) can be texel X -- the last texel's
// clamped taps at coordinate W included, because the interval is closed.  [*lo, *hi], empty when *lo > *hi.
//   1. the exact inverse of the affine map in double, one index wider on both sides: what float rounding of the coordinate
//      moves across an end of the interval is at most one index away wherever a coordinate's rounding error is below one step
//      (any map below 2^21 texels a side);
//   2. grid_coord is monotone in j (a rounded product and a rounded sum of monotone terms, s > 0), so the range is then
//      corrected with the forward's own coordinate: extended while the neighbour outside still lies in the interval, and cut
//      back while an end lies outside.  After the extension no index outside the range can contribute whatever step 1
//      estimated, and the cut removes only indices that do not.
// The result holds at most 2 / s + 1 indices where coordinates are exact, and never more than 2 / s + 4 below 2^21 texels.
BANET_HD void grid_candidates(int X, int n, float s, float o, int* lo, int* hi) {
  const double a = ((double)X - 1.0 - (double)o) / (double)s, b = ((double)X + 1.0 - (double)o) / (double)s;
  double l = floor(a) - 1.0, h = ceil(b) + 1.0;
  l = l < 0.0 ? 0.0 : (l > (double)n ? (double)n : l);
  h = h > (double)(n - 1) ? (double)(n - 1) : (h < -1.0 ? -1.0 : h);
  int jl = (int)l, jh = (int)h;
  const double x0 = (double)X - 1.0, x1 = (double)X + 1.0;
  while (jl > 0 && (double)grid_coord(jl - 1, s, o) >= x0) --jl;
  while (jh < n - 1 && (double)grid_coord(jh + 1, s, o) <= x1) ++jh;
  while (jl <= jh && (double)grid_coord(jl, s, o) < x0) ++jl;
  while (jh >= jl && (double)grid_coord(jh, s, o) > x1) --jh;
  *lo = jl;
  *hi = jh;
}

// 0 = supported; -1 = nonsense (BANET_ERR_INVALID_ARG); -3 = outside the supported geometry (BANET_ERR_UNSUPPORTED)
inline int grid_check_axis(int n_out, int n_in, float s, float o) {
  if (n_out <= 0 || !(s > 0.f) || !(s < INFINITY) || !(o == o) || !(fabsf(o) < INFINITY)) return -1;
  if (s < kGridMinStep || s > kGridMaxStep) return -3;
  // monotone in j: the first and the last coordinate bound them all
  if ((double)grid_coord(0, s, o) < -1.0 || (double)grid_coord(n_out - 1, s, o) > (double)n_in) return -3;
  return 0;
}

inline int grid_check_shape(int B, int H, int W, int C, int n_levels) {
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || n_levels <= 0) return -1;
  if (n_levels > kGridMaxLevels || C > 256 || B > 65535) return -3;
  if ((unsigned long long)H * W * C >= (1ull << 30)) return -3;
  return 0;
}

inline int grid_check_level(int H, int W, int C, int Ho, int Wo, float sx, float sy, float ox, float oy) {
  if (Ho <= 0 || Wo <= 0) return -1;
  if ((unsigned long long)Ho * Wo * C >= (1ull << 30)) return -3;
  const int rx = grid_check_axis(Wo, W, sx, ox), ry = grid_check_axis(Ho, H, sy, oy);
  if (rx == -1 || ry == -1) return -1;
  return rx ? rx : ry;
}

}  // namespace banet
