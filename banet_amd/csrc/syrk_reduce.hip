// ba_reduce2_kernel: the partial rows of the gather and of every SYRK form -> AtA / Atb / |r| / nvalid, in fixed order.
#include "kernels.hpp"

namespace banet {

// --------------------------------------------------------------------------------------
// fixed-order reduction of the per-workgroup partials of both kernels into AtA / Atb / |r| / nvalid
// (the deterministic counterpart of utils.cu:181-198 ColumnReduceSimpleKernel)
// --------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ba_reduce2_kernel(const float* __restrict__ gpart, int Gg, int gstride,
                                                         const float* __restrict__ spart, int Gs, int sstride,
                                                         const int32_t* active, int active_stride, int K, int C, int pairs,
                                                         float* __restrict__ AtA, float* __restrict__ Atb,
                                                         float* __restrict__ absres, float* __restrict__ nvalid) {
  // Parameter order [pose_1 .. pose_pairs | depth]; the gather partials of pair i are the rows of
  // virtual window b pairs + i.  Pose blocks of different pairs do not couple: exact zeros.
  // 64 output elements per 256-thread block; the four thread groups rq = 0..3 split the SYRK partial rows of an element into
  // four contiguous runs (a small batch has up to one row per CU: 256 dependent adds in one thread were 26 us at one window)
  // and are added ((q0 + q1) + (q2 + q3)) through LDS; the gather rows of an element are summed by group 0 alone, in the
  // order mlp.hpp's role workgroup uses.  Fixed orders: bit-reproducible.
  __shared__ float sQ[4][64];
  const int b = blockIdx.y;
  if (active != nullptr && active[(size_t)b * active_stride] == 0) return;
  const int P6 = 6 * pairs, P = P6 + K;
  const int rq = threadIdx.x >> 6, ej = threadIdx.x & 63;
  const int e = blockIdx.x * 64 + ej;
  const int total = P * P + P + C + 1;
  const bool live = e < total;
  int off = 0, pair = -1;      // pair >= 0: one pair's gather rows; -2: gather rows of all pairs; -1: syrk rows
  bool zero = false;
  float sign = 1.f;
  if (e < P * P) {
    const int i = e / P, j = e - i * P;
    if (i < P6 && j < P6) {
      if (i / 6 != j / 6) {
        zero = true;
      } else {
        pair = i / 6;
        const int ii = i % 6, jj = j % 6;
        const int lo = ii < jj ? ii : jj, hi = ii < jj ? jj : ii;
        off = 6 * lo - lo * (lo - 1) / 2 + (hi - lo);
      }
    } else if (i < P6 || j < P6) {   // H_cd: bundle sign (J = [-Jc | jd b], bundlenet.py:60)
      const int c = i < P6 ? i : j, k = (i < P6 ? j : i) - P6;
      off = c * K + k;
      sign = -1.f;
    } else {
      off = (P6 + 1) * K + (i - P6) * K + (j - P6);
    }
  } else if (e < P * P + P) {
    const int i = e - P * P;
    if (i < P6) {
      pair = i / 6;
      off = 21 + i % 6;
    } else {                         // Atb_d: d = F1 - F2w (bundlenet.py:234)
      off = P6 * K + (i - P6);
      sign = -1.f;
    }
  } else if (e < P * P + P + C) {
    pair = -2;
    off = kGHdr + (e - P * P - P);
  } else {
    pair = -2;
    off = 27;
  }
  float v = 0.f;
  const bool from_s = pair == -1;
  if (live && !zero && (from_s || rq == 0)) {
    const int p0 = pair == -2 ? 0 : pair, p1 = pair == -2 ? pairs : pair + 1;
    for (int pp = p0; pp < (from_s ? p0 + 1 : p1); ++pp) {   // fixed order: pairs, then rows
      const float* p = from_s ? spart + (size_t)b * Gs * sstride + off : gpart + ((size_t)b * pairs + pp) * Gg * gstride + off;
      const size_t st = from_s ? sstride : gstride;
      int i = 0, n = Gg;
      if (from_s) {            // this group's run of the SYRK rows
        i = (Gs * rq) >> 2;
        n = (Gs * (rq + 1)) >> 2;
      }
      float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
      for (; i + 3 < n; i += 4) {
        s0 += p[(size_t)(i + 0) * st];
        s1 += p[(size_t)(i + 1) * st];
        s2 += p[(size_t)(i + 2) * st];
        s3 += p[(size_t)(i + 3) * st];
      }
      for (; i < n; ++i) s0 += p[(size_t)i * st];
      v += (s0 + s1) + (s2 + s3);
    }
    v *= sign;
  }
  sQ[rq][ej] = v;
  __syncthreads();
  if (rq != 0 || !live) return;
  if (from_s && !zero) v = (sQ[0][ej] + sQ[1][ej]) + (sQ[2][ej] + sQ[3][ej]);
  if (e < P * P)
    AtA[(size_t)b * P * P + e] = v;
  else if (e < P * P + P)
    Atb[(size_t)b * P + (e - P * P)] = v;
  else if (e < P * P + P + C)
    absres[(size_t)b * C + (e - P * P - P)] = v;
  else
    nvalid[b] = v;
}

void launch_reduce2(const float* gpart, int Gg, int gstride, const float* spart, int Gs, int sstride,
                    const int32_t* active, int active_stride, int B, int K, int C, int pairs, float* AtA, float* Atb,
                    float* absres, float* nvalid, hipStream_t s) {
  const int P = 6 * pairs + K, total = P * P + P + C + 1;
  hipLaunchKernelGGL(ba_reduce2_kernel, dim3((total + 63) / 64, B), dim3(256), 0, s, gpart, Gg, gstride, spart, Gs,
                     sstride, active, active_stride, K, C, pairs, AtA, Atb, absres, nvalid);
}

}  // namespace banet
