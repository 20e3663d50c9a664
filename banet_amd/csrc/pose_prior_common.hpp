// The pose prior's forward chain, shared by pose_prior.hip (the term) and pose_prior_grad.hip (its backward): Re = R R0^T, te, the
// atan2 angle, k = theta / sin(theta), J^-1 with c(theta), rho, Q with a1..a3(|phi|) and -J^-1 Q J^-1, templated on the scalar type.
//   S = float     the forward's own arithmetic, expression for expression what pose_prior.hip held before the move: the bits
//                 ba_pose_prior_add_kernel adds, and the r_i / Jr_i the backward recomputes
//   S = PoseDual  a value and its tangent along one input entry (forward mode).  Every 0 / 0 of the chain is taken analytically:
//                 the angle gives theta^2 and k with tangents that never divide by s = |vee(Re - Re^T)| / 2 alone, |phi| gives
//                 |phi|^2 with the tangent 2 phi . dphi, and the coefficients are series in theta^2 over the whole supported range
//                 (the closed forms' derivatives cancel: dc/dtheta at 0.5 is 1e-3 of its terms), with their own orders.
// Device code only; included after kernels.hpp.
#pragma once

namespace banet {

constexpr float kPoseThetaLog = 1e-3f;      // below: theta / sin(theta) by its series (0 / 0 at theta = 0)
constexpr float kPoseThetaSeries = 0.5f;    // below: the coefficients of J^-1 and Q by their series (the closed forms cancel)

struct PoseDual {
  float v, t;
};

__device__ __forceinline__ PoseDual operator+(PoseDual a, PoseDual b) { return {a.v + b.v, a.t + b.t}; }
__device__ __forceinline__ PoseDual operator-(PoseDual a, PoseDual b) { return {a.v - b.v, a.t - b.t}; }
__device__ __forceinline__ PoseDual operator-(PoseDual a) { return {-a.v, -a.t}; }
__device__ __forceinline__ PoseDual operator*(PoseDual a, PoseDual b) { return {a.v * b.v, fmaf(a.v, b.t, a.t * b.v)}; }
__device__ __forceinline__ PoseDual operator*(float a, PoseDual b) { return {a * b.v, a * b.t}; }
__device__ __forceinline__ PoseDual operator+(float a, PoseDual b) { return {a + b.v, b.t}; }
__device__ __forceinline__ PoseDual operator-(float a, PoseDual b) { return {a - b.v, -b.t}; }
__device__ __forceinline__ PoseDual operator-(PoseDual a, float b) { return {a.v - b, a.t}; }

// a b + c
__device__ __forceinline__ float pose_fma(float a, float b, float c) { return fmaf(a, b, c); }
__device__ __forceinline__ PoseDual pose_fma(PoseDual a, PoseDual b, PoseDual c) {
  return {fmaf(a.v, b.v, c.v), fmaf(a.v, b.t, fmaf(a.t, b.v, c.t))};
}
__device__ __forceinline__ float pose_const(float, float x) { return x; }
__device__ __forceinline__ PoseDual pose_const(PoseDual, float x) { return {x, 0.f}; }

template <typename S>
struct M3 {
  S v[9];
};

template <typename S>
__device__ __forceinline__ M3<S> m3_mul(const M3<S>& a, const M3<S>& b) {
  M3<S> c;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      c.v[3 * i + j] = pose_fma(a.v[3 * i + 2], b.v[6 + j], pose_fma(a.v[3 * i + 1], b.v[3 + j], a.v[3 * i] * b.v[j]));
  return c;
}

template <typename S>
__device__ __forceinline__ M3<S> m3_hat(S x, S y, S z) {
  M3<S> h;
  const S o = pose_const(x, 0.f);
  h.v[0] = o, h.v[1] = -z, h.v[2] = y;
  h.v[3] = z, h.v[4] = o, h.v[5] = -x;
  h.v[6] = -y, h.v[7] = x, h.v[8] = o;
  return h;
}

// c: J^-1 = I - 1/2 F + c F^2;  a1..a3: Q = 1/2 P + a1 (FP + PF + FPF) + a2 (FFP + PFF - 3 FPF) + a3 (FPFF + FFPF)
// float: t is the angle (t2 is not read)
__device__ __forceinline__ void pose_coefficients(float t, float, float* c, float* a1, float* a2, float* a3) {
  const float t2 = t * t;
  if (t < kPoseThetaSeries) {
    *c = 1.f / 12 + t2 * (1.f / 720 + t2 * (1.f / 30240 + t2 * (1.f / 1209600)));
    *a1 = 1.f / 6 - t2 * (1.f / 120 - t2 * (1.f / 5040 - t2 * (1.f / 362880)));
    *a2 = 1.f / 24 - t2 * (1.f / 720 - t2 * (1.f / 40320 - t2 * (1.f / 3628800)));
    *a3 = 1.f / 120 - t2 * (1.f / 2520 - t2 * (1.f / 120960 - t2 * (1.f / 9979200)));
    return;
  }
  float s, co, sh, ch;
  sincosf(t, &s, &co);
  sincosf(0.5f * t, &sh, &ch);
  *c = 1.f / t2 - ch / (2.f * t * sh);   // (1 + cos) / sin = cot(theta / 2): finite at pi
  *a1 = (t - s) / (t2 * t);
  *a2 = (t2 + 2.f * co - 2.f) / (2.f * t2 * t2);
  *a3 = (2.f * t - 3.f * s + t * co) / (2.f * t2 * t2 * t);
}

// The tangent's coefficients: functions of t2 = theta^2 alone (d|phi| = phi . dphi / |phi| never appears), by their series up to
// theta = pi.  c_n = |B_2n| / (2n)! (radius 2 pi: 18 terms leave 2e-10 of c' at theta = 3), a1 = sum (-1)^n t2^n / (2n + 3)!,
// a2 = sum (-1)^n t2^n / (2n + 4)!, a3 = sum (-1)^n (n + 1) t2^n / (2n + 5)! (entire: 13 terms leave 1e-14).
constexpr float kPoseGradC[18] = {8.333333333e-02f, 1.388888889e-03f, 3.306878307e-05f, 8.267195767e-07f, 2.087675699e-08f, 5.284190139e-10f,
                                  1.338253653e-11f, 3.389680296e-13f, 8.586062056e-15f, 2.174868699e-16f, 5.509002828e-18f, 1.395446469e-19f,
                                  3.534707040e-21f, 8.953517427e-23f, 2.267952452e-24f, 5.744790669e-26f, 1.455172476e-27f, 3.685994941e-29f};
constexpr float kPoseGradA1[13] = {1.666666667e-01f, -8.333333333e-03f, 1.984126984e-04f, -2.755731922e-06f, 2.505210839e-08f,
                                   -1.605904384e-10f, 7.647163732e-13f, -2.811457254e-15f, 8.220635247e-18f, -1.957294106e-20f,
                                   3.868170171e-23f, -6.446950284e-26f, 9.183689864e-29f};
constexpr float kPoseGradA2[13] = {4.166666667e-02f, -1.388888889e-03f, 2.480158730e-05f, -2.755731922e-07f, 2.087675699e-09f,
                                   -1.147074560e-11f, 4.779477332e-14f, -1.561920697e-16f, 4.110317623e-19f, -8.896791392e-22f,
                                   1.611737571e-24f, -2.479596263e-27f, 3.279889237e-30f};
constexpr float kPoseGradA3[13] = {8.333333333e-03f, -3.968253968e-04f, 8.267195767e-06f, -1.002084335e-07f, 8.029521918e-10f,
                                   -4.588298239e-12f, 1.968020078e-14f, -6.576508197e-17f, 1.761564696e-19f, -3.868170171e-22f,
                                   7.091645313e-25f, -1.102042784e-27f, 1.470295175e-30f};

template <int N>
__device__ __forceinline__ PoseDual pose_series(const float (&k)[N], PoseDual t2) {
  float p = k[N - 1], d = 0.f;   // Horner on the value and on the derivative with respect to t2
#pragma unroll
  for (int n = N - 2; n >= 0; --n) {
    d = fmaf(d, t2.v, p);
    p = fmaf(p, t2.v, k[n]);
  }
  return {p, d * t2.t};
}

__device__ __forceinline__ void pose_coefficients(PoseDual, PoseDual t2, PoseDual* c, PoseDual* a1, PoseDual* a2, PoseDual* a3) {
  *c = pose_series(kPoseGradC, t2);
  *a1 = pose_series(kPoseGradA1, t2);
  *a2 = pose_series(kPoseGradA2, t2);
  *a3 = pose_series(kPoseGradA3, t2);
}

// the rotation angle from s = |w|, w = vee(Re - Re^T) / 2, and c = (tr Re - 1) / 2: theta = atan2(s, c), theta^2, k = theta / s
__device__ __forceinline__ float pose_sine(float wx, float wy, float wz) { return sqrtf(fmaf(wz, wz, fmaf(wy, wy, wx * wx))); }
__device__ __forceinline__ void pose_angle(float, float, float, float s, float c, float* theta, float* theta2, float* k) {
  *theta = atan2f(s, c);
  *theta2 = 0.f;   // (not read: the float coefficients square the angle themselves)
  if (*theta < kPoseThetaLog) {
    const float t2 = *theta * *theta;
    *k = 1.f + t2 * (1.f / 6 + t2 * (7.f / 360));
  } else {
    *k = *theta / fmaxf(s, 1e-6f);   // (past the supported range, near pi: finite)
  }
}

// The tangent: with s ds = w . dw and n2 = s^2 + c^2,  d(theta^2) = 2 theta (c ds - s dc) / n2 = 2 (k c (w . dw) - theta s dc) / n2
// (k = theta / s, by atan's series in (s / c)^2 below the threshold: finite at s = 0), and
//   below the threshold, where the forward's k is a function of theta^2 alone:  dk = (1/6 + 7/180 theta^2) d(theta^2)
//   above it, k = theta / s:  dk = (w . dw) (c / n2 - k) / s^2 - dc / n2     (the difference carries 1 ulp of k: 1e-7 of dphi)
// The branch is the forward's own, on the same bits of theta.
__device__ __forceinline__ PoseDual pose_sine(PoseDual wx, PoseDual wy, PoseDual wz) {   // -> {s, w . dw}
  return {sqrtf(fmaf(wz.v, wz.v, fmaf(wy.v, wy.v, wx.v * wx.v))), fmaf(wz.v, wz.t, fmaf(wy.v, wy.t, wx.v * wx.t))};
}
__device__ __forceinline__ void pose_angle(PoseDual wx, PoseDual wy, PoseDual wz, PoseDual sw, PoseDual c, PoseDual* theta,
                                           PoseDual* theta2, PoseDual* k) {
  const float s2 = fmaf(wz.v, wz.v, fmaf(wy.v, wy.v, wx.v * wx.v));
  const float s = sw.v, wdw = sw.t;
  const float th = atan2f(s, c.v);
  const float n2 = fmaf(c.v, c.v, s2);
  const float t2 = th * th;
  float kv, kr, kt;
  const bool series = th < kPoseThetaLog;
  if (series) {
    kv = 1.f + t2 * (1.f / 6 + t2 * (7.f / 360));
    const float z = s2 / (c.v * c.v);
    kr = (1.f - z * (1.f / 3 - z * (1.f / 5))) / c.v;
  } else {
    kv = th / fmaxf(s, 1e-6f);
    kr = kv;
  }
  const float dt2 = 2.f * (kr * c.v * wdw - th * s * c.t) / n2;
  if (series) kt = (1.f / 6 + t2 * (7.f / 180)) * dt2;
  else kt = wdw * ((c.v / n2 - kv) / fmaxf(s2, 1e-12f)) - c.t / n2;
  *theta = {th, 0.f};   // (not read: the tangent's coefficients are functions of theta^2)
  *theta2 = {t2, dt2};
  *k = {kv, kt};
}

// |phi| and |phi|^2 for the coefficients of Q
__device__ __forceinline__ void pose_norm(float px, float py, float pz, float* t, float* t2) {
  *t = sqrtf(fmaf(pz, pz, fmaf(py, py, px * px)));
  *t2 = 0.f;
}
__device__ __forceinline__ void pose_norm(PoseDual px, PoseDual py, PoseDual pz, PoseDual* t, PoseDual* t2) {
  *t2 = {fmaf(pz.v, pz.v, fmaf(py.v, py.v, px.v * px.v)), 2.f * fmaf(pz.v, pz.t, fmaf(py.v, py.t, px.v * px.t))};
  *t = {0.f, 0.f};
}

// r [6] and Jr [6][6] (row-major) of one pose; R, R0 [9], T, T0 [3]
template <typename S>
__device__ void pose_log_jr(const S* __restrict__ R, const S* __restrict__ T, const S* __restrict__ R0, const S* __restrict__ T0,
                            S* __restrict__ r, S* __restrict__ Jr) {
  M3<S> Re;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      Re.v[3 * i + j] = pose_fma(R[3 * i + 2], R0[3 * j + 2], pose_fma(R[3 * i + 1], R0[3 * j + 1], R[3 * i] * R0[3 * j]));
  S te[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) te[i] = T[i] - pose_fma(Re.v[3 * i + 2], T0[2], pose_fma(Re.v[3 * i + 1], T0[1], Re.v[3 * i] * T0[0]));
  const S wx = 0.5f * (Re.v[7] - Re.v[5]), wy = 0.5f * (Re.v[2] - Re.v[6]), wz = 0.5f * (Re.v[3] - Re.v[1]);
  const S s = pose_sine(wx, wy, wz);
  const S c = 0.5f * (Re.v[0] + Re.v[4] + Re.v[8] - 1.f);
  S theta, theta2, k;
  pose_angle(wx, wy, wz, s, c, &theta, &theta2, &k);
  const S px = k * wx, py = k * wy, pz = k * wz;
  S cc, a1, a2, a3;
  pose_coefficients(theta, theta2, &cc, &a1, &a2, &a3);
  const M3<S> F = m3_hat(px, py, pz);
  const M3<S> FF = m3_mul(F, F);
  M3<S> Ji;
#pragma unroll
  for (int e = 0; e < 9; ++e) Ji.v[e] = ((e & 3) == 0 ? 1.f : 0.f) - 0.5f * F.v[e] + cc * FF.v[e];
  S rho[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) rho[i] = pose_fma(Ji.v[3 * i + 2], te[2], pose_fma(Ji.v[3 * i + 1], te[1], Ji.v[3 * i] * te[0]));
  r[0] = px, r[1] = py, r[2] = pz, r[3] = rho[0], r[4] = rho[1], r[5] = rho[2];
  // Q and the lower-left block -J^-1 Q J^-1
  pose_norm(px, py, pz, &theta, &theta2);
  pose_coefficients(theta, theta2, &cc, &a1, &a2, &a3);
  const M3<S> Pm = m3_hat(rho[0], rho[1], rho[2]);
  const M3<S> FP = m3_mul(F, Pm), PF = m3_mul(Pm, F);
  const M3<S> FPF = m3_mul(FP, F);
  const M3<S> FFP = m3_mul(F, FP), PFF = m3_mul(PF, F), FPFF = m3_mul(FPF, F), FFPF = m3_mul(F, FPF);
  M3<S> Q;
#pragma unroll
  for (int e = 0; e < 9; ++e)
    Q.v[e] = 0.5f * Pm.v[e] + a1 * (FP.v[e] + PF.v[e] + FPF.v[e]) + a2 * (FFP.v[e] + PFF.v[e] - 3.f * FPF.v[e]) + a3 * (FPFF.v[e] + FFPF.v[e]);
  const M3<S> Bl = m3_mul(m3_mul(Ji, Q), Ji);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      Jr[6 * i + j] = Ji.v[3 * i + j];
      Jr[6 * i + 3 + j] = pose_const(px, 0.f);
      Jr[6 * (i + 3) + j] = -Bl.v[3 * i + j];
      Jr[6 * (i + 3) + 3 + j] = Ji.v[3 * i + j];
    }
}

}  // namespace banet
