// The pose prior inside the LM loop (include/banet_hip.h (5f); plan: pose_prior_plan.hpp).  The update convention is the solve's
// (solve.hip; oracle _se3_update): delta = [w; t], R' = exp(w) R, T' = V(w) t + exp(w) T, i.e. T' = Exp(delta) o T with
// Exp([phi; rho]) = (exp(phi), V(phi) rho) -- a left perturbation, the tangent banet_ba_marginals_f32's pose_cov is expressed in.
// Per window, with prior poses (R0_i, T0_i), i < pairs, and a joint information matrix Lambda [m][m], m = 6 pairs:
//   E_i = T_i o T0_i^-1:  Re = R_i R0_i^T,  te = T_i - Re T0_i         r_i = Log(E_i) = [phi; rho],  rho = V(phi)^-1 te
//   Jr  = blockdiag_i J_l(r_i)^-1,   J_l^-1 = [[J^-1, 0], [-J^-1 Q J^-1, J^-1]],   J = V(phi),   Q: Barfoot's Q(rho, phi)
//   AtA[0:m, 0:m] += scale Jr^T Lambda Jr         Atb[0:m] -= scale Jr^T Lambda r                     (Gauss-Newton; row stride P)
// between launch_assemble and launch_solve of every iteration, before the damping.  No workspace, no once-per-level pass: r and Jr
// change with the state.  One workgroup of four waves per window, whatever the shape:
//   1. all threads stage Lambda in LDS; thread i < pairs computes r_i and the 6 x 6 block Jr_i into LDS
//   2. M = Lambda Jr (6-term fma chains) and u = Lambda r (one m-term chain per row) into LDS
//   3. H = Jr^T M and v = Jr^T u (6-term chains); one lane per element read-modify-writes AtA and Atb (4-byte accesses: a row of
//      AtA has stride P)
// No atomics; every output element is written by exactly one lane; every summation order is a function of pairs alone, never of B:
// a window's bits are the same alone and in any batch.  At R = R0, T = T0 with Re = I exactly: phi = 0, Jr = I and r = 0 exactly,
// so the block gets fl(scale Lambda) and Atb keeps its bits.
#include "kernels.hpp"

namespace banet {

constexpr int kPosePriorM = 6 * kPosePriorPairsMax;
constexpr float kPoseThetaLog = 1e-3f;      // below: theta / sin(theta) by its series (0 / 0 at theta = 0)
constexpr float kPoseThetaSeries = 0.5f;    // below: the coefficients of J^-1 and Q by their series (the closed forms cancel)

struct PosePriorArgs {
  int pairs, m, P;
  float scale;
  const float* R;        // [B][pairs][3][3] the state's
  const float* T;        // [B][pairs][3]
  const float* R0;       // [B][pairs][3][3] the prior's
  const float* T0;       // [B][pairs][3]
  const float* Lambda;   // [B][m][m]
  float* AtA;            // [B][P][P]
  float* Atb;            // [B][P]
};

struct M3 {
  float v[9];
};

__device__ __forceinline__ M3 m3_mul(const M3& a, const M3& b) {
  M3 c;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) c.v[3 * i + j] = fmaf(a.v[3 * i + 2], b.v[6 + j], fmaf(a.v[3 * i + 1], b.v[3 + j], a.v[3 * i] * b.v[j]));
  return c;
}

__device__ __forceinline__ M3 m3_hat(float x, float y, float z) {
  M3 h;
  h.v[0] = 0.f, h.v[1] = -z, h.v[2] = y;
  h.v[3] = z, h.v[4] = 0.f, h.v[5] = -x;
  h.v[6] = -y, h.v[7] = x, h.v[8] = 0.f;
  return h;
}

// c: J^-1 = I - 1/2 F + c F^2;  a1..a3: Q = 1/2 P + a1 (FP + PF + FPF) + a2 (FFP + PFF - 3 FPF) + a3 (FPFF + FFPF)
__device__ __forceinline__ void pose_coefficients(float t, float* c, float* a1, float* a2, float* a3) {
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

// r [6] and Jr [6][6] (row-major) of one pose; R, R0 [9], T, T0 [3]
__device__ void pose_log_jr(const float* __restrict__ R, const float* __restrict__ T, const float* __restrict__ R0,
                            const float* __restrict__ T0, float* __restrict__ r, float* __restrict__ Jr) {
  M3 Re;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) Re.v[3 * i + j] = fmaf(R[3 * i + 2], R0[3 * j + 2], fmaf(R[3 * i + 1], R0[3 * j + 1], R[3 * i] * R0[3 * j]));
  float te[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) te[i] = T[i] - fmaf(Re.v[3 * i + 2], T0[2], fmaf(Re.v[3 * i + 1], T0[1], Re.v[3 * i] * T0[0]));
  const float wx = 0.5f * (Re.v[7] - Re.v[5]), wy = 0.5f * (Re.v[2] - Re.v[6]), wz = 0.5f * (Re.v[3] - Re.v[1]);
  const float s = sqrtf(fmaf(wz, wz, fmaf(wy, wy, wx * wx)));
  const float c = 0.5f * (Re.v[0] + Re.v[4] + Re.v[8] - 1.f);
  const float theta = atan2f(s, c);
  float k;
  if (theta < kPoseThetaLog) {
    const float t2 = theta * theta;
    k = 1.f + t2 * (1.f / 6 + t2 * (7.f / 360));
  } else {
    k = theta / fmaxf(s, 1e-6f);   // (past the supported range, near pi: finite)
  }
  const float px = k * wx, py = k * wy, pz = k * wz;
  float cc, a1, a2, a3;
  pose_coefficients(theta, &cc, &a1, &a2, &a3);
  const M3 F = m3_hat(px, py, pz);
  const M3 FF = m3_mul(F, F);
  M3 Ji;
#pragma unroll
  for (int e = 0; e < 9; ++e) Ji.v[e] = ((e & 3) == 0 ? 1.f : 0.f) - 0.5f * F.v[e] + cc * FF.v[e];
  float rho[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) rho[i] = fmaf(Ji.v[3 * i + 2], te[2], fmaf(Ji.v[3 * i + 1], te[1], Ji.v[3 * i] * te[0]));
  r[0] = px, r[1] = py, r[2] = pz, r[3] = rho[0], r[4] = rho[1], r[5] = rho[2];
  // Q and the lower-left block -J^-1 Q J^-1
  pose_coefficients(sqrtf(fmaf(pz, pz, fmaf(py, py, px * px))), &cc, &a1, &a2, &a3);
  const M3 Pm = m3_hat(rho[0], rho[1], rho[2]);
  const M3 FP = m3_mul(F, Pm), PF = m3_mul(Pm, F);
  const M3 FPF = m3_mul(FP, F);
  const M3 FFP = m3_mul(F, FP), PFF = m3_mul(PF, F), FPFF = m3_mul(FPF, F), FFPF = m3_mul(F, FPF);
  M3 Q;
#pragma unroll
  for (int e = 0; e < 9; ++e)
    Q.v[e] = 0.5f * Pm.v[e] + a1 * (FP.v[e] + PF.v[e] + FPF.v[e]) + a2 * (FFP.v[e] + PFF.v[e] - 3.f * FPF.v[e]) + a3 * (FPFF.v[e] + FFPF.v[e]);
  const M3 Bl = m3_mul(m3_mul(Ji, Q), Ji);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      Jr[6 * i + j] = Ji.v[3 * i + j];
      Jr[6 * i + 3 + j] = 0.f;
      Jr[6 * (i + 3) + j] = -Bl.v[3 * i + j];
      Jr[6 * (i + 3) + 3 + j] = Ji.v[3 * i + j];
    }
}

__global__ __launch_bounds__(kPosePriorThreads) void ba_pose_prior_add_kernel(const PosePriorArgs a) {
  __shared__ float sL[kPosePriorM * kPosePriorM];   // Lambda [m][m]
  __shared__ float sM[kPosePriorM * kPosePriorM];   // Lambda Jr [m][m]
  __shared__ float sJ[kPosePriorPairsMax * 36];     // Jr_i [6][6]
  __shared__ float sr[kPosePriorM], su[kPosePriorM];
  const int tid = threadIdx.x, m = a.m, mm = m * m, pairs = a.pairs;
  const size_t b = blockIdx.x;
  const float* __restrict__ Lam = a.Lambda + b * mm;
  for (int idx = tid; idx < mm; idx += kPosePriorThreads) sL[idx] = Lam[idx];
  if (tid < pairs) {
    const size_t p = b * pairs + tid;
    pose_log_jr(a.R + 9 * p, a.T + 3 * p, a.R0 + 9 * p, a.T0 + 3 * p, sr + 6 * tid, sJ + 36 * tid);
  }
  __syncthreads();
  // M[k][6 j + q] = sum_e Lambda[k][6 j + e] Jr_j[e][q];   u[k] = sum_l Lambda[k][l] r[l]
  for (int idx = tid; idx < mm + m; idx += kPosePriorThreads) {
    if (idx < mm) {
      const int k = idx / m, col = idx - k * m, j = col / 6, q = col - 6 * j;
      const float* l = sL + k * m + 6 * j;
      const float* jr = sJ + 36 * j + q;
      float acc = 0.f;
#pragma unroll
      for (int e = 0; e < 6; ++e) acc = fmaf(l[e], jr[6 * e], acc);
      sM[idx] = acc;
    } else {
      const int k = idx - mm;
      float acc = 0.f;
      for (int l = 0; l < m; ++l) acc = fmaf(sL[k * m + l], sr[l], acc);
      su[k] = acc;
    }
  }
  __syncthreads();
  // H[6 i + q][col] = sum_e Jr_i[e][q] M[6 i + e][col];   v[6 i + q] = sum_e Jr_i[e][q] u[6 i + e]
  float* __restrict__ A = a.AtA + b * a.P * a.P;
  float* __restrict__ tb = a.Atb + b * a.P;
  for (int idx = tid; idx < mm + m; idx += kPosePriorThreads) {
    const bool mat = idx < mm;
    const int row = mat ? idx / m : idx - mm, col = mat ? idx - row * m : 0;
    const int i = row / 6, q = row - 6 * i;
    const float* jr = sJ + 36 * i + q;
    const float* x = mat ? sM + 6 * i * m + col : su + 6 * i;
    const int xs = mat ? m : 1;
    float acc = 0.f;
#pragma unroll
    for (int e = 0; e < 6; ++e) acc = fmaf(jr[6 * e], x[e * xs], acc);
    const float add = __fmul_rn(a.scale, acc);
    if (mat) A[(size_t)row * a.P + col] = __fadd_rn(A[(size_t)row * a.P + col], add);
    else tb[row] = __fsub_rn(tb[row], add);
  }
}

int launch_pose_prior_add(const PosePriorRun& run, const float* R, const float* T, float* AtA, float* Atb, hipStream_t s) {
  const PosePriorPlan& pl = run.pl;
  if (!pl.on) return BANET_OK;
  PosePriorArgs a;
  a.pairs = pl.pairs;
  a.m = pl.m;
  a.P = pl.P;
  a.scale = run.pp.scale;
  a.R = R;
  a.T = T;
  a.R0 = run.pp.R0;
  a.T0 = run.pp.T0;
  a.Lambda = run.pp.Lambda;
  a.AtA = AtA;
  a.Atb = Atb;
  hipLaunchKernelGGL(ba_pose_prior_add_kernel, dim3(pl.grid), dim3(kPosePriorThreads), 0, s, a);
  if (hipGetLastError() != hipSuccess) return BANET_ERR_LAUNCH;
  return BANET_OK;
}

}  // namespace banet

using namespace banet;

extern "C" {

int banet_pose_prior_apply_f32(const banet_level_t* lv, const banet_pose_prior_t* pp, const float* R, const float* T, float* AtA,
                               float* Atb, banet_stream_t stream) {
  if (!lv || !R || !T || !AtA || !Atb) return BANET_ERR_INVALID_ARG;
  PosePriorRun run{};
  const int rc = plan_pose_prior(lv, pp, &run.pl);
  if (rc != BANET_OK) return rc;
  if (!run.pl.on) return BANET_OK;   // the empty prior: nothing is launched
  run.pp = *pp;
  return launch_pose_prior_add(run, R, T, AtA, Atb, static_cast<hipStream_t>(stream));
}

}  // extern "C"
