// Depth observations and coefficient priors inside the LM loop (include/banet_hip.h (5d); plan: prior_plan.hpp).  Per window the
// solve additionally minimises  scale (1/2 Wc^T Lambda Wc - eta^T Wc + 1/2 sum_n w_n (obs_n - depth_n - b_n . Wc)^2);  with
// G = sum w b b^T, g = sum w (obs - depth) b over the points banet_basis_fit_f32 counts:
//   Le = fl(scale fl(G + Lambda))     ee = fl(scale fl(g + eta))       (a half that is not given is left out)
//   AtA[m+i, m+j] += Le[i,j]          Atb[m+i] += ee[i] - sum_j Le[i,j] Wc[j]        m = 6 pairs, row stride P
//   once per level  (launch_prior_setup)   G, g by the Gram pass and fold of basisfit.hip (launch_fit_gram_fold: the bits of
//                   banet_basis_fit_f32's normal / rhs), then prior_combine_kernel, which writes every element of Le and ee
//   every iteration (launch_prior_add)     ba_prior_add_kernel between launch_assemble and launch_solve: one wave per row of Le
// D = depth + b . Wc is linear in Wc, so G and g do not change over a level's iterations; only Le . Wc does.
// No atomics; every output element is written by exactly one lane; every summation order is a function of N and K alone, never
// of B: a window's bits are the same alone and in any batch.
#include "kernels.hpp"

namespace banet {

// ---- once per level -----------------------------------------------------------------------------------------------------------------
struct PriorCombineArgs {
  int K;
  float scale;
  const float* Lambda;   // [B][K][K] or nullptr
  const float* eta;      // [B][K]    or nullptr
  const float* G;        // [B][K][K] or nullptr (no observations)
  const float* g;        // [B][K]    or nullptr
  float* Le;
  float* ee;
};

// One thread per element of Le [K][K] and ee [K] of window blockIdx.y; two roundings each (sum, then scale), no contraction.
// 4-byte loads: Lambda / eta are the caller's and may be only 4-byte aligned.
__global__ __launch_bounds__(kPriorThreads) void prior_combine_kernel(const PriorCombineArgs a) {
  const int K = a.K, KK = K * K;
  const int idx = blockIdx.x * kPriorThreads + threadIdx.x;
  if (idx >= KK + K) return;
  const size_t b = blockIdx.y;
  if (idx < KK) {
    const size_t o = b * KK + idx;
    const float v = (a.G && a.Lambda) ? __fadd_rn(a.G[o], a.Lambda[o]) : a.G ? a.G[o] : a.Lambda[o];
    a.Le[o] = __fmul_rn(a.scale, v);
  } else {
    const size_t o = b * K + (idx - KK);
    const float v = (a.g && a.eta) ? __fadd_rn(a.g[o], a.eta[o]) : a.g ? a.g[o] : a.eta ? a.eta[o] : 0.f;
    a.ee[o] = __fmul_rn(a.scale, v);
  }
}

// ---- every iteration ----------------------------------------------------------------------------------------------------------------
struct PriorAddArgs {
  int K, m, P;
  int rows;          // B K
  const float* Le;   // [B][K][K], 256-byte aligned (workspace)
  const float* ee;   // [B][K]
  const float* Wc;   // [B][K]
  float* AtA;        // [B][P][P]
  float* Atb;        // [B][P]
};

// One wave per row i of Le[b].  Lane l owns the four-column chunks c = l, l + 64, ...: columns 4 c .. 4 c + 3, ascending.  It adds
// its Le values into the depth block of AtA (4-byte read-modify-write: a row of AtA starts at (m + i) P + m floats, not a multiple
// of four) and runs ONE fma chain over its columns for Le[i,:] . Wc; the 64 chains meet in the fixed butterfly of wave_sum and lane 0
// writes Atb.  V4: Le and Wc by 16-byte loads (K % 4 == 0, Wc 16-byte aligned); otherwise 4-byte loads of the same columns into the
// same chain, columns past K as zeros -- equal bits either way.  The order depends on K alone.
template <bool V4>
__global__ __launch_bounds__(kPriorThreads) void ba_prior_add_kernel(const PriorAddArgs a) {
  const int row = blockIdx.x * (kPriorThreads / kWave) + wave_id();
  if (row >= a.rows) return;   // wave-uniform
  const int K = a.K, lane = lane_id();
  const int b = row / K, i = row - b * K;
  const float* __restrict__ L = a.Le + (size_t)row * K;
  const float* __restrict__ w = a.Wc + (size_t)b * K;
  float* __restrict__ A = a.AtA + ((size_t)b * a.P + a.m + i) * a.P + a.m;
  float acc = 0.f;
  for (int j = 4 * lane; j < K; j += 4 * kWave) {
    float l[4], x[4];
    if constexpr (V4) {
      const float4 lv = *reinterpret_cast<const float4*>(L + j), wv = *reinterpret_cast<const float4*>(w + j);
      l[0] = lv.x, l[1] = lv.y, l[2] = lv.z, l[3] = lv.w;
      x[0] = wv.x, x[1] = wv.y, x[2] = wv.z, x[3] = wv.w;
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        l[q] = j + q < K ? L[j + q] : 0.f;
        x[q] = j + q < K ? w[j + q] : 0.f;
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) acc = fmaf(l[q], x[q], acc);
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (j + q < K) A[j + q] += l[q];
  }
  acc = wave_sum(acc);
  if (lane == 0) {
    float* t = a.Atb + (size_t)b * a.P + a.m + i;
    *t = *t + (a.ee[row] - acc);
  }
}

PriorRun make_prior_run(const banet_level_t* lv, const banet_prior_t* pr, const PriorPlan& pl, void* ws) {
  PriorRun r{};
  r.pl = pl;
  if (!pl.on) return r;
  r.pr = *pr;
  r.B = lv->B;
  char* w = static_cast<char*>(ws);
  r.Le = reinterpret_cast<float*>(w + pl.off_Le);
  r.ee = reinterpret_cast<float*>(w + pl.off_ee);
  if (pl.obs) {
    r.part = reinterpret_cast<float*>(w + pl.off_part);
    r.G = reinterpret_cast<float*>(w + pl.off_G);
    r.g = reinterpret_cast<float*>(w + pl.off_g);
  }
  return r;
}

int launch_prior_setup(const banet_level_t* lv, const PriorRun& run, hipStream_t s) {
  const PriorPlan& pl = run.pl;
  if (!pl.on) return BANET_OK;
  if (pl.obs) {
    const int rc = launch_fit_gram_fold(lv, pl.fit, run.pr.obs_depth, run.pr.obs_weight, run.part, run.G, run.g, nullptr, nullptr, nullptr, s);
    if (rc != BANET_OK) return rc;
  }
  PriorCombineArgs c;
  c.K = pl.K;
  c.scale = run.pr.scale;
  c.Lambda = run.pr.Lambda;
  c.eta = run.pr.eta;
  c.G = run.G;
  c.g = run.g;
  c.Le = run.Le;
  c.ee = run.ee;
  const int total = pl.K * pl.K + pl.K;
  hipLaunchKernelGGL(prior_combine_kernel, dim3((total + kPriorThreads - 1) / kPriorThreads, run.B), dim3(kPriorThreads), 0, s, c);
  if (hipGetLastError() != hipSuccess) return BANET_ERR_LAUNCH;
  return BANET_OK;
}

int launch_prior_add(const PriorRun& run, const float* Wc, float* AtA, float* Atb, hipStream_t s) {
  const PriorPlan& pl = run.pl;
  if (!pl.on) return BANET_OK;
  PriorAddArgs a;
  a.K = pl.K;
  a.m = pl.m;
  a.P = pl.P;
  a.rows = run.B * pl.K;
  a.Le = run.Le;
  a.ee = run.ee;
  a.Wc = Wc;
  a.AtA = AtA;
  a.Atb = Atb;
  const bool v4 = (pl.K & 3) == 0 && (reinterpret_cast<uintptr_t>(Wc) & 15u) == 0;
  if (v4) hipLaunchKernelGGL(ba_prior_add_kernel<true>, dim3(pl.add_grid), dim3(kPriorThreads), 0, s, a);
  else hipLaunchKernelGGL(ba_prior_add_kernel<false>, dim3(pl.add_grid), dim3(kPriorThreads), 0, s, a);
  if (hipGetLastError() != hipSuccess) return BANET_ERR_LAUNCH;
  return BANET_OK;
}

}  // namespace banet

using namespace banet;

extern "C" {

size_t banet_prior_workspace_bytes(const banet_level_t* lv, const banet_prior_t* pr) {
  PriorPlan pl;
  if (plan_prior_layout(lv, pr, 0, &pl) != BANET_OK) return 0;
  return pl.bytes;
}

int banet_prior_apply_f32(const banet_level_t* lv, const banet_prior_t* pr, const float* Wc, float* AtA, float* Atb, void* ws,
                          size_t workspace_bytes, banet_stream_t stream) {
  if (!lv || !Wc || !AtA || !Atb) return BANET_ERR_INVALID_ARG;
  PriorPlan pl;
  const int rc = plan_prior(lv, pr, 0, &pl);
  if (rc != BANET_OK) return rc;
  if (!pl.on) return BANET_OK;   // the empty prior: nothing is launched
  if (pl.obs && (!lv->depth || !lv->basis)) return BANET_ERR_INVALID_ARG;
  if (!ws || workspace_bytes < pl.bytes || (reinterpret_cast<uintptr_t>(ws) & 255u) != 0) return BANET_ERR_WORKSPACE;
  const PriorRun run = make_prior_run(lv, pr, pl, ws);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int rs = launch_prior_setup(lv, run, s);
  if (rs != BANET_OK) return rs;
  return launch_prior_add(run, Wc, AtA, Atb, s);
}

}  // extern "C"
