// ba_residual_kernel / ba_residual_sums_kernel -- banet_ba_residual_f32: what a level costs at a given state, per pixel.
//
// For every window b, target frame f (banet_level_t.pairs) and point n (file:line citations are the reference's):
//   D = D0 + Bs.W                         bundlenet.py:208      once per point, reused for every frame of the window
//   X = (R_f p) D + T_f ; px, py ; mask   bundlenet.py:209-224,155 / legacy/ba.py:239-251 -- the float32 statements of the
//                                         gathers: strip_geometry (quad_common.hpp) on a dense level, gather_generic.hip's on sparse points
//   F2w = four bilinear taps of the first C channels of the target row (row stride C, or 3C with tgt_has_grad), x0+1 / y0+1
//         clamped to W-1 / H-1 (utils_python.py:96-99), summed ((I00 w00 + I01 w01) + I10 w10) + I11 w11
//   d_c = F2w_c - F1_c   (F1 = the source row; the sign does not reach the outputs)
//   sq[b,f,n] = sum_c d_c^2   ab[b,f,n] = sum_c |d_c|   mask[b,f,n] = 1 / 0   proj[b,f,n] = (px, py), optional
// Every element of sq / ab / mask is written; a point outside the image (or with a NaN projection) reads no tap and gets exact
// zeros; proj is unspecified there.  (legacy_avg_residual of the reference's CheckUpdate, legacy/ba.py:306-324, is
// N / sum mask x sum_n ab / N per window: the two sums of the second launch.)
//
// Lanes: 16 per point, four points per wave instruction, two such steps (8 points) in flight per wave.
//   C = 128: 8 channels per lane as two 16-byte loads (channels 4l .. 4l+3 and 64+4l .. 64+4l+3: a row of 16 lanes reads
//            256 contiguous bytes per instruction); K = 128: the same split of the basis row, the lane's 8 coefficients in registers;
//   any other C <= 256 / K <= 256 (odd ones too): lanes stride over the channels / coefficients, 16 apart.
//   Channel sums and the depth dot: row16_sum (DPP inside the 16-lane row) -- no shuffles through the LDS crossbar.
// A streaming kernel: one barrier at the start (the window's poses go to LDS once, 48 bytes per frame), none in the loop, no
// atomics; a wave walks 8-point units with the grid's stride, so the grid is free to follow the launch (it does not enter any result).
//
// Second launch (only when sums are asked for): one workgroup per (b, f) reduces the three maps over n in an order that depends
// on N alone -- thread t adds elements t, t + 1024, ... in sequence, then a fixed binary tree over the 1024 threads:
//   sums[b,f,0..3] = sum sq, sum ab, the in-image count (an integer, stored as float), max_n sq.
// So a window's bits are the same alone and in any batch, and the entry needs no workspace.
#include "quad_common.hpp"

namespace banet {

struct ResidualArgs {
  banet_level_t lv;
  const float* R;
  const float* T;
  const float* Wc;
  float* sq;             // [B][pairs][N]
  float* ab;             // [B][pairs][N]
  unsigned char* mask;   // [B][pairs][N]
  float* proj;           // [B][pairs][N][2] or nullptr
  int pairs;
  int units;             // 8-point units per window
};

constexpr int kResStepPts = 4;                 // points per wave instruction (16 lanes each)
constexpr int kResSteps = 2;                   // steps in flight per wave
constexpr int kResUnitPts = kResStepPts * kResSteps;
constexpr int kResChunks = 16;                 // plain path: channels l, l + 16, ... (C <= 256)
constexpr int kSumThreads = 1024;
constexpr int kResPoseLds = 16;                // target frames whose pose is staged in LDS (more: read from memory per frame)

struct ResGeo {
  float dx, dy;
  int x0, y0;
  bool m;
};

// sparse points: the geometry phase of ba_gather_kernel (gather_generic.hip), statement for statement, without the Jacobians
__device__ __forceinline__ ResGeo sparse_geometry(const banet_level_t& lv, int b, const float (&Rm)[9], const float (&Tv)[3], bool valid,
                                                  int pt, float D) {
  const int N = lv.N, W = lv.W, H = lv.H;
  float p0 = 0.f, p1 = 0.f, p2 = 1.f, fx = 1.f, fy = 1.f, ox = 0.f, oy = 0.f;
  if (valid) {
    const size_t o = (size_t)b * 3 * N;
    p0 = lv.rays[o + pt];
    p1 = lv.rays[o + N + pt];
    p2 = lv.rays[o + 2 * (size_t)N + pt];
    const size_t q = (size_t)b * N + pt;
    fx = lv.fx[q];
    fy = lv.fy[q];
    ox = lv.ox[q];
    oy = lv.oy[q];
  }
  const float rx = Rm[0] * p0 + Rm[1] * p1 + Rm[2] * p2;
  const float ry = Rm[3] * p0 + Rm[4] * p1 + Rm[5] * p2;
  const float rz = Rm[6] * p0 + Rm[7] * p1 + Rm[8] * p2;
  const float X = rx * D + Tv[0], Y = ry * D + Tv[1], Z = rz * D + Tv[2];
  const float x = X / Z, y = Y / Z;
  const float pxl = fx * x + ox, pyl = fy * y + oy;
  ResGeo g;
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
  return g;
}

// a 16-byte row piece that is streamed exactly once (basis, source): non-temporal
__device__ __forceinline__ float4 ld16_nt(const float* p) {
  const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
  return make_float4(v.x, v.y, v.z, v.w);
}

__device__ __forceinline__ void res_acc(const float4& i00, const float4& i01, const float4& i10, const float4& i11, const float4& f1,
                                        float w00, float w01, float w10, float w11, float& sq, float& ab) {
  const float a[4] = {i00.x, i00.y, i00.z, i00.w}, bq[4] = {i01.x, i01.y, i01.z, i01.w}, c[4] = {i10.x, i10.y, i10.z, i10.w},
              e[4] = {i11.x, i11.y, i11.z, i11.w}, s[4] = {f1.x, f1.y, f1.z, f1.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float f = ((a[k] * w00 + bq[k] * w01) + c[k] * w10) + e[k] * w11;
    const float d = f - s[k];
    sq += d * d;
    ab += fabsf(d);
  }
}

// C128: C == 128, 16-byte loads; KM: 0 = no basis, 1 = K == 128 with 16-byte loads, 2 = any K, lanes stride over the coefficients
template <bool C128, int KM>
__global__ __launch_bounds__(kBlock) void ba_residual_kernel(const ResidualArgs a) {
  const banet_level_t& lv = a.lv;
  const int b = blockIdx.y;
  const int lane = lane_id(), row = lane >> 4, l = lane & 15;
  const int N = lv.N, C = lv.C, K = lv.K, H = lv.H, W = lv.W, pairs = a.pairs;
  const int Ct = lv.tgt_has_grad ? 3 * C : C;
  const bool dense = lv.dense != 0;
  const float* __restrict__ src_b = lv.src + (size_t)b * N * C;
  const float* __restrict__ dep_b = lv.depth + (size_t)b * N;
  const float* __restrict__ bas_b = KM ? lv.basis + (size_t)b * N * K : nullptr;
  const float* __restrict__ wc_b = KM ? a.Wc + (size_t)b * K : nullptr;

  float wreg[8];   // KM == 1: this lane's coefficients 4l .. 4l+3, 64+4l .. 64+4l+3
  if constexpr (KM == 1) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      wreg[e] = wc_b[4 * l + e];
      wreg[4 + e] = wc_b[64 + 4 * l + e];
    }
  }

  // the window's poses, staged once: read per (unit, frame) from memory they are vector loads whose wait also drains the taps the
  // wave has in flight (quad_common.hpp, load_pose_intr); an LDS read waits on its own counter
  __shared__ float s_pose[kResPoseLds][12];
  if ((int)threadIdx.x < min(pairs, kResPoseLds) * 12) {
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

  const int gw = blockIdx.x * kNumWaves + wave_id(), nw = gridDim.x * kNumWaves;
  for (int u = gw; u < a.units; u += nw) {   // wave-uniform
    int pt[kResSteps];
    bool valid[kResSteps];
    float D[kResSteps];
    float4 f1a[kResSteps], f1b[kResSteps];   // C128: the source row, kept over the frames
    // ---- depth, once per point -------------------------------------------------------------
#pragma unroll
    for (int s = 0; s < kResSteps; ++s) {
      const int n = u * kResUnitPts + s * kResStepPts + row;
      valid[s] = n < N;
      pt[s] = valid[s] ? n : 0;              // rows past the end read point 0 (always there) and store nothing
    }
    float dot[kResSteps];
#pragma unroll
    for (int s = 0; s < kResSteps; ++s) {
      dot[s] = 0.f;
      if constexpr (KM == 1) {
        const float* brow = bas_b + (size_t)pt[s] * 128;
        const float4 b0 = ld16_nt(brow + 4 * l);
        const float4 b1 = ld16_nt(brow + 64 + 4 * l);
        float acc = b0.x * wreg[0];
        acc = fmaf(b0.y, wreg[1], acc);
        acc = fmaf(b0.z, wreg[2], acc);
        acc = fmaf(b0.w, wreg[3], acc);
        acc = fmaf(b1.x, wreg[4], acc);
        acc = fmaf(b1.y, wreg[5], acc);
        acc = fmaf(b1.z, wreg[6], acc);
        acc = fmaf(b1.w, wreg[7], acc);
        dot[s] = acc;
      } else if constexpr (KM == 2) {
        const float* brow = bas_b + (size_t)pt[s] * K;
        float acc = 0.f;
        for (int k = l; k < K; k += 16) acc = fmaf(brow[k], wc_b[k], acc);
        dot[s] = acc;
      }
      if constexpr (C128) {
        const float* srow = src_b + (size_t)pt[s] * 128;
        f1a[s] = ld16_nt(srow + 4 * l);
        f1b[s] = ld16_nt(srow + 64 + 4 * l);
      }
    }
#pragma unroll
    for (int s = 0; s < kResSteps; ++s) {
      D[s] = dep_b[pt[s]];
      if constexpr (KM != 0) D[s] += row16_sum(dot[s]);
    }

    // ---- the window's target frames ------------------------------------------------------------
    for (int f = 0; f < pairs; ++f) {
      const int vb = b * pairs + f;
      const float* __restrict__ tgt_f = lv.tgt + (size_t)vb * H * W * Ct;
      ResGeo g[kResSteps];
      PoseIntr pq;   // = load_pose_intr(lv, b, R_f, T_f): 16 wave-uniform scalars
#pragma unroll
      for (int i = 0; i < 9; ++i) pq.R[i] = rfl(f < kResPoseLds ? s_pose[f][i] : a.R[(size_t)vb * 9 + i]);
#pragma unroll
      for (int i = 0; i < 3; ++i) pq.T[i] = rfl(f < kResPoseLds ? s_pose[f][9 + i] : a.T[(size_t)vb * 3 + i]);
      pq.fx0 = fx0;
      pq.fy0 = fy0;
      pq.ox0 = ox0;
      pq.oy0 = oy0;
      if (dense) {
#pragma unroll
        for (int s = 0; s < kResSteps; ++s) {
          const int py = pt[s] / W, px = pt[s] - py * W;
          SGeo sg;
          strip_geometry(lv, pq, valid[s], px, py, D[s], sg);
          g[s].m = (sg.flags & kPixInMask) != 0;
          g[s].dx = sg.dx;
          g[s].dy = sg.dy;
          g[s].x0 = sg.x0;
          g[s].y0 = sg.y0;
        }
      } else {
#pragma unroll
        for (int s = 0; s < kResSteps; ++s) g[s] = sparse_geometry(lv, b, pq.R, pq.T, valid[s], pt[s], D[s]);
      }

      // the four taps as one row pointer and two small strides: the +1 neighbours are clamped (stride 0; their weight is 0 there)
      const float* r00[kResSteps];
      int sx[kResSteps], sy[kResSteps];
      float w00[kResSteps], w01[kResSteps], w10[kResSteps], w11[kResSteps];
#pragma unroll
      for (int s = 0; s < kResSteps; ++s) {
        // in the mask: 0 <= x0 <= W-1, 0 <= y0 <= H-1
        const int x0 = g[s].x0, y0 = g[s].y0;
        r00[s] = tgt_f + ((size_t)y0 * W + x0) * Ct;
        sx[s] = x0 + 1 <= W - 1 ? Ct : 0;
        sy[s] = y0 + 1 <= H - 1 ? W * Ct : 0;
        const float dx = g[s].dx, dy = g[s].dy;
        w00[s] = (1.f - dx) * (1.f - dy);
        w01[s] = dx * (1.f - dy);
        w10[s] = (1.f - dx) * dy;
        w11[s] = dx * dy;
      }

      float sq[kResSteps], ab[kResSteps];
#pragma unroll
      for (int s = 0; s < kResSteps; ++s) sq[s] = ab[s] = 0.f;
      if constexpr (C128) {
        float4 t[kResSteps][8];
#pragma unroll
        for (int s = 0; s < kResSteps; ++s) {
#pragma unroll
          for (int i = 0; i < 8; ++i) t[s][i] = make_float4(0.f, 0.f, 0.f, 0.f);
          if (g[s].m) {   // a masked point reads no tap
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
        for (int s = 0; s < kResSteps; ++s) {
          float q = 0.f, r = 0.f;
          res_acc(t[s][0], t[s][1], t[s][2], t[s][3], f1a[s], w00[s], w01[s], w10[s], w11[s], q, r);
          res_acc(t[s][4], t[s][5], t[s][6], t[s][7], f1b[s], w00[s], w01[s], w10[s], w11[s], q, r);
          sq[s] = g[s].m ? q : 0.f;
          ab[s] = g[s].m ? r : 0.f;
        }
      } else {
#pragma unroll 1
        for (int i = 0; i < kResChunks; ++i) {
          if (i * 16 >= C) break;   // wave-uniform
          const int c = i * 16 + l;
          const bool ok = c < C;
          const int cc = ok ? c : 0;
          float t[kResSteps][5];
#pragma unroll
          for (int s = 0; s < kResSteps; ++s) {
#pragma unroll
            for (int k = 0; k < 5; ++k) t[s][k] = 0.f;
            if (g[s].m) {
              t[s][0] = r00[s][cc];
              t[s][1] = r00[s][sx[s] + cc];
              t[s][2] = r00[s][sy[s] + cc];
              t[s][3] = r00[s][sy[s] + sx[s] + cc];
              t[s][4] = src_b[(size_t)pt[s] * C + cc];
            }
          }
#pragma unroll
          for (int s = 0; s < kResSteps; ++s) {
            const float fv = ((t[s][0] * w00[s] + t[s][1] * w01[s]) + t[s][2] * w10[s]) + t[s][3] * w11[s];
            const float d = (ok && g[s].m) ? fv - t[s][4] : 0.f;
            sq[s] += d * d;
            ab[s] += fabsf(d);
          }
        }
      }

#pragma unroll
      for (int s = 0; s < kResSteps; ++s) {
        const float tq = row16_sum(sq[s]), ta = row16_sum(ab[s]);
        if (l == 0 && valid[s]) {
          const size_t o = (size_t)vb * N + pt[s];
          a.sq[o] = tq;
          a.ab[o] = ta;
          a.mask[o] = g[s].m ? (unsigned char)1 : (unsigned char)0;
          if (a.proj != nullptr) {
            // in the mask px = x0 + dx exactly (dx = px - floor(px) is exact there); elsewhere unspecified: zeros
            a.proj[2 * o] = (float)g[s].x0 + g[s].dx;
            a.proj[2 * o + 1] = (float)g[s].y0 + g[s].dy;
          }
        }
      }
    }
  }
}

// one workgroup per (window, frame); the order depends on N alone
__global__ __launch_bounds__(kSumThreads) void ba_residual_sums_kernel(const float* __restrict__ sq, const float* __restrict__ ab,
                                                                       const unsigned char* __restrict__ mask, float* __restrict__ sums,
                                                                       int N) {
  __shared__ float s_sq[kSumThreads], s_ab[kSumThreads], s_mx[kSumThreads];
  __shared__ int s_n[kSumThreads];
  const int t = threadIdx.x;
  const size_t o = (size_t)blockIdx.x * N;
  float a0 = 0.f, a1 = 0.f, mx = 0.f;
  int cnt = 0;
#pragma unroll 4
  for (int i = t; i < N; i += kSumThreads) {
    const float q = sq[o + i];
    a0 += q;
    a1 += ab[o + i];
    cnt += mask[o + i];
    mx = fmaxf(mx, q);
  }
  s_sq[t] = a0;
  s_ab[t] = a1;
  s_mx[t] = mx;
  s_n[t] = cnt;
  for (int h = kSumThreads / 2; h >= 1; h >>= 1) {
    __syncthreads();
    if (t < h) {
      s_sq[t] += s_sq[t + h];
      s_ab[t] += s_ab[t + h];
      s_mx[t] = fmaxf(s_mx[t], s_mx[t + h]);
      s_n[t] += s_n[t + h];
    }
  }
  if (t == 0) {
    float* out = sums + (size_t)blockIdx.x * 4;
    out[0] = s_sq[0];
    out[1] = s_ab[0];
    out[2] = (float)s_n[0];
    out[3] = s_mx[0];
  }
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// the shapes the assembly pass launches a gather for (plan.hpp: plan_gather_steps; the C = 128 kernels take every K their plan
// admits): banet_ba_residual_f32 refuses the others with the assembly's code although its own kernel has no such limit
int residual_shape_supported(const banet_level_t* lv) {
  if ((lv->C & 1) && lv->C > 128) return BANET_ERR_UNSUPPORTED;
  if ((lv->K & 1) && lv->K > 128) return BANET_ERR_UNSUPPORTED;
  return BANET_OK;
}

int launch_residual(const banet_level_t* lv, const float* R, const float* T, const float* Wc, const banet_residual_out_t* out,
                    hipStream_t s) {
  ResidualArgs a;
  a.lv = *lv;
  a.R = R;
  a.T = T;
  a.Wc = Wc;
  a.sq = out->sq;
  a.ab = out->ab;
  a.mask = out->mask;
  a.proj = out->proj;
  a.pairs = npairs(lv);
  a.units = (lv->N + kResUnitPts - 1) / kResUnitPts;
  // one resident round of 8 workgroups per CU, split over the windows; the grid enters no result
  const int want = (a.units + kNumWaves - 1) / kNumWaves;
  int G = (num_cus() * 8 + lv->B - 1) / lv->B;
  if (G > want) G = want;
  if (G < 1) G = 1;
  const dim3 grid(G, lv->B), block(kBlock);
  // 16-byte loads need 16-byte aligned rows (C = 128: every row of a 16-byte aligned tensor is); anything else takes the plain path
  const bool c128 = lv->C == 128 && aligned16(lv->src) && aligned16(lv->tgt);
  const int km = lv->K == 0 ? 0 : (c128 && lv->K == 128 && aligned16(lv->basis)) ? 1 : 2;
  if (c128 && km == 0) hipLaunchKernelGGL((ba_residual_kernel<true, 0>), grid, block, 0, s, a);
  else if (c128 && km == 1) hipLaunchKernelGGL((ba_residual_kernel<true, 1>), grid, block, 0, s, a);
  else if (c128) hipLaunchKernelGGL((ba_residual_kernel<true, 2>), grid, block, 0, s, a);
  else if (km == 0) hipLaunchKernelGGL((ba_residual_kernel<false, 0>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((ba_residual_kernel<false, 2>), grid, block, 0, s, a);
  if (hipGetLastError() != hipSuccess) return BANET_ERR_LAUNCH;
  if (out->sums != nullptr) {
    hipLaunchKernelGGL(ba_residual_sums_kernel, dim3(lv->B * a.pairs), dim3(kSumThreads), 0, s, out->sq, out->ab, out->mask, out->sums,
                       lv->N);
    if (hipGetLastError() != hipSuccess) return BANET_ERR_LAUNCH;
  }
  return BANET_OK;
}

}  // namespace banet
