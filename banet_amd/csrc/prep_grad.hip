// Adjoints of the per-level preparation kernels of prep.hip (what tf.gradients derives for bundlenet.py:320,343-344,385,397):
//   resampler  ddata [B,H,W,C] and dwarp [B,N,2] of ba_resample_kernel, both modes (tf.contrib.resampler / interpolate2d2)
//   depth out  dinit [B,N], dbasis [B,N,K] and dWc [B,K] of ba_depth_output_kernel
// No float atomics anywhere (global or LDS): the map gradient is gathered per texel from point lists that a stable radix sort
// of the points' cell keys put in ascending point order; dWc is per-block partials folded in a fixed order.  Everything is
// enqueued on the caller's stream with no allocation and no synchronisation (graph-capturable).
#include "kernels.hpp"

namespace banet {

namespace {

constexpr int kRsTile = 1024;    // radix-sort keys per workgroup (256 threads x 4 rounds)
constexpr int kRsScan = 1024;    // threads of the per-window scan of the digit histograms
constexpr int kNoTap = 0x7fffffff;

// ---- the bilinear footprint of one point, as ba_resample_kernel computes it -----------------------------------------------
// The four taps of a point hang off its cell (cx, cy) = (floor x, floor y): tap (i, j) is texel (cx + i, cy + j) (mode 1: each
// coordinate clamped into the image).  Cells run over [-1, W-1] x [-1, H-1] (mode 1: the floor clamped into that range, which
// leaves the tap texels unchanged), key = (cy + 1) (W + 1) + cx + 1; a point mode 0 does not sample gets key (H + 1)(W + 1).
// Tap numbering = the forward's sum order: mode 0 a(0,0) b(1,1) c(0,1) d(1,0); mode 1 00(0,0) 01(1,0) 10(0,1) 11(1,1).
struct Foot {
  bool ok;                    // sampled (mode 0); always true in mode 1
  int cx, cy;                 // cell
  float w[4];                 // tap weights in tap order
  float dwx[4], dwy[4];       // d w / d x, d w / d y (floor held constant: the one-sided derivative at an integer coordinate)
};

__device__ __forceinline__ Foot footprint(float x, float y, int H, int W, int mode) {
  Foot f;
  if (mode == 0) {
    f.ok = (x > -1.f) && (y > -1.f) && (x < (float)W) && (y < (float)H);
    const float xs = f.ok ? x : 0.f, ys = f.ok ? y : 0.f;
    const float fxf = floorf(xs), fyf = floorf(ys);
    const float dx = (fxf + 1.f) - xs, dy = (fyf + 1.f) - ys;
    f.cx = (int)fxf;
    f.cy = (int)fyf;
    f.w[0] = dx * dy;                  // a (fx, fy)
    f.w[1] = (1.f - dx) * (1.f - dy);  // b (cx, cy)
    f.w[2] = dx * (1.f - dy);          // c (fx, cy)
    f.w[3] = (1.f - dx) * dy;          // d (cx, fy)
    // d dx / d x = -1, d dy / d y = -1
    f.dwx[0] = -dy, f.dwx[1] = 1.f - dy, f.dwx[2] = -(1.f - dy), f.dwx[3] = dy;
    f.dwy[0] = -dx, f.dwy[1] = 1.f - dx, f.dwy[2] = dx, f.dwy[3] = -(1.f - dx);
  } else {
    f.ok = true;
    const float x0f = floorf(x), y0f = floorf(y);
    const float dx = x - x0f, dy = y - y0f;
    f.w[0] = (1.f - dx) * (1.f - dy);
    f.w[1] = dx * (1.f - dy);
    f.w[2] = (1.f - dx) * dy;
    f.w[3] = dx * dy;
    f.dwx[0] = -(1.f - dy), f.dwx[1] = 1.f - dy, f.dwx[2] = -dy, f.dwx[3] = dy;
    f.dwy[0] = -(1.f - dx), f.dwy[1] = -dx, f.dwy[2] = 1.f - dx, f.dwy[3] = dx;
    // NaN / inf: index 0 / saturated, as ba_resample_kernel; then into the cell range
    const float xc = (x0f == x0f) ? fminf(fmaxf(x0f, -1e9f), 1e9f) : 0.f, yc = (y0f == y0f) ? fminf(fmaxf(y0f, -1e9f), 1e9f) : 0.f;
    f.cx = min(max((int)xc, -1), W - 1);
    f.cy = min(max((int)yc, -1), H - 1);
  }
  return f;
}

__device__ __forceinline__ int tap_of(int mode, int i, int j) { return mode == 0 ? (i == j ? i : 2 + i) : i + 2 * j; }

// ---- stable LSD radix sort of the cell keys, 8 bits per pass, values = point indices ------------------------------------------
__global__ __launch_bounds__(256) void rg_keys_kernel(const float* __restrict__ warp, int* __restrict__ key, int* __restrict__ val, int N,
                                                      int H, int W, int mode) {
  const int b = blockIdx.y, n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const size_t i = (size_t)b * N + n;
  const Foot f = footprint(warp[2 * i], warp[2 * i + 1], H, W, mode);
  key[i] = f.ok ? (f.cy + 1) * (W + 1) + f.cx + 1 : (H + 1) * (W + 1);
  val[i] = n;
}

// per (window, tile) digit counts, digit-major: hist[b][d][tile] (LDS integer atomics only)
__global__ __launch_bounds__(256) void rg_hist_kernel(const int* __restrict__ key, int* __restrict__ hist, int N, int ntiles, int shift) {
  __shared__ int sH[256];
  const int b = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
  sH[tid] = 0;
  __syncthreads();
  for (int r = 0; r < kRsTile / 256; ++r) {
    const int i = tile * kRsTile + r * 256 + tid;
    if (i < N) atomicAdd(&sH[(key[(size_t)b * N + i] >> shift) & 255], 1);
  }
  __syncthreads();
  hist[((size_t)b * 256 + tid) * ntiles + tile] = sH[tid];
}

// exclusive scan of one window's 256 x ntiles counts, in place
__global__ __launch_bounds__(kRsScan) void rg_scan_kernel(int* __restrict__ hist, int len) {
  __shared__ int sS[kRsScan];
  const int b = blockIdx.x, tid = threadIdx.x;
  int* __restrict__ h = hist + (size_t)b * len;
  int carry = 0;
  for (int base = 0; base < len; base += kRsScan) {
    const int i = base + tid;
    const int v = i < len ? h[i] : 0;
    sS[tid] = v;
    __syncthreads();
    for (int d = 1; d < kRsScan; d <<= 1) {
      const int t = tid >= d ? sS[tid - d] : 0;
      __syncthreads();
      sS[tid] += t;
      __syncthreads();
    }
    if (i < len) h[i] = carry + sS[tid] - v;
    carry += sS[kRsScan - 1];
    __syncthreads();
  }
}

// scatter: destination = scanned (digit, tile) offset + rank among the tile's earlier keys with the same digit.  The rank inside a
// wave comes from ballots (lanes of equal digit), across the tile's waves and rounds from per-wave counts in LDS: stable.
__global__ __launch_bounds__(256) void rg_scatter_kernel(const int* __restrict__ kin, const int* __restrict__ vin, int* __restrict__ kout,
                                                         int* __restrict__ vout, const int* __restrict__ hist, int N, int ntiles,
                                                         int shift) {
  __shared__ int sBase[256];
  __shared__ int sCnt[kNumWaves][256];
  const int b = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  sBase[tid] = hist[((size_t)b * 256 + tid) * ntiles + tile];
  for (int k = 0; k < kNumWaves; ++k) sCnt[k][tid] = 0;
  __syncthreads();
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int r = 0; r < kRsTile / 256; ++r) {
    const int i = tile * kRsTile + r * 256 + tid;
    const bool valid = i < N;
    const int k = valid ? kin[(size_t)b * N + i] : 0, v = valid ? vin[(size_t)b * N + i] : 0;
    const int d = (k >> shift) & 255;
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const bool on = (d >> bit) & 1;
      const unsigned long long m = __ballot(on);
      peers &= on ? m : ~m;
    }
    const int rank = __popcll(peers & below);
    if (valid && rank == 0) sCnt[w][d] = __popcll(peers);
    __syncthreads();
    if (valid) {
      int pos = sBase[d] + rank;
      for (int q = 0; q < w; ++q) pos += sCnt[q][d];
      kout[(size_t)b * N + pos] = k;
      vout[(size_t)b * N + pos] = v;
    }
    __syncthreads();
    int add = 0;
    for (int q = 0; q < kNumWaves; ++q) {
      add += sCnt[q][tid];
      sCnt[q][tid] = 0;
    }
    sBase[tid] += add;
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void rg_zero_kernel(int2* __restrict__ cs, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) cs[i] = make_int2(0, 0);
}

// [start, end) of every cell's run in the sorted keys (cells without points keep (0, 0))
__global__ __launch_bounds__(256) void rg_bounds_kernel(const int* __restrict__ key, int2* __restrict__ cs, int N, int ncells) {
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const int* __restrict__ k = key + (size_t)b * N;
  const int c = k[i];
  if (c >= ncells) return;
  int2* __restrict__ cb = cs + (size_t)b * ncells;
  if (i == 0 || k[i - 1] != c) cb[c].x = i;
  if (i == N - 1 || k[i + 1] != c) cb[c].y = i + 1;
}

// ---- ddata: one wave per texel, lanes over channels -------------------------------------------------------------------------
// The texel's (cell, tap) sources are merged in ascending (point, tap) order: every cell's run is in ascending point order, and a
// point that lands on the texel through two taps (mode 1, clamped) adds them in tap order.  acc starts at the old value
// (accumulate) or +0 (overwrite), so overwriting is bit-identical to accumulating into zeros.
template <int CJ>
__global__ __launch_bounds__(256) void rg_map_kernel(const float* __restrict__ warp, const float* __restrict__ gout, const int* __restrict__ sval,
                                                     const int2* __restrict__ cs, float* __restrict__ ddata, int N, int C, int H, int W,
                                                     int mode, int overwrite) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int wv = blockIdx.x * kNumWaves + (threadIdx.x >> 6), nw = gridDim.x * kNumWaves;
  const int HW = H * W, ncells = (H + 1) * (W + 1);
  const int* __restrict__ sv = sval + (size_t)b * N;
  const int2* __restrict__ cb = cs + (size_t)b * ncells;
  const float* __restrict__ wp = warp + (size_t)b * N * 2;
  const float* __restrict__ g = gout + (size_t)b * N * C;
  for (int t = wv; t < HW; t += nw) {
    const int Y = t / W, X = t - Y * W;
    // per axis: slot 0 (X, tap 0), slot 1 (X - 1, tap 1); mode 1 only: slot 2 (-1, tap 0) on the first and slot 3 (W - 1, tap 1)
    // on the last column (the clamped taps)
    const int xs[4] = {X, X - 1, -1, W - 1}, ys[4] = {Y, Y - 1, -1, H - 1};
    const bool xv[4] = {true, true, mode == 1 && X == 0, mode == 1 && X == W - 1};
    const bool yv[4] = {true, true, mode == 1 && Y == 0, mode == 1 && Y == H - 1};
    int pos[16], end[16], tap[16], head[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int a = q & 3, c = q >> 2;
      pos[q] = 0, end[q] = 0, tap[q] = tap_of(mode, a & 1, c & 1), head[q] = kNoTap;
      if (xv[a] && yv[c]) {
        const int2 r = cb[(ys[c] + 1) * (W + 1) + xs[a] + 1];
        pos[q] = r.x, end[q] = r.y;
        if (r.x < r.y) head[q] = sv[r.x] * 4 + tap[q];
      }
    }
    float acc[CJ];
    float* __restrict__ o = ddata + ((size_t)b * HW + t) * C;
#pragma unroll
    for (int j = 0; j < CJ; ++j) {
      const int c = lane + 64 * j;
      acc[j] = (!overwrite && c < C) ? o[c] : 0.f;
    }
    for (;;) {
      int best = kNoTap, bq = 0;
#pragma unroll
      for (int q = 0; q < 16; ++q)
        if (head[q] < best) best = head[q], bq = q;
      if (best == kNoTap) break;
#pragma unroll
      for (int q = 0; q < 16; ++q)
        if (q == bq) {
          ++pos[q];
          head[q] = pos[q] < end[q] ? sv[pos[q]] * 4 + tap[q] : kNoTap;
        }
      const int n = best >> 2, tp = best & 3;
      const Foot f = footprint(wp[2 * n], wp[2 * n + 1], H, W, mode);
      const float wt = tp == 0 ? f.w[0] : tp == 1 ? f.w[1] : tp == 2 ? f.w[2] : f.w[3];
      const float* __restrict__ gr = g + (size_t)n * C;
#pragma unroll
      for (int j = 0; j < CJ; ++j) {
        const int c = lane + 64 * j;
        if (c < C) acc[j] = fmaf(wt, gr[c], acc[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < CJ; ++j) {
      const int c = lane + 64 * j;
      if (c < C) o[c] = acc[j];
    }
  }
}

// ---- dwarp: one wave per point, lanes over channels, fixed-order wave reduction -------------------------------------------------
__global__ __launch_bounds__(256) void rg_warp_kernel(const float* __restrict__ data, const float* __restrict__ warp,
                                                      const float* __restrict__ gout, float* __restrict__ dwarp, int N, int C, int H,
                                                      int W, int mode) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int wv = blockIdx.x * kNumWaves + (threadIdx.x >> 6), nw = gridDim.x * kNumWaves;
  const float* __restrict__ img = data + (size_t)b * H * W * C;
  for (int n = wv; n < N; n += nw) {
    const size_t i = (size_t)b * N + n;
    const Foot f = footprint(warp[2 * i], warp[2 * i + 1], H, W, mode);
    float sx = 0.f, sy = 0.f;
    if (f.ok) {
      const float* p[4];
      float m[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int ti = mode == 0 ? (q == 0 || q == 2 ? 0 : 1) : (q & 1);
        const int tj = mode == 0 ? (q == 0 || q == 3 ? 0 : 1) : (q >> 1);
        const int xi = f.cx + ti, yi = f.cy + tj;
        m[q] = (mode == 1 || (xi >= 0 && yi >= 0 && xi <= W - 1 && yi <= H - 1)) ? 1.f : 0.f;
        p[q] = img + ((size_t)min(max(yi, 0), H - 1) * W + min(max(xi, 0), W - 1)) * C;
      }
      const float* __restrict__ g = gout + i * C;
      for (int c = lane; c < C; c += 64) {
        const float v0 = m[0] * p[0][c], v1 = m[1] * p[1][c], v2 = m[2] * p[2][c], v3 = m[3] * p[3][c];
        const float gc = g[c];
        sx = fmaf(gc, ((f.dwx[0] * v0 + f.dwx[1] * v1) + f.dwx[2] * v2) + f.dwx[3] * v3, sx);
        sy = fmaf(gc, ((f.dwy[0] * v0 + f.dwy[1] * v1) + f.dwy[2] * v2) + f.dwy[3] * v3, sy);
      }
    }
    sx = wave_sum(sx);
    sy = wave_sum(sy);
    if (lane == 0) dwarp[2 * i] = sx, dwarp[2 * i + 1] = sy;
  }
}

// ---- depth output: dinit = gout, dbasis = gout W^T (one wave per row), dWc = sum_n gout basis (block partials + fixed fold) ----
__global__ __launch_bounds__(256) void dog_rows_kernel(const float* __restrict__ Wc, const float* __restrict__ gout, float* __restrict__ dinit,
                                                       float* __restrict__ dbasis, int N, int K, int overwrite) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int wv = blockIdx.x * kNumWaves + (threadIdx.x >> 6), nw = gridDim.x * kNumWaves;
  const float* __restrict__ wb = Wc + (size_t)b * K;
  for (int n = wv; n < N; n += nw) {
    const size_t r = (size_t)b * N + n;
    const float gv = gout[r];
    if (dinit && lane == 0) dinit[r] = overwrite ? gv : dinit[r] + gv;
    if (dbasis) {
      float* __restrict__ o = dbasis + r * K;
      for (int k = lane; k < K; k += 64) o[k] = overwrite ? gv * wb[k] : o[k] + gv * wb[k];
    }
  }
}

__global__ __launch_bounds__(256) void dog_part_kernel(const float* __restrict__ basis, const float* __restrict__ gout, float* __restrict__ part,
                                                       int N, int K, int rows) {
  const int b = blockIdx.y, gi = blockIdx.x, G = gridDim.x;
  const int n0 = gi * rows, n1 = min(N, n0 + rows);
  for (int k = threadIdx.x; k < K; k += blockDim.x) {
    float acc = 0.f;
    for (int n = n0; n < n1; ++n) acc = fmaf(gout[(size_t)b * N + n], basis[((size_t)b * N + n) * K + k], acc);
    part[((size_t)b * G + gi) * K + k] = acc;
  }
}

__global__ __launch_bounds__(256) void dog_fold_kernel(const float* __restrict__ part, float* __restrict__ dWc, int G, int K, int overwrite) {
  const int b = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
  if (k >= K) return;
  float s = overwrite ? 0.f : dWc[(size_t)b * K + k];
  for (int gi = 0; gi < G; ++gi) s += part[((size_t)b * G + gi) * K + k];
  dWc[(size_t)b * K + k] = s;
}

// ---- workspace plans ----------------------------------------------------------------------------------------------------
struct RgPlan {
  int ntiles, passes, ncells;
  size_t off_k0, off_v0, off_k1, off_v1, off_hist, off_cs, bytes;
};

void rg_plan(int B, int N, int H, int W, RgPlan* pl) {
  pl->ntiles = (N + kRsTile - 1) / kRsTile;
  pl->ncells = (H + 1) * (W + 1);
  int bits = 1;
  while ((pl->ncells >> bits) != 0) ++bits;     // keys 0 .. ncells (the unsampled sentinel)
  pl->passes = (bits + 7) / 8;
  Arena ar;
  pl->off_k0 = ar.take((size_t)B * N * 4);
  pl->off_v0 = ar.take((size_t)B * N * 4);
  pl->off_k1 = ar.take((size_t)B * N * 4);
  pl->off_v1 = ar.take((size_t)B * N * 4);
  pl->off_hist = ar.take((size_t)B * 256 * pl->ntiles * 4);
  pl->off_cs = ar.take((size_t)B * pl->ncells * 8);
  pl->bytes = ar.off;
}

int dog_blocks(int N) { return std::max(1, std::min(256, (N + 255) / 256)); }

}  // namespace

bool resample_grad_supported(int B, int N, int C, int H, int W) {
  return C <= 256 && (unsigned long long)B * H * W * C < (1ull << 32) && N < (1 << 28) &&
         (unsigned long long)(H + 1) * (W + 1) < (1ull << 30);
}

size_t resample_grad_workspace_bytes(int B, int N, int C, int H, int W) {
  RgPlan pl;
  rg_plan(B, N, H, W, &pl);
  (void)C;
  return pl.bytes;
}

int launch_resample_grad(const float* data, const float* warp, const float* gout, float* ddata, float* dwarp, int B, int N, int C, int H,
                         int W, int mode, int overwrite, void* ws, hipStream_t s) {
  if (dwarp) {
    const int gx = std::min((N + kNumWaves - 1) / kNumWaves, 4096);
    hipLaunchKernelGGL(rg_warp_kernel, dim3(gx, B), dim3(256), 0, s, data, warp, gout, dwarp, N, C, H, W, mode);
  }
  if (ddata) {
    RgPlan pl;
    rg_plan(B, N, H, W, &pl);
    char* base = static_cast<char*>(ws);
    int* k[2] = {reinterpret_cast<int*>(base + pl.off_k0), reinterpret_cast<int*>(base + pl.off_k1)};
    int* v[2] = {reinterpret_cast<int*>(base + pl.off_v0), reinterpret_cast<int*>(base + pl.off_v1)};
    int* hist = reinterpret_cast<int*>(base + pl.off_hist);
    int2* cs = reinterpret_cast<int2*>(base + pl.off_cs);
    const dim3 gp((N + 255) / 256, B), gt(pl.ntiles, B);
    hipLaunchKernelGGL(rg_keys_kernel, gp, dim3(256), 0, s, warp, k[0], v[0], N, H, W, mode);
    for (int p = 0; p < pl.passes; ++p) {
      const int src = p & 1, dst = src ^ 1;
      hipLaunchKernelGGL(rg_hist_kernel, gt, dim3(256), 0, s, k[src], hist, N, pl.ntiles, 8 * p);
      hipLaunchKernelGGL(rg_scan_kernel, dim3(B), dim3(kRsScan), 0, s, hist, 256 * pl.ntiles);
      hipLaunchKernelGGL(rg_scatter_kernel, gt, dim3(256), 0, s, k[src], v[src], k[dst], v[dst], hist, N, pl.ntiles, 8 * p);
    }
    const int fin = pl.passes & 1;
    const size_t ncs = (size_t)B * pl.ncells;
    hipLaunchKernelGGL(rg_zero_kernel, dim3((unsigned)std::min<size_t>((ncs + 255) / 256, 4096)), dim3(256), 0, s, cs, ncs);
    hipLaunchKernelGGL(rg_bounds_kernel, gp, dim3(256), 0, s, k[fin], cs, N, pl.ncells);
    const int gm = std::max(1, std::min((H * W + kNumWaves - 1) / kNumWaves, (4096 + B - 1) / B));
    const dim3 grid(gm, B), block(256);
    if (C <= 64)
      hipLaunchKernelGGL(rg_map_kernel<1>, grid, block, 0, s, warp, gout, v[fin], cs, ddata, N, C, H, W, mode, overwrite);
    else if (C <= 128)
      hipLaunchKernelGGL(rg_map_kernel<2>, grid, block, 0, s, warp, gout, v[fin], cs, ddata, N, C, H, W, mode, overwrite);
    else if (C <= 192)
      hipLaunchKernelGGL(rg_map_kernel<3>, grid, block, 0, s, warp, gout, v[fin], cs, ddata, N, C, H, W, mode, overwrite);
    else
      hipLaunchKernelGGL(rg_map_kernel<4>, grid, block, 0, s, warp, gout, v[fin], cs, ddata, N, C, H, W, mode, overwrite);
  }
  return hipGetLastError() == hipSuccess ? BANET_OK : BANET_ERR_LAUNCH;
}

size_t depth_output_grad_workspace_bytes(int B, int N, int K) { return align_up((size_t)B * dog_blocks(N) * K * 4, 256); }

int launch_depth_output_grad(const float* basis, const float* Wc, const float* gout, float* dinit, float* dbasis, float* dWc, int B,
                             int N, int K, int overwrite, void* ws, hipStream_t s) {
  if (dinit || dbasis) {
    const int gx = std::min((N + kNumWaves - 1) / kNumWaves, 4096);
    hipLaunchKernelGGL(dog_rows_kernel, dim3(gx, B), dim3(256), 0, s, Wc, gout, dinit, dbasis, N, K, overwrite);
  }
  if (dWc) {
    const int G = dog_blocks(N), rows = (N + G - 1) / G;
    const int threads = std::min(256, (K + 63) / 64 * 64);
    float* part = static_cast<float*>(ws);
    hipLaunchKernelGGL(dog_part_kernel, dim3(G, B), dim3(threads), 0, s, basis, gout, part, N, K, rows);
    hipLaunchKernelGGL(dog_fold_kernel, dim3((K + 255) / 256, B), dim3(256), 0, s, part, dWc, G, K, overwrite);
  }
  return hipGetLastError() == hipSuccess ? BANET_OK : BANET_ERR_LAUNCH;
}

}  // namespace banet
