// Dense adjoint (driver, derivation and the kernel list in launch order: adjoint.hip): the target-cell lists -- the three-launch
// scan, adj_fill_kernel and, in fold mode, adj_cellsort_kernel / adj_bigcell_kernel.  The deterministic sample-stats gradient
// (sstats.hip) builds its lists with the same scan and fill.
#include "adjoint_common.hpp"

namespace banet {
namespace adj {

namespace {

// ---- target cell lists ---------------------------------------------------------------------------------------------
// Exclusive scan of the per-cell counts of every window, in three small launches (chunk sums -> scan of the chunk sums -> scan
// inside the chunks): 1024 cells per 256-thread workgroup.  (A one-workgroup-per-window scan took 0.76 ms at 640x480.)

__global__ __launch_bounds__(256) void adj_scan_sums_kernel(const int* __restrict__ cnt, int* __restrict__ chunk_sum, int HW, int nchunks) {
  __shared__ int sRed[4];
  const int b = blockIdx.y, ch = blockIdx.x, tid = threadIdx.x;
  const int* __restrict__ c = cnt + (size_t)b * HW;
  int s = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int i = ch * kScanChunk + 4 * tid + e;
    s += i < HW ? c[i] : 0;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
  if ((tid & 63) == 0) sRed[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) chunk_sum[(size_t)b * nchunks + ch] = (sRed[0] + sRed[1]) + (sRed[2] + sRed[3]);
}

__global__ __launch_bounds__(kScanThreads) void adj_scan_offsets_kernel(int* __restrict__ chunk_sum, int nchunks) {
  __shared__ int sSum[kScanThreads];
  const int b = blockIdx.x, tid = threadIdx.x;
  int* __restrict__ c = chunk_sum + (size_t)b * nchunks;
  int carry = 0;
  for (int base = 0; base < nchunks; base += kScanThreads) {     // in place: chunk sums -> exclusive offsets
    const int i = base + tid;
    const int v = i < nchunks ? c[i] : 0;
    sSum[tid] = v;
    __syncthreads();
    for (int d = 1; d < kScanThreads; d <<= 1) {
      const int t = tid >= d ? sSum[tid - d] : 0;
      __syncthreads();
      sSum[tid] += t;
      __syncthreads();
    }
    if (i < nchunks) c[i] = carry + sSum[tid] - v;
    carry += sSum[kScanThreads - 1];
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void adj_scan_apply_kernel(const int* __restrict__ cnt, const int* __restrict__ chunk_off,
                                                             int* __restrict__ start, int* __restrict__ cursor, int HW, int nchunks) {
  __shared__ int sSum[256];
  const int b = blockIdx.y, ch = blockIdx.x, tid = threadIdx.x;
  const int* __restrict__ c = cnt + (size_t)b * HW;
  int v[4], s = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int i = ch * kScanChunk + 4 * tid + e;
    v[e] = i < HW ? c[i] : 0;
    s += v[e];
  }
  sSum[tid] = s;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    const int t = tid >= d ? sSum[tid - d] : 0;
    __syncthreads();
    sSum[tid] += t;
    __syncthreads();
  }
  int run = chunk_off[(size_t)b * nchunks + ch] + sSum[tid] - s;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int i = ch * kScanChunk + 4 * tid + e;
    if (i < HW) {
      start[2 * ((size_t)b * HW + i)] = run;        // (start, count) pairs: one 8-byte load per cell in adj_map_kernel
      start[2 * ((size_t)b * HW + i) + 1] = v[e];
      cursor[(size_t)b * HW + i] = run;
    }
    run += v[e];
  }
}

__global__ void adj_fill_kernel(const float* __restrict__ frac, int* __restrict__ cursor, int* __restrict__ list, int N, int HW) {
  const int b = blockIdx.y, n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const int key = __float_as_int(frac[((size_t)b * N + n) * kFrac]);
  if (key < 0) return;
  const int slot = atomicAdd(&cursor[(size_t)b * HW + key], 1);   // the consumer orders each cell's entries itself
  list[(size_t)b * N + slot] = n;
}

// One thread per target cell: order the cell's pixel list (adj_fill_kernel's slots come from an atomic cursor) and write the
// records in list order, key replaced by the pixel index.  Fuller cells (a collapsed warp) go to the big-cell queue.
__global__ void adj_cellsort_kernel(const int2* __restrict__ cs, int* __restrict__ list, const float* __restrict__ frac,
                                    float* __restrict__ lrec, int2* __restrict__ lidx, int* __restrict__ bigq, int N, int HW, int W,
                                    int bigq_cap) {
  const int b = blockIdx.y, cell = blockIdx.x * blockDim.x + threadIdx.x;
  if (cell >= HW) return;
  const int2 v = cs[(size_t)b * HW + cell];
  const int s0 = v.x, L = v.y;
  if (L == 0) return;
  int* __restrict__ li = list + (size_t)b * N + s0;
  if (L > kSortSerial) {
    const int slot = atomicAdd(&bigq[0], 1);
    if (slot < bigq_cap) bigq[1 + slot] = b * HW + cell;     // (cap = every possible big cell: never exceeded)
    return;
  }
  for (int i = 1; i < L; ++i) {
    const int key = li[i];
    int j = i - 1;
    while (j >= 0 && li[j] > key) {
      li[j + 1] = li[j];
      --j;
    }
    li[j + 1] = key;
  }
  const float* __restrict__ fr = frac + (size_t)b * N * kFrac;
  float* __restrict__ lr = lrec + ((size_t)b * N + s0) * kFrac;
  int2* __restrict__ lx = lidx + (size_t)b * N + s0;
  const int cy = cell / W, cxy = (cell - cy * W) | (cy << 16);      // (W, H < 65536)
  for (int i = 0; i < L; ++i) {
    const int n = li[i];
    const f32x4 r0 = *reinterpret_cast<const f32x4*>(fr + (size_t)n * kFrac), r1 = *reinterpret_cast<const f32x4*>(fr + (size_t)n * kFrac + 4);
    *reinterpret_cast<f32x4*>(lr + (size_t)i * kFrac) = f32x4{__int_as_float(n), r0[1], r0[2], r0[3]};
    *reinterpret_cast<f32x4*>(lr + (size_t)i * kFrac + 4) = r1;
    lx[i] = make_int2(n, cxy);
  }
}

// One workgroup per queued cell: rank sort through list2 (pixel indices are distinct), then the records.  O(L^2 / 256) -- only a
// degenerate warp (hundreds of pixels in one texel cell) gets here; adj_map_kernel's per-texel selection had the same order.
__global__ __launch_bounds__(256) void adj_bigcell_kernel(const int2* __restrict__ cs, int* __restrict__ list, int* __restrict__ list2,
                                                          const float* __restrict__ frac, float* __restrict__ lrec,
                                                          int2* __restrict__ lidx, const int* __restrict__ bigq, int N, int HW, int W,
                                                          int bigq_cap) {
  const int nbig = min(bigq[0], bigq_cap);
  for (int qi = blockIdx.x; qi < nbig; qi += gridDim.x) {
    const int gc = bigq[1 + qi], b = gc / HW;
    const int2 v = cs[gc];
    const int s0 = v.x, L = v.y;
    int* __restrict__ li = list + (size_t)b * N + s0;
    int* __restrict__ lo = list2 + (size_t)b * N + s0;
    for (int e = threadIdx.x; e < L; e += 256) {
      const int me = li[e];
      int rank = 0;
      for (int j = 0; j < L; ++j) rank += li[j] < me ? 1 : 0;
      lo[rank] = me;
    }
    __syncthreads();
    const float* __restrict__ fr = frac + (size_t)b * N * kFrac;
    float* __restrict__ lr = lrec + ((size_t)b * N + s0) * kFrac;
    int2* __restrict__ lx = lidx + (size_t)b * N + s0;
    const int cell = gc - b * HW, cy = cell / W, cxy = (cell - cy * W) | (cy << 16);
    for (int e = threadIdx.x; e < L; e += 256) {
      const int n = lo[e];
      const f32x4 r0 = *reinterpret_cast<const f32x4*>(fr + (size_t)n * kFrac), r1 = *reinterpret_cast<const f32x4*>(fr + (size_t)n * kFrac + 4);
      *reinterpret_cast<f32x4*>(lr + (size_t)e * kFrac) = f32x4{__int_as_float(n), r0[1], r0[2], r0[3]};
      *reinterpret_cast<f32x4*>(lr + (size_t)e * kFrac + 4) = r1;
      lx[e] = make_int2(n, cxy);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < L; e += 256) li[e] = lo[e];     // (the list itself in order too: diagnostics, the old per-texel path)
    __syncthreads();
  }
}

}  // namespace

void launch_cell_scan(const int* cnt, int* start, int* cursor, int* chunk_tmp, int B, int HW, hipStream_t s) {
  const int nchunks = (HW + kScanChunk - 1) / kScanChunk;
  hipLaunchKernelGGL(adj_scan_sums_kernel, dim3(nchunks, B), dim3(256), 0, s, cnt, chunk_tmp, HW, nchunks);
  hipLaunchKernelGGL(adj_scan_offsets_kernel, dim3(B), dim3(kScanThreads), 0, s, chunk_tmp, nchunks);
  hipLaunchKernelGGL(adj_scan_apply_kernel, dim3(nchunks, B), dim3(256), 0, s, cnt, chunk_tmp, start, cursor, HW, nchunks);
}

void launch_adj_fill(const float* frac, int* cursor, int* list, int B, int N, int HW, hipStream_t s) {
  hipLaunchKernelGGL(adj_fill_kernel, dim3((N + 255) / 256, B), dim3(256), 0, s, frac, cursor, list, N, HW);
}

void launch_adj_cellsort(const AdjArgs& a, int bigq_cap, hipStream_t s) {
  const int B = a.lv.B, N = a.lv.N, W = a.lv.W, HW = a.lv.H * W;
  const int2* cs = reinterpret_cast<const int2*>(a.start);
  hipLaunchKernelGGL(adj_cellsort_kernel, dim3((HW + 255) / 256, B), dim3(256), 0, s, cs, a.list, a.frac, a.lrec, a.lidx, a.bigq, N, HW, W,
                     bigq_cap);
  hipLaunchKernelGGL(adj_bigcell_kernel, dim3(64), dim3(256), 0, s, cs, a.list, a.list2, a.frac, a.lrec, a.lidx, a.bigq, N, HW, W, bigq_cap);
}

}  // namespace adj
}  // namespace banet
