// Dense adjoint (driver, derivation and the kernel list in launch order: adjoint.hip): the round-6 tile kernels of fold mode
// (BANET_ADJOINT_FOLD_TARGET) -- adj_tile_kernel, adj_tile2_kernel.  The sorted cell lists they walk: adjoint_cells.hip.
#include "adjoint_common.hpp"

namespace banet {
namespace adj {

namespace {

// ---- round 6: the target map's gradient per 8x8 texel tile, without the 3C rows in memory -------------------------------
// Until round 5 every pixel wrote its 3C adjoint row of the sampled [f|gx|gy] vector (1.5 KB), adj_map2_kernel gathered four of
// them per texel into the [f|gx|gy] map adjoint dmap3 (another 1.5 KB per texel, read-modify-write over the iterations) and
// target_map_adjoint4_kernel folded grad_fixed^T once per level: 8+ KB of traffic per pixel and iteration, 30 GB of buffers at 32
// windows of 640x480.  Here ONE wave owns a tile of TW x TH target texels exclusively: it walks the cell lists of the tile and of
// the ring around it ((TW + 3) x (TH + 3) cells: every pixel whose 12-texel footprint -- four bilinear taps plus their
// central-difference neighbours -- touches the tile), recomputes the pixel's channel adjoints (-dd, dgx, dgy) from its source row,
// the 12 target texels of its cell and the eight per-pixel scalars adj_pixel*_kernel left in its record, and accumulates
// grad_fixed^T of them (bundlenet.py:92-100, REFLECT rim -> 0) straight into the tile's accumulators in LDS, in a fixed order
// (cells row-major, ascending pixel index inside a cell): no float atomics between waves, bit-reproducible, and the only thing
// written is the target map's gradient itself -- once per tile.

template <int V> struct VecOf;
template <> struct VecOf<1> { typedef float T; };
template <> struct VecOf<2> { typedef float T __attribute__((ext_vector_type(2))); };
template <int V> __device__ __forceinline__ typename VecOf<V>::T vsplat(float x);
template <> __device__ __forceinline__ float vsplat<1>(float x) { return x; }
template <> __device__ __forceinline__ VecOf<2>::T vsplat<2>(float x) { return VecOf<2>::T{x, x}; }

// CJ x V x 64 >= C: lane owns the V consecutive channels V lane + 64 V j (+ e); V = 2 needs an even C.  One wave per workgroup;
// LDS = (TW TH + 1) CJ V 64 floats, the V accumulators of (texel t, chunk j) of this lane side by side at ((t CJ + j) 64 + lane) V
// (8-byte accesses, conflict-free); slot TW TH is a dummy that takes the footprint texels outside the tile (no branch per
// destination).
// Work items are numbered so that the eight XCDs (workgroup id mod 8) each walk a contiguous range of tiles: the target halo and the
// source rows that neighbouring tiles share then meet in one L2.
// Memory pipeline: the record two pixels ahead, the source row one pixel ahead and the 12 target texels of the next non-empty cell
// are requested at the top of an iteration and a full s_waitcnt vmcnt(0) closes it (after ~300 instructions of arithmetic): the
// loop header then has nothing pending, so the compiler's conservative wait counts at the loop join cannot stall on loads that
// were only just issued (the first version of this kernel did exactly that: 3.4 us per pixel).
__device__ __forceinline__ void wait_vm0() { __builtin_amdgcn_s_waitcnt(0x0F70); }   // vmcnt(0), expcnt / lgkmcnt untouched

template <int CJ, int V, int TW, int TH>
__global__ __launch_bounds__(64) void adj_tile_kernel(const AdjArgs a, int tiles_x, int ntiles, int total, int chunk) {
  typedef typename VecOf<V>::T vec;
  static_assert((TW + 3) * (TH + 3) <= 128, "the tile's cell table is two entries per lane");
  constexpr int kSlotV = CJ * 64;               // vecs per texel slot: accumulator of (texel t, chunk j) of this lane at (t CJ + j) 64 + lane
  extern __shared__ __attribute__((aligned(16))) float sAcc[];
  vec* sAccV = reinterpret_cast<vec*>(sAcc);
  const int lane = threadIdx.x;
  const int kk = blockIdx.x >> 3, work = (blockIdx.x & 7) * chunk + kk;
  if (kk >= chunk || work >= total) return;
  const int b = work / ntiles, tile = work - b * ntiles;
  const int tyi = tile / tiles_x, tx0 = (tile - tyi * tiles_x) * TW, ty0 = tyi * TH;
  const int N = a.lv.N, C = a.lv.C, H = a.lv.H, W = a.lv.W, HW = H * W;
  const float* __restrict__ src_b = a.lv.src + (size_t)b * N * C;
  const float* __restrict__ tgt_b = a.lv.tgt + (size_t)b * HW * C;
  const float* __restrict__ lrec = a.lrec + (size_t)b * N * kFrac;
  const int2* __restrict__ cs = reinterpret_cast<const int2*>(a.start) + (size_t)b * HW;
  bool cok[CJ];
  int coff[CJ];
  vec ga[CJ];
#pragma unroll
  for (int j = 0; j < CJ; ++j) {
    const int c = V * lane + 64 * V * j;
    cok[j] = c < C;
    coff[j] = cok[j] ? c : 0;
    ga[j] = *reinterpret_cast<const vec*>(a.gabs + (size_t)b * C + coff[j]);
    if (!cok[j]) ga[j] = vsplat<V>(0.f);
  }
  for (int i = lane; i < (TW * TH + 1) * kSlotV; i += 64) sAccV[i] = vsplat<V>(0.f);

  // the cells whose pixels can touch the tile: x0 in [tx0 - 2, tx0 + TW], y0 in [ty0 - 2, ty0 + TH], clipped to the image
  const int cxa = max(tx0 - 2, 0), cxb = min(tx0 + TW, W - 1), ncx = cxb - cxa + 1;
  const int cya = max(ty0 - 2, 0), cyb = min(ty0 + TH, H - 1), ncy = cyb - cya + 1, ncell = ncx * ncy;
  int cst[2], ccn[2];
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int id = lane + 64 * e;
    const bool ok = id < ncell;
    const int r = id / ncx, c = id - r * ncx;
    const int2 v = cs[ok ? (cya + r) * W + cxa + c : 0];
    cst[e] = v.x;
    ccn[e] = ok ? v.y : 0;
  }
  unsigned long long q0 = __ballot(ccn[0] > 0), q1 = __ballot(ccn[1] > 0);
  auto next_cell = [&]() -> int {      // pops the id of the next non-empty cell in row-major order, -1 = none
    int id = -1;
    if (q0) {
      id = __builtin_ctzll(q0);
      q0 &= q0 - 1;
    } else if (q1) {
      id = 64 + __builtin_ctzll(q1);
      q1 &= q1 - 1;
    }
    return id;
  };
  auto cell_range = [&](int id, int& s, int& L) {
    const int l = id & 63;
    s = id < 64 ? __builtin_amdgcn_readlane(cst[0], l) : __builtin_amdgcn_readlane(cst[1], l);
    L = id < 64 ? __builtin_amdgcn_readlane(ccn[0], l) : __builtin_amdgcn_readlane(ccn[1], l);
  };
  const unsigned rowB = (unsigned)W * (unsigned)C, laneoff = 0;     // floats per target row
  (void)laneoff;
  auto load_tex = [&](int id, vec (&tx)[4][4][CJ]) {
    const int r0 = id / ncx, cx = cxa + id - r0 * ncx, cy = cya + r0;
    unsigned xo[4], yo[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      xo[k] = (unsigned)min(max(cx - 1 + k, 0), W - 1) * (unsigned)C;
      yo[k] = (unsigned)min(max(cy - 1 + k, 0), H - 1) * rowB;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int cc = 0; cc < 4; ++cc) {
        if ((r == 0 || r == 3) && (cc == 0 || cc == 3)) continue;
        const float* __restrict__ row = tgt_b + (yo[r] + xo[cc]);      // (a window's target map is < 2^32 floats: plan check)
#pragma unroll
        for (int j = 0; j < CJ; ++j) tx[r][cc][j] = *reinterpret_cast<const vec*>(row + coff[j]);
      }
  };
  auto load_rec = [&](int i, f32x4& r0, f32x4& r1) {
    r0 = *reinterpret_cast<const f32x4*>(lrec + (size_t)i * kFrac);
    r1 = *reinterpret_cast<const f32x4*>(lrec + (size_t)i * kFrac + 4);
  };
  auto load_src = [&](int n, vec (&f)[CJ]) {
#pragma unroll
    for (int j = 0; j < CJ; ++j) f[j] = *reinterpret_cast<const vec*>(src_b + (size_t)n * C + coff[j]);
  };
  // the pixels in walking order: the list segments of a row of cells are contiguous (the list is sorted by cell), so the sequence
  // is row by row [start of the row's first cell, end of its last)
  auto row_range = [&](int r, int& rs, int& re) {
    int s2, L2, Lx;
    cell_range(r * ncx, rs, Lx);
    cell_range(r * ncx + ncx - 1, s2, L2);
    re = s2 + L2;
  };
  struct Seq {
    int i, r, re;     // list index (-1: done), its row of cells, the row's end
  };
  auto seq_from = [&](int r0) -> Seq {
    for (int r = r0; r < ncy; ++r) {
      int rs, re;
      row_range(r, rs, re);
      if (rs < re) return Seq{rs, r, re};
    }
    return Seq{-1, ncy, 0};
  };
  auto seq_next = [&](const Seq& q) -> Seq {
    if (q.i < 0) return q;
    if (q.i + 1 < q.re) return Seq{q.i + 1, q.r, q.re};
    return seq_from(q.r + 1);
  };
  Seq p0 = seq_from(0);
  if (p0.i >= 0) {
    vec tex[4][4][CJ], texn[4][4][CJ], f1[CJ], f1n[CJ];
    f32x4 ra0, ra1, rb0 = {0.f, 0.f, 0.f, 0.f}, rb1 = rb0, rc0 = rb0, rc1 = rb0;     // records of this pixel, the next, the one after
    int cur = next_cell(), s, L;
    cell_range(cur, s, L);
    int e = s + L;
    load_rec(p0.i, ra0, ra1);
    Seq p1 = seq_next(p0);
    if (p1.i >= 0) load_rec(p1.i, rb0, rb1);
    load_tex(cur, tex);
    load_src(__builtin_amdgcn_readfirstlane(__float_as_int(ra0[0])), f1);
    int nxt = next_cell(), sn = 0, Ln = 0;        // the following non-empty cell: its texels travel while this cell's pixels are worked on
    bool want_texn = false;
    if (nxt >= 0) {
      cell_range(nxt, sn, Ln);
      want_texn = true;
    }
    wait_vm0();
    while (true) {
      const int n1 = __builtin_amdgcn_readfirstlane(__float_as_int(rb0[0]));
      const Seq p2 = seq_next(p1);
      if (p2.i >= 0) load_rec(p2.i, rc0, rc1);
      if (p1.i >= 0) load_src(n1, f1n);
      if (want_texn) {
        load_tex(nxt, texn);
        want_texn = false;
      }
      // ---- this pixel: cell (x0, y0), fractions, the per-pixel scalars of adj_pixel*_kernel
      const int r0 = cur / ncx, x0 = cxa + cur - r0 * ncx, y0 = cya + r0;
      const float ax = ra0[1], ay = ra0[2], dg1 = ra0[3], dg2 = ra1[0], dM11 = ra1[1], dM12 = ra1[2], dM22 = ra1[3];
      float cf[4], cgx[4], cgy[4];      // tap weight x (in image, gx defined, gy defined): adj_pixel*_kernel's wt, fin, hx, hy
      vec Sf[CJ], Sgx[CJ], Sgy[CJ];
      if (x0 >= 1 && y0 >= 1 && x0 + 2 <= W - 1 && y0 + 2 <= H - 1) {      // the whole footprint inside the image, off the rim
        const float bx = 1.f - ax, by = 1.f - ay;
        cf[0] = bx * by, cf[1] = ax * by, cf[2] = bx * ay, cf[3] = ax * ay;
#pragma unroll
        for (int t = 0; t < 4; ++t) cgx[t] = cgy[t] = 0.5f * cf[t];
#pragma unroll
        for (int j = 0; j < CJ; ++j) {
          Sf[j] = cf[0] * tex[1][1][j] + cf[1] * tex[1][2][j] + cf[2] * tex[2][1][j] + cf[3] * tex[2][2][j];
          Sgx[j] = cgx[0] * (tex[1][2][j] - tex[1][0][j]) + cgx[1] * (tex[1][3][j] - tex[1][1][j]) + cgx[2] * (tex[2][2][j] - tex[2][0][j]) +
                   cgx[3] * (tex[2][3][j] - tex[2][1][j]);
          Sgy[j] = cgy[0] * (tex[2][1][j] - tex[0][1][j]) + cgy[1] * (tex[2][2][j] - tex[0][2][j]) + cgy[2] * (tex[3][1][j] - tex[1][1][j]) +
                   cgy[3] * (tex[3][2][j] - tex[1][2][j]);
        }
      } else {
#pragma unroll
        for (int j = 0; j < CJ; ++j) Sf[j] = Sgx[j] = Sgy[j] = vsplat<V>(0.f);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int ix = t & 1, iy = t >> 1;
          const int tx = x0 + ix, ty = y0 + iy;
          const bool in = tx <= W - 1 && ty <= H - 1;
          const float hx = (in && tx > 0 && tx < W - 1) ? 0.5f : 0.f, hy = (in && ty > 0 && ty < H - 1) ? 0.5f : 0.f;
          const float fin = in ? 1.f : 0.f;
          const float wx = ix ? ax : 1.f - ax, wy = iy ? ay : 1.f - ay;
          const float wt = wx * wy;
          cf[t] = wt * fin;
          cgx[t] = wt * hx;
          cgy[t] = wt * hy;
#pragma unroll
          for (int j = 0; j < CJ; ++j) {
            Sf[j] += cf[t] * tex[1 + iy][1 + ix][j];
            Sgx[j] += cgx[t] * (tex[1 + iy][2 + ix][j] - tex[1 + iy][ix][j]);
            Sgy[j] += cgy[t] * (tex[2 + iy][1 + ix][j] - tex[iy][1 + ix][j]);
          }
        }
      }
      vec af[CJ], agx[CJ], agy[CJ];     // the adjoint of the sampled (f, gx, gy): what the 3C row held
#pragma unroll
      for (int j = 0; j < CJ; ++j) {
        if (!cok[j]) {
          Sf[j] = Sgx[j] = Sgy[j] = vsplat<V>(0.f);
          f1[j] = vsplat<V>(0.f);
        }
        const vec d = f1[j] - Sf[j];
        vec sg;
        if constexpr (V == 1) {
          sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
        } else {
#pragma unroll
          for (int q = 0; q < V; ++q) sg[q] = d[q] > 0.f ? 1.f : (d[q] < 0.f ? -1.f : 0.f);
        }
        af[j] = -(dg1 * Sgx[j] + dg2 * Sgy[j] + sg * ga[j]);
        agx[j] = 2.f * (dM11 * Sgx[j] + dM12 * Sgy[j]) + dg1 * d;
        agy[j] = 2.f * (dM12 * Sgx[j] + dM22 * Sgy[j]) + dg2 * d;
      }
      // ---- grad_fixed^T into the tile: the 4x4-minus-corners footprint; a texel outside the tile goes to the dummy slot.
      // Plain read-modify-write, all 12 reads before the 12 writes: the accumulators belong to this wave alone (LDS float
      // atomics -- ds_add_f32 -- measured ~240 ns each here: 5.8 us per pixel with 24 of them)
      {
        const int ux = x0 - 1 - tx0, uy = y0 - 1 - ty0;     // footprint column cc / row r -> tile column ux + cc / row uy + r
        int xo[4], yo[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          xo[k] = (unsigned)(ux + k) < (unsigned)TW ? (ux + k) * kSlotV : -1;
          yo[k] = (unsigned)(uy + k) < (unsigned)TH ? (uy + k) * TW * kSlotV : -1;
        }
        constexpr int kR[12] = {1, 1, 2, 2, 0, 3, 0, 3, 1, 1, 2, 2}, kC[12] = {0, 3, 0, 3, 1, 1, 2, 2, 1, 2, 1, 2};
        vec* dst[12];
        vec val[12][CJ], old[12][CJ];
#pragma unroll
        for (int k = 0; k < 12; ++k) {
          const int o = (xo[kC[k]] | yo[kR[k]]) < 0 ? TW * TH * kSlotV : xo[kC[k]] + yo[kR[k]];
          dst[k] = sAccV + o + lane;
        }
        // gx of tap (ix, iy) = hx (T[tx + 1] - T[tx - 1]), gy = hy (T[ty + 1] - T[ty - 1]); an inner texel also takes its tap's own
        // value, the x-neighbour tap's gx (it is that tap's right / left neighbour) and the y-neighbour tap's gy
        const float k8[8] = {-cgx[0], cgx[1], -cgx[2], cgx[3], -cgy[0], cgy[2], -cgy[1], cgy[3]};
#pragma unroll
        for (int j = 0; j < CJ; ++j) {
#pragma unroll
          for (int k = 0; k < 4; ++k) val[k][j] = k8[k] * agx[j];
#pragma unroll
          for (int k = 4; k < 8; ++k) val[k][j] = k8[k] * agy[j];
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            const int ix = t & 1, iy = t >> 1;
            const float kx = ix ? cgx[2 * iy] : -cgx[2 * iy + 1], ky = iy ? cgy[ix] : -cgy[2 + ix];
            val[8 + t][j] = cf[t] * af[j] + kx * agx[j] + ky * agy[j];
          }
        }
#pragma unroll
        for (int k = 0; k < 12; ++k)
#pragma unroll
          for (int j = 0; j < CJ; ++j) old[k][j] = dst[k][j * 64];
#pragma unroll
        for (int k = 0; k < 12; ++k)
#pragma unroll
          for (int j = 0; j < CJ; ++j) dst[k][j * 64] = old[k][j] + val[k][j];
      }
      // ---- advance: everything requested above has had the arithmetic to arrive
      if (p1.i < 0) break;
      wait_vm0();
      ra0 = rb0;
      ra1 = rb1;
      rb0 = rc0;
      rb1 = rc1;
#pragma unroll
      for (int j = 0; j < CJ; ++j) f1[j] = f1n[j];
      if (p1.i >= e) {                  // into the next non-empty cell: its texels become current, the cell after it is requested
        cur = nxt;
        e = sn + Ln;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int cc = 0; cc < 4; ++cc)
#pragma unroll
            for (int j = 0; j < CJ; ++j) tex[r][cc][j] = texn[r][cc][j];
        nxt = next_cell();
        if (nxt >= 0) {
          cell_range(nxt, sn, Ln);
          want_texn = true;             // requested at the top of the next iteration
        }
      }
      p0 = p1;
      p1 = p2;
    }
  }
  // ---- the tile's texels: written once (overwrite_map) or added to the gradient of the earlier iterations
  float* __restrict__ out_b = a.dmap3 + (size_t)b * HW * C;
  for (int t = 0; t < TW * TH; ++t) {
    const int X = tx0 + (t % TW), Y = ty0 + t / TW;
    if (X >= W || Y >= H) continue;
#pragma unroll
    for (int j = 0; j < CJ; ++j) {
      if (!cok[j]) continue;
      const vec v = sAccV[(t * CJ + j) * 64 + lane];
      vec* o = reinterpret_cast<vec*>(out_b + (size_t)(Y * W + X) * C + coff[j]);
      *o = a.overwrite_map ? v : *o + v;
    }
  }
}

// ---- two visits per wave instruction (C % 4 == 0, C <= 128): a HALF wave per pixel, 4 channels per lane --------------------------
// adj_tile_kernel above is bound by VALU issue: ~450 instructions per visit of which only a third is channel arithmetic (measured:
// no tile shape moves it, 1420 SIMD cycles per visit).  Here lanes 0-31 and 32-63 work on two different pixels of the tile's walking
// order (visit k and visit k + half: the two halves of the sequence, so that the pair's footprints are usually disjoint), every
// per-pixel quantity is a per-lane value, every row access one 16-byte load per lane: the same instruction stream serves two visits.
//   * walking order = the cell rows' list segments back to back; a lane finds its list index by a select chain over the row table
//     (<= TH + 3 rows, uniform); lidx gives (pixel, cell), lrec the fractions and the five scalars;
//   * two register sets (this pair / next pair), the loop unrolled twice so that nothing is copied; the (pixel, cell) pair two
//     iterations ahead; one full s_waitcnt vmcnt(0) per iteration after the arithmetic (see adj_tile_kernel);
//   * accumulators: (TH + 1) x (TW + 1) slots of 32 lanes x 16 bytes -- the extra row and column take what falls outside the tile,
//     so a destination's address is row offset + column offset (unsigned min clamps either to the dummy), no select per texel;
//   * the two halves' 12-texel footprints may overlap: then the read-modify-write runs half by half (two exec-masked phases, in
//     order: deterministic), else once for the whole wave.
typedef float f32x3 __attribute__((ext_vector_type(3)));
template <int TW, int TH>
__global__ __launch_bounds__(64) void adj_tile2_kernel(const AdjArgs a, int tiles_x, int ntiles, int total, int chunk) {
  constexpr int MAXR = TH + 3, SW = TW + 1, SH = TH + 1;
  extern __shared__ __attribute__((aligned(16))) float sAcc[];
  f32x4* sAccV = reinterpret_cast<f32x4*>(sAcc);               // slot (uy, ux), lane hl: (uy SW + ux) 32 + hl
  const int lane = threadIdx.x, hl = lane & 31, hi = lane >> 5;
  const int kk = blockIdx.x >> 3, work = (blockIdx.x & 7) * chunk + kk;
  if (kk >= chunk || work >= total) return;
  const int b = work / ntiles, tile = work - b * ntiles;
  const int tyi = tile / tiles_x, tx0 = (tile - tyi * tiles_x) * TW, ty0 = tyi * TH;
  const int N = a.lv.N, C = a.lv.C, H = a.lv.H, W = a.lv.W, HW = H * W;
  const float* __restrict__ src_b = a.lv.src + (size_t)b * N * C;
  const float* __restrict__ tgt_b = a.lv.tgt + (size_t)b * HW * C;
  const float* __restrict__ lrec = a.lrec + (size_t)b * N * kFrac;
  const int2* __restrict__ lidx = a.lidx + (size_t)b * N;
  const int2* __restrict__ cs = reinterpret_cast<const int2*>(a.start) + (size_t)b * HW;
  const bool cok = 4 * hl < C;
  const int coff = cok ? 4 * hl : 0;
  f32x4 ga = *reinterpret_cast<const f32x4*>(a.gabs + (size_t)b * C + coff);
  if (!cok) ga = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int i = lane; i < SH * SW * 32; i += 64) sAccV[i] = f32x4{0.f, 0.f, 0.f, 0.f};

  // the rows of cells whose pixels can touch the tile, their list segments, the running visit count (all uniform)
  const int cxa = max(tx0 - 2, 0), cxb = min(tx0 + TW, W - 1);
  const int cya = max(ty0 - 2, 0), cyb = min(ty0 + TH, H - 1), ncy = cyb - cya + 1;
  int rsv = 0, cntv = 0;
  if (lane < ncy) {
    const int2 c0 = cs[(cya + lane) * W + cxa], c1 = cs[(cya + lane) * W + cxb];
    rsv = c0.x;
    cntv = c1.x + c1.y - c0.x;
  }
  // visit v of row r has list index v + base_r, base_r = (start of the row's segment) - (visits before the row); a lane adds up the
  // steps base_r - base_{r-1} of the rows it has passed (a sum of conditional terms: a select CHAIN over base_r is turned into a
  // lookup table in scratch memory by the compiler, one scratch load per index)
  int cum[MAXR + 1], step[MAXR];
  cum[0] = 0;
  int prev = 0;
#pragma unroll
  for (int r = 0; r < MAXR; ++r) {
    const int cnt = __builtin_amdgcn_readlane(cntv, r);         // (rows >= ncy hold 0)
    const int bs = __builtin_amdgcn_readlane(rsv, r) - cum[r];
    step[r] = bs - prev;
    prev = bs;
    cum[r + 1] = cum[r] + cnt;
  }
  const int nv = cum[MAXR], half = (nv + 1) >> 1;
  auto list_index = [&](int k) -> int {      // the list index of this lane's visit in iteration k (clamped to a valid one)
    const int v = min(k + hi * half, nv - 1);
    int idx = v + step[0];
#pragma unroll
    for (int r = 1; r < MAXR; ++r) idx += step[r] & -(int)(v >= cum[r]);
    return idx;
  };
  struct Set {                 // one pair of visits: everything its arithmetic needs
    f32x3 r0;                  // (ax, ay, dg1) -- 12 bytes: a 16-byte load would leave a dead register (the pixel index) that the
    f32x4 r1;                  // compiler re-uses at once, waiting for the load it belongs to;  (dg2, dM11, dM12, dM22)
    f32x4 f1;                  // the pixel's source row, this lane's 4 channels
    f32x4 tex[4][4];           // the 4x4-minus-corners target texels of its cell
    int xy;                    // x0 | y0 << 16
  };
  // every row address = a wave-uniform base + an unsigned 32-bit BYTE offset (adj_fold_supported: a window's maps stay below 4 GB):
  // the loads take the base from scalar registers, no 64-bit address arithmetic per load
  const char* const src_c = reinterpret_cast<const char*>(src_b);
  const char* const tgt_c = reinterpret_cast<const char*>(tgt_b);
  const char* const lrec_c = reinterpret_cast<const char*>(lrec);
  const unsigned rowb = (unsigned)C * 4u, coffb = (unsigned)coff * 4u, pitchb = (unsigned)W * rowb;
  auto request = [&](int i, const int2 nx, Set& q) {
    const unsigned ib = (unsigned)i * (unsigned)(kFrac * 4);
    q.r0 = *reinterpret_cast<const f32x3*>(lrec_c + (ib + 4u));
    q.r1 = *reinterpret_cast<const f32x4*>(lrec_c + (ib + 16u));
    q.f1 = *reinterpret_cast<const f32x4*>(src_c + (__umul24((unsigned)nx.x, rowb) + coffb));      // (24-bit multiplies: full rate; N, W C 4 < 2^24: adj_fold_supported)
    q.xy = nx.y;
    const int cx = nx.y & 0xffff, cy = nx.y >> 16;
    unsigned xo[4], yo[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      xo[k] = __umul24((unsigned)min(max(cx - 1 + k, 0), W - 1), rowb) + coffb;
      yo[k] = __umul24((unsigned)min(max(cy - 1 + k, 0), H - 1), pitchb);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int cc = 0; cc < 4; ++cc) {
        if ((r == 0 || r == 3) && (cc == 0 || cc == 3)) continue;
        q.tex[r][cc] = *reinterpret_cast<const f32x4*>(tgt_c + (yo[r] + xo[cc]));
      }
  };
  auto work_on = [&](int k, const Set& q) {
    const bool live = k + hi * half < nv;                       // (an odd count: the upper half idles in the last iteration)
    const int x0 = q.xy & 0xffff, y0 = q.xy >> 16;
    const float ax = q.r0[0], ay = q.r0[1], dg1 = q.r0[2], dg2 = q.r1[0], dM11 = q.r1[1], dM12 = q.r1[2], dM22 = q.r1[3];
    float cf[4], cgx[4], cgy[4];      // tap weight x (in image, gx defined, gy defined): adj_pixel*_kernel's wt, fin, hx, hy
    const bool inner = x0 >= 1 && y0 >= 1 && x0 + 2 <= W - 1 && y0 + 2 <= H - 1;
    if (__all(inner)) {               // (wave-uniform) both footprints inside the image, off the rim
      const float bx = 1.f - ax, by = 1.f - ay;
      cf[0] = bx * by, cf[1] = ax * by, cf[2] = bx * ay, cf[3] = ax * ay;
#pragma unroll
      for (int t = 0; t < 4; ++t) cgx[t] = cgy[t] = 0.5f * cf[t];
    } else {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int ix = t & 1, iy = t >> 1;
        const int tx = x0 + ix, ty = y0 + iy;
        const bool in = tx <= W - 1 && ty <= H - 1;
        const float hx = (in && tx > 0 && tx < W - 1) ? 0.5f : 0.f, hy = (in && ty > 0 && ty < H - 1) ? 0.5f : 0.f;
        const float wx = ix ? ax : 1.f - ax, wy = iy ? ay : 1.f - ay;
        const float wt = wx * wy;
        cf[t] = in ? wt : 0.f;
        cgx[t] = wt * hx;
        cgy[t] = wt * hy;
      }
    }
    f32x4 Sf = cf[0] * q.tex[1][1] + cf[1] * q.tex[1][2] + cf[2] * q.tex[2][1] + cf[3] * q.tex[2][2];
    f32x4 Sgx = cgx[0] * (q.tex[1][2] - q.tex[1][0]) + cgx[1] * (q.tex[1][3] - q.tex[1][1]) + cgx[2] * (q.tex[2][2] - q.tex[2][0]) +
                cgx[3] * (q.tex[2][3] - q.tex[2][1]);
    f32x4 Sgy = cgy[0] * (q.tex[2][1] - q.tex[0][1]) + cgy[1] * (q.tex[2][2] - q.tex[0][2]) + cgy[2] * (q.tex[3][1] - q.tex[1][1]) +
                cgy[3] * (q.tex[3][2] - q.tex[1][2]);
    f32x4 f1 = q.f1;
    if (!cok || !live) {
      Sf = Sgx = Sgy = f32x4{0.f, 0.f, 0.f, 0.f};
      f1 = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const f32x4 d = f1 - Sf;
    f32x4 sg;
#pragma unroll
    for (int e = 0; e < 4; ++e) sg[e] = d[e] > 0.f ? 1.f : (d[e] < 0.f ? -1.f : 0.f);
    const f32x4 af = -(dg1 * Sgx + dg2 * Sgy + sg * ga);
    const f32x4 agx = 2.f * (dM11 * Sgx + dM12 * Sgy) + dg1 * d;
    const f32x4 agy = 2.f * (dM12 * Sgx + dM22 * Sgy) + dg2 * d;
    // ---- grad_fixed^T into the tile (see adj_tile_kernel); footprint column cc / row r -> slot column ux + cc / row uy + r, clamped
    // (unsigned) to the dummy column TW / row TH; an idle half goes to the dummy corner altogether
    const int ux = live ? x0 - 1 - tx0 : TW, uy = live ? y0 - 1 - ty0 : TH;
    unsigned xo[4], yo[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      xo[k] = min((unsigned)(ux + k), (unsigned)TW) * 32u + (unsigned)hl;
      yo[k] = min((unsigned)(uy + k), (unsigned)TH) * (unsigned)(SW * 32);
    }
    constexpr int kR[12] = {1, 1, 2, 2, 0, 3, 0, 3, 1, 1, 2, 2}, kC[12] = {0, 3, 0, 3, 1, 1, 2, 2, 1, 2, 1, 2};
    const float k8[8] = {-cgx[0], cgx[1], -cgx[2], cgx[3], -cgy[0], cgy[2], -cgy[1], cgy[3]};
    // do the two halves' footprints overlap?  (uniform: the other half's cell through a lane read)
    const int xyo = __builtin_amdgcn_readlane(q.xy, 32), xyl = __builtin_amdgcn_readlane(q.xy, 0);
    const int ddx = (xyo & 0xffff) - (xyl & 0xffff), ddy = (xyo >> 16) - (xyl >> 16);
    const bool apart = ddx >= 4 || ddx <= -4 || ddy >= 4 || ddy <= -4 || k + half >= nv;
    {                                     // all 12 destinations at once: 48 registers of values + 48 of old contents
      constexpr int ND = 12;
      f32x4 val[ND];
      f32x4* dst[ND];
#pragma unroll
      for (int u = 0; u < ND; ++u) {
        const int kd = u;
        dst[u] = sAccV + (yo[kR[kd]] + xo[kC[kd]]);
        if (kd < 4) {
          val[u] = k8[kd] * agx;
        } else if (kd < 8) {
          val[u] = k8[kd] * agy;
        } else {
          const int t = kd - 8, ix = t & 1, iy = t >> 1;
          const float kx = ix ? cgx[2 * iy] : -cgx[2 * iy + 1], ky = iy ? cgy[ix] : -cgy[2 + ix];
          val[u] = cf[t] * af + kx * agx + ky * agy;
        }
      }
      if (apart) {
        f32x4 old[ND];
#pragma unroll
        for (int u = 0; u < ND; ++u) old[u] = *dst[u];
#pragma unroll
        for (int u = 0; u < ND; ++u) *dst[u] = old[u] + val[u];
      } else {
#pragma unroll
        for (int ph = 0; ph < 2; ++ph) {
          if (hi == ph) {
            f32x4 old[ND];
#pragma unroll
            for (int u = 0; u < ND; ++u) old[u] = *dst[u];
#pragma unroll
            for (int u = 0; u < ND; ++u) *dst[u] = old[u] + val[u];
          }
          // the other half reads what this half wrote: lanes of one wave, but different THREADS to the compiler -- without the
          // fence it may move the second phase's loads above the first phase's (exec-masked) stores
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");     // (and the next visit's reads stay behind this visit's writes)
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  };

  if (nv > 0) {
    Set A, B;
    int2 nx1, nx2 = make_int2(0, 0);
    int i1, i2;                           // the list indices of iterations k + 1 / k + 2 (each computed once: ~20 instructions)
    {
      const int i0 = list_index(0);
      const int2 nx0 = lidx[i0];
      request(i0, nx0, A);
      i1 = list_index(1);                 // (clamped: valid even when there is no second iteration)
      nx1 = lidx[i1];
    }
    wait_vm0();
    for (int k = 0; k < half; k += 2) {
      // iteration k on A: request k + 1 into B, the (pixel, cell) of k + 2.  Unconditionally (list_index clamps past the end: the
      // last iteration requests a valid pair it never uses) -- a conditional request makes the compiler merge the register set with
      // its old contents by copies that wait for the loads just issued
      request(i1, nx1, B);
      i2 = list_index(k + 2);
      nx2 = lidx[i2];
      work_on(k, A);
      wait_vm0();
      nx1 = nx2;
      i1 = i2;
      if (k + 1 >= half) break;
      // iteration k + 1 on B: request k + 2 into A
      request(i1, nx1, A);
      i2 = list_index(k + 3);
      nx2 = lidx[i2];
      work_on(k + 1, B);
      wait_vm0();
      nx1 = nx2;
      i1 = i2;
    }
  }
  // ---- the tile's texels: written once (overwrite_map) or added to the gradient of the earlier iterations; a half wave per texel
  float* __restrict__ out_b = a.dmap3 + (size_t)b * HW * C;
  for (int t2 = 0; t2 < TW * TH; t2 += 2) {
    const int t = t2 + hi;
    const int uy = t / TW, ux = t - uy * TW, X = tx0 + ux, Y = ty0 + uy;
    if (t >= TW * TH || X >= W || Y >= H || !cok) continue;
    const f32x4 v = sAccV[(uy * SW + ux) * 32 + hl];
    f32x4* o = reinterpret_cast<f32x4*>(out_b + (size_t)(Y * W + X) * C + coff);
    *o = a.overwrite_map ? v : *o + v;
  }
}

}  // namespace

// ---- launch of the tile kernel: everything -- (channel chunks, vector width), tile shape, grid, LDS -- from the plan ----
template <typename Kernel>
void launch_tile_kernel(Kernel* k, const AdjArgs& a, const AdjPlan& pl, hipStream_t s) {
  if (pl.tile_lds > 64 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.tile_lds);
  hipLaunchKernelGGL(k, dim3(8 * pl.tile_chunk), dim3(64), pl.tile_lds, s, a, pl.tiles_x, pl.ntiles, pl.tile_total, pl.tile_chunk);
}

template <int CJ, int V>
int launch_adj_tile_cv(const AdjArgs& a, const AdjPlan& pl, hipStream_t s) {
  switch (pl.tile_shape) {
#define BANET_X(k, tw, th) \
  case k: launch_tile_kernel(&adj_tile_kernel<CJ, V, tw, th>, a, pl, s); return BANET_OK;
    BANET_ADJ_TILE_SHAPE_LIST(BANET_X)
#undef BANET_X
  }
  return BANET_ERR_UNSUPPORTED;
}

// (assert: plan_detail::choose_adj_tile takes (tile_cj, tile_v) and tile_shape from the lists below, so BANET_ERR_UNSUPPORTED
//  cannot be returned for a plan that returned BANET_OK)
int launch_adj_tile(const AdjArgs& a, const AdjPlan& pl, hipStream_t s) {
  if (pl.tile_v == 0) {     // two visits per wave instruction
    switch (pl.tile_shape) {
#define BANET_X(k, tw, th) \
  case k: launch_tile_kernel(&adj_tile2_kernel<tw, th>, a, pl, s); return BANET_OK;
      BANET_ADJ_TILE2_SHAPE_LIST(BANET_X)
#undef BANET_X
    }
    return BANET_ERR_UNSUPPORTED;
  }
  switch (pl.tile_cj * 8 + pl.tile_v) {
#define BANET_X(cj, v) \
  case cj * 8 + v: return launch_adj_tile_cv<cj, v>(a, pl, s);
    BANET_ADJ_TILE_CV_LIST(BANET_X)
#undef BANET_X
  }
  return BANET_ERR_UNSUPPORTED;
}

}  // namespace adj
}  // namespace banet
