// The host-side plan of the dense adjoint (adjoint.hip and the adjoint_*.hip files behind it) and of the deterministic
// sample-stats gradient (sstats.hip): which instantiation of every kernel runs, on what grid, with how much dynamic LDS, and where
// every buffer lies in the workspace.  Host-only, plain C++17 (no HIP include), in the manner of plan.hpp: the launchers switch on
// the fields of a plan and decide nothing themselves, and tests/native/adjoint_plan_host.cpp compiles this header with g++ so that
// the tests ask the plan what a level launches (tests/adjoint_cases.py, tests/test_adjoint_cases_cpu.py).
#pragma once
#include "plan.hpp"

namespace banet {

// ---- layout constants ----------------------------------------------------------------------------------------------------------
constexpr int kAdjMaxCJ = 4;    // C <= 256
constexpr int kAdjMaxKJ = 4;    // K <= 256 (K <= 128: adj_basis_kernel keeps the whole K x (K+16) seed block in LDS; above: column chunks)
constexpr int kAdjHdr = 16;     // partial row: dR (9), dT (3), pad, then dWc (K)
constexpr int kScanThreads = 1024;
constexpr int kScanChunk = 1024;    // cells per workgroup of the cell scan (adjoint_cells.hip)
constexpr int kFrac = 8;        // per-pixel record of the map adjoint: key (int; -1 = outside), ax, ay, dg1, dg2, dM11, dM12, dM22
constexpr int kSortSerial = 32;     // cells with up to this many pixels are ordered by one thread (insertion sort)
constexpr int kAdjB6Threads = 512;  // adj_basis6_kernel: two waves per SIMD
constexpr int kAdjWideNBC = 6;      // adj_basis_wide_kernel: 16-column blocks of the seed per chunk

// ---- the compiled instantiations, each list written once -------------------------------------------------------------------------
// The launchers instantiate from these lists, the plan takes "supported" from them and the host test program enumerates them.
// adj_pixel_kernel<CJ, KJ, true>, sparse points (not compiled for > 2 channel chunks with > 2 coefficient chunks)
#define BANET_ADJ_POINT_LIST(X) X(1, 1) X(2, 1) X(3, 1) X(4, 1) X(1, 2) X(2, 2) X(3, 2) X(4, 2) X(1, 3) X(2, 3) X(1, 4) X(2, 4)
// adj_pixel_kernel<CJ, KJ>, dense
#define BANET_ADJ_PIXEL_LIST(X) \
  X(1, 1) X(2, 1) X(3, 1) X(4, 1) X(1, 2) X(2, 2) X(3, 2) X(4, 2) X(1, 3) X(2, 3) X(3, 3) X(4, 3) X(1, 4) X(2, 4) X(3, 4) X(4, 4)
// adj_pixel2_kernel<CJ4, OW>
#define BANET_ADJ_PIXEL2_LIST(X) X(1, true) X(1, false)
// the seed GEMM: adj_basis_kernel<NK>, adj_basis6_kernel<NK, REUSE> (both REUSE), adj_basis_wide_kernel<NK, kAdjWideNBC>
#define BANET_ADJ_SEED_F32_LIST(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8)
#define BANET_ADJ_SEED_B6_LIST(X) X(2) X(3) X(4) X(5) X(6) X(7) X(8)
#define BANET_ADJ_SEED_WIDE_LIST(X) X(12) X(16)
// the per-texel gather: adj_map2_kernel<J4, J3> (half a wave per texel) and adj_map_kernel<J3>, 3C <= 64 J3
#define BANET_ADJ_MAP_LIST(X) X(2, 3) X(3, 6) X(6, 12)
// adj_tile_kernel<CJ, V, TW, TH>: (channel chunks, vector width) x tile shape (BANET_ADJOINT_TILE_SHAPE number, TW, TH); a shape
// number that is in neither shape list is shape 0
#define BANET_ADJ_TILE_CV_LIST(X) X(1, 2) X(2, 2) X(1, 1) X(2, 1) X(4, 1)
//                                                  LDS per wave at C = 128 / waves per CU / visits per pixel
#define BANET_ADJ_TILE_SHAPE_LIST(X)              \
  X(0, 8, 4) /* 16.5 KB / 9 / 2.4 (also shape 1) */ \
  X(2, 4, 4) /*  8.5 KB / 18 / 3.1 */               \
  X(3, 8, 2) /*  8.5 KB / 18 / 3.4 */               \
  X(4, 8, 7) /* 28.5 KB / 5 / 2.0 */                \
  X(5, 4, 2) /*  4.5 KB / 32 / 4.4 */
// adj_tile2_kernel<TW, TH>:                        LDS per wave / waves per CU by LDS / visits per pixel
#define BANET_ADJ_TILE2_SHAPE_LIST(X)               \
  X(0, 8, 4)   /* 23.0 KB / 7 / 2.4 (also shape 8) */ \
  X(9, 8, 3)   /* 18.4 KB / 8 / 2.75 */               \
  X(10, 8, 5)  /* 27.6 KB / 5 / 2.2 */                \
  X(11, 8, 7)  /* 36.9 KB / 4 / 1.96 */               \
  X(12, 16, 3) /* 34.8 KB / 4 / 2.4 */                \
  X(13, 16, 2) /* 26.1 KB / 6 / 2.97 */

enum AdjSeed { kAdjSeedNone = 0, kAdjSeedF32 = 1, kAdjSeedB6 = 2, kAdjSeedWide = 3 };   // pose only / adj_basis / adj_basis6 / adj_basis_wide
enum AdjPixel { kAdjPixelPoint = 0, kAdjPixelOne = 1, kAdjPixelTwo = 2 };               // adj_pixel<.., true> / adj_pixel / adj_pixel2

// ---- the target-cell lists and the per-texel gather: shared by the dense adjoint and the deterministic sample-stats gradient -----
struct AdjCellPlan {
  size_t off_frac, off_cnt, off_start, off_cursor, off_list, off_part, off_chunks;
  int Gm;             // workgroups per window of the per-texel gather
  int map_half;       // 1: adj_map2_kernel (half a wave per texel), 0: adj_map_kernel (kDevAdjTexelPerWave, or 3C % 4 != 0)
  int map_j3;         // J3 of BANET_ADJ_MAP_LIST
};

// The sub-layout, in arena order: records, cell counts (+ cnt_extra bytes), (start, count) pairs, cursors, lists, the caller's
// part_bytes (the adjoint's partial rows; 0 = none), the scan's chunk sums.  lv_flags: banet_level_t.flags.
inline int plan_adj_cells(Arena* ar, size_t B, size_t N, size_t HW, int C, int lv_flags, size_t cnt_extra, size_t part_bytes, AdjCellPlan* c) {
  c->off_frac = ar->take(B * N * kFrac * 4);
  c->off_cnt = ar->take(B * HW * 4 + cnt_extra);
  c->off_start = ar->take(B * HW * 8);
  c->off_cursor = ar->take(B * HW * 4);
  c->off_list = ar->take(B * N * 4);
  c->off_part = ar->take(part_bytes);
  c->off_chunks = ar->take(B * ((HW + kScanChunk - 1) / kScanChunk) * 4);
  c->Gm = (int)std::max<size_t>(1, std::min<size_t>((HW + 3) / 4, (size_t)((4096 + B - 1) / B)));
  const int C3 = 3 * C, J3 = (C3 + 63) / 64;
  c->map_half = ((C3 & 3) == 0 && !(lv_flags & kDevAdjTexelPerWave)) ? 1 : 0;   // one texel per wave (A/B)
  c->map_j3 = 0;
#define BANET_X(j4, j3) \
  if (c->map_j3 == 0 && J3 <= j3) c->map_j3 = j3;
  BANET_ADJ_MAP_LIST(BANET_X)
#undef BANET_X
  return c->map_j3 ? BANET_OK : BANET_ERR_UNSUPPORTED;
}

// ---- the dense adjoint -----------------------------------------------------------------------------------------------------------
struct AdjPlan : AdjCellPlan {
  int G, Ga;
  int fold;           // adj_tile_kernel instead of the 3C rows + per-texel gather (BANET_ADJOINT_FOLD_TARGET)
  int bigq_cap;
  size_t off_S, off_z2, off_arec, off_arow, off_lrec, off_list2, off_lidx, bytes;
  // the seed GEMM
  int seed;           // AdjSeed
  int seed_nk;        // NK of the instantiation
  int reuse_z;        // adj_basis6_kernel<NK, true> (BANET_ADJOINT_REUSE_DEPTH_SEED; the other forms recompute: same result)
  int seed_grid;      // workgroups per window
  size_t seed_lds;    // dynamic LDS bytes (above 64 KB the launch sets the function attribute)
  // the per-pixel kernel
  int pixel;          // AdjPixel
  int pixel_cj, pixel_kj;   // point / one-pixel kernel: <CJ, KJ>; two-pixel kernel: <CJ4 = pixel_cj, OW = pixel_ow>
  int pixel_ow;
  // fold mode: the tile kernel
  int tile_cj, tile_v;      // adj_tile_kernel<CJ, V, TW, TH>; tile_v = 0: adj_tile2_kernel<TW, TH>
  int tile_shape;           // the shape number of its shape list
  int tile_tw, tile_th;
  int tiles_x, ntiles, tile_total, tile_chunk;   // tiles per row / per window / in all, and per eighth of the grid (8 tile_chunk workgroups)
  size_t tile_lds;
};

namespace plan_detail {

inline bool adj_supported(const banet_level_t* lv) {
  const bool var_ok = (lv->variant == BANET_BUNDLE && lv->K >= 1 && lv->K <= 64 * kAdjMaxKJ) ||
                      (lv->variant == BANET_BUNDLE_CAMERA && lv->K == 0);     // pose only: bundlenet.py:122-191, depth fixed
  const bool dense_ok = lv->dense == 1 && lv->tgt_has_grad == 0 && lv->N == lv->H * lv->W;
  // round 5: sparse points in the reference's layout (conv1 [B,N,C], rays + per-point intrinsics, [f|gx|gy] target map)
  const bool sparse_ok = lv->dense == 0 && lv->tgt_has_grad == 1 && lv->rays && lv->fx && lv->fy && lv->ox && lv->oy && lv->H >= 2 && lv->W >= 2;
  return var_ok && (dense_ok || sparse_ok) && lv->pairs <= 1 && lv->C >= 1 && lv->C <= 64 * kAdjMaxCJ && lv->N >= 1;
}

// fold mode: the dense layout (the target map holds features, gradients are formed from it), any C the pixel kernels take
inline bool adj_fold_supported(const banet_level_t* lv) {
  // (the tile kernels address a window's maps with 32-bit byte offsets built by 24-bit multiplies: pixel index, bytes per texel row)
  return lv->dense == 1 && lv->tgt_has_grad == 0 && (size_t)lv->H * lv->W * lv->C < ((size_t)1 << 30) && lv->N < (1 << 24) &&
         (size_t)lv->W * lv->C < ((size_t)1 << 22);
}

inline int choose_adj_seed(const banet_level_t* lv, int flags, AdjPlan* pl) {
  const int K = lv->K, NK = (K + 15) / 16;
  const bool b6 = !(lv->flags & kDevAdjFp32Mfma);   // the bf16x6 form of the GEMM-shaped piece (kDevAdjFp32Mfma: fp32 MFMA, A/B)
  pl->reuse_z = ((flags & BANET_ADJOINT_REUSE_DEPTH_SEED) && b6 && K > 16 && K <= 128) ? 1 : 0;
  pl->seed_grid = pl->Ga;
  if (NK == 0) {            // pose only: no depth block
    pl->seed = kAdjSeedNone;
  } else if (NK == 1 || (NK <= 8 && !b6)) {
    pl->seed = kAdjSeedF32;
    pl->seed_nk = NK;
    pl->seed_lds = (size_t)(16 * NK) * (16 * NK + 20) * sizeof(float);
  } else if (NK <= 8) {
    pl->seed = kAdjSeedB6;
    pl->seed_nk = NK;
    pl->seed_grid = std::max(1, pl->Ga / 2);
    pl->seed_lds = (size_t)((NK + 1) / 2) * (NK + 1) * 3 * 64 * 16;
  } else {
    pl->seed = kAdjSeedWide;
    pl->seed_nk = NK <= 12 ? 12 : 16;
    pl->seed_lds = (size_t)(16 * pl->seed_nk) * (16 * kAdjWideNBC + 20) * sizeof(float);
  }
  bool found = pl->seed == kAdjSeedNone;
#define BANET_X(nk) found = found || (pl->seed == kAdjSeedF32 && pl->seed_nk == nk);
  BANET_ADJ_SEED_F32_LIST(BANET_X)
#undef BANET_X
#define BANET_X(nk) found = found || (pl->seed == kAdjSeedB6 && pl->seed_nk == nk);
  BANET_ADJ_SEED_B6_LIST(BANET_X)
#undef BANET_X
#define BANET_X(nk) found = found || (pl->seed == kAdjSeedWide && pl->seed_nk == nk);
  BANET_ADJ_SEED_WIDE_LIST(BANET_X)
#undef BANET_X
  return found ? BANET_OK : BANET_ERR_UNSUPPORTED;
}

inline int choose_adj_pixel(const banet_level_t* lv, int flags, AdjPlan* pl) {
  const int C = lv->C, K = lv->K, N = lv->N;
  const int CJ = (C + 63) / 64, KJ = std::max(1, (K + 63) / 64);
  bool found = false;
  if (!lv->dense) {   // sparse points, [f|gx|gy] target map: one point per wave
    pl->pixel = kAdjPixelPoint;
    pl->pixel_cj = CJ;
    pl->pixel_kj = KJ;
#define BANET_X(cj, kj) found = found || (CJ == cj && KJ == kj);
    BANET_ADJ_POINT_LIST(BANET_X)
#undef BANET_X
  } else if ((C & 3) == 0 && (K & 3) == 0 && C <= 128 && K <= 128 && !(lv->flags & kDevAdjPixelPerWave) &&   // one pixel per wave (A/B)
             (size_t)N * 3 * C < ((size_t)1 << 30) && N < (1 << 24)) {   // (32-bit byte offsets inside a window: its largest array is the N x 3C adjoint rows; 24-bit multiplies)
    pl->pixel = kAdjPixelTwo;     // (C = 256: 264 B of spills -> the one-pixel kernel)
    pl->pixel_cj = 1;
    pl->pixel_ow = (flags & BANET_ADJOINT_OVERWRITE) ? 1 : 0;
    found = true;
  } else {
    pl->pixel = kAdjPixelOne;
    pl->pixel_cj = CJ;
    pl->pixel_kj = KJ;
#define BANET_X(cj, kj) found = found || (CJ == cj && KJ == kj);
    BANET_ADJ_PIXEL_LIST(BANET_X)
#undef BANET_X
  }
  return found ? BANET_OK : BANET_ERR_UNSUPPORTED;
}

// (channel chunks, vector width) by C; tile shape by flags bits 4-7, BANET_ADJOINT_TILE_SHAPE(k): development switch (A/B), 0 = default
inline void choose_adj_tile(const banet_level_t* lv, int flags, AdjPlan* pl) {
  const int C = lv->C, shape = (flags >> 4) & 15;
  pl->tile_shape = 0;
  if ((C & 3) == 0 && C <= 128 && (shape == 0 || shape >= 8) && lv->W < 65536 && lv->H < 65536) {     // two visits per wave instruction
    pl->tile_cj = 1;
    pl->tile_v = 0;
#define BANET_X(k, tw, th) \
  if (shape == k || k == 0) pl->tile_shape = k, pl->tile_tw = tw, pl->tile_th = th;
    BANET_ADJ_TILE2_SHAPE_LIST(BANET_X)
#undef BANET_X
    pl->tile_lds = (size_t)(pl->tile_tw + 1) * (pl->tile_th + 1) * 32 * 16;       // 512 bytes per slot, one dummy row and column
  } else {
    pl->tile_v = (C & 1) == 0 ? 2 : 1;
    pl->tile_cj = (C & 1) == 0 ? (C <= 128 ? 1 : 2) : (C <= 64 ? 1 : C <= 128 ? 2 : 4);
#define BANET_X(k, tw, th) \
  if (shape == k || k == 0) pl->tile_shape = k, pl->tile_tw = tw, pl->tile_th = th;
    BANET_ADJ_TILE_SHAPE_LIST(BANET_X)
#undef BANET_X
    pl->tile_lds = (size_t)(pl->tile_tw * pl->tile_th + 1) * pl->tile_cj * pl->tile_v * 64 * sizeof(float);     // + the dummy slot
  }
  pl->tiles_x = (lv->W + pl->tile_tw - 1) / pl->tile_tw;
  pl->ntiles = pl->tiles_x * ((lv->H + pl->tile_th - 1) / pl->tile_th);
  pl->tile_total = pl->ntiles * lv->B;
  pl->tile_chunk = (pl->tile_total + 7) / 8;
}

}  // namespace plan_detail

// flags: the BANET_ADJOINT_* bits of the call.  BANET_OK, or BANET_ERR_UNSUPPORTED where a kernel the level needs is not compiled.
inline int plan_adjoint(const banet_level_t* lv, int flags, AdjPlan* pl) {
  using namespace plan_detail;
  *pl = AdjPlan{};
  if (!adj_supported(lv)) return BANET_ERR_UNSUPPORTED;
  if ((flags & BANET_ADJOINT_FOLD_TARGET) && !adj_fold_supported(lv)) return BANET_ERR_UNSUPPORTED;
  pl->fold = (flags & BANET_ADJOINT_FOLD_TARGET) ? 1 : 0;
  const size_t B = lv->B, N = lv->N, C = lv->C, K = lv->K, P = 6 + K, HW = (size_t)lv->H * lv->W;   // (dense: HW == N)
  const int per = (int)((2048 + B - 1) / B);                         // ~8 waves per CU over the whole chip
  pl->G = (int)std::max<size_t>(1, std::min<size_t>((N + 63) / 64, (size_t)(per + kNumWaves - 1) / kNumWaves));
  pl->Ga = (int)std::max<size_t>(1, std::min<size_t>((N + 63) / 64, (size_t)((512 + B - 1) / B)));
  pl->bigq_cap = (int)(B * N / (kSortSerial + 1) + 1);               // every cell that could hold more than kSortSerial pixels
  Arena ar;
  pl->off_S = ar.take(B * P * P * 4);
  pl->off_z2 = ar.take(B * N * K * 4);
  pl->off_arec = ar.take(B * N * 8 * 4);
  pl->off_arow = pl->fold ? 0 : ar.take(B * N * 3 * C * 4);
  // fold: the big-cell queue follows the cell counts, its counter zeroed with them
  int rc = plan_adj_cells(&ar, B, N, HW, lv->C, lv->flags, pl->fold ? (size_t)(1 + pl->bigq_cap) * 4 : 0,
                          B * (size_t)pl->G * kNumWaves * (kAdjHdr + K) * 4, pl);
  pl->off_lrec = pl->fold ? ar.take(B * N * kFrac * 4) : 0;
  pl->off_list2 = pl->fold ? ar.take(B * N * 4) : 0;
  pl->off_lidx = pl->fold ? ar.take(B * N * 8) : 0;
  pl->bytes = ar.off;
  if (rc == BANET_OK) rc = choose_adj_seed(lv, flags, pl);
  if (rc == BANET_OK) rc = choose_adj_pixel(lv, flags, pl);
  if (rc == BANET_OK && pl->fold) choose_adj_tile(lv, flags, pl);
  if (rc != BANET_OK) *pl = AdjPlan{};      // a refused plan is all zeros: no layout, no kernel
  return rc;
}

// ---- the deterministic sample-stats gradient (sstats.hip: sstats_rows_kernel, then the cell lists and the per-texel gather) -------
struct SstatsDetPlan : AdjCellPlan {
  int G;              // workgroups per window of sstats_rows_kernel: 16 points per wave
  size_t off_arow, bytes;
};

inline int plan_sample_stats_grad_det(int B, int N, int C, int H, int W, SstatsDetPlan* pl) {
  *pl = SstatsDetPlan{};
  if (B <= 0 || N <= 0 || C < 1 || C > 64 * kAdjMaxCJ || H <= 0 || W <= 0) return BANET_ERR_UNSUPPORTED;
  pl->G = (N + 16 * kNumWaves - 1) / (16 * kNumWaves);
  Arena ar;
  pl->off_arow = ar.take((size_t)B * N * 3 * C * 4);
  const int rc = plan_adj_cells(&ar, B, N, (size_t)H * W, C, 0, 0, 0, pl);
  pl->bytes = ar.off;
  if (rc != BANET_OK) *pl = SstatsDetPlan{};
  return rc;
}

}  // namespace banet
