// What the translation units of the dense adjoint share (adjoint.hip, the driver, and adjoint_seed / _pixel / _cells / _tile / _map.hip;
// sstats.hip borrows the cell lists and the per-texel gather): the kernels' argument block and the internal launchers.  The
// namespace is a named one on purpose: in an anonymous namespace every translation unit would have an AdjArgs of its own.
// Every launcher takes a plan of adjoint_plan.hpp and switches on its fields; a field without a compiled instantiation is
// BANET_ERR_UNSUPPORTED.  The launchers only enqueue: the driver asks hipGetLastError() once at the end.
#pragma once
#include "kernels.hpp"
#include "adjoint_plan.hpp"

namespace banet {
namespace adj {

struct AdjArgs {
  banet_level_t lv;
  const float* R;
  const float* T;
  const float* Wc;
  const float* S;     // [B][P][P]
  const float* gb;    // [B][P]
  const float* gabs;  // [B][C]
  float* z2;          // [B][N][K]
  float* arec;        // [B][N][8]   q0..q5, zeta, e
  float* arow;        // [B][N][3C]  (nullptr in fold mode: the rows are never materialised)
  float* frac;        // [B][N][kFrac]   key (int), ax, ay, dg1, dg2, dM11, dM12, dM22
  int* cnt;           // [B][HW]
  int* start;         // [B][HW][2]  (start, count)
  int* cursor;        // [B][HW]
  int* list;          // [B][N]
  float* part;        // [B][G * 4][kAdjHdr + K]
  int G;
  float* dsrc;
  float* ddepth;
  float* dbasis;
  float* dmap3;
  float* dpose;
  int overwrite;      // 1: dsrc / ddepth / dbasis are WRITTEN (every entry, zeros where nothing contributes) instead of accumulated
  int overwrite_map;  // 1: the same for dmap3
  // fold mode (round 6, adj_tile_kernel): dmap3 is the target map's gradient itself, [B][H][W][C]
  float* lrec;        // [B][N][kFrac]  the records in cell-list order, key replaced by the pixel index
  int* list2;         // [B][N]         scratch of the big-cell sort
  int2* lidx;         // [B][N]         (pixel index, x0 | y0 << 16) in cell-list order: what adj_tile2_kernel addresses with
  int* bigq;          // [1 + B*N/32]   queue of the cells with more than kSortSerial entries (bigq[0] = their number)
  int reuse_z;        // BANET_ADJOINT_REUSE_DEPTH_SEED: z2 / zeta / e of the previous call on this workspace are valid (adj_basis6_kernel)
};

// adjoint_seed.hip: adj_sym_kernel (S = (gAtA + gAtA^T)/2), then the seed GEMM of pl.seed (nothing for kAdjSeedNone)
void launch_adj_sym(const float* gAtA, float* S, int B, int P, hipStream_t s);
int launch_adj_seed(const AdjArgs& a, const AdjPlan& pl, hipStream_t s);
// adjoint_pixel.hip: the per-pixel kernel of pl.pixel; the per-wave partials -> dpose
int launch_adj_pixel(const AdjArgs& a, const AdjPlan& pl, hipStream_t s);
void launch_adj_fold(const float* part, int rows, int B, int K, float* dpose, hipStream_t s);
// adjoint_cells.hip: cell counts -> (start, count) pairs and cursors; the cell lists; fold mode: every list in ascending pixel order
void launch_cell_scan(const int* cnt, int* start, int* cursor, int* chunk_tmp, int B, int HW, hipStream_t s);
void launch_adj_fill(const float* frac, int* cursor, int* list, int B, int N, int HW, hipStream_t s);
void launch_adj_cellsort(const AdjArgs& a, int bigq_cap, hipStream_t s);
// adjoint_tile.hip: the tile kernel of pl.tile_*
int launch_adj_tile(const AdjArgs& a, const AdjPlan& pl, hipStream_t s);
// adjoint_map.hip: the per-texel gather of (c.map_half, c.map_j3) on c.Gm workgroups per window
int launch_adj_map(const AdjArgs& a, const AdjCellPlan& c, hipStream_t s);

}  // namespace adj
}  // namespace banet
