// host build of the dense adjoint's plan (banet_amd/csrc/adjoint_plan.hpp) for tests/adjoint_cases.py and
// tests/test_adjoint_cases_cpu.py: what a level launches, asked of the code itself.  No ROCm needed.
#include <cstdio>
#include <string>

#include "../../banet_amd/csrc/adjoint_plan.hpp"

// one level per row of `desc`: B, N, C, K, H, W, dense, tgt_has_grad, pairs, variant, flags (banet_level_t.flags), adjoint flags
// (BANET_ADJOINT_*).  A sparse level (dense = 0) gets non-null rays / intrinsics pointers: the plan only checks their presence.
constexpr int kDescInts = 12;
#define ADJ_PLAN_FIELDS(X)                                                                                                        \
  X(rc) X(G) X(Ga) X(Gm) X(fold) X(bigq_cap) X(off_S) X(off_z2) X(off_arec) X(off_arow) X(off_frac) X(off_cnt) X(off_start)      \
  X(off_cursor) X(off_list) X(off_part) X(off_chunks) X(off_lrec) X(off_list2) X(off_lidx) X(bytes) X(seed) X(seed_nk) X(reuse_z) \
  X(seed_grid) X(seed_lds) X(pixel) X(pixel_cj) X(pixel_kj) X(pixel_ow) X(map_half) X(map_j3) X(tile_cj) X(tile_v) X(tile_shape) \
  X(tile_tw) X(tile_th) X(tiles_x) X(ntiles) X(tile_total) X(tile_chunk) X(tile_lds)

extern "C" const char* banet_test_adjoint_plan_fields() {
#define X(f) #f " "
  return "desc_ints=12 " ADJ_PLAN_FIELDS(X);
#undef X
}

namespace {

std::string fmt(const char* f, int a = 0, int b = 0, int c = 0, int d = 0) {
  char buf[96];
  snprintf(buf, sizeof buf, f, a, b, c, d);
  return buf;
}

// the instantiation a plan names, spelled as in the sources ("" = nothing launched)
std::string seed_name(const banet::AdjPlan& p) {
  switch (p.seed) {
    case banet::kAdjSeedF32: return fmt("adj_basis_kernel<%d>", p.seed_nk);
    case banet::kAdjSeedB6: return fmt(p.reuse_z ? "adj_basis6_kernel<%d, true>" : "adj_basis6_kernel<%d, false>", p.seed_nk);
    case banet::kAdjSeedWide: return fmt("adj_basis_wide_kernel<%d, %d>", p.seed_nk, banet::kAdjWideNBC);
  }
  return "";
}
std::string pixel_name(const banet::AdjPlan& p) {
  switch (p.pixel) {
    case banet::kAdjPixelPoint: return fmt("adj_pixel_kernel<%d, %d, true>", p.pixel_cj, p.pixel_kj);
    case banet::kAdjPixelOne: return fmt("adj_pixel_kernel<%d, %d>", p.pixel_cj, p.pixel_kj);
    case banet::kAdjPixelTwo: return fmt(p.pixel_ow ? "adj_pixel2_kernel<%d, true>" : "adj_pixel2_kernel<%d, false>", p.pixel_cj);
  }
  return "";
}
std::string map_name(const banet::AdjCellPlan& c) {
#define X(j4, j3) \
  if (c.map_j3 == j3) return c.map_half ? fmt("adj_map2_kernel<%d, %d>", j4, j3) : fmt("adj_map_kernel<%d>", j3);
  BANET_ADJ_MAP_LIST(X)
#undef X
  return "";
}
std::string tile_name(const banet::AdjPlan& p) {
  return p.tile_v == 0 ? fmt("adj_tile2_kernel<%d, %d>", p.tile_tw, p.tile_th) : fmt("adj_tile_kernel<%d, %d, %d, %d>", p.tile_cj, p.tile_v, p.tile_tw, p.tile_th);
}

}  // namespace

// out: one row of ADJ_PLAN_FIELDS per level; names (may be null): one line per level, "seed|pixel|map|tile" -- map is empty in fold
// mode and tile outside it, all four are empty for a refused level.  Returns the bytes `names` needs (with its terminator).
extern "C" size_t banet_test_adjoint_plan_sweep(const int32_t* desc, int n, int64_t* out, char* names, size_t names_cap) {
  static const float dummy[1] = {0.f};
  std::string all;
  for (int i = 0; i < n; ++i, desc += kDescInts) {
    banet_level_t lv = {};
    lv.B = desc[0], lv.N = desc[1], lv.C = desc[2], lv.K = desc[3], lv.H = desc[4], lv.W = desc[5];
    lv.dense = desc[6], lv.tgt_has_grad = desc[7], lv.pairs = desc[8], lv.variant = desc[9], lv.flags = desc[10];
    lv.scale = 1.f;
    if (!lv.dense) lv.rays = lv.fx = lv.fy = lv.ox = lv.oy = dummy;
    struct : banet::AdjPlan { int rc; } p;
    p.rc = banet::plan_adjoint(&lv, desc[11], &p);
    if (out) {
#define X(f) *out++ = (int64_t)p.f;
      ADJ_PLAN_FIELDS(X)
#undef X
    }
    if (p.rc == BANET_OK) all += seed_name(p) + "|" + pixel_name(p) + "|" + (p.fold ? "" : map_name(p)) + "|" + (p.fold ? tile_name(p) : "");
    all += "\n";
  }
  if (names && names_cap > all.size()) all.copy(names, all.size()), names[all.size()] = 0;
  return all.size() + 1;
}

// every instantiation of the X-macro lists, "list=name" per line
extern "C" const char* banet_test_adjoint_instantiations() {
  static std::string s;
  s.clear();
#define X(cj, kj) s += "point=" + fmt("adj_pixel_kernel<%d, %d, true>", cj, kj) + "\n";
  BANET_ADJ_POINT_LIST(X)
#undef X
#define X(cj, kj) s += "pixel=" + fmt("adj_pixel_kernel<%d, %d>", cj, kj) + "\n";
  BANET_ADJ_PIXEL_LIST(X)
#undef X
#define X(cj4, ow) s += "pixel2=" + fmt("adj_pixel2_kernel<%d, " #ow ">", cj4) + "\n";
  BANET_ADJ_PIXEL2_LIST(X)
#undef X
#define X(nk) s += "seed=" + fmt("adj_basis_kernel<%d>", nk) + "\n";
  BANET_ADJ_SEED_F32_LIST(X)
#undef X
#define X(nk) s += "seed=" + fmt("adj_basis6_kernel<%d, false>", nk) + "\nseed=" + fmt("adj_basis6_kernel<%d, true>", nk) + "\n";
  BANET_ADJ_SEED_B6_LIST(X)
#undef X
#define X(nk) s += "seed=" + fmt("adj_basis_wide_kernel<%d, %d>", nk, banet::kAdjWideNBC) + "\n";
  BANET_ADJ_SEED_WIDE_LIST(X)
#undef X
#define X(j4, j3) s += "map=" + fmt("adj_map2_kernel<%d, %d>", j4, j3) + "\nmap=" + fmt("adj_map_kernel<%d>", j3) + "\n";
  BANET_ADJ_MAP_LIST(X)
#undef X
#define X(k, tw, th) s += "tile2=" + fmt("adj_tile2_kernel<%d, %d>", tw, th) + "\n";
  BANET_ADJ_TILE2_SHAPE_LIST(X)
#undef X
#define X(k, tw, th) s += "tile=" + fmt("adj_tile_kernel<%d, %d, %d, %d>", cj_, v_, tw, th) + "\n";
#define CV(cj, v)                \
  {                              \
    const int cj_ = cj, v_ = v;  \
    BANET_ADJ_TILE_SHAPE_LIST(X) \
  }
  BANET_ADJ_TILE_CV_LIST(CV)
#undef CV
#undef X
  return s.c_str();
}

// the deterministic sample-stats gradient: one row of `desc` = B, N, C, H, W; out: rc, G, Gm, map_half, map_j3, off_arow, off_frac,
// off_cnt, off_start, off_cursor, off_list, off_chunks, bytes
#define SSTATS_PLAN_FIELDS(X) \
  X(rc) X(G) X(Gm) X(map_half) X(map_j3) X(off_arow) X(off_frac) X(off_cnt) X(off_start) X(off_cursor) X(off_list) X(off_chunks) X(bytes)

extern "C" const char* banet_test_sstats_det_plan_fields() {
#define X(f) #f " "
  return "desc_ints=5 " SSTATS_PLAN_FIELDS(X);
#undef X
}

extern "C" void banet_test_sstats_det_plan_sweep(const int32_t* desc, int n, int64_t* out) {
  for (int i = 0; i < n; ++i, desc += 5) {
    struct : banet::SstatsDetPlan { int rc; } p;
    p.rc = banet::plan_sample_stats_grad_det(desc[0], desc[1], desc[2], desc[3], desc[4], &p);
#define X(f) *out++ = (int64_t)p.f;
    SSTATS_PLAN_FIELDS(X)
#undef X
  }
}
