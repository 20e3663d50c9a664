// Backward of the fused dense bundle assembly: given the upstream gradients of one assembly pass,
//   gAtA [B,P,P], gAtb [B,P], gabs [B,C] = dL / d(AtA, Atb, sum_n |d|),
// the gradients with respect to everything the pass read -- source map, target map, depth, depth basis, pose (R, T)
// and depth coefficients Wc.  It is what TF autodiff + the registered EquationConstructionGrad (bundlenet.py:79-82,
// utils.cu:465-694) compute for the statements bundlenet.py:206-263, restated per pixel without J, G or d in memory
// (derivation and float64 statement: dense_adjoint.py of the test oracle, validated there against finite differences).
//
// With S = (gAtA + gAtA^T)/2, b = the pixel's basis row, J = [Jc | jd b^T], M = G^T G, g = G^T d:
//   q = S_cd b, z = S_dd b, zeta = b.z, e = gAtb_d.b, t = Jc q + jd zeta
//   dM = (Jc S_cc + jd q^T) Jc^T + t jd^T,  dg = Jc gAtb_c + jd e          -> channel adjoints of (gx, gy, d)
//   dJc = 2 M (Jc S_cc + jd q^T) + g gAtb_c^T,  djd = 2 M t + g e          -> geometry adjoint -> dD, dR, dT
//   dbasis = 2 s z + 2 S_cd^T u + r gAtb_d + dD Wc   (u, s, r = the forward's per-pixel records)
// Kernels, in launch order:
//   adj_sym_kernel      S = (gAtA + gAtA^T)/2
//   adj_basis_kernel    the one GEMM-shaped piece, [N x K] . [K x (K+7)] per window on v_mfma_f32_16x16x4_f32 (exact fp32):
//                       z2 = 2 S_dd b (written), per-pixel records (q, zeta, e)
//   adj_pixel_kernel    one wave per pixel, lane = channel / coefficient: recomputes depth, warp, taps, M, g; writes
//                       dsrc, ddepth, dbasis (+=: every pixel is owned by one wave), the pixel's 3C adjoint row of the sampled
//                       [f|gx|gy] vector, its target cell + bilinear fractions; per-wave partial sums of dR, dT, dWc
//   adj_scan / adj_fill target cell -> list of the source pixels whose bilinear footprint starts there (integer atomics only)
//   adj_map_kernel      one wave per target texel: GATHERS the (<= 4 cells) contributions in ascending pixel order into the
//                       [f|gx|gy] map adjoint -- no float atomics, bit-reproducible (the sparse-layout ba_sample_stats_grad_kernel
//                       scatters with atomics instead)
//   adj_fold_kernel     per-wave partials -> dpose [B, 12 + K] in fixed order
// and, once per level after all iterations, target_map_adjoint_kernel: d tgt += dmap_f + grad_fixed^T (dmap_gx, dmap_gy)
// (REFLECT rim: bundlenet.py:92-100).
//
// This file is the driver: it runs plan_adjoint (adjoint_plan.hpp: every choice of kernel, grid, LDS size and workspace
// offset), fills the kernels' argument block and issues the launch sequence.  The kernels and their launchers:
// adjoint_seed.hip (adj_sym, adj_basis*), adjoint_pixel.hip (adj_pixel*, adj_fold), adjoint_cells.hip (adj_scan*, adj_fill,
// adj_cellsort, adj_bigcell), adjoint_tile.hip (adj_tile*, fold mode), adjoint_map.hip (adj_map*, target_map_adjoint*).
#include "adjoint_common.hpp"

namespace banet {

size_t dense_adjoint_workspace_bytes(const banet_level_t* lv, int flags) {
  AdjPlan pl;
  return plan_adjoint(lv, flags, &pl) == BANET_OK ? pl.bytes : 0;
}

int launch_dense_adjoint(const banet_level_t* lv, const float* R, const float* T, const float* Wc, const float* gAtA,
                         const float* gAtb, const float* gabs, float* dsrc, float* dmap3, float* ddepth, float* dbasis,
                         float* dpose, int flags, void* ws, hipStream_t s) {
  using namespace adj;
  AdjPlan pl;
  int rc = plan_adjoint(lv, flags, &pl);
  if (rc != BANET_OK) return rc;
  char* base = static_cast<char*>(ws);
  const int B = lv->B, N = lv->N, K = lv->K, P = 6 + K, HW = lv->H * lv->W;
  AdjArgs a;
  a.lv = *lv;
  a.R = R;
  a.T = T;
  a.Wc = Wc;
  float* S = reinterpret_cast<float*>(base + pl.off_S);
  a.S = S;
  a.gb = gAtb;
  a.gabs = gabs;
  a.z2 = reinterpret_cast<float*>(base + pl.off_z2);
  a.arec = reinterpret_cast<float*>(base + pl.off_arec);
  a.arow = pl.fold ? nullptr : reinterpret_cast<float*>(base + pl.off_arow);
  a.frac = reinterpret_cast<float*>(base + pl.off_frac);
  a.cnt = reinterpret_cast<int*>(base + pl.off_cnt);
  a.start = reinterpret_cast<int*>(base + pl.off_start);
  a.cursor = reinterpret_cast<int*>(base + pl.off_cursor);
  a.list = reinterpret_cast<int*>(base + pl.off_list);
  a.part = reinterpret_cast<float*>(base + pl.off_part);
  a.lrec = pl.fold ? reinterpret_cast<float*>(base + pl.off_lrec) : nullptr;
  a.list2 = pl.fold ? reinterpret_cast<int*>(base + pl.off_list2) : nullptr;
  a.lidx = pl.fold ? reinterpret_cast<int2*>(base + pl.off_lidx) : nullptr;
  a.bigq = pl.fold ? a.cnt + (size_t)B * HW : nullptr;
  a.G = pl.G;
  a.dsrc = dsrc;
  a.ddepth = ddepth;
  a.dbasis = dbasis;
  a.dmap3 = dmap3;
  a.dpose = dpose;
  a.overwrite = (flags & BANET_ADJOINT_OVERWRITE) ? 1 : 0;
  a.overwrite_map = (flags & BANET_ADJOINT_OVERWRITE_MAP) ? 1 : 0;
  a.reuse_z = pl.reuse_z;

  launch_adj_sym(gAtA, S, B, P, s);
  if (hipMemsetAsync(a.cnt, 0, ((size_t)B * HW + (pl.fold ? 1 : 0)) * sizeof(int), s) != hipSuccess) return BANET_ERR_LAUNCH;
  if (pl.seed == kAdjSeedNone) {   // pose only: no depth block -> q = zeta = e = 0; the pixel kernels read (never use) one basis / z2 element
    if (hipMemsetAsync(a.arec, 0, (size_t)B * N * 8 * sizeof(float), s) != hipSuccess) return BANET_ERR_LAUNCH;
    a.lv.basis = a.arec;
    a.z2 = a.arec;
    a.dbasis = a.arec;       // (adj_pixel2_kernel reads its rows unconditionally at clamped offsets: a valid address, never written)
  }
  if ((rc = launch_adj_seed(a, pl, s)) != BANET_OK) return rc;
  if ((rc = launch_adj_pixel(a, pl, s)) != BANET_OK) return rc;
  launch_cell_scan(a.cnt, a.start, a.cursor, reinterpret_cast<int*>(base + pl.off_chunks), B, HW, s);
  launch_adj_fill(a.frac, a.cursor, a.list, B, N, HW, s);
  if (pl.fold) {
    launch_adj_cellsort(a, pl.bigq_cap, s);
    rc = launch_adj_tile(a, pl, s);
  } else {
    rc = launch_adj_map(a, pl, s);
  }
  if (rc != BANET_OK) return rc;
  launch_adj_fold(a.part, pl.G * kNumWaves, B, K, dpose, s);
  return hipGetLastError() == hipSuccess ? BANET_OK : BANET_ERR_LAUNCH;
}

}  // namespace banet
