// The host-side launch plans of one assembly pass: which gather / SYRK kernel runs, on what grid, how many partial rows it
// writes (the summation tree) and where every buffer lies in the workspace; every launch of a gather pass and of a SYRK pass as a list
// of steps (plan_gather_steps: queue zeroing, kernel instantiation, grid, block, LDS, fold -- gather.hip walks it; plan_syrk_steps:
// pre-passes, kernel instantiation, job, grid, LDS -- syrk.hip walks it), the statistics mode of a pass (SyrkStats), the lambda-MLP role
// decision (plan_syrk_role) and the lists of compiled gather / SYRK instantiations.  Host-only, plain C++17 (no HIP include): the .hip
// files take the plans AND the occupancy numbers of their __launch_bounds__ from here, and tests/native/plan_host.cpp compiles this header
// with g++ to pin every decision (tests/test_plan_cpu.py, tests/test_gather_steps_cpu.py, tests/test_syrk_steps_cpu.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/banet_hip.h"
#include "dev_flags.hpp"

// workgroups per CU (= waves per SIMD) the gather kernels are compiled for: their __launch_bounds__ and the plans' resident rounds
#ifndef BANET_GATHER_WAVES
#define BANET_GATHER_WAVES 3   // ba_gather_kernel
#endif
#ifndef BANET_G128P_WAVES
#define BANET_G128P_WAVES 2   // ba_gather128p_kernel: workgroups per CU (its prefetch registers need 256 VGPRs)
#endif
#ifndef BANET_G128_WAVES
#define BANET_G128_WAVES 3   // ba_gather128_kernel: workgroups per CU (= waves per SIMD) of its launch bounds
#endif

namespace banet {

constexpr int kWave = 64;         // CDNA wavefront
constexpr int kTilePix = 64;      // source pixels per workgroup tile (8x8 patch in dense mode)
constexpr int kBlock = 256;       // 4 waves
constexpr int kNumWaves = kBlock / kWave;
constexpr int kGHdr = 32;         // gather partial header: 21 H_cc + 6 Atb_c + nvalid (+pad), then C x sum|d|
constexpr int kFoldRows = 64;     // ba_fold_kernel sums this many consecutive partial rows into one
constexpr int kRecMaxBlocks = 32; // workgroups per window of the fp16 SYRK's record-maxima pre-pass

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Bump allocator of the workspace layouts: 256-byte aligned offsets in the order of the take() calls; `off` ends as the total.
struct Arena {
  size_t off = 0;
  size_t take(size_t bytes) {
    const size_t at = off;
    off = align_up(off + bytes, 256);
    return at;
  }
};

inline int npairs(const banet_level_t* lv) { return lv->pairs > 1 ? lv->pairs : 1; }
// the batch size every kernel / arithmetic-form / partial-row decision is taken from (banet_level_t.policy): the launch's own, or
// -- BANET_POLICY_BATCH_INVARIANT -- the canonical one, so that a window's bits do not depend on who shares its launch
inline int selection_batch(const banet_level_t* lv) { return lv->policy == BANET_POLICY_BATCH_INVARIANT ? BANET_CANONICAL_BATCH : lv->B; }

// ---- gather ----------------------------------------------------------------------------
struct GatherPlan {
  int G, tiles, tiles_x, tiles_y, groups, pstride;
  int c128;     // 1: ba_gather128_kernel (dynamic tile queue, one partial row per tile)
  int patch;    // 1: ba_gather128p_kernel (same interface; taps from wave-private LDS patches) for large levels
  int strip;    // ba_gather128s_kernel (work items = 16-pixel-wide strip segments, rolling LDS window): pixel rows per segment
                //    (32 or 16; 0 = another kernel); tiles_x / tiles_y / tiles then count segments
  int quad;     // 1: ba_gather128q_kernel (work items = 4x4 pixel blocks, one step per item): latency-bound launches; tiles_x / tiles_y / tiles count items
  int strip_fp; // strip kernel, multi-frame windows: a workgroup = `pairs` waves on one segment, wave p against target frame p
  int rows;     // partial rows per window written by the gather kernel (tiles or G)
  int frows;    // rows per window handed to ba_reduce2_kernel (after ba_fold_kernel when rows > kFoldRows)
  int nbands;   // tile-queue bands (8 = one per XCD)
  int pairloop; // patch kernel: target frames looped over inside a tile (grid y = windows)
  int qshift;   // 2: quarter-tile work items (levels with fewer tiles than resident waves)
  int tile_pts; // generic kernel, sparse points: points per wave item (64; 16 on latency-bound launches)
  size_t off_fold, off_queue;   // inside the partial region
  size_t partial_bytes, rec_bytes;
};

constexpr int kStrip8PerWave = 2;     // 8-row strip segments: fewest per resident wave (tools/gpu_r4_k.sh)
constexpr int kQuadRounds = 12;      // ba_gather128q_kernel: most items per resident wave (measured, profiles/r04_run6_*: wins up to 19200 items -- 640x480 x 1, 160x120 x 8, 80x60 x 32 -- loses at 38400)
constexpr int kStripSegW = 16, kStripSegH = 32, kStripMinW = 21;   // = kStripW, kStripH, kWinTex of strip_plan.hpp (asserted in gather128s.hip)
constexpr int kGenericBlocksPerCU = BANET_GATHER_WAVES;  // ba_gather_kernel: launch bounds
constexpr int kC128BlocksPerCU = BANET_G128_WAVES;       // ba_gather128_kernel: launch bounds (LDS: 18 KB)
constexpr int kPatchBlocksPerCU = BANET_G128P_WAVES;     // ba_gather128p_kernel: launch bounds

// ba_gather128s_kernel's LDS: per wave the rolling window (7 rows x kStripMinW texels x 32 channels) + 128 floats of row statistics
// (= kSWaveLdsFloats, asserted in gather128s.hip); a frame-parallel workgroup holds `pairs` of them + [nch][64] depths + 4 words
constexpr int kStripWaveLdsFloats = 7 * kStripMinW * 32 + 128;
inline size_t strip_fp_lds_bytes(int pairs, int nch) { return ((size_t)pairs * kStripWaveLdsFloats + (size_t)nch * 64 + 4) * sizeof(float); }

namespace plan_detail {

inline bool use_c128(const banet_level_t* lv) {
  return lv->C == 128 && !lv->tgt_has_grad && !(lv->flags & kDevGenericGather) && (lv->K & 3) == 0 && lv->K <= 256;
}

// The strip gather (gather128s.hip: 16 x 32-pixel segments, rolling LDS window, target map fetched 1.44 x instead of 2.15 x)
// where a launch has at least 4 segments per resident wave (coarser items than the 8x8 tiles: below that the tail of the
// last round costs more than the halo saves).  kDevForceStripGather: at any size (parity tests); kDevNoStripGather: off (A/B).
inline bool choose_strip(const banet_level_t* lv, int kCUs, int Bsel, GatherPlan* pl) {
  if (!(pl->c128 && lv->dense && !(lv->flags & kDevNoStripGather) && lv->W >= kStripMinW && lv->W < 4096 && lv->H < 4096 &&
        (size_t)lv->N * lv->C * 4 < ((size_t)1 << 31)))
    return false;
  // segment height: 16 rows.  32-row segments fetch less (target rows 35/32 x instead of 19/16 x: launch 1.12 x vs 1.16 x the
  // algorithmic bytes) but lose 5 % at every size measured (640x480 x 32: 3396 vs 3230 us, x 256: 27.3 vs 26.1 ms, 5-frame
  // windows 11.03 vs 10.77 ms; profiles/r03_run11_*, r03_run12_*): half as many, twice as long work items leave a longer
  // tail in the last round of the queue.  kDevStripRows32: 32-row segments (A/B, parity tests).
  const int sxn = (lv->W + kStripSegW - 1) / kStripSegW;
  // Mid-size two-frame launches (too few 16-row segments per wave, too many pixels for the 4x4-item kernel: 160x120 x 32,
  // 320x240 x 8 .. 16, 640x480 x 2 .. 4): 8-row segments (target rows 11/8 x) where the launch has at least kStrip8PerWave of
  // them per resident wave.  kDevForceStripGather + kDevQuarterTiles: force them (parity tests); A/B: kDevNoStripGather (no strip gather at all).
  const int np = npairs(lv);
  const int syn16 = (lv->H + kStripSegH / 2 - 1) / (kStripSegH / 2), syn8 = (lv->H + 7) / 8;
  const bool force8 = (lv->flags & kDevForceStripGather) && (lv->flags & kDevQuarterTiles);
  const bool low = force8 || (np == 1 && !(lv->flags & (kDevStripRows32 | kDevForceStripGather)) &&
                              (long long)sxn * syn16 * Bsel < 4LL * kCUs * 8 &&
                              (long long)sxn * syn8 * Bsel >= (long long)kStrip8PerWave * kCUs * 8 &&
                              (long long)((lv->W + 3) / 4) * ((lv->H + 3) / 4) * Bsel > (long long)kQuadRounds * kCUs * 8);
  const int segh = (lv->flags & kDevStripRows32) ? kStripSegH : low ? 8 : kStripSegH / 2;
  const int syn = (lv->H + segh - 1) / segh;
  // (A single resident round at tiny batches -- every segment on a wave of its own -- does not pay: one segment is a serial chain
  // of ~200-270 us whatever the load; batch 1: 640x480 270 vs 272 us, 320x240 205 vs 168 us for the tile kernels.)
  // multi-frame windows: frame-parallel workgroups (gather128s.hip, FP) -- `pairs` waves per segment, so a launch has
  // 2048 / pairs resident work-item slots instead of 2048.  kDevStripFrameLoop: the frames looped over inside one wave (A/B).
  const bool fp = np >= 2 && np <= 7 && segh == kStripSegH / 2 && !(lv->flags & kDevStripFrameLoop);
  const int fp_wg_per_cu = fp ? (int)std::min<size_t>(8 / np, (size_t)(160 * 1024) / strip_fp_lds_bytes(np, 4)) : 0;
  const long long slots = fp ? (long long)kCUs * fp_wg_per_cu : (long long)kCUs * 8;
  if (!((long long)sxn * syn * Bsel >= 4LL * slots || low || (lv->flags & kDevForceStripGather))) return false;
  pl->strip = segh;
  pl->strip_fp = fp ? 1 : 0;
  pl->tiles_x = sxn;
  pl->tiles_y = syn;
  pl->tiles = sxn * syn;
  pl->pairloop = 1;
  const int resident = fp ? kCUs * fp_wg_per_cu : kCUs * 4;   // 128-thread workgroups, 4 per CU (2 waves per SIMD); FP: by LDS / waves
  int G = (resident + lv->B - 1) / lv->B;
  const int want = fp ? pl->tiles : (pl->tiles + 1) / 2;      // one item per wave (FP: per workgroup) at least
  if (G > want) G = want;
  if (G < 1) G = 1;
  pl->G = G;
  pl->nbands = 1;
  return true;
}

// Latency-bound launches (coarse levels, small batches): ba_gather128q_kernel -- 4x4-pixel items, the whole item one step,
// ~4x shorter serial chain per item than a tile's 16 steps (gather128q.hip) -- while the launch has at most kQuadRounds items
// per resident wave (2 workgroups x 4 waves per CU); beyond that the tile kernels' shared stencils win.
// kDevForceQuadGather: at any size (parity tests, A/B); kDevNoQuadGather: off.
inline bool choose_quad(const banet_level_t* lv, int kCUs, int Bsel, GatherPlan* pl) {
  // (kDevForcePatchGather / kDevDirectGather force the patch / direct tile kernels)
  if (!(pl->c128 && lv->dense && !(lv->flags & (kDevNoQuadGather | kDevForcePatchGather | kDevDirectGather)))) return false;
  const int qxn = (lv->W + 3) / 4, qyn = (lv->H + 3) / 4;
  const long long qitems = (long long)qxn * qyn * Bsel * npairs(lv);
  // (multi-frame windows: every virtual window redoes the depth dot -- half the limit: cfg-3's 40x30 x 32 x 4 = 9600 items wins,
  //  cfg-5's 80x60 x 8 x 7 = 16800 loses 329 vs 210 us, profiles/r04_run9_*)
  const long long qlimit = (long long)kQuadRounds * kCUs * 8 / (npairs(lv) > 1 ? 2 : 1);
  if (!(qitems <= qlimit || (lv->flags & kDevForceQuadGather))) return false;
  const int VBq = lv->B * npairs(lv);
  pl->quad = 1;
  pl->tiles_x = qxn;
  pl->tiles_y = qyn;
  pl->tiles = qxn * qyn;
  int G = (kCUs * 2 + VBq - 1) / VBq;            // one resident round of 256-thread workgroups, 2 per CU
  const int want = (pl->tiles + kNumWaves - 1) / kNumWaves;
  if (G > want) G = want;
  if (G < 1) G = 1;
  pl->G = G;
  pl->nbands = 1;
  return true;
}

// The 8x8-tile kernels -- patch, direct (C = 128) or generic -- take every launch the two above left.
// One resident round: the gather is latency-bound per wave (measured: a second, partial round of
// workgroups takes as long as the first), so the grid is what the chip holds at once, split
// across the windows.
inline void choose_tile(const banet_level_t* lv, int kCUs, int Bsel, GatherPlan* pl) {
  // Large dense levels (>= 4 tiles per resident wave): ba_gather128p_kernel -- wave-private LDS patches with a
  // software-pipelined box prefetch, 2 workgroups per CU (measured 640x480 x 8: 138 -> 125 us/window, 320x240 x 8:
  // 48 -> 38); smaller levels are latency-bound and keep the 3-per-CU direct kernel.  kDevDirectGather: direct (A/B).
  pl->patch = (pl->c128 && lv->dense && !(lv->flags & kDevDirectGather) &&
               ((long long)pl->tiles * Bsel * npairs(lv) >= 4LL * kCUs * kPatchBlocksPerCU * kNumWaves ||
                (lv->flags & kDevForcePatchGather))) ? 1 : 0;   // kDevForcePatchGather: at any size (parity tests)
  const int resident = kCUs * (pl->patch ? kPatchBlocksPerCU : pl->c128 ? kC128BlocksPerCU : kGenericBlocksPerCU);
  const int VB = lv->B * npairs(lv);   // virtual windows
  const int VBsel = Bsel * npairs(lv);
  // the generic kernel publishes one partial row per WORKGROUP (rows = G), so its grid is part of the arithmetic: taken from Bsel;
  // the C = 128 kernels publish one row per work item in a fixed place, their grid is free to follow the launch
  const int Bgrid = pl->c128 ? lv->B : Bsel;
  // the patch kernel loops over a window's target frames inside a tile (depth dot once per window) where a window alone has
  // >= 4 tiles per resident wave; below that the 4x coarser items cost more than the shared depth saves (80x60 x 32
  // windows x 4 frames: 327 -> 478 us) and a work item stays one pair's tile
  pl->pairloop = (pl->patch && npairs(lv) > 1 && ((long long)pl->tiles * Bsel >= 4LL * kCUs * kPatchBlocksPerCU * kNumWaves ||
                                                   (lv->flags & kDevPatchPairLoop))) ? 1 : 0;   // kDevPatchPairLoop: force it (parity tests)
  const int gy = pl->pairloop ? Bgrid : Bgrid * npairs(lv);
  int target = (resident + gy - 1) / gy;
  // Mid-size levels (a few tiles per wave at most) start all their waves in the same phase: measured, ~1300 waves
  // finish a tile in 67 us but 2560 need 169 us (160x120 x 8: one tile per wave 21.1 us/window, two per wave on half
  // the waves 16.7).  Such levels run on at most 320 workgroups (1280 waves).
  if (pl->c128 && !pl->patch && (long long)pl->tiles * VBsel < 4LL * kCUs * kPatchBlocksPerCU * kNumWaves)
    target = std::min(target, (320 + VB - 1) / VB);
  // quarter-tile work items pay (measured: 40x30 x 8 windows 94 -> 50 us) only while they still leave the chip
  // mostly empty -- at most one item per SIMD; beyond that the redone depth dot / geometry costs more than
  // the shorter step chain saves (80x60 x 8: 101 -> 132 us).  kDevNoQuarterTiles: off (A/B).
  pl->qshift = (pl->c128 && !pl->patch && pl->tiles <= 32 && (long long)pl->tiles * VBsel * 4 <= (long long)kCUs * 4 &&
                !(lv->flags & kDevNoQuarterTiles)) ? 2 : 0;
  if (pl->c128 && !pl->patch && (lv->flags & kDevQuarterTiles)) pl->qshift = 2;   // kDevQuarterTiles: force quarter tiles (A/B)   // (80x60 x 2 windows, also 640 items, LOSES 82 vs 51 us: coarsest levels only)
  int G = pl->c128 ? ((pl->tiles << pl->qshift) + 3) / 4 : pl->groups;
  if (G > target) {
    G = target >= 8 ? (target & ~7) : target;   // several work items per wave: one resident round, no more
  } else if (G >= 8) {
    G = (G + 7) & ~7;   // every item gets its own wave in ONE round (rounding down left a few items for a second
                        // pass: 2x the latency of a level that is pure latency); surplus workgroups find nothing and exit
  }
  if (G < 1) G = 1;
  pl->G = G;
  pl->nbands = (G & 7) == 0 ? 8 : 1;
}

// The partial region: [rows x row] [frows x row, when ba_fold_kernel runs] [tile-queue heads]; then the per-pixel records.
// The C = 128 kernels write one row per work item, the generic kernel one per workgroup.
inline void layout_partials(GatherPlan* pl, const banet_level_t* lv) {
  const int VB = lv->B * npairs(lv);   // virtual windows
  pl->pstride = kGHdr + lv->C;
  pl->rows = pl->c128 ? (pl->tiles << pl->qshift) : pl->G;
  pl->frows = pl->rows > kFoldRows ? (pl->rows + kFoldRows - 1) / kFoldRows : pl->rows;
  const size_t row_bytes = (size_t)VB * pl->pstride * sizeof(float);
  pl->off_fold = align_up(row_bytes * pl->rows, 256);
  pl->off_queue = pl->off_fold + (pl->frows != pl->rows ? align_up(row_bytes * pl->frows, 256) : 0);
  pl->partial_bytes = pl->off_queue + align_up((size_t)VB * 8 * sizeof(int), 256);
  pl->rec_bytes = lv->K > 0 ? align_up((size_t)VB * lv->N * 8 * sizeof(float), 256) : 0;
}

}  // namespace plan_detail

// kCUs: compute units of the part the launch is planned for (the .hip callers pass num_cus()).
inline int plan_gather(const banet_level_t* lv, int kCUs, GatherPlan* pl) {
  using namespace plan_detail;
  *pl = GatherPlan{};
  // 1. validate
  if (!lv || lv->B <= 0 || lv->N <= 0 || lv->C <= 0 || lv->K < 0 || lv->H < 4 || lv->W < 4) return BANET_ERR_INVALID_ARG;
  // (the field was a must-be-zero pad until round 4: anything but the two policies is a caller's garbage, not "throughput")
  if (lv->policy != BANET_POLICY_THROUGHPUT && lv->policy != BANET_POLICY_BATCH_INVARIANT) return BANET_ERR_INVALID_ARG;
  if (lv->C > 256 || lv->K > 256) return BANET_ERR_UNSUPPORTED;
  if (lv->dense && lv->N != lv->H * lv->W) return BANET_ERR_INVALID_ARG;
  const int Bsel = selection_batch(lv);   // decisions: Bsel; grids and buffer sizes: lv->B
  // 2. tiling: 8x8-pixel tiles of a dense level, or runs of tile_pts sparse points
  if (lv->dense) {
    pl->tiles_x = (lv->W + 7) / 8;
    pl->tiles_y = (lv->H + 7) / 8;
    pl->tiles = pl->tiles_x * pl->tiles_y;
    pl->tile_pts = kTilePix;
  } else {
    // Sparse points: 64 per wave item -- or 16 (round 6) while four times as many items still fit one resident round: the item is
    // a serial chain of its points (the reference's own tracker, N = 4096 at batch 1: 64 items = 64 waves on 16 CUs, 54 us per launch)
    // (chosen before c128 is known, though only ba_gather_kernel honours tile_pts -- kept as it is here)
    const long long items64 = (long long)((lv->N + kTilePix - 1) / kTilePix) * Bsel * npairs(lv);
    pl->tile_pts = (4 * items64 <= (long long)kCUs * kGenericBlocksPerCU * kNumWaves && !(lv->flags & kDevSparseItems64)) ? 16 : kTilePix;   // kDevSparseItems64: 64 (A/B)
    pl->tiles = (lv->N + pl->tile_pts - 1) / pl->tile_pts;
  }
  pl->groups = (pl->tiles + 3) / 4;
  pl->c128 = use_c128(lv) ? 1 : 0;
  // 3. the kernel: the first candidate that takes the launch (each fills its own choices: work items, grid, bands)
  if (!choose_strip(lv, kCUs, Bsel, pl) && !choose_quad(lv, kCUs, Bsel, pl)) choose_tile(lv, kCUs, Bsel, pl);
  // 4. the partial buffer
  layout_partials(pl, lv);
  return BANET_OK;
}

// ---- the gather launch as data --------------------------------------------------------------
// What gather.hip enqueues for one pass: plan_gather_steps lists every launch in order, with its kernel, template parameters, grid,
// block and LDS; the driver walks the list and decides nothing (tests/native/plan_host.cpp dumps it, tests/test_gather_steps_cpu.py
// pins it).

// The compiled instantiations, each list written once: the per-file launch code instantiates from these lists, plan_gather_steps takes
// "supported" from them and the host test program enumerates them.
#define BANET_GATHER_GENERIC_K_(X, vec, ch, grad) X(vec, ch, grad, 1, 0) X(vec, ch, grad, 2, 1) X(vec, ch, grad, 2, 2) X(vec, ch, grad, 1, 1) X(vec, ch, grad, 1, 2)
#define BANET_GATHER_GENERIC_C_(X, grad) \
  BANET_GATHER_GENERIC_K_(X, 2, 1, grad) BANET_GATHER_GENERIC_K_(X, 2, 2, grad) BANET_GATHER_GENERIC_K_(X, 1, 1, grad) BANET_GATHER_GENERIC_K_(X, 1, 2, grad)
#define BANET_GATHER_GENERIC_LIST(X) BANET_GATHER_GENERIC_C_(X, false) BANET_GATHER_GENERIC_C_(X, true)   // ba_gather_kernel<VEC, CH, GRAD, KVEC, KCH>: 4 x 2 x 5
#define BANET_GATHER_DIRECT_LIST(X) X(0) X(1) X(2)                                                         // ba_gather128_kernel<KV4>
#define BANET_GATHER_PATCH_LIST(X) X(0, 2, true) X(0, 2, false) X(1, 4, false) X(1, 2, false) X(1, 2, true) X(2, 2, true) X(2, 2, false)   // ba_gather128p_kernel<KV4, US, FS>
#define BANET_GATHER_STRIP_KV4_(X, kv4) X(kv4, 2, false) X(kv4, 4, false) X(kv4, 8, false) X(kv4, 4, true)
#define BANET_GATHER_STRIP_LIST(X) BANET_GATHER_STRIP_KV4_(X, 0) BANET_GATHER_STRIP_KV4_(X, 1) BANET_GATHER_STRIP_KV4_(X, 2)           // ba_gather128s_kernel<KV4, NCH, FP>
#define BANET_GATHER_QUAD_LIST(X) X(0) X(1) X(2)                                                           // ba_gather128q_kernel<KV4>

enum GatherStepKind {
  kGatherStepZero = 0,   // zero_iters_kernel on the tile-queue heads (t0 words)
  kGatherStepGeneric,    // ba_gather_kernel<t0 = VEC, t1 = CH, t2 = GRAD, t3 = KVEC, t4 = KCH>
  kGatherStepDirect,     // ba_gather128_kernel<t0 = KV4>
  kGatherStepPatch,      // ba_gather128p_kernel<t0 = KV4, t1 = US, t2 = FS>
  kGatherStepStrip,      // ba_gather128s_kernel<t0 = KV4, t1 = NCH, t2 = FP>
  kGatherStepQuad,       // ba_gather128q_kernel<t0 = KV4>
  kGatherStepFold,       // ba_fold_kernel
};
struct GatherStep {
  int kind;                  // GatherStepKind
  int t0, t1, t2, t3, t4;    // template parameters (kGatherStepZero: t0 = words to zero)
  int gx, gy, block;
  int lds;                   // dynamic LDS bytes
  int lds_attr;              // 1: the launch sets the function attribute for its dynamic LDS
};
constexpr int kGatherMaxSteps = 3;   // zero, the gather kernel, fold
struct GatherSteps {
  int n;
  GatherStep step[kGatherMaxSteps];
};

namespace plan_detail {

inline bool gather_step_compiled(const GatherStep& st) {
  bool found = false;
  switch (st.kind) {
    case kGatherStepGeneric:
#define BANET_X(vec, ch, grad, kvec, kch) found = found || (st.t0 == vec && st.t1 == ch && st.t2 == (grad ? 1 : 0) && st.t3 == kvec && st.t4 == kch);
      BANET_GATHER_GENERIC_LIST(BANET_X)
#undef BANET_X
      return found;
    case kGatherStepDirect:
#define BANET_X(kv4) found = found || st.t0 == kv4;
      BANET_GATHER_DIRECT_LIST(BANET_X)
#undef BANET_X
      return found;
    case kGatherStepPatch:
#define BANET_X(kv4, us, fs) found = found || (st.t0 == kv4 && st.t1 == us && st.t2 == (fs ? 1 : 0));
      BANET_GATHER_PATCH_LIST(BANET_X)
#undef BANET_X
      return found;
    case kGatherStepStrip:
#define BANET_X(kv4, nch, fp) found = found || (st.t0 == kv4 && st.t1 == nch && st.t2 == (fp ? 1 : 0));
      BANET_GATHER_STRIP_LIST(BANET_X)
#undef BANET_X
      return found;
    case kGatherStepQuad:
#define BANET_X(kv4) found = found || st.t0 == kv4;
      BANET_GATHER_QUAD_LIST(BANET_X)
#undef BANET_X
      return found;
  }
  return true;   // the zeroing and the fold are not templates
}

// 128-coefficient chunks of a basis row in the C = 128 kernels (K % 4 == 0, K <= 256), -1: no such kernel
inline int gather_kv4(int K) { return K == 0 ? 0 : ((K & 3) == 0 && K <= 128) ? 1 : ((K & 3) == 0 && K <= 256) ? 2 : -1; }

}  // namespace plan_detail

// The launches of one gather pass, in order.  pl: plan_gather's for lv; reset_queue: the pass zeroes the tile-queue heads first (the LM
// loop's later iterations find them zeroed by the solve kernel).  BANET_ERR_UNSUPPORTED (and an empty list) where the gather kernel
// is not compiled: the generic kernel at odd C above 128 or odd K above 128.
inline int plan_gather_steps(const banet_level_t* lv, const GatherPlan& pl, bool reset_queue, GatherSteps* out) {
  using namespace plan_detail;
  *out = GatherSteps{};
  const int pairs = npairs(lv), VB = lv->B * pairs, C = lv->C, K = lv->K;
  GatherStep k{kGatherStepGeneric, 0, 0, 0, 0, 0, pl.G, VB, kBlock, 0, 0};
  if (!pl.c128) {
    // two channels (coefficients) per lane where the count is even, one chunk of 64 lanes where it fits: up to 256 even, 128 odd
    const bool ceven = (C & 1) == 0, keven = (K & 1) == 0;
    k.t0 = ceven ? 2 : 1;
    k.t1 = C <= 64 * k.t0 ? 1 : C <= 128 * k.t0 ? 2 : 0;
    k.t2 = lv->tgt_has_grad ? 1 : 0;
    k.t3 = (K > 0 && keven) ? 2 : 1;
    k.t4 = K == 0 ? 0 : K <= 64 * k.t3 ? 1 : K <= 128 * k.t3 ? 2 : -1;
  } else if (pl.quad) {
    k.kind = kGatherStepQuad;
    k.t0 = gather_kv4(K);
  } else if (pl.strip) {
    // frame-parallel workgroups: `pairs` waves on dynamic LDS, 16-row segments only
    if ((pl.strip != 8 && pl.strip != 16 && pl.strip != 32) || (pl.strip_fp && (pl.strip != 16 || pairs < 2 || pairs > 7))) return BANET_ERR_INVALID_ARG;
    k.kind = kGatherStepStrip;
    k.t0 = gather_kv4(K);
    k.t1 = pl.strip / 4;   // NCH: 4-row chunks per segment
    k.t2 = pl.strip_fp ? 1 : 0;
    k.gy = lv->B;
    k.block = pl.strip_fp ? kWave * pairs : 128;
    k.lds = pl.strip_fp ? (int)strip_fp_lds_bytes(pairs, 4) : 0;
    k.lds_attr = k.lds > 64 * 1024 ? 1 : 0;
  } else if (pl.patch) {
    const int kv4 = gather_kv4(K);
    // kDevPatchOnePerCU (A/B experiment, experiments/README.md): 60 KB of unused dynamic LDS per workgroup -> ONE workgroup per CU
    // (one gather wave per SIMD), the occupancy a wave-specialised gather + MFMA-accumulator kernel would leave the gather;
    // kDevPatchUnits4: 4-step units, kDevPatchPacked: the packed patch with flat loads (A/B, experiments/README.md)
    const bool one = (lv->flags & kDevPatchOnePerCU) != 0, u4 = (lv->flags & kDevPatchUnits4) != 0, packed = (lv->flags & kDevPatchPacked) != 0;
    // the fixed-stride patch addresses the maps with 32-bit buffer offsets
    const bool small = (size_t)lv->H * lv->W * C * 4 < ((size_t)1 << 31) && (size_t)lv->N * C * 4 < ((size_t)1 << 31);
    k.kind = kGatherStepPatch;
    k.t0 = kv4;
    k.t1 = (kv4 == 1 && u4) ? 4 : 2;
    k.t2 = (small && !packed && !one && k.t1 == 2) ? 1 : 0;
    k.gy = pl.pairloop ? lv->B : VB;
    if (kv4 == 1 && k.t1 == 2 && one) k.lds = 60 * 1024, k.lds_attr = 1;   // the one instantiation the experiment runs on
  } else {
    k.kind = kGatherStepDirect;
    k.t0 = gather_kv4(K);
  }
  if (!gather_step_compiled(k)) return BANET_ERR_UNSUPPORTED;
  if (pl.c128 && reset_queue) out->step[out->n++] = GatherStep{kGatherStepZero, VB * 8, 0, 0, 0, 0, (VB * 8 + 63) / 64, 1, 64, 0, 0};
  out->step[out->n++] = k;
  if (pl.frows != pl.rows) out->step[out->n++] = GatherStep{kGatherStepFold, 0, 0, 0, 0, 0, pl.frows, VB, 256, 0, 0};
  return BANET_OK;
}

// ---- syrk ------------------------------------------------------------------------------
enum SyrkKind {          // SyrkPlan.direct
  kSyrkLds = 0,          // the LDS-tiled kernel (syrk_lds.hip), any K <= 256
  kSyrkMfma32 = 1,       // ba_syrk_direct_kernel (syrk_mfma32.hip: fp32 MFMA, A/B only)
  kSyrkBf16x6 = 2,       // ba_syrk_bf16x6_kernel (syrk_bf16x6.hip: K = 64 / 128, <= 4 target frames)
  kSyrkWide = 3,         // the jobs of syrk_wide.hip (K = 256, or K = 128 with more than 4 target frames)
};
struct SyrkPlan {
  int Gs, tiles, pstride, nb;
  int x3;       // ba_syrk_bf16x6_kernel, opt-in: three products instead of six (kDevSyrkThreeProducts)
  int direct;   // SyrkKind
  int f16;      // ba_syrk_bf16x6_kernel: the fp16 two-piece form is eligible (plan_syrk); f16_standalone: also in a single assembly pass
  int f16_standalone;
  size_t off_colmax, off_recmax;   // f16: [B][K] basis column maxima, [B][32][2] record maxima, inside the partial buffer
  size_t off_aux;        // kSyrkWide: per-pixel (s, r) sums over the frames, inside the partial buffer
  size_t partial_bytes;
};

constexpr long long kSyrkF16Pixels = 32LL * 76800;   // 320x240 x 32 windows, 640x480 x 8
inline size_t syrk_wide_aux_bytes(int B, int N, int pairs) { return pairs > 1 ? align_up((size_t)B * N * 2 * sizeof(float), 256) : 0; }

inline int nb_for_k(int K) {   // 16-column blocks of the LDS-tiled kernel
  if (K <= 0) return 0;
  if (K <= 16) return 1;
  if (K <= 32) return 2;
  if (K <= 64) return 4;
  if (K <= 128) return 8;
  if (K <= 256) return 16;
  return -1;
}

// Bsel: the batch the decisions are taken from (selection_batch); flags: banet_level_t.flags; cus: as plan_gather's kCUs
inline int plan_syrk(int B, int Bsel, int N, int K, int pairs, int flags, int cus, SyrkPlan* pl) {
  *pl = SyrkPlan{};
  pl->nb = nb_for_k(K);
  if (pl->nb < 0) return BANET_ERR_UNSUPPORTED;
  if (K == 0) return BANET_OK;   // no depth block: nothing runs
  pl->tiles = (N + kTilePix - 1) / kTilePix;
  // K = 64 / 128: barrier-free kernels, one wave per SIMD, one workgroup per CU in all: ba_syrk_bf16x6_kernel
  // (default) or ba_syrk_direct_kernel (fp32 MFMA; kDevSyrkNoBf16x6, A/B only)
  pl->direct = ((K == 64 || K == 128) && pairs <= 4) ? ((flags & kDevSyrkNoBf16x6) ? kSyrkMfma32 : kSyrkBf16x6) : kSyrkLds;
  // OPT-IN (kDevSyrkThreeProducts, K = 128): the three largest of the six products only -- a two-piece split, 16 significand bits per
  // operand, ~2^-16 relative error per product instead of 2^-24.  Not the product path and not what bench.py's `value` is measured
  // with (its dtype is "f32": fp32-exact products); measured beside it: profiles/r03_run31_*, DESIGN.md section 7.
  pl->x3 = (pl->direct == kSyrkBf16x6 && K == 128 && (flags & kDevSyrkThreeProducts)) ? 1 : 0;
  // K = 256, or K = 128 with more than 4 target frames: the job kernels of syrk_wide.hip (kDevSyrkNoBf16x6: the LDS-tiled kernel, A/B)
  if (!(flags & kDevSyrkNoBf16x6) && (K == 256 || (K == 128 && pairs > 4))) pl->direct = kSyrkWide;
  int target = (((pl->direct || pl->nb > 8) ? cus : 2 * cus) + Bsel - 1) / Bsel;   // Gs = partial rows per window: part of the arithmetic, hence from Bsel   // LDS kernel: 2 resident workgroups per CU (1 at K > 128)
  int G = pl->direct ? (N + 4 * 4 * 16 - 1) / (4 * 4 * 16) : pl->tiles / 4;   // direct: >= 16 quads per wave
  if (G > target) G = target;
  if (G < 1) G = 1;
  pl->Gs = G;
  pl->pstride = (int)align_up((size_t)(6 * pairs + 1) * K + (size_t)K * K, 4);
  pl->partial_bytes = align_up((size_t)B * G * pl->pstride * sizeof(float), 256);
  pl->off_aux = pl->partial_bytes;
  if (pl->direct == kSyrkWide) pl->partial_bytes += syrk_wide_aux_bytes(B, N, pairs);
  // The fp16 two-piece form of ba_syrk_bf16x6_kernel (half the MFMAs, 5 instead of 9 split instructions per two values, the same
  // accuracy class: ~2^-21 per product against the reference's fp32 GEMM) where the launch is throughput-bound -- at least
  // kSyrkF16Pixels pixels in all -- so that its two small pre-passes (basis column maxima once per level, record maxima per pass)
  // are noise.  LM loop (banet_lm_level_f32) only; the single assembly pass keeps the exact bf16 form unless kDevSyrkF16 asks
  // for this one (tests).  kDevNoSyrkF16: never (A/B).
  pl->f16 = ((pl->direct == kSyrkBf16x6 || pl->direct == kSyrkWide) && !pl->x3 && !(flags & kDevNoSyrkF16) && ((long long)N * Bsel >= kSyrkF16Pixels || (flags & kDevSyrkF16))) ? 1 : 0;
  pl->f16_standalone = (pl->f16 && (flags & kDevSyrkF16)) ? 1 : 0;
  pl->off_colmax = pl->partial_bytes;
  pl->off_recmax = pl->off_colmax + (pl->f16 ? align_up((size_t)B * K * sizeof(float), 256) : 0);
  if (pl->f16) pl->partial_bytes = pl->off_recmax + align_up((size_t)B * kRecMaxBlocks * 2 * sizeof(float), 256);
  return BANET_OK;
}

// ---- the SYRK launch as data ---------------------------------------------------------------
// What syrk.hip enqueues for one pass: plan_syrk_steps lists every launch -- pre-passes included -- in order, with its kernel,
// template parameters, job, grid and LDS; the driver walks the list and decides nothing (tests/native/plan_host.cpp dumps it,
// tests/test_syrk_steps_cpu.py pins it).

// The column maxima of the fp16 two-piece form in one pass of a level (the basis does not change within a level)
enum SyrkStats {
  kSyrkStatsExact = -1,         // the exact bf16 form
  kSyrkStatsF16Compute = 0,     // the fp16 form; compute the basis column maxima now
  kSyrkStatsF16InPlace = 1,     // the fp16 form; the maxima are in place
  kSyrkStatsExactHarvest = 2,   // the exact form that also leaves the maxima (first iteration of a level)
};
// iteration `it` of a level's LM loop: the first pass runs the exact form and leaves the maxima on the way (no extra pass over the
// basis), the later ones the fp16 form with them; a one-iteration call computes them up front instead
inline SyrkStats syrk_stats_of_iteration(const SyrkPlan& pl, int it, int max_iters) {
  if (!pl.f16) return kSyrkStatsExact;
  if (it > 0) return kSyrkStatsF16InPlace;
  return max_iters > 1 ? kSyrkStatsExactHarvest : kSyrkStatsF16Compute;
}
// a single assembly pass: the exact form unless kDevSyrkF16 asks for the fp16 one
inline SyrkStats syrk_stats_of_single_pass(const SyrkPlan& pl) { return pl.f16_standalone ? kSyrkStatsF16Compute : kSyrkStatsExact; }

// The lambda MLP as a role workgroup of the SYRK launch (ba_syrk_bf16x6_kernel only: one more workgroup per window, hidden behind
// the SYRK workgroups, off the solve kernel's critical path; C <= 256: the role's LDS scratch)
// ... and coarse levels at any batch (N <= kRoleSmallLevel pixels: their SYRK is a latency chain of 1-3 steps per wave, so a
// window's 7 workgroups take what 8 take, and the solve kernel loses the 19 us MLP: 40x30 .. 160x120 x 32 windows).
// Small batches only (B <= 8) otherwise: the SYRK kernel runs one workgroup per CU (512 registers per wave), so the role workgroups
// need CUs of their own -- at B = 32 (8 + 1 workgroups per window = 288 > 256 CUs) a second round of workgroups doubled
// the SYRK time (640x480 x 32: 1326 -> 2457 us); with B <= 8 one SYRK workgroup per window is given up where needed.
constexpr int kRoleSmallLevel = 19200;   // pixels: levels whose SYRK launch is latency-bound
struct SyrkRole {
  int on;
  int Gs;   // partial rows per window to launch and reduce with: pl.Gs, or one fewer (the workspace stays sized from pl.Gs)
};
// bundle_mlp: a bundle level whose damping comes from the lambda MLP; Bsel: selection_batch (the role changes Gs, i.e. the
// summation split: decided like every other selection); flags: banet_level_t.flags (kDevMlpInSolve: MLP inside the solve kernel, A/B)
inline SyrkRole plan_syrk_role(const SyrkPlan& pl, bool bundle_mlp, int Bsel, int N, int C, int flags, int cus) {
  const bool on = bundle_mlp && pl.direct == kSyrkBf16x6 && C <= 256 && (C & 3) == 0 &&
                  ((long long)Bsel * (pl.Gs + 1) <= cus || (Bsel <= 8 && pl.Gs >= 16) || (N <= kRoleSmallLevel && pl.Gs >= 4)) &&
                  !(flags & kDevMlpInSolve);
  return SyrkRole{on ? 1 : 0, (on && (long long)Bsel * (pl.Gs + 1) > cus) ? pl.Gs - 1 : pl.Gs};
}

// The compiled instantiations, each list written once: the launchers instantiate from these lists, plan_syrk_steps takes
// "supported" from them and the host test program enumerates them.
#define BANET_SYRK_LDS_LIST(X) X(1) X(2) X(4) X(8) X(16)       // ba_syrk_kernel<NB>
#define BANET_SYRK_FRAMES_LIST(X) X(1) X(2) X(3) X(4)          // PAIRS of the two register kernels, PT of the slice jobs: crossed with
#define BANET_SYRK_MFMA32_LIST(X) X(1) X(2)                    // ba_syrk_direct_kernel<KH, PAIRS>: KH
#define BANET_SYRK_BF16X6_LIST(X) X(1, 0) X(1, 1) X(1, 16) X(2, 0) X(2, 1) X(2, 3) X(2, 16)   // ba_syrk_bf16x6_kernel<KH, PAIRS, T0>: (KH, T0)
#define BANET_SYRK_SLICE_LIST(X) X(true, false) X(true, true) X(false, false) X(false, true)   // ba_syrk_slice_kernel<PT, DD, F16>: (DD, F16)
#define BANET_SYRK_RECT_LIST(X) X(false) X(true)               // ba_syrk_rect_kernel<F16>

enum SyrkStepKind {
  kSyrkStepZero = 0,   // zero_iters_kernel on the column maxima (j0 words)
  kSyrkStepColmax,     // ba_colmax_kernel
  kSyrkStepRecmax,     // ba_recmax_kernel
  kSyrkStepSrsum,      // ba_srsum_kernel
  kSyrkStepLds,        // ba_syrk_kernel<t0 = NB>, job j0 = pass
  kSyrkStepMfma32,     // ba_syrk_direct_kernel<t0 = KH, t1 = PAIRS>
  kSyrkStepBf16x6,     // ba_syrk_bf16x6_kernel<t0 = KH, t1 = PAIRS, t2 = T0>
  kSyrkStepSlice,      // ba_syrk_slice_kernel<t0 = PT, t1 = DD, t2 = F16>, job j0 = koff, j1 = p0
  kSyrkStepRect,       // ba_syrk_rect_kernel<t0 = F16>, job j0 = r0, j1 = c0
};
struct SyrkStep {
  int kind;           // SyrkStepKind
  int t0, t1, t2;     // template parameters
  int j0, j1;         // job parameters
  int gx, gy, block;
  int lds;            // dynamic LDS bytes
  int lds_attr;       // 1: more than 64 KB, the launch sets the function attribute
};
// The project's largest windows (8 target frames) need 10: zero, colmax, recmax, srsum, four slices, two rectangles at K = 256.  The
// API does not bound the frames of a window, and the LDS-tiled kernel takes one pass per frame: the list holds up to 64 frames in
// every form (wide jobs: 4 + 2 x 16 + 2); beyond that plan_syrk_steps refuses.
constexpr int kSyrkMaxSteps = 64;
struct SyrkSteps {
  int n;
  SyrkStep step[kSyrkMaxSteps];
};

namespace plan_detail {

inline bool syrk_step_compiled(const SyrkStep& st) {
  bool frames = false, found = false;
#define BANET_X(p) frames = frames || (st.kind == kSyrkStepSlice ? st.t0 : st.t1) == p;
  BANET_SYRK_FRAMES_LIST(BANET_X)
#undef BANET_X
  switch (st.kind) {
    case kSyrkStepLds:
#define BANET_X(nb) found = found || st.t0 == nb;
      BANET_SYRK_LDS_LIST(BANET_X)
#undef BANET_X
      return found;
    case kSyrkStepMfma32:
#define BANET_X(kh) found = found || st.t0 == kh;
      BANET_SYRK_MFMA32_LIST(BANET_X)
#undef BANET_X
      return found && frames;
    case kSyrkStepBf16x6:
#define BANET_X(kh, t) found = found || (st.t0 == kh && st.t2 == t);
      BANET_SYRK_BF16X6_LIST(BANET_X)
#undef BANET_X
      return found && frames;
    case kSyrkStepSlice:
#define BANET_X(dd, f16) found = found || (st.t1 == (dd ? 1 : 0) && st.t2 == (f16 ? 1 : 0));
      BANET_SYRK_SLICE_LIST(BANET_X)
#undef BANET_X
      return found && frames;
    case kSyrkStepRect:
#define BANET_X(f16) found = found || st.t0 == (f16 ? 1 : 0);
      BANET_SYRK_RECT_LIST(BANET_X)
#undef BANET_X
      return found;
  }
  return true;   // the pre-passes are not templates
}

// appends a step on (gx, B) workgroups; false where the list is full or the instantiation is not compiled
inline bool syrk_push(SyrkSteps* out, int kind, int t0, int t1, int t2, int j0, int j1, int gx, int gy, int block, size_t lds = 0) {
  const SyrkStep st{kind, t0, t1, t2, j0, j1, gx, gy, block, (int)lds, lds > 64 * 1024 ? 1 : 0};
  if (out->n >= kSyrkMaxSteps || !syrk_step_compiled(st)) return false;
  out->step[out->n++] = st;
  return true;
}

}  // namespace plan_detail

// The launches of one SYRK pass, in order.  pl: plan_syrk's; cus: as plan_gather's kCUs; role: plan_syrk_role's, or {0, pl.Gs}.
// BANET_ERR_UNSUPPORTED (and an empty list) where a step has no compiled kernel: nb outside BANET_SYRK_LDS_LIST (K = 0 among
// them: launch_assemble does not call the SYRK then), wide jobs at K other than 128 or 256.
inline int plan_syrk_steps(const SyrkPlan& pl, int B, int N, int K, int pairs, int cus, SyrkStats stats, const SyrkRole& role, SyrkSteps* out) {
  using namespace plan_detail;
  *out = SyrkSteps{};
  const int Gs = role.Gs;
  bool ok = true;
  if (pl.direct == kSyrkBf16x6 || pl.direct == kSyrkWide) {
    if (pl.direct == kSyrkWide && K != 128 && K != 256) return BANET_ERR_UNSUPPORTED;
    const bool maxima = pl.f16 && stats != kSyrkStatsExact;
    // THE difference between the two: ba_syrk_bf16x6_kernel<.., .., 1> harvests the column maxima while it runs the exact form; the
    // wide jobs have no such variant, so "exact form that also leaves the maxima" is, for them, a colmax pass plus the fp16 form
    // already on that iteration
    const bool harvest = maxima && stats == kSyrkStatsExactHarvest && pl.direct == kSyrkBf16x6;
    const bool f16 = maxima && !harvest;
    const bool colmax = f16 && stats != kSyrkStatsF16InPlace;
    if (harvest || colmax) ok = ok && syrk_push(out, kSyrkStepZero, 0, 0, 0, B * K, 0, (B * K + 63) / 64, 1, 64);
    if (colmax) ok = ok && syrk_push(out, kSyrkStepColmax, 0, 0, 0, 0, 0, std::max(1, std::min((N + 255) / 256, (8 * cus + B - 1) / B)), B, 256);
    if (f16) ok = ok && syrk_push(out, kSyrkStepRecmax, 0, 0, 0, 0, 0, kRecMaxBlocks, B, 256);
    if (pl.direct == kSyrkBf16x6) {
      const int T0 = harvest ? 1 : f16 ? 16 : pl.x3 ? 3 : 0;
      ok = ok && syrk_push(out, kSyrkStepBf16x6, K / 64, pairs, T0, 0, 0, Gs + role.on, B, kBlock);
    } else {
      // s and r summed over the window's frames by a small pre-pass, so that the jobs do not depend on the number of frames
      if (pairs > 1) ok = ok && syrk_push(out, kSyrkStepSrsum, 0, 0, 0, 0, 0, (N + 255) / 256, B, 256);
      for (int koff = 0; koff < K; koff += 128)        // the symmetric 128 x 128 diagonal slices, H_cd of up to 4 frames each
        for (int p0 = 0; p0 < pairs; p0 += 4)
          ok = ok && syrk_push(out, kSyrkStepSlice, std::min(pairs - p0, 4), p0 == 0 ? 1 : 0, f16 ? 1 : 0, koff, p0, Gs, B, kBlock);
      for (int r0 = 0; r0 < K; r0 += 128)              // off-diagonal 128 x 64 rectangles above the diagonal slices
        for (int c0 = r0 + 128; c0 < K; c0 += 64) ok = ok && syrk_push(out, kSyrkStepRect, f16 ? 1 : 0, 0, 0, r0, c0, Gs, B, kBlock);
    }
  } else if (pl.direct == kSyrkMfma32) {
    ok = syrk_push(out, kSyrkStepMfma32, K / 64, pairs, 0, 0, 0, Gs, B, kBlock);
  } else {
    // LDS-tiled kernel: one pass per pair (H_dd / Atb_d in pass 0); [2][64][KP] basis rows + [2][64][8] records, or the epilogue's [4][8][KPAD]
    const size_t KPAD = (size_t)pl.nb * 16, KP = KPAD + 16;
    const size_t lds = std::max((size_t)2 * kTilePix * KP + 2 * kTilePix * 8, (size_t)4 * 8 * KPAD) * sizeof(float);
    for (int pass = 0; pass < pairs; ++pass) ok = ok && syrk_push(out, kSyrkStepLds, pl.nb, 0, 0, pass, 0, Gs, B, kBlock, lds);
  }
  if (!ok) *out = SyrkSteps{};
  return ok ? BANET_OK : BANET_ERR_UNSUPPORTED;
}

// ---- one assembly pass = gather + syrk + reduce -----------------------------------------
struct AsmPlan {
  GatherPlan g;
  SyrkPlan s;
  int P;
  size_t ws_bytes;      // gather partials + records + syrk partials
  size_t off_rec, off_spart;
};

inline int plan_assemble(const banet_level_t* lv, int cus, AsmPlan* pl) {
  *pl = AsmPlan{};
  int rc = plan_gather(lv, cus, &pl->g);
  if (rc != BANET_OK) return rc;
  rc = plan_syrk(lv->B, selection_batch(lv), lv->N, lv->K, npairs(lv), lv->flags, cus, &pl->s);
  if (rc != BANET_OK) return rc;
  pl->P = 6 * npairs(lv) + lv->K;
  pl->off_rec = pl->g.partial_bytes;
  pl->off_spart = pl->off_rec + pl->g.rec_bytes;
  pl->ws_bytes = pl->off_spart + pl->s.partial_bytes;
  return BANET_OK;
}

}  // namespace banet
