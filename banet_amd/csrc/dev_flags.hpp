// Every bit of banet_level_t.flags that a source of libbanet_hip.so consults, named once.  Plain C++: the host-only plans
// (plan.hpp, adjoint_plan.hpp), the kernels and the CPU tests (tests/native/plan_host.cpp) read the same names; banet_amd/_capi.py repeats
// them for Python and tests/test_plan_cpu.py compares the two.  0 in production.  The seven public bits are the
// BANET_FLAG_* values of include/banet_hip.h; the others are development switches (A/B experiments, parity tests,
// tools/prof_assemble.py) with no promise of stability.
#pragma once
#include "../../include/banet_hip.h"

namespace banet {

enum DevFlags : unsigned {
  // ---- ablation (tools/prof_assemble.py): switch phases of a gather kernel off; the results are wrong ----
  kDevAblateTaps = 1u << 0,          // every tap reads one fixed interior texel / point (generic kernel; BANET_ABLATE builds of the tile kernels)
  kDevAblateSourceRows = 1u << 1,    // patch kernel, BANET_ABLATE builds: every source row = pixels 0..3
  kDevSparseItems64 = 1u << 1,       // plan: sparse points stay 64 per wave item, never 16 (A/B; the bit's meaning outside BANET_ABLATE builds)
  kDevAblateDepthDot = 1u << 2,      // no depth dot (generic kernel; BANET_ABLATE builds of the patch kernel)
  kDevAblateGather = 1u << 3,        // no gather loop (generic kernel) / no tap arithmetic (BANET_ABLATE builds of the patch kernel)
  // ---- gather selection and its A/B switches ----
  kDevNoQuarterTiles = 1u << 4,      // direct tile kernel: never quarter-tile work items (A/B)
  kDevGenericGather = 1u << 5,       // force the generic kernel where the C = 128 kernels would run (A/B experiments only)
  kDevDirectGather = 1u << 6,        // the direct tile kernel instead of the patch kernel (A/B); also keeps the 4x4-item kernel off
  kDevPatchNoStaging = 1u << 7,      // patch kernel: no pixel group stages its bounding box in LDS (A/B)
  kDevSyrkNoBf16x6 = 1u << 8,        // SYRK: ba_syrk_direct_kernel (fp32 MFMA) / the LDS-tiled kernel instead of the bf16x6 / wide kernels (A/B)
  kDevForcePatchGather = BANET_FLAG_FORCE_PATCH_GATHER,   // bit 9: the patch kernel at any size (parity tests)
  kDevQuarterTiles = 1u << 10,       // force quarter-tile work items (A/B); with kDevForceStripGather: 8-row strip segments (parity tests)
  kDevPatchNoStagger = 1u << 11,     // patch kernel: the waves of a workgroup start together (A/B)
  kDevPatchPairLoop = 1u << 12,      // patch kernel: force the loop over a window's target frames inside a tile (parity tests)
  kDevPatchOnePerCU = 1u << 13,      // patch kernel: 60 KB of unused dynamic LDS -> one workgroup per CU (A/B experiment, experiments/README.md)
  kDevPatchUnits4 = 1u << 14,        // patch kernel: 4-step units (A/B, experiments/README.md)
  kDevMlpInSolve = 1u << 15,         // LM loop: the lambda MLP inside the solve kernel, no role workgroups in the SYRK launch (A/B)
  kDevPatchPacked = 1u << 16,        // patch kernel: the packed patch with flat loads (A/B)
  kDevPatchColumnMajor = 1u << 17,   // patch kernel, 2-step units: column-major unit order (experiment)
  kDevForceStripGather = BANET_FLAG_FORCE_STRIP_GATHER,   // bit 18: the strip kernel at any size (parity tests)
  kDevNoStripGather = 1u << 19,      // never the strip kernel (A/B)
  kDevStripDirectRows = 1u << 20,    // strip kernel: every pixel row takes the direct (window-less) path (parity tests)
  kDevStripRows32 = 1u << 21,        // strip kernel: 32-row segments (A/B, parity tests)
  kDevStripFrameLoop = 1u << 22,     // strip kernel: a window's frames looped over inside one wave, no frame-parallel workgroups (A/B)
  kDevSolveLdltOnly = 1u << 23,      // solve: blocked LDL^T only, no conjugate gradients (A/B and parity tests)
  kDevSyrkF16 = BANET_FLAG_SYRK_F16,                      // bit 24: the fp16 two-piece SYRK also in a single assembly pass and at any launch size
  kDevForceQuadGather = BANET_FLAG_FORCE_QUAD_GATHER,     // bit 25: the 4x4-pixel-item kernel at any size (parity tests, A/B)
  // ---- dense adjoint (read by its plan, adjoint_plan.hpp; kernels: adjoint_seed / _pixel / _map.hip) ----
  kDevAdjFp32Mfma = 1u << 26,        // the fp32-MFMA kernel instead of the bf16x6 form of the GEMM-shaped piece (A/B)
  kDevAdjPixelPerWave = 1u << 27,    // one pixel per wave (A/B)
  kDevAdjTexelPerWave = 1u << 28,    // target-map kernel: one texel per wave (A/B)
  kDevSyrkThreeProducts = BANET_FLAG_SYRK_THREE_PRODUCTS, // bit 29: opt-in, K = 128: the three largest of the six bf16 products only
  kDevNoQuadGather = BANET_FLAG_NO_QUAD_GATHER,           // bit 30: never the 4x4-pixel-item kernel
  kDevNoSyrkF16 = (unsigned)BANET_FLAG_NO_SYRK_F16,       // bit 31: never the fp16 two-piece SYRK (A/B)
};

}  // namespace banet
