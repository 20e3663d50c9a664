// host build of the launch plans (banet_amd/csrc/plan.hpp, dev_flags.hpp) for tests/test_plan_cpu.py: no ROCm needed
#include <string>

#include "../../banet_amd/csrc/plan.hpp"

// one level per row of `desc`: B, N, C, K, H, W, dense, tgt_has_grad, pairs, policy, flags
constexpr int kDescInts = 11;
// one row of `out` per level: the return code and every field of the three plan structs
#define PLAN_FIELDS(X)                                                                                                      \
  X(rc) X(g.G) X(g.tiles) X(g.tiles_x) X(g.tiles_y) X(g.groups) X(g.pstride) X(g.c128) X(g.patch) X(g.strip) X(g.quad)      \
  X(g.strip_fp) X(g.rows) X(g.frows) X(g.nbands) X(g.pairloop) X(g.qshift) X(g.tile_pts) X(g.off_fold) X(g.off_queue)       \
  X(g.partial_bytes) X(g.rec_bytes) X(s.Gs) X(s.tiles) X(s.pstride) X(s.nb) X(s.x3) X(s.direct) X(s.f16) X(s.f16_standalone) \
  X(s.off_colmax) X(s.off_recmax) X(s.off_aux) X(s.partial_bytes) X(P) X(ws_bytes) X(off_rec) X(off_spart)

extern "C" const char* banet_test_plan_fields() {
#define X(f) #f " "
  return "desc_ints=11 " PLAN_FIELDS(X);
#undef X
}

extern "C" void banet_test_plan_sweep(const int32_t* desc, int n, int cus, int64_t* out) {
  for (int i = 0; i < n; ++i, desc += kDescInts) {
    banet_level_t lv = {};
    lv.B = desc[0], lv.N = desc[1], lv.C = desc[2], lv.K = desc[3], lv.H = desc[4], lv.W = desc[5];
    lv.dense = desc[6], lv.tgt_has_grad = desc[7], lv.pairs = desc[8], lv.policy = desc[9], lv.flags = desc[10];
    lv.scale = 1.f;
    struct : banet::AsmPlan { int rc; } p;
    p.rc = banet::plan_assemble(&lv, cus, &p);
#define X(f) *out++ = (int64_t)p.f;
    PLAN_FIELDS(X)
#undef X
  }
}

// every name of dev_flags.hpp with its value, "name=value" per line (compared with the block in banet_amd/_capi.py)
#define DEV_FLAGS(X)                                                                                                        \
  X(kDevAblateTaps) X(kDevAblateSourceRows) X(kDevSparseItems64) X(kDevAblateDepthDot) X(kDevAblateGather)                  \
  X(kDevNoQuarterTiles) X(kDevGenericGather) X(kDevDirectGather) X(kDevPatchNoStaging) X(kDevSyrkNoBf16x6)                  \
  X(kDevForcePatchGather) X(kDevQuarterTiles) X(kDevPatchNoStagger) X(kDevPatchPairLoop) X(kDevPatchOnePerCU)               \
  X(kDevPatchUnits4) X(kDevMlpInSolve) X(kDevPatchPacked) X(kDevPatchColumnMajor) X(kDevForceStripGather)                   \
  X(kDevNoStripGather) X(kDevStripDirectRows) X(kDevStripRows32) X(kDevStripFrameLoop) X(kDevSolveLdltOnly) X(kDevSyrkF16)  \
  X(kDevForceQuadGather) X(kDevAdjFp32Mfma) X(kDevAdjPixelPerWave) X(kDevAdjTexelPerWave) X(kDevSyrkThreeProducts)          \
  X(kDevNoQuadGather) X(kDevNoSyrkF16)

extern "C" const char* banet_test_dev_flags() {
  static std::string s;
  s.clear();
#define X(n) s += #n "=" + std::to_string((unsigned)banet::n) + "\n";
  DEV_FLAGS(X)
#undef X
  return s.c_str();
}
