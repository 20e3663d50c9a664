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

// ---- the SYRK step list and the role decision (tests/test_syrk_steps_cpu.py) -------------------------------------------------------
#include <cstdio>
#include <set>

namespace {

std::string fmt(const char* f, int a = 0, int b = 0, int c = 0, int d = 0) {
  char buf[96];
  snprintf(buf, sizeof buf, f, a, b, c, d);
  return buf;
}
const char* tf(int v) { return v ? "true" : "false"; }

// the kernel a step names, spelled as in the sources
std::string step_kernel(const banet::SyrkStep& st) {
  switch (st.kind) {
    case banet::kSyrkStepZero: return "zero_iters_kernel";
    case banet::kSyrkStepColmax: return "ba_colmax_kernel";
    case banet::kSyrkStepRecmax: return "ba_recmax_kernel";
    case banet::kSyrkStepSrsum: return "ba_srsum_kernel";
    case banet::kSyrkStepLds: return fmt("ba_syrk_kernel<%d>", st.t0);
    case banet::kSyrkStepMfma32: return fmt("ba_syrk_direct_kernel<%d, %d>", st.t0, st.t1);
    case banet::kSyrkStepBf16x6: return fmt("ba_syrk_bf16x6_kernel<%d, %d, %d>", st.t0, st.t1, st.t2);
    case banet::kSyrkStepSlice: return fmt("ba_syrk_slice_kernel<%d, ", st.t0) + tf(st.t1) + ", " + tf(st.t2) + ">";
    case banet::kSyrkStepRect: return std::string("ba_syrk_rect_kernel<") + tf(st.t0) + ">";
  }
  return "?";
}
// "kernel job(..) grid(x, y) block n lds n[ attr]": job = words to zero / pass / (koff, p0) / (r0, c0), empty for the others
std::string step_line(const banet::SyrkStep& st) {
  std::string job = "job()";
  if (st.kind == banet::kSyrkStepZero || st.kind == banet::kSyrkStepLds) job = fmt("job(%d)", st.j0);
  if (st.kind == banet::kSyrkStepSlice || st.kind == banet::kSyrkStepRect) job = fmt("job(%d, %d)", st.j0, st.j1);
  return step_kernel(st) + " " + job + fmt(" grid(%d, %d) block %d lds %d", st.gx, st.gy, st.block, st.lds) + (st.lds_attr ? " attr" : "");
}

struct LevelSteps {
  int rc_plan, rc;
  banet::SyrkRole role;
  banet::SyrkSteps steps;
};
// role_mode 0: no role; 1: decided as for a bundle level whose damping comes from the lambda MLP.  stats: a SyrkStats value, or
// kStatsSinglePass = what a single assembly pass of the level runs with
constexpr int kStatsSinglePass = 100;
LevelSteps level_steps(const int32_t* desc, int cus, int stats, int role_mode) {
  banet_level_t lv = {};
  lv.B = desc[0], lv.N = desc[1], lv.C = desc[2], lv.K = desc[3], lv.H = desc[4], lv.W = desc[5];
  lv.dense = desc[6], lv.tgt_has_grad = desc[7], lv.pairs = desc[8], lv.policy = desc[9], lv.flags = desc[10];
  lv.scale = 1.f;
  LevelSteps r = {};
  banet::AsmPlan p;
  r.rc_plan = r.rc = banet::plan_assemble(&lv, cus, &p);
  if (r.rc_plan != BANET_OK) return r;
  r.role = banet::plan_syrk_role(p.s, role_mode != 0, banet::selection_batch(&lv), lv.N, lv.C, lv.flags, cus);
  const banet::SyrkStats mode = stats == kStatsSinglePass ? banet::syrk_stats_of_single_pass(p.s) : (banet::SyrkStats)stats;
  r.rc = banet::plan_syrk_steps(p.s, lv.B, lv.N, lv.K, banet::npairs(&lv), cus, mode, r.role, &r.steps);
  return r;
}

}  // namespace

// one line per level of `desc` (rows as banet_test_plan_sweep's): "rc=<plan_syrk_steps' code> role=<on> Gs=<rows launched>" and then
// "; <step>" per launch, in order.  Returns the bytes `text` needs (with its terminator).
extern "C" size_t banet_test_syrk_steps(const int32_t* desc, int n, int cus, int stats, int role_mode, char* text, size_t cap) {
  std::string all;
  for (int i = 0; i < n; ++i, desc += kDescInts) {
    const LevelSteps r = level_steps(desc, cus, stats, role_mode);
    all += fmt("rc=%d role=%d Gs=%d", r.rc, r.role.on, r.role.Gs);
    for (int k = 0; k < r.steps.n; ++k) all += "; " + step_line(r.steps.step[k]);
    all += "\n";
  }
  if (text && cap > all.size()) all.copy(text, all.size()), text[all.size()] = 0;
  return all.size() + 1;
}

// the same over many levels without the text: out = (plan_assemble's code, plan_syrk_steps' code, steps) per level; returns the
// distinct kernels the steps named, one per line
extern "C" const char* banet_test_syrk_steps_sweep(const int32_t* desc, int n, int cus, int stats, int role_mode, int32_t* out) {
  static std::string s;
  std::set<std::string> seen;
  for (int i = 0; i < n; ++i, desc += kDescInts) {
    const LevelSteps r = level_steps(desc, cus, stats, role_mode);
    *out++ = r.rc_plan, *out++ = r.rc, *out++ = r.steps.n;
    for (int k = 0; k < r.steps.n; ++k) seen.insert(step_kernel(r.steps.step[k]));
  }
  s.clear();
  for (const std::string& k : seen) s += k + "\n";
  return s.c_str();
}

extern "C" int banet_test_syrk_max_steps() { return banet::kSyrkMaxSteps; }

// every instantiation of the X-macro lists, one per line
extern "C" const char* banet_test_syrk_instantiations() {
  static std::string s;
  s.clear();
#define X(nb) s += fmt("ba_syrk_kernel<%d>\n", nb);
  BANET_SYRK_LDS_LIST(X)
#undef X
  // (frames first: the list of frame counts is crossed with each of the three lists below)
#define FRAMES(p) s += fmt(f_, p, a_, b_);
#define X(kh)                                                 \
  {                                                           \
    const char* f_ = "ba_syrk_direct_kernel<%2$d, %1$d>\n";   \
    const int a_ = kh, b_ = 0;                                \
    BANET_SYRK_FRAMES_LIST(FRAMES)                            \
  }
  BANET_SYRK_MFMA32_LIST(X)
#undef X
#define X(kh, t)                                                    \
  {                                                                 \
    const char* f_ = "ba_syrk_bf16x6_kernel<%2$d, %1$d, %3$d>\n";   \
    const int a_ = kh, b_ = t;                                      \
    BANET_SYRK_FRAMES_LIST(FRAMES)                                  \
  }
  BANET_SYRK_BF16X6_LIST(X)
#undef X
#define X(dd, f16)                                                        \
  {                                                                       \
    const char* f_ = "ba_syrk_slice_kernel<%1$d, " #dd ", " #f16 ">\n";   \
    const int a_ = 0, b_ = 0;                                             \
    BANET_SYRK_FRAMES_LIST(FRAMES)                                        \
  }
  BANET_SYRK_SLICE_LIST(X)
#undef X
#undef FRAMES
#define X(f16) s += "ba_syrk_rect_kernel<" #f16 ">\n";
  BANET_SYRK_RECT_LIST(X)
#undef X
  return s.c_str();
}

// plan_syrk_role on hand-made plans: one row of `desc` = Gs, direct, bundle_mlp, Bsel, N, C, flags, cus; out = (on, Gs) per row
extern "C" void banet_test_syrk_role(const int32_t* desc, int n, int32_t* out) {
  for (int i = 0; i < n; ++i, desc += 8) {
    banet::SyrkPlan pl = {};
    pl.Gs = desc[0], pl.direct = desc[1];
    const banet::SyrkRole r = banet::plan_syrk_role(pl, desc[2] != 0, desc[3], desc[4], desc[5], desc[6], desc[7]);
    *out++ = r.on, *out++ = r.Gs;
  }
}

// the statistics mode of iteration `it` of `max_iters` and of a single pass, for a plan with the given f16 / f16_standalone
extern "C" void banet_test_syrk_stats(int f16, int f16_standalone, int it, int max_iters, int32_t* out) {
  banet::SyrkPlan pl = {};
  pl.f16 = f16, pl.f16_standalone = f16_standalone;
  out[0] = banet::syrk_stats_of_iteration(pl, it, max_iters);
  out[1] = banet::syrk_stats_of_single_pass(pl);
}

// ---- the gather step list (tests/test_gather_steps_cpu.py) --------------------------------------------------------------------------
namespace {

std::string gather_step_kernel(const banet::GatherStep& st) {
  switch (st.kind) {
    case banet::kGatherStepZero: return "zero_iters_kernel";
    case banet::kGatherStepGeneric:
      return fmt("ba_gather_kernel<%d, %d, ", st.t0, st.t1) + tf(st.t2) + fmt(", %d, %d>", st.t3, st.t4);
    case banet::kGatherStepDirect: return fmt("ba_gather128_kernel<%d>", st.t0);
    case banet::kGatherStepPatch: return fmt("ba_gather128p_kernel<%d, %d, ", st.t0, st.t1) + tf(st.t2) + ">";
    case banet::kGatherStepStrip: return fmt("ba_gather128s_kernel<%d, %d, ", st.t0, st.t1) + tf(st.t2) + ">";
    case banet::kGatherStepQuad: return fmt("ba_gather128q_kernel<%d>", st.t0);
    case banet::kGatherStepFold: return "ba_fold_kernel";
  }
  return "?";
}
// "kernel[ words(n)] grid(x, y) block n lds n[ attr]": words = what the zeroing step clears
std::string gather_step_line(const banet::GatherStep& st) {
  return gather_step_kernel(st) + (st.kind == banet::kGatherStepZero ? fmt(" words(%d)", st.t0) : std::string()) +
         fmt(" grid(%d, %d) block %d lds %d", st.gx, st.gy, st.block, st.lds) + (st.lds_attr ? " attr" : "");
}

struct LevelGatherSteps {
  int rc_plan, rc;
  banet::GatherSteps steps;
};
LevelGatherSteps level_gather_steps(const int32_t* desc, int cus, int reset_queue) {
  banet_level_t lv = {};
  lv.B = desc[0], lv.N = desc[1], lv.C = desc[2], lv.K = desc[3], lv.H = desc[4], lv.W = desc[5];
  lv.dense = desc[6], lv.tgt_has_grad = desc[7], lv.pairs = desc[8], lv.policy = desc[9], lv.flags = desc[10];
  lv.scale = 1.f;
  LevelGatherSteps r = {};
  banet::GatherPlan g;
  r.rc_plan = r.rc = banet::plan_gather(&lv, cus, &g);
  if (r.rc_plan == BANET_OK) r.rc = banet::plan_gather_steps(&lv, g, reset_queue != 0, &r.steps);
  return r;
}

}  // namespace

// one line per level of `desc` (rows as banet_test_plan_sweep's): "rc=<plan_gather_steps' code>" and then "; <step>" per launch, in
// order.  Returns the bytes `text` needs (with its terminator).
extern "C" size_t banet_test_gather_steps(const int32_t* desc, int n, int cus, int reset_queue, char* text, size_t cap) {
  std::string all;
  for (int i = 0; i < n; ++i, desc += kDescInts) {
    const LevelGatherSteps r = level_gather_steps(desc, cus, reset_queue);
    all += fmt("rc=%d", r.rc);
    for (int k = 0; k < r.steps.n; ++k) all += "; " + gather_step_line(r.steps.step[k]);
    all += "\n";
  }
  if (text && cap > all.size()) all.copy(text, all.size()), text[all.size()] = 0;
  return all.size() + 1;
}

// the same over many levels without the text: out = (plan_gather's code, plan_gather_steps' code, steps) per level; returns the distinct
// kernels the steps named, one per line
extern "C" const char* banet_test_gather_steps_sweep(const int32_t* desc, int n, int cus, int reset_queue, int32_t* out) {
  static std::string s;
  std::set<std::string> seen;
  for (int i = 0; i < n; ++i, desc += kDescInts) {
    const LevelGatherSteps r = level_gather_steps(desc, cus, reset_queue);
    *out++ = r.rc_plan, *out++ = r.rc, *out++ = r.steps.n;
    for (int k = 0; k < r.steps.n; ++k) seen.insert(gather_step_kernel(r.steps.step[k]));
  }
  s.clear();
  for (const std::string& k : seen) s += k + "\n";
  return s.c_str();
}

extern "C" int banet_test_gather_max_steps() { return banet::kGatherMaxSteps; }

// every instantiation of the X-macro lists, one per line
extern "C" const char* banet_test_gather_instantiations() {
  static std::string s;
  s.clear();
#define X(vec, ch, grad, kvec, kch) s += "ba_gather_kernel<" #vec ", " #ch ", " #grad ", " #kvec ", " #kch ">\n";
  BANET_GATHER_GENERIC_LIST(X)
#undef X
#define X(kv4) s += "ba_gather128_kernel<" #kv4 ">\n";
  BANET_GATHER_DIRECT_LIST(X)
#undef X
#define X(kv4, us, fs) s += "ba_gather128p_kernel<" #kv4 ", " #us ", " #fs ">\n";
  BANET_GATHER_PATCH_LIST(X)
#undef X
#define X(kv4, nch, fp) s += "ba_gather128s_kernel<" #kv4 ", " #nch ", " #fp ">\n";
  BANET_GATHER_STRIP_LIST(X)
#undef X
#define X(kv4) s += "ba_gather128q_kernel<" #kv4 ">\n";
  BANET_GATHER_QUAD_LIST(X)
#undef X
  return s.c_str();
}

// plan_gather_steps on a hand-made plan (what plan_gather never produces): desc = one level row, then strip, strip_fp; returns its code
extern "C" int banet_test_gather_steps_of_strip(const int32_t* desc, int strip, int strip_fp) {
  banet_level_t lv = {};
  lv.B = desc[0], lv.N = desc[1], lv.C = desc[2], lv.K = desc[3], lv.H = desc[4], lv.W = desc[5];
  lv.dense = desc[6], lv.tgt_has_grad = desc[7], lv.pairs = desc[8], lv.policy = desc[9], lv.flags = desc[10];
  banet::GatherPlan g = {};
  g.c128 = 1, g.G = 1, g.strip = strip, g.strip_fp = strip_fp;
  banet::GatherSteps steps;
  const int rc = banet::plan_gather_steps(&lv, g, false, &steps);
  return rc != BANET_OK && steps.n != 0 ? 1 : rc;
}

// the dynamic LDS of a frame-parallel strip workgroup
extern "C" size_t banet_test_strip_fp_lds_bytes(int pairs, int nch) { return banet::strip_fp_lds_bytes(pairs, nch); }
