// host build of the solve's plan (banet_amd/csrc/solve_plan.hpp) for tests/test_solve_plan_cpu.py: the method, the LDS-or-workspace
// switch and the LDS layout of every shape, asked of the code itself.  No ROCm needed.
#include "../../banet_amd/csrc/solve_plan.hpp"

#define SOLVE_PLAN_FIELDS(X)                                                                                                   \
  X(rc) X(P) X(C) X(method) X(big) X(ld) X(arows) X(ldw) X(off_A) X(off_X) X(off_H0) X(off_H1) X(off_Avg) X(off_Red) X(off_Scal) \
  X(off_Part) X(off_Perm) X(end) X(lds_attr) X(lds) X(big_floats)

#define SOLVE_PLAN_CONSTANTS(X)                                                                                                \
  X(kSolveThreads) X(kSolveWaves) X(kGrid) X(kPanel) X(kSolveLdsMax) X(kLdsAttrAbove) X(kSolveMlpPartFloats) X(kSolveRedFloats)  \
  X(kSolveScalAt) X(kSolvePermTail) X(kLuScratchFloats) X(kPcgRhs) X(kPcgRedFloats) X(kLdltFixedFloats) X(kSolveQr6)            \
  X(kSolveInverse6) X(kSolveLu) X(kSolveCgLdlt) X(kSolveLdlt) X(kDevSolveLdltOnly)

extern "C" const char* banet_test_solve_plan_fields() {
#define X(f) #f " "
  return "desc_ints=6 " SOLVE_PLAN_FIELDS(X);
#undef X
}

extern "C" const char* banet_test_solve_plan_constant_names() {
#define X(f) #f " "
  return SOLVE_PLAN_CONSTANTS(X);
#undef X
}

extern "C" void banet_test_solve_plan_constants(int64_t* out) {
#define X(f) *out++ = (int64_t)banet::f;
  SOLVE_PLAN_CONSTANTS(X)
#undef X
}

// one plan per row of `desc`: which (0: plan_solve, 1: plan_spd_solve), variant, P, C, lm.solver, flags.  out: one row of
// SOLVE_PLAN_FIELDS
extern "C" void banet_test_solve_plan_sweep(const int64_t* desc, int n, int64_t* out) {
  for (int i = 0; i < n; ++i, desc += 6) {
    struct : banet::SolvePlan { int rc; } p;
    p.rc = desc[0] ? banet::plan_spd_solve((int)desc[2], &p)
                   : banet::plan_solve((int)desc[1], (int)desc[2], (int)desc[3], (int)desc[4], (int)desc[5], &p);
#define X(f) *out++ = (int64_t)p.f;
    SOLVE_PLAN_FIELDS(X)
#undef X
  }
}
