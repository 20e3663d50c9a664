// The host-side plan of the solve-and-update kernel (solve.hip) and of banet_spd_solve_f32 (spd_solve.hip): which solver runs for
// a shape, whether the matrix lives in LDS or in the caller's workspace, the strides, and where every region of the dynamic LDS
// begins.  The kernels set their pointers as smem + offset and dispatch on `method`; the launchers read lds / lds_attr; the
// workspace queries read big / big_floats.  Host-only, plain C++17 (no HIP include), in the manner of prior_plan.hpp:
// tests/native/solve_plan_host.cpp compiles this header with g++ (tests/test_solve_plan_cpu.py sweeps it).
#pragma once
#include "plan.hpp"

namespace banet {

constexpr int kSolveThreads = 1024;   // 16 waves: 4 per SIMD, so the latency-bound phases overlap
constexpr int kSolveWaves = kSolveThreads / kWave;
constexpr int kGrid = 32;             // 2-D cyclic thread grid of the register-resident LU: systems of up to kGrid - 1 unknowns
constexpr int kPanel = 16;            // columns per panel of the blocked LDL^T
constexpr size_t kSolveLdsMax = 160 * 1024;    // usable LDS of a workgroup
constexpr size_t kLdsAttrAbove = 64 * 1024;    // more dynamic LDS than this: hipFuncAttributeMaxDynamicSharedMemorySize before the launch

constexpr int kSolveMlpPartFloats = 4 * kSolveThreads;   // mlp_layer's partial sums: input slices x outputs <= 4 per thread
constexpr int kSolveRedFloats = 24;   // block_sum's per-wave values [kSolveWaves], 4 spare, then the 4 scalars at kSolveScalAt
constexpr int kSolveScalAt = 20;      // pivot index, pivot reciprocal, the accept / terminate flag, spare
constexpr int kSolvePermTail = 8;     // spare ints behind the LU's row order [P]
// what each solver carves from the scratch region (sPart), in floats
constexpr int kLuScratchFloats = 2 * kGrid + kGrid + kGrid;       // two column buffers, the pivot row, the used-row marks (ints)
constexpr int kPcgRhs = 2;            // right-hand sides per sweep (b1 and a12 of the Schur step): one search direction each
constexpr int kPcgRedFloats = 2 * 4 * kSolveWaves;                // two reduction buffers used alternately, 4 values per wave
constexpr int kLdltFixedFloats = kPanel * kPanel + kPanel;        // U11 and the reciprocal pivots, behind W^T [kPanel][ldw]
constexpr int kLdltScratchSlack = 288;   // what solve_scratch_floats adds to W^T: kLdltFixedFloats and 16 spare

inline int round4(int n) { return (n + 3) & ~3; }
inline int ldlt_ld(int n) {  // row stride: >= round16(n), odd multiple of 4 (conflict-free b128 by row)
  int ld = ((n + 15) & ~15) + 4;
  while ((ld & 7) != 4) ld += 4;
  return ld;
}
inline int ldlt_ldw(int n) { return ((n + 1 + 3) & ~3) + 4; }   // W^T row stride
inline int solve_scratch_floats(int P) {   // MLP partials or the LDL^T scratch, whichever is larger
  const int need = P >= kGrid ? kPanel * ldlt_ldw(P) + kLdltScratchSlack : 0;
  return need > kSolveMlpPartFloats ? ((need + 3) & ~3) : kSolveMlpPartFloats;
}
inline size_t solve_big_floats(int P) { return (size_t)(P + 4) * ldlt_ld(P); }   // per window: the matrix in the workspace

enum SolveMethod {
  kSolveQr6,        // legacy 6 x 6: Householder QR on one thread
  kSolveInverse6,   // legacy 6 x 6: explicit inverse on one thread (BANET_SOLVER_INVERSE)
  kSolveLu,         // P < kGrid: pivoted LU in registers
  kSolveCgLdlt,     // P >= kGrid, matrix in LDS: Jacobi-PCG with the Schur step; the blocked LDL^T where it gives up
  kSolveLdlt,       // P >= kGrid: the blocked LDL^T alone (matrix in the workspace, CG does not fit, or kDevSolveLdltOnly)
};
// the blocked solvers keep the right-hand side as row P of the matrix (stride ldlt_ld), the others as column P (stride P + 2)
constexpr bool solve_method_blocked(int method) { return method == kSolveCgLdlt || method == kSolveLdlt; }

// Offsets are in floats from the start of the dynamic LDS, each a multiple of 4 (float4 accesses), in the kernel's order:
//   A [arows][ld] (absent when big) | X [P] | H0 [4 C] MLP ping | H1 [4 C] MLP pong | Avg [C] | Red [kSolveRedFloats], Scal inside it
//   | Part [solve_scratch_floats(P)] MLP partial sums, then the solver's scratch | Perm [P + kSolvePermTail] ints
// A -DBANET_TIMING build writes four floats past X[P]: they land in the padding of X and the start of H0, which is dead by then
// (spd_solve_kernel: in X's own 8 spare floats).
struct SolvePlan {
  int P, C;
  int method;         // SolveMethod
  int big;            // the matrix lives in the caller's workspace, big_floats per window, not in LDS
  int ld, arows;      // the matrix's row stride and rows (with the right-hand side and padding)
  int ldw;            // blocked: W^T row stride of the LDL^T
  int off_A, off_X, off_H0, off_H1, off_Avg, off_Red, off_Scal, off_Part, off_Perm, end;
  int lds_attr;       // lds > kLdsAttrAbove
  size_t lds;         // bytes of dynamic LDS = 4 end
  size_t big_floats;  // big: solve_big_floats(P), else 0
};

namespace plan_detail {

// the update kernel's regions behind a matrix of a_floats floats
inline void solve_carve(SolvePlan* pl, int a_floats) {
  const int P = pl->P, C = pl->C;
  pl->off_A = 0;
  pl->off_X = pl->off_A + a_floats;
  pl->off_H0 = pl->off_X + round4(P);
  pl->off_H1 = pl->off_H0 + 4 * C;
  pl->off_Avg = pl->off_H1 + 4 * C;
  pl->off_Red = pl->off_Avg + round4(C);
  pl->off_Scal = pl->off_Red + kSolveScalAt;
  pl->off_Part = pl->off_Red + kSolveRedFloats;
  pl->off_Perm = pl->off_Part + solve_scratch_floats(P);
  pl->end = pl->off_Perm + P + kSolvePermTail;
  pl->lds = (size_t)pl->end * sizeof(float);
  pl->lds_attr = pl->lds > kLdsAttrAbove ? 1 : 0;
}

}  // namespace plan_detail

// The plan of ba_solve_update_kernel for a variant (BANET_LEGACY_LM .. BANET_BUNDLE), P unknowns, C channels, lm.solver and the
// level's flags.  BANET_OK, or BANET_ERR_UNSUPPORTED where the vectors and scratch alone exceed the LDS; big / big_floats (what the
// workspace queries report) are filled either way.  A caller without a workspace refuses a big plan itself.
inline int plan_solve(int variant, int P, int C, int solver, int flags, SolvePlan* pl) {
  *pl = SolvePlan{};
  pl->P = P;
  pl->C = C;
  const bool blocked = P >= kGrid;
  pl->ld = blocked ? ldlt_ld(P) : P + 2;
  pl->arows = blocked ? P + 4 : P;
  pl->ldw = blocked ? ldlt_ldw(P) : 0;
  plan_detail::solve_carve(pl, round4(pl->arows * pl->ld));
  if (pl->lds > kSolveLdsMax) {   // K = 256 windows (P up to 6 * 7 + 256): only the vectors and the scratch stay in LDS
    pl->big = 1;
    pl->big_floats = solve_big_floats(P);
    plan_detail::solve_carve(pl, 0);
  }
  const bool legacy = variant == BANET_LEGACY_LM || variant == BANET_LEGACY_FIXED;
  if (legacy && P == 6) {         // the only shape of the one-thread solvers
    pl->method = solver == BANET_SOLVER_INVERSE ? kSolveInverse6 : kSolveQr6;
  } else if (P <= kGrid - 1) {    // pose-only variants: pivoted LU as tf.matrix_solve
    pl->method = kSolveLu;
  } else if (pl->big) {
    pl->method = kSolveLdlt;
  } else {
    // pcg_schur_solve covers 4 threads per row and needs kPcgRhs search directions and its reduction buffers in the scratch region:
    // a system beyond either (none is LDS-resident today: the matrix stops fitting at P ~ 190) goes straight to the factorisation
    const bool cg_fits = 4 * P <= kSolveThreads && kPcgRhs * round4(P) + kPcgRedFloats <= solve_scratch_floats(P);
    pl->method = cg_fits && !(flags & kDevSolveLdltOnly) ? kSolveCgLdlt : kSolveLdlt;
  }
  return pl->lds > kSolveLdsMax ? BANET_ERR_UNSUPPORTED : BANET_OK;
}

// The plan of spd_solve_kernel: A [P + 4][ld] with the right-hand side as row P | X [P + 8] | Part [solve_scratch_floats(P)]; the
// other offsets stay 0.  BANET_ERR_UNSUPPORTED below kGrid unknowns (the blocked factorisation wants at least two panels) and
// where the matrix does not fit the LDS.
inline int plan_spd_solve(int P, SolvePlan* pl) {
  *pl = SolvePlan{};
  pl->P = P;
  if (P < kGrid) return BANET_ERR_UNSUPPORTED;
  pl->method = kSolveLdlt;
  pl->ld = ldlt_ld(P);
  pl->arows = P + 4;
  pl->ldw = ldlt_ldw(P);
  pl->off_X = round4(pl->arows * pl->ld);
  pl->off_Part = pl->off_X + round4(P + 8);
  pl->end = pl->off_Part + solve_scratch_floats(P);
  pl->lds = (size_t)pl->end * sizeof(float);
  pl->lds_attr = pl->lds > kLdsAttrAbove ? 1 : 0;
  return pl->lds > kSolveLdsMax ? BANET_ERR_UNSUPPORTED : BANET_OK;
}

}  // namespace banet
