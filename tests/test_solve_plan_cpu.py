"""The solve's host-side plan (csrc/solve_plan.hpp), compiled with g++ and swept over P = 6 .. 304, C in {1, 3, 32, 64, 128, 256}, the
four variants, both lm.solver values, with and without kDevSolveLdltOnly: the LDS layout (order, no overlap, alignment, total), the
LDS-or-workspace switch and the byte counts against the arithmetic the kernels carried before the plan existed (restated here in
a few lines), the scratch each planned solver needs against the scratch region, the method table, and the plan of
banet_spd_solve_f32 against what the small-step adjoint accepts.  The workspace queries of the built library are compared with
the plan, and with recorded values on the level shapes of ws_contract.py.  No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import solve_cases as sc
import ws_contract as wsc

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
os.environ.setdefault("BANET_NUM_CUS", "256")
OK, ERR_UNSUPPORTED = 0, -3
LEGACY_LM, LEGACY_FIXED, BUNDLE_CAMERA, BUNDLE = 0, 1, 2, 3
SOLVER_QR, SOLVER_INVERSE = 0, 1
P_RANGE = range(6, 305)
CHANNELS = (1, 3, 32, 64, 128, 256)
LDS_MAX = 160 * 1024
up = lambda n: (n + 255) // 256 * 256
r4 = lambda n: (n + 3) & ~3


@pytest.fixture(scope="module")
def capi():
    from banet_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _capi


@pytest.fixture(scope="module")
def plan_lib(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("solve_plan")), "libsolve_plan_host.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", out,
                           os.path.join(ROOT, "tests", "native", "solve_plan_host.cpp")])
    L = ctypes.CDLL(out)
    L.banet_test_solve_plan_fields.restype = ctypes.c_char_p
    L.banet_test_solve_plan_constant_names.restype = ctypes.c_char_p
    return L


@pytest.fixture(scope="module")
def k(plan_lib):
    """the header's named constants"""
    names = plan_lib.banet_test_solve_plan_constant_names().decode().split()
    out = (ctypes.c_int64 * len(names))()
    plan_lib.banet_test_solve_plan_constants(out)
    return dict(zip(names, out))


def plan_rows(L, rows):
    """rows of (which, variant, P, C, solver, flags) -> {field: int64 array}"""
    fields = L.banet_test_solve_plan_fields().decode().split()
    assert fields[0] == "desc_ints=6"
    names = fields[1:]
    desc = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1, 6)
    out = np.zeros((len(desc), len(names)), dtype=np.int64)
    L.banet_test_solve_plan_sweep(desc.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(desc),
                                  out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)))
    return {n: out[:, i] for i, n in enumerate(names)}


@pytest.fixture(scope="module")
def sweep(plan_lib, k):
    rows = [(0, v, P, C, s, f) for v in (LEGACY_LM, LEGACY_FIXED, BUNDLE_CAMERA, BUNDLE) for P in P_RANGE for C in CHANNELS
            for s in (SOLVER_QR, SOLVER_INVERSE) for f in (0, k["kDevSolveLdltOnly"])]
    p = plan_rows(plan_lib, rows)
    d = np.asarray(rows, dtype=np.int64)
    p.update(variant=d[:, 1], solver=d[:, 4], flags=d[:, 5])
    assert np.array_equal(p["P"], d[:, 2]) and np.array_equal(p["C"], d[:, 3])
    assert len(rows) == 4 * 299 * 6 * 2 * 2
    return p


# ---- the arithmetic of the kernels before the plan, restated -------------------------------------------------------------------------
def old_ld(n):
    ld = ((n + 15) & ~15) + 4
    while ld & 7 != 4:
        ld += 4
    return ld


old_ldw = lambda n: ((n + 1 + 3) & ~3) + 4


def old_scratch(P):
    need = 16 * old_ldw(P) + 288 if P >= 32 else 0
    return r4(need) if need > 4096 else 4096


def old_lds_bytes(P, C, big):
    ld, arows = (old_ld(P), P + 4) if P >= 32 else (P + 2, P)
    return 4 * ((0 if big else r4(arows * ld)) + r4(P) + 8 * C + r4(C) + 24 + old_scratch(P) + P + 8)


def old_spd_lds_bytes(P):
    return 4 * (r4((P + 4) * old_ld(P)) + r4(P + 8) + old_scratch(P))


# ---- layout ------------------------------------------------------------------------------------------------------------------------
REGIONS = ("off_A", "off_X", "off_H0", "off_H1", "off_Avg", "off_Red", "off_Part", "off_Perm", "end")


def test_regions_are_in_the_kernels_order_aligned_and_end_at_lds(sweep, k):
    p = sweep
    assert (p["rc"] == OK).all()                            # every shape of the sweep is planned
    P, C, big = p["P"], p["C"], p["big"]
    sizes = {"off_A": np.where(big == 1, 0, p["arows"] * p["ld"]), "off_X": P, "off_H0": 4 * C, "off_H1": 4 * C, "off_Avg": C,
             "off_Red": np.full_like(P, k["kSolveRedFloats"]), "off_Part": np.full_like(P, k["kSolveMlpPartFloats"]),
             "off_Perm": P + k["kSolvePermTail"]}
    assert (p["off_A"] == 0).all()
    for a, b in zip(REGIONS[:-1], REGIONS[1:]):
        assert (p[a] + sizes[a] <= p[b]).all(), (a, b)      # in order, each with room for its contents: no overlap
        assert (p[a] % 4 == 0).all(), a
    # the scalars live in the last four floats of Red, behind block_sum's per-wave values
    assert (p["off_Scal"] == p["off_Red"] + k["kSolveScalAt"]).all() and (p["off_Scal"] % 4 == 0).all()
    assert k["kSolveWaves"] <= k["kSolveScalAt"] and k["kSolveScalAt"] + 4 <= k["kSolveRedFloats"]
    assert (p["end"] == p["off_Perm"] + P + k["kSolvePermTail"]).all()
    assert (p["lds"] == 4 * p["end"]).all() and (p["lds"] <= k["kSolveLdsMax"]).all()
    assert (p["lds_attr"] == (p["lds"] > k["kLdsAttrAbove"])).all()
    assert k["kSolveLdsMax"] == LDS_MAX and k["kLdsAttrAbove"] == 64 * 1024
    # a -DBANET_TIMING build writes four floats past X[P]: they stay inside X's padding and H0 (C >= 1: 4 C >= 4 floats)
    assert (p["off_X"] + P + 4 <= p["off_H1"]).all()


def test_lds_big_and_strides_equal_the_arithmetic_before_the_plan(sweep):
    p = sweep
    for i in range(0, len(p["P"]), 4):                      # (solver and flags do not enter: one row of every four, then all of them)
        P, C = int(p["P"][i]), int(p["C"][i])
        big = old_lds_bytes(P, C, False) > LDS_MAX
        want = (int(big), old_lds_bytes(P, C, big), (P + 4) * old_ld(P) if big else 0, old_ld(P) if P >= 32 else P + 2,
                P + 4 if P >= 32 else P, old_ldw(P) if P >= 32 else 0, old_scratch(P))
        for j in range(i, i + 4):
            got = (p["big"][j], p["lds"][j], p["big_floats"][j], p["ld"][j], p["arows"][j], p["ldw"][j], p["off_Perm"][j] - p["off_Part"][j])
            assert tuple(int(v) for v in got) == want, (P, C, j - i)
    # the switch sits where test_solve_cases_cpu.py finds it: between 150 and 200, never back to the LDS above it
    for C in CHANNELS:
        sel = (p["C"] == C) & (p["variant"] == BUNDLE) & (p["solver"] == 0) & (p["flags"] == 0)
        bigs = p["big"][sel]
        first = int(np.argmax(bigs)) + 6
        assert 150 < first <= 201 and not bigs[:first - 6].any() and bigs[first - 6:].all(), (C, first)


def test_workspace_queries_of_the_library_are_the_plans(capi, sweep):
    p = sweep
    L = capi.lib()
    B = sc.B_WINDOWS
    sel = (p["variant"] == BUNDLE) & (p["solver"] == 0) & (p["flags"] == 0)
    n = 0
    for P, C, big, fl in zip(p["P"][sel], p["C"][sel], p["big"][sel], p["big_floats"][sel]):
        if P < 7:
            continue
        got = sc.solve_workspace_bytes(B, int(C), int(P))
        assert got == (up(B * int(fl) * 4) if big else 0), (P, C)
        n += 1
    assert n == 298 * len(CHANNELS)
    # P counts, not how it splits into poses and coefficients; the other variants and flags plan the same bytes
    for variant, K, pairs, flags in (("bundle", 256, 8, 0), ("bundle", 200, 2, 1 << 23), ("bundle_camera", 0, 40, 0)):
        lv = sc.bare_level(variant, B, 100, 32, K, pairs, flags)
        P = 6 * pairs + K
        assert L.banet_ba_solve_update_workspace_bytes(ctypes.byref(lv)) == up(B * (P + 4) * old_ld(P) * 4)


# banet_lm_level_workspace_bytes before the plan existed, at BANET_NUM_CUS = 256, on the level shapes of ws_contract.abi_cases
# (B, H, W, K, pairs, policy): the solve's matrix is the carve's last region where the plan says big
LEVEL_BYTES = {(2, 41, 57, 0, 1, 0): 217856, (2, 37, 53, 0, 3, 1): 139520, (2, 41, 57, 32, 1, 0): 468992, (1, 10, 13, 32, 3, 1): 54272,
               (2, 41, 57, 128, 1, 0): 1894400, (2, 37, 53, 128, 3, 1): 1889280, (2, 30, 40, 128, 7, 0): 2402304,
               (4, 120, 160, 128, 1, 0): 23566080, (2, 35, 45, 256, 1, 0): 5153280, (1, 37, 53, 256, 7, 1): 3791872,
               (2, 41, 57, 176, 1, 0): 3244544, (2, 41, 57, 188, 1, 1): 3352064, (32, 60, 80, 128, 1, 0): 31192320}


def test_level_workspace_bytes_are_unchanged(capi):
    L = capi.lib()
    for (B, H, W, K, pairs, policy), want in LEVEL_BYTES.items():
        lv = wsc._abi_level(capi, 4096, B, H, W, K, pairs, policy=policy)
        assert L.banet_lm_level_workspace_bytes(ctypes.byref(lv)) == want, (B, H, W, K, pairs, policy)
        P = 6 * pairs + K                                   # C = 128
        big = old_lds_bytes(P, 128, False) > LDS_MAX
        assert L.banet_ba_solve_update_workspace_bytes(ctypes.byref(lv)) == (up(B * (P + 4) * old_ld(P) * 4) if big else 0)


# ---- scratch ---------------------------------------------------------------------------------------------------------------------------
def test_the_scratch_region_covers_every_planned_solver(sweep, k):
    p = sweep
    room = p["off_Perm"] - p["off_Part"]
    assert (room >= k["kSolveMlpPartFloats"]).all()         # the MLP's partial sums, whatever solves
    assert k["kLuScratchFloats"] == 3 * k["kGrid"] + k["kGrid"]       # two column buffers and the pivot row; the used-row marks (ints)
    assert k["kPcgRedFloats"] == 2 * 4 * k["kSolveWaves"] and k["kPcgRhs"] == 2
    assert k["kLdltFixedFloats"] == k["kPanel"] * k["kPanel"] + k["kPanel"] == 272
    lu = p["method"] == k["kSolveLu"]
    assert (room[lu] >= k["kLuScratchFloats"]).all() and lu.any()
    assert (p["off_Perm"] + p["P"] <= p["end"]).all()       # the LU's row order
    cg = p["method"] == k["kSolveCgLdlt"]
    n1 = np.where(p["variant"] == BUNDLE, p["P"] - 1, p["P"])         # the undamped last coefficient leaves by the Schur step
    need_cg = k["kPcgRhs"] * ((n1 + 3) & ~3) + k["kPcgRedFloats"]
    assert (room[cg] >= need_cg[cg]).all() and cg.any()
    assert (4 * p["P"][cg] <= k["kSolveThreads"]).all()     # four threads per row
    ldlt = cg | (p["method"] == k["kSolveLdlt"])            # the fallback of the conjugate gradients as well
    need_ldlt = k["kPanel"] * p["ldw"] + k["kLdltFixedFloats"]
    assert (room[ldlt] >= need_ldlt[ldlt]).all() and (p["ldw"][ldlt] >= p["P"][ldlt] + 1).all() and ldlt.any()
    assert (p["ld"][ldlt] >= ((p["P"][ldlt] + 15) & ~15)).all() and (p["ld"][ldlt] % 8 == 4).all()
    assert (p["arows"][ldlt] >= p["P"][ldlt] + 1).all()     # the right-hand side is row P


# ---- method table ------------------------------------------------------------------------------------------------------------------
def test_method_table(sweep, k):
    p = sweep
    P, v, big = p["P"], p["variant"], p["big"] == 1
    legacy6 = ((v == LEGACY_LM) | (v == LEGACY_FIXED)) & (P == 6)
    ldlt_only = p["flags"] == k["kDevSolveLdltOnly"]
    cg_fits = (4 * P <= k["kSolveThreads"]) & (2 * ((P + 3) & ~3) + 8 * k["kSolveWaves"] <= p["off_Perm"] - p["off_Part"])
    want = np.select([legacy6 & (p["solver"] == SOLVER_INVERSE), legacy6, P <= k["kGrid"] - 1, big, cg_fits & ~ldlt_only],
                     [k["kSolveInverse6"], k["kSolveQr6"], k["kSolveLu"], k["kSolveLdlt"], k["kSolveCgLdlt"]], k["kSolveLdlt"])
    assert np.array_equal(p["method"], want)
    assert k["kGrid"] == 32
    # each of them occurs, the one-thread solvers on the legacy 6 x 6 system only, and P = 6 of the bundle variants is the LU's
    for m in ("kSolveQr6", "kSolveInverse6", "kSolveLu", "kSolveCgLdlt", "kSolveLdlt"):
        assert (p["method"] == k[m]).any(), m
    small = (p["method"] == k["kSolveQr6"]) | (p["method"] == k["kSolveInverse6"])
    assert np.array_equal(small, legacy6)
    assert (p["method"][(P == 6) & (v >= BUNDLE_CAMERA)] == k["kSolveLu"]).all()
    assert (p["method"][(P >= 32) & ~big & ~ldlt_only] == k["kSolveCgLdlt"]).all()      # today every LDS-resident system has room for CG
    assert (p["method"][(P >= 32) & ldlt_only] == k["kSolveLdlt"]).all() and (p["method"][big] == k["kSolveLdlt"]).all()
    assert not (p["method"][~cg_fits] == k["kSolveCgLdlt"]).any()
    # the right-hand side is row P exactly where a blocked solver runs
    blocked = (p["method"] == k["kSolveCgLdlt"]) | (p["method"] == k["kSolveLdlt"])
    assert np.array_equal(blocked, P >= 32) and (p["arows"][~blocked] == P[~blocked]).all() and (p["ld"][~blocked] == P[~blocked] + 2).all()


def test_conjugate_gradients_are_not_planned_where_they_do_not_fit(plan_lib, k):
    """beyond the sweep: the predicate that no shape of today fails, on systems that would need the matrix in LDS and more rows
    than a quarter of the workgroup -- the plan is the workspace's there, and the factorisation's"""
    p = plan_rows(plan_lib, [(0, BUNDLE, P, 32, 0, 0) for P in (256, 257, 400, 1000)])
    assert (p["method"] == k["kSolveLdlt"]).all() and (p["big"] == 1).all() and (p["rc"] == OK).all()
    far = plan_rows(plan_lib, [(0, BUNDLE, 4000, 32, 0, 0)])            # vectors and scratch alone exceed the LDS
    assert far["rc"][0] == ERR_UNSUPPORTED and far["big"][0] == 1 and far["big_floats"][0] == 4004 * old_ld(4000)


# ---- the SPD plan ------------------------------------------------------------------------------------------------------------------
def test_spd_plan_limits_and_the_small_step(plan_lib, capi, k):
    Ps = list(range(1, 401))
    p = plan_rows(plan_lib, [(1, 0, P, 0, 0, 0) for P in Ps])
    L = capi.lib()
    N = 100
    pmax = 0
    for i, P in enumerate(Ps):
        fits = P >= 32 and old_spd_lds_bytes(P) <= LDS_MAX
        assert (p["rc"][i] == OK) == fits and p["rc"][i] in (OK, ERR_UNSUPPORTED), P
        if P >= 32:
            assert p["lds"][i] == old_spd_lds_bytes(P) and p["lds_attr"][i] == (p["lds"][i] > 64 * 1024), P
            assert (p["ld"][i], p["arows"][i], p["ldw"][i]) == (old_ld(P), P + 4, old_ldw(P)), P
            assert p["off_X"][i] >= p["arows"][i] * p["ld"][i] and p["off_Part"][i] >= p["off_X"][i] + P + 8, P     # (+ 8: the timing build's slots)
            assert p["off_X"][i] % 4 == 0 and p["off_Part"][i] % 4 == 0 and p["end"][i] * 4 == p["lds"][i], P
            assert p["end"][i] - p["off_Part"][i] >= k["kPanel"] * p["ldw"][i] + k["kLdltFixedFloats"], P
            assert p["method"][i] == k["kSolveLdlt"] and p["big"][i] == 0, P
        if fits:
            pmax = P
        if P >= 7:                                          # small_step_supported: its own Cholesky below 32, this plan from there on
            nb = L.banet_small_step_adjoint_workspace_bytes(BUNDLE, 3, N, 32, P - 6, 1)
            assert (nb > 0) == (P < 32 or fits), P
    assert 134 <= pmax < 200 and all(p["rc"][i] == ERR_UNSUPPORTED for i, P in enumerate(Ps) if P > pmax)
    assert L.banet_small_step_adjoint_workspace_bytes(BUNDLE_CAMERA, 3, N, 32, 0, pmax // 6) > 0
    assert L.banet_small_step_adjoint_workspace_bytes(BUNDLE_CAMERA, 3, N, 32, 0, pmax // 6 + 1) == 0
