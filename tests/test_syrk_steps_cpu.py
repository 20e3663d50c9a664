"""What a SYRK pass launches (banet_amd/csrc/plan.hpp: plan_syrk_steps, plan_syrk_role, the two statistics-mode functions and the
lists of compiled instantiations), pinned on the CPU: plan.hpp compiled with g++ (tests/native/plan_host.cpp), asked for the ordered
launches of a level and compared with lists WRITTEN BY HAND from the launcher this plan replaced (launch_syrk / launch_syrk_wide of the
commit before it).  Nothing expected here is produced by plan.hpp.

A step prints as  `kernel<template parameters> job(job parameters) grid(x, y) block n lds bytes[ attr]`  (attr: the launch sets the
function attribute for more than 64 KB of dynamic LDS).  All levels below: C = 128 unless the form says otherwise, 256 CUs."""
import ctypes

import numpy as np
import pytest

import assembly_cases as ac
import test_plan_cpu as tp

CUS = 256
EXACT, F16_COMPUTE, F16_IN_PLACE, EXACT_HARVEST, SINGLE_PASS = -1, 0, 1, 2, 100      # SyrkStats; 100 = as a single assembly pass
MODES = (EXACT, F16_COMPUTE, F16_IN_PLACE, EXACT_HARVEST)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    L = tp.build_host_lib(tmp_path_factory.mktemp("syrk_steps"))
    L.banet_test_syrk_steps.restype = ctypes.c_size_t
    L.banet_test_syrk_steps.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]
    L.banet_test_syrk_steps_sweep.restype = ctypes.c_char_p
    L.banet_test_syrk_steps_sweep.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    L.banet_test_syrk_instantiations.restype = ctypes.c_char_p
    L.banet_test_syrk_stats.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p]
    L.banet_test_syrk_role.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    return L


def level(B, H, W, K, pairs, flags=0, C=128, policy=0):
    return (B, H * W, C, K, H, W, 1, 0, pairs, policy, flags)


def steps_of(lib, levels, stats, role_mode=0, cus=CUS):
    """-> [(rc, role on, Gs launched, [step, ...])] of plan_syrk_steps for every level"""
    desc = np.ascontiguousarray(np.asarray(levels, np.int64).astype(np.int32))
    need = lib.banet_test_syrk_steps(desc.ctypes.data, len(desc), cus, stats, role_mode, None, 0)
    buf = ctypes.create_string_buffer(need)
    lib.banet_test_syrk_steps(desc.ctypes.data, len(desc), cus, stats, role_mode, buf, need)
    out = []
    for line in buf.value.decode().split("\n")[:-1]:
        head, *steps = line.split("; ")
        rc, role, gs = (int(t.split("=")[1]) for t in head.split())
        out.append((rc, role, gs, steps))
    assert len(out) == len(levels)
    return out


# ---- the notation of the hand-written lists: every number is an argument ---------------------------------------------------------
def K_(name, job, gx, gy, block=256, lds=0, attr=False):
    return "%s job(%s) grid(%d, %d) block %d lds %d%s" % (name, job, gx, gy, block, lds, " attr" if attr else "")


def zero(words, gx):
    return K_("zero_iters_kernel", "%d" % words, gx, 1, block=64)


def colmax(gx, B):
    return K_("ba_colmax_kernel", "", gx, B)


def recmax(B):
    return K_("ba_recmax_kernel", "", 32, B)


def srsum(gx, B):
    return K_("ba_srsum_kernel", "", gx, B)


def bf16x6(KH, P, T0, gx, B):
    return K_("ba_syrk_bf16x6_kernel<%d, %d, %d>" % (KH, P, T0), "", gx, B)


def mfma32(KH, P, gx, B):
    return K_("ba_syrk_direct_kernel<%d, %d>" % (KH, P), "", gx, B)


def slice_(PT, DD, F16, koff, p0, gx, B):
    return K_("ba_syrk_slice_kernel<%d, %s, %s>" % (PT, DD, F16), "%d, %d" % (koff, p0), gx, B)


def rect(F16, r0, c0, gx, B):
    return K_("ba_syrk_rect_kernel<%s>" % F16, "%d, %d" % (r0, c0), gx, B)


# ba_syrk_kernel<NB>: dynamic LDS = max(2 x 64 x (16 NB + 16) + 2 x 64 x 8, 4 x 8 x 16 NB) floats
LDS_BYTES = {1: 20480, 2: 28672, 4: 45056, 8: 77824, 16: 143360}


def lds(NB, npass, gx, B):
    return [K_("ba_syrk_kernel<%d>" % NB, "%d" % p, gx, B, lds=LDS_BYTES[NB], attr=LDS_BYTES[NB] > 65536) for p in range(npass)]


# ---- 1. every SYRK form of the case table at three shapes and two batch sizes, as a single assembly pass runs it -------------------
FORM_SHAPES = ((23, 21), (32, 48), (480, 640))                       # N = 483, 1536, 307200
FORM_BATCHES = (2, 32)
# Gs by hand (plan_syrk): register kernels and wide jobs  min(ceil(N / 256), ceil(256 / B));
#                         LDS-tiled                       min(ceil(N / 64) / 4, ceil(512 / B)), at nb = 16 ceil(256 / B)
GS_REG = {(483, 2): 2, (1536, 2): 6, (307200, 2): 128, (483, 32): 2, (1536, 32): 6, (307200, 32): 8}
GS_LDS = {(483, 2): 2, (1536, 2): 6, (307200, 2): 256, (483, 32): 2, (1536, 32): 6, (307200, 32): 16}
GS_LDS16 = {(483, 2): 2, (1536, 2): 6, (307200, 2): 128, (483, 32): 2, (1536, 32): 6, (307200, 32): 8}
# ba_colmax_kernel's grid  max(1, min(ceil(N / 256), ceil(8 x 256 / B)));  ba_srsum_kernel's  ceil(N / 256)
COLMAX_G = {(483, 2): 2, (1536, 2): 6, (307200, 2): 1024, (483, 32): 2, (1536, 32): 6, (307200, 32): 64}
SRSUM_G = {483: 2, 1536: 6, 307200: 1200}
ZERO = {(2, 64): (128, 2), (2, 128): (256, 4), (2, 256): (512, 8), (32, 64): (2048, 32), (32, 128): (4096, 64), (32, 256): (8192, 128)}   # (B, K) -> (words, grid)


def wide_jobs(K, pairs, F16, g, B):
    """the jobs of launch_syrk_wide, written out per (K, frames)"""
    T, F = "true", "false"
    return {(256, 1): [slice_(1, T, F16, 0, 0, g, B), slice_(1, T, F16, 128, 0, g, B), rect(F16, 0, 128, g, B), rect(F16, 0, 192, g, B)],
            (256, 2): [slice_(2, T, F16, 0, 0, g, B), slice_(2, T, F16, 128, 0, g, B), rect(F16, 0, 128, g, B), rect(F16, 0, 192, g, B)],
            (256, 5): [slice_(4, T, F16, 0, 0, g, B), slice_(1, F, F16, 0, 4, g, B), slice_(4, T, F16, 128, 0, g, B), slice_(1, F, F16, 128, 4, g, B),
                       rect(F16, 0, 128, g, B), rect(F16, 0, 192, g, B)],
            (256, 7): [slice_(4, T, F16, 0, 0, g, B), slice_(3, F, F16, 0, 4, g, B), slice_(4, T, F16, 128, 0, g, B), slice_(3, F, F16, 128, 4, g, B),
                       rect(F16, 0, 128, g, B), rect(F16, 0, 192, g, B)],
            (128, 5): [slice_(4, T, F16, 0, 0, g, B), slice_(1, F, F16, 0, 4, g, B)],
            (128, 7): [slice_(4, T, F16, 0, 0, g, B), slice_(3, F, F16, 0, 4, g, B)]}[(K, pairs)]


def expected_form(form, tag, K, pairs, N, B):
    """the launches of one configuration of ac.syrk_forms() in a single assembly pass, read off the old launcher"""
    key = (N, B)
    if form == "lds":
        NB = {4: 1, 12: 1, 20: 2, 36: 4, 200: 16, 5: 1, 33: 4, 16: 1, 128: 8, 256: 16}[K]      # kDevSyrkNoBf16x6 at K = 128 / 256, 5 frames
        return lds(NB, pairs, (GS_LDS16 if NB == 16 else GS_LDS)[key], B)
    g = GS_REG[key]
    if form == "direct":
        return [mfma32(K // 64, pairs, g, B)]
    if form == "bf16x6":             # (480x640 x 32 is eligible for the fp16 form, but a single pass runs it only with kDevSyrkF16)
        return [bf16x6(K // 64, 4, 0, g, B)]
    if form == "bf16x6_f16":
        return [zero(*ZERO[(B, K)]), colmax(COLMAX_G[key], B), recmax(B), bf16x6(K // 64, 4, 16, g, B)]
    if form == "three_products":
        return [bf16x6(2, 1, 3, g, B)]
    sums = [srsum(SRSUM_G[N], B)] if pairs > 1 else []
    if form == "wide":
        return sums + wide_jobs(K, pairs, "false", g, B)
    assert form == "wide_f16"
    return [zero(*ZERO[(B, K)]), colmax(COLMAX_G[key], B), recmax(B)] + sums + wide_jobs(K, pairs, "true", g, B)


def test_every_form_of_the_case_table(lib):
    cases, want = [], []
    for form, configs in ac.syrk_forms().items():
        for tag, C, K, pairs, bits, _ in configs:
            for H, W in FORM_SHAPES:
                for B in FORM_BATCHES:
                    cases.append(level(B, H, W, K, pairs, int(bits), C=C))
                    want.append((form, tag, K, pairs, H, W, B, expected_form(form, tag, K, pairs, H * W, B)))
    assert len(cases) == 31 * 6
    for (rc, role, gs, steps), (form, tag, K, pairs, H, W, B, exp) in zip(steps_of(lib, cases, SINGLE_PASS), want):
        assert rc == 0 and role == 0 and steps == exp, (form, tag, K, pairs, H, W, B, steps, exp)


# ---- 2. the four statistics modes: 60 x 80 (N = 4800), B = 2, kDevSyrkF16 (the fp16 form eligible); Gs = min(19, 128) = 19 ------------
def test_statistics_modes_of_a_bf16x6_level(lib):
    f16 = tp.dev_flags(lib)["kDevSyrkF16"]
    for K, KH, words, zg in ((64, 1, 128, 2), (128, 2, 256, 4)):
        for P in (1, 4):
            want = {EXACT: [bf16x6(KH, P, 0, 19, 2)],
                    F16_COMPUTE: [zero(words, zg), colmax(19, 2), recmax(2), bf16x6(KH, P, 16, 19, 2)],
                    F16_IN_PLACE: [recmax(2), bf16x6(KH, P, 16, 19, 2)],
                    EXACT_HARVEST: [zero(words, zg), bf16x6(KH, P, 1, 19, 2)]}     # the kernel harvests the maxima itself: no colmax pass
            for mode in MODES:
                (rc, role, gs, steps), = steps_of(lib, [level(2, 60, 80, K, P, f16)], mode)
                assert rc == 0 and gs == 19 and steps == want[mode], (K, P, mode, steps)
            # without eligibility every mode is the exact form
            for mode in MODES:
                (rc, role, gs, steps), = steps_of(lib, [level(2, 60, 80, K, P, 0)], mode)
                assert steps == want[EXACT], (K, P, mode, steps)


def test_statistics_modes_of_a_wide_level(lib):
    f16 = tp.dev_flags(lib)["kDevSyrkF16"]
    for K, P, words, zg in ((256, 1, 512, 8), (256, 2, 512, 8), (256, 7, 512, 8), (128, 5, 256, 4), (128, 7, 256, 4)):
        sums = [srsum(19, 2)] if P > 1 else []
        maxima = [zero(words, zg), colmax(19, 2), recmax(2)]
        want = {EXACT: sums + wide_jobs(K, P, "false", 19, 2),
                F16_COMPUTE: maxima + sums + wide_jobs(K, P, "true", 19, 2),
                F16_IN_PLACE: [recmax(2)] + sums + wide_jobs(K, P, "true", 19, 2),
                # THE difference from ba_syrk_bf16x6_kernel: no in-kernel harvest, so a colmax pass and the fp16 form on that iteration already
                EXACT_HARVEST: maxima + sums + wide_jobs(K, P, "true", 19, 2)}
        for mode in MODES:
            (rc, role, gs, steps), = steps_of(lib, [level(2, 60, 80, K, P, f16)], mode)
            assert rc == 0 and gs == 19 and steps == want[mode], (K, P, mode, steps)


def test_lds_tiled_kernel_at_each_nb(lib):
    # 60 x 80: 75 tiles -> Gs = 18 (cap 256, 128 at nb = 16); K = 100 / 200 avoid the register kernels
    for K, NB in ((6, 1), (32, 2), (40, 4), (100, 8), (200, 16)):
        for P in (1, 5):
            (rc, role, gs, steps), = steps_of(lib, [level(2, 60, 80, K, P)], EXACT)
            assert rc == 0 and steps == lds(NB, P, 18, 2), (K, P, steps)
    assert "lds 143360 attr" in lds(16, 1, 18, 2)[0] and "lds 77824 attr" in lds(8, 1, 18, 2)[0] and lds(4, 1, 18, 2)[0].endswith("lds 45056")


def test_fp32_mfma_kernel(lib):
    no6 = tp.dev_flags(lib)["kDevSyrkNoBf16x6"]
    for K in (64, 128):
        for P in (1, 2, 3, 4):
            for mode in MODES:                                            # no fp16 form: the mode changes nothing
                (rc, role, gs, steps), = steps_of(lib, [level(2, 60, 80, K, P, no6)], mode)
                assert rc == 0 and steps == [mfma32(K // 64, P, 19, 2)], (K, P, steps)


def test_role_workgroup_in_the_grid(lib):
    # 60 x 80 x 2: 2 x (19 + 1) <= 256 -> one more workgroup per window, Gs as planned
    (rc, role, gs, steps), = steps_of(lib, [level(2, 60, 80, 128, 1)], EXACT, role_mode=1)
    assert (rc, role, gs) == (0, 1, 19) and steps == [bf16x6(2, 1, 0, 20, 2)]
    # 480 x 640 x 8: Gs = 32, 8 x 33 > 256, B <= 8 and Gs >= 16 -> one SYRK workgroup given up: 31 rows, 32 workgroups
    (rc, role, gs, steps), = steps_of(lib, [level(8, 480, 640, 128, 1)], EXACT, role_mode=1)
    assert (rc, role, gs) == (0, 1, 31) and steps == [bf16x6(2, 1, 0, 32, 8)]
    # the other kernels carry no role
    (rc, role, gs, steps), = steps_of(lib, [level(2, 60, 80, 256, 1)], EXACT, role_mode=1)
    assert (rc, role, gs) == (0, 0, 19) and steps == wide_jobs(256, 1, "false", 19, 2)


# ---- 3. the sweep: capacity, refusals, the compiled lists -------------------------------------------------------------------------
SWEEP_FLAGS = ("kDevSyrkNoBf16x6", "kDevSyrkF16", "kDevSyrkThreeProducts", "kDevNoSyrkF16")


def sweep_levels():
    """test_plan_cpu.sweep_levels(), and -- its frame counts are 1, 2, 4, 5, 7, 8 -- one shape with 3 and 6 frames, which the
    instantiations <.., 3, ..> of the register kernels, <3, true, ..> and <2, false, ..> of the slice jobs need"""
    levels, _ = tp.sweep_levels()
    extra = [(B, 60 * 80, 128, K, 60, 80, 1, 0, pairs, 0) for K in tp.KS for pairs in (3, 6) for B in (2, 32)]
    return np.concatenate([levels, np.asarray(extra, np.int32)])


def test_sweep_capacity_refusals_and_instantiations(lib):
    levels = sweep_levels()
    flags = tp.dev_flags(lib)
    compiled = set(lib.banet_test_syrk_instantiations().decode().split("\n")[:-1])
    assert len(compiled) == 5 + 2 * 4 + 7 * 4 + 4 * 4 + 2
    prepasses = {"zero_iters_kernel", "ba_colmax_kernel", "ba_recmax_kernel", "ba_srsum_kernel"}
    reached, most = set(), 0
    for word in [0] + [w for label, w in tp.flag_words(flags) if label in SWEEP_FLAGS]:
        desc = np.ascontiguousarray(np.concatenate([levels, np.full((len(levels), 1), word, np.int32)], axis=1))
        for mode in MODES:
            for role_mode in (0, 1):
                out = np.zeros((len(desc), 3), np.int32)
                names = lib.banet_test_syrk_steps_sweep(desc.ctypes.data, len(desc), CUS, mode, role_mode, out.ctypes.data)
                reached |= set(names.decode().split("\n")[:-1])
                rc_plan, rc, n = out[:, 0], out[:, 1], out[:, 2]
                planned = rc_plan == 0
                # REFUSALS, from the old launcher: it returned BANET_ERR_UNSUPPORTED for nb outside 1, 2, 4, 8, 16 and for wide jobs at
                # K other than 128 / 256.  plan_syrk gives nb = 0 at K = 0 (launch_assemble does not call the SYRK then) and never
                # another such nb, and plans wide jobs at K = 128 / 256 only: the one refusal of the sweep is K = 0.
                refused = planned & (desc[:, 3] == 0)
                assert ((rc == -3) == refused)[planned].all() and (rc[planned & ~refused] == 0).all()      # BANET_ERR_UNSUPPORTED = -3
                assert (n[~planned | refused] == 0).all() and (n[planned & ~refused] >= 1).all()
                most = max(most, int(n.max()))
    assert most == 10 and most <= lib.banet_test_syrk_max_steps()      # zero, colmax, recmax, srsum, four slices, two rectangles
    assert reached - prepasses <= compiled, sorted(reached - prepasses - compiled)
    assert prepasses <= reached
    assert compiled <= reached, "compiled but reached by no level of the sweep: %s" % sorted(compiled - reached)


def test_more_frames_than_the_list_holds_are_refused(lib):
    (rc, _, _, steps), = steps_of(lib, [level(2, 23, 21, 20, 64)], EXACT)
    assert rc == 0 and len(steps) == 64 == lib.banet_test_syrk_max_steps()
    (rc, _, _, steps), = steps_of(lib, [level(2, 23, 21, 20, 65)], EXACT)
    assert rc == -3 and steps == []


# ---- 4. the statistics mode of an iteration, the role decision ----------------------------------------------------------------------
def test_statistics_mode_of_an_iteration_and_of_a_single_pass(lib):
    def ask(f16, alone, it, iters):
        out = np.zeros(2, np.int32)
        lib.banet_test_syrk_stats(f16, alone, it, iters, out.ctypes.data)
        return tuple(out.tolist())
    # the old expressions: pl.s.f16 ? (it == 0 ? (max_iters > 1 ? 2 : 0) : 1) : -1   and   pl.s.f16_standalone ? 0 : -1
    assert ask(0, 0, 0, 3) == (EXACT, EXACT) and ask(0, 0, 2, 3) == (EXACT, EXACT)
    assert ask(1, 0, 0, 3) == (EXACT_HARVEST, EXACT) and ask(1, 0, 1, 3) == (F16_IN_PLACE, EXACT) and ask(1, 0, 2, 3) == (F16_IN_PLACE, EXACT)
    assert ask(1, 1, 0, 1) == (F16_COMPUTE, F16_COMPUTE) and ask(1, 1, 0, 2) == (EXACT_HARVEST, F16_COMPUTE)


def test_role_decision(lib):
    """plan_syrk_role against the condition of the old lm_level_plan:
         bundle level with the MLP, ba_syrk_bf16x6_kernel, C <= 256, C % 4 == 0, not kDevMlpInSolve, and one of
           (1) Bsel (Gs + 1) <= CUs,  (2) Bsel <= 8 && Gs >= 16,  (3) N <= 19200 && Gs >= 4;
         Gs one fewer where Bsel (Gs + 1) > CUs."""
    in_solve = tp.dev_flags(lib)["kDevMlpInSolve"]
    big = 307200
    #        Gs direct mlp Bsel N     C    flags cus     on Gs
    table = [(7, 2, 1, 32, big, 128, 0, 256,             1, 7),       # (1) 32 x 8 = 256 <= 256
             (8, 2, 1, 32, big, 128, 0, 256,             0, 8),       # (1) 288 > 256, (2) Bsel > 8, (3) N too large
             (32, 2, 1, 8, big, 128, 0, 256,             1, 31),      # (2) 8 x 33 = 264 > 256: one workgroup given up
             (16, 2, 1, 8, big, 128, 0, 64,              1, 15),      # (2) at its lower edge of Gs
             (15, 2, 1, 8, big, 128, 0, 64,              0, 15),      # (2) Gs < 16
             (32, 2, 1, 9, big, 128, 0, 256,             0, 32),      # (2) Bsel > 8
             (27, 2, 1, 9, big, 128, 0, 256,             1, 27),      # ... but (1): 9 x 28 = 252
             (8, 2, 1, 32, 19200, 128, 0, 256,           1, 7),       # (3) at its upper edge of N, reduced
             (8, 2, 1, 32, 19201, 128, 0, 256,           0, 8),       # (3) N too large
             (4, 2, 1, 128, 4800, 128, 0, 256,           1, 3),       # (3) at its lower edge of Gs
             (3, 2, 1, 128, 4800, 128, 0, 256,           0, 3),       # (3) Gs < 4
             (7, 2, 0, 32, big, 128, 0, 256,             0, 7),       # not a bundle level with the MLP
             (7, 0, 1, 32, big, 128, 0, 256,             0, 7),       # the LDS-tiled kernel,
             (7, 1, 1, 32, big, 128, 0, 256,             0, 7),       # the fp32-MFMA kernel
             (7, 3, 1, 32, big, 128, 0, 256,             0, 7),       # and the wide jobs carry no role
             (7, 2, 1, 32, big, 256, 0, 256,             1, 7),
             (7, 2, 1, 32, big, 260, 0, 256,             0, 7),       # C > 256
             (7, 2, 1, 32, big, 126, 0, 256,             0, 7),       # C % 4
             (7, 2, 1, 32, big, 128, in_solve, 256,      0, 7)]
    desc = np.ascontiguousarray(np.asarray([r[:8] for r in table], np.int64).astype(np.int32))
    out = np.zeros((len(table), 2), np.int32)
    lib.banet_test_syrk_role(desc.ctypes.data, len(table), out.ctypes.data)
    assert out.tolist() == [list(r[8:]) for r in table]
