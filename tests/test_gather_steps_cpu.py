"""What a gather pass launches (banet_amd/csrc/plan.hpp: plan_gather_steps, the lists of compiled gather instantiations and the one
definition of the frame-parallel strip workgroup's LDS size), pinned on the CPU: plan.hpp compiled with g++
(tests/native/plan_host.cpp), asked for the ordered launches of a level and compared with lists WRITTEN BY HAND from the launchers this
plan replaced (prepare_gather / launch_gather / finish_gather with launch_c / launch_k, launch_gather128, launch_gather128p,
launch_gather128s and launch_gather128q of the commit before it).  Nothing expected here is produced by plan_gather_steps.

Two kinds of expectation:
  * lists with every number written out, the grid worked out by hand from plan_gather's rules (sections 1, 3, 4, 5);
  * the old launchers restated in Python (old_launches), which took their grid from GatherPlan: the fields G, rows, frows, pairloop,
    strip, strip_fp, quad, patch, c128 of the plan (pinned by tests/golden/plan_digests.json, not changed by the step list) go in,
    the kernel spelling, grid, block, LDS and attribute come out, for every flag set of the case table (section 2).

A step prints as  `kernel[ words(n)] grid(x, y) block n lds bytes[ attr]`  (words: what the zeroing step clears; attr: the launch sets
the function attribute for its dynamic LDS).  256 CUs throughout."""
import ctypes

import numpy as np
import pytest

import assembly_cases as ac
import test_plan_cpu as tp

CUS = 256
UNSUPPORTED = -3


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    L = tp.build_host_lib(tmp_path_factory.mktemp("gather_steps"))
    L.banet_test_gather_steps.restype = ctypes.c_size_t
    L.banet_test_gather_steps.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]
    L.banet_test_gather_steps_sweep.restype = ctypes.c_char_p
    L.banet_test_gather_steps_sweep.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    L.banet_test_gather_instantiations.restype = ctypes.c_char_p
    L.banet_test_gather_steps_of_strip.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    L.banet_test_strip_fp_lds_bytes.restype = ctypes.c_size_t
    L.banet_test_strip_fp_lds_bytes.argtypes = [ctypes.c_int, ctypes.c_int]
    return L


def level(B, H, W, K, pairs, flags=0, C=128, grad=0, dense=1, N=None, policy=0):
    return (B, H * W if N is None else N, C, K, H, W, dense, grad, pairs, policy, flags)


def _desc(levels):
    d = np.asarray(levels, np.int64)
    d[:, 10] = np.where(d[:, 10] >= (1 << 31), d[:, 10] - (1 << 32), d[:, 10])     # the flag word as int32
    return np.ascontiguousarray(d.astype(np.int32))


def steps_of(lib, levels, reset_queue=True, cus=CUS):
    """-> [(rc, [step, ...])] of plan_gather_steps for every level"""
    desc = _desc(levels)
    need = lib.banet_test_gather_steps(desc.ctypes.data, len(desc), cus, int(reset_queue), None, 0)
    buf = ctypes.create_string_buffer(need)
    lib.banet_test_gather_steps(desc.ctypes.data, len(desc), cus, int(reset_queue), buf, need)
    out = []
    for line in buf.value.decode().split("\n")[:-1]:
        head, *steps = line.split("; ")
        out.append((int(head.split("=")[1]), steps))
    assert len(out) == len(levels)
    return out


def plans_of(lib, levels, cus=CUS):
    """-> one dict of GatherPlan fields ("G", "rows", ...) per level, from plan_assemble"""
    desc = _desc(levels)
    names = tp.fields(lib)
    out = np.zeros((len(desc), len(names)), np.int64)
    lib.banet_test_plan_sweep(desc.ctypes.data_as(ctypes.c_void_p), len(desc), cus, out.ctypes.data_as(ctypes.c_void_p))
    return [{n[2:] if n.startswith("g.") else n: int(v) for n, v in zip(names, row)} for row in out]


# ---- the notation of the hand-written lists: every number is an argument ---------------------------------------------------------
def K_(name, gx, gy, block=256, lds=0, attr=False):
    return "%s grid(%d, %d) block %d lds %d%s" % (name, gx, gy, block, lds, " attr" if attr else "")


def zero(words, gx):
    return K_("zero_iters_kernel words(%d)" % words, gx, 1, block=64)


def fold(gx, gy):
    return K_("ba_fold_kernel", gx, gy)


def generic(VEC, CH, GRAD, KVEC, KCH, gx, gy):
    return K_("ba_gather_kernel<%d, %d, %s, %d, %d>" % (VEC, CH, GRAD, KVEC, KCH), gx, gy)


def direct(KV4, gx, gy):
    return K_("ba_gather128_kernel<%d>" % KV4, gx, gy)


def patch(KV4, US, FS, gx, gy, lds=0, attr=False):
    return K_("ba_gather128p_kernel<%d, %d, %s>" % (KV4, US, FS), gx, gy, lds=lds, attr=attr)


def strip(KV4, NCH, FP, gx, gy, block=128, lds=0, attr=False):
    return K_("ba_gather128s_kernel<%d, %d, %s>" % (KV4, NCH, FP), gx, gy, block=block, lds=lds, attr=attr)


def quad(KV4, gx, gy):
    return K_("ba_gather128q_kernel<%d>" % KV4, gx, gy)


# the frame-parallel strip workgroup's dynamic LDS, written out: (frames x (7 x 21 x 32 + 128) + 4 x 64 + 4) floats
FP_LDS = {2: 39696, 3: 59024, 4: 78352, 5: 97680, 6: 117008, 7: 136336}


# ---- 1. lists written out in full; the grids by hand from plan_gather's rules ------------------------------------------------------
def test_lists_written_out(lib):
    F = tp.dev_flags(lib)
    force_strip = F["kDevForceStripGather"]
    gen = F["kDevGenericGather"] | F["kDevNoQuadGather"]
    fpatch = F["kDevForcePatchGather"] | F["kDevNoQuadGather"]
    table = [
        # forced strip, 32 x 48, 4 frames: 3 x 2 16-row segments, one per frame-parallel workgroup of 4 waves; 2 x 4 x 8 queue words
        (level(2, 32, 48, 128, 4, force_strip), [zero(64, 1), strip(1, 4, "true", 6, 2, block=256, lds=78352, attr=True)]),
        # ... 23 x 21, 7 frames: 2 x 2 segments, 7 waves, 136336 B
        (level(2, 23, 21, 128, 7, force_strip), [zero(112, 2), strip(1, 4, "true", 4, 2, block=448, lds=136336, attr=True)]),
        # the plan's own choice at 480 x 640 x 32: 40 x 30 16-row segments, 1024 resident 128-thread workgroups / 32 windows;
        # 1200 rows per window -> 19 after the fold
        (level(32, 480, 640, 128, 1), [zero(256, 4), strip(1, 4, "false", 32, 32), fold(19, 32)]),
        # ... three frames, K = 256: frame-parallel, 2 workgroups per CU by LDS (163840 / 59024), 512 / 32 per window; below 64 KB: no attribute
        (level(32, 480, 640, 256, 3), [zero(768, 12), strip(2, 4, "true", 16, 32, block=192, lds=59024), fold(19, 96)]),
        # the generic kernel (forced) at 23 x 21: 9 tiles = 3 groups of 4, one partial row per workgroup: no queue, no fold
        (level(2, 23, 21, 20, 1, gen), [generic(2, 1, "false", 2, 1, 3, 2)]),
        # the plan's own choice at 32 x 48 x 2: 12 x 8 4x4 items, 4 per workgroup; 96 rows -> 2 after the fold
        (level(2, 32, 48, 20, 1), [zero(16, 1), quad(1, 24, 2), fold(2, 2)]),
        # forced patch at 37 x 53: 7 x 5 tiles -> 9 workgroups, rounded up to 16; 35 rows: no fold
        (level(2, 37, 53, 128, 1, fpatch), [zero(16, 1), patch(1, 2, "true", 16, 2)]),
        # ... three frames: grid y = 6 virtual windows; with the frames looped over inside a tile: y = 2 windows
        (level(2, 37, 53, 20, 3, fpatch), [zero(48, 1), patch(1, 2, "true", 16, 6)]),
        (level(2, 37, 53, 20, 3, fpatch | F["kDevPatchPairLoop"]), [zero(48, 1), patch(1, 2, "true", 16, 2)]),
    ]
    for (lv, want), (rc, steps) in zip(table, steps_of(lib, [t[0] for t in table])):
        assert rc == 0 and steps == want, (lv, steps, want)


def test_with_and_without_the_zeroing_step(lib):
    lv = level(32, 480, 640, 128, 1)
    (rc, steps), = steps_of(lib, [lv], reset_queue=True)
    assert rc == 0 and steps == [zero(256, 4), strip(1, 4, "false", 32, 32), fold(19, 32)]
    (rc, steps), = steps_of(lib, [lv], reset_queue=False)
    assert rc == 0 and steps == [strip(1, 4, "false", 32, 32), fold(19, 32)]
    # the generic kernel has no queue: prepare_gather zeroed it for the C = 128 kernels only
    gen = tp.dev_flags(lib)["kDevGenericGather"] | tp.dev_flags(lib)["kDevNoQuadGather"]
    for reset in (True, False):
        (rc, steps), = steps_of(lib, [level(2, 23, 21, 20, 1, gen)], reset_queue=reset)
        assert rc == 0 and steps == [generic(2, 1, "false", 2, 1, 3, 2)]


# ---- 2. every gather flag set of the case table: the old launchers restated, their grid from GatherPlan ------------------------------
def old_launches(lv, pl, F, reset_queue=True):
    """prepare_gather + launch_gather + finish_gather of the commit before the step list, statement for statement; lv: a level row,
    pl: its GatherPlan fields.  -> (rc, [step, ...]) with the launches enqueued before a refusal dropped (the accepted difference: the
    old code had already zeroed the queue then; no C = 128 launcher refuses a K that use_c128 lets through, so it never showed)"""
    B, N, C, K, H, W, dense, grad, pairs, policy, flags = lv
    pairs = max(pairs, 1)
    out = []
    if reset_queue and pl["c128"]:
        words = B * pairs * 8
        out.append(zero(words, (words + 63) // 64))
    gx, vb = pl["G"], B * pairs
    k4 = (K & 3) == 0
    if pl["c128"] and pl["quad"]:
        if K == 0: out.append(quad(0, gx, vb))
        elif k4 and K <= 128: out.append(quad(1, gx, vb))
        elif k4 and K <= 256: out.append(quad(2, gx, vb))
        else: return UNSUPPORTED, []
    elif pl["c128"] and pl["strip"]:
        seg_h = pl["strip"]
        tall, low = seg_h == 32, seg_h == 8
        assert seg_h in (8, 16, 32)
        if pl["strip_fp"]:
            assert not tall and not low and 2 <= pairs <= 7
            shm = (pairs * (7 * 21 * 32 + 128) + 4 * 64 + 4) * 4
            kv4 = 0 if K == 0 else 1 if k4 and K <= 128 else 2 if k4 and K <= 256 else None
            if kv4 is None: return UNSUPPORTED, []
            out.append(strip(kv4, 4, "true", gx, B, block=64 * pairs, lds=shm, attr=shm > 64 * 1024))
        else:
            nch = 8 if tall else 2 if low else 4
            kv4 = 0 if K == 0 else 1 if k4 and K <= 128 else 2 if k4 and K <= 256 else None
            if kv4 is None: return UNSUPPORTED, []
            out.append(strip(kv4, nch, "false", gx, B))
    elif pl["c128"] and pl["patch"]:
        gy = B if pl["pairloop"] else vb
        dyn = 60 * 1024 if flags & F["kDevPatchOnePerCU"] else 0
        u4, packed = bool(flags & F["kDevPatchUnits4"]), bool(flags & F["kDevPatchPacked"])
        small = H * W * C * 4 < (1 << 31) and N * C * 4 < (1 << 31)
        fs = small and not packed and not dyn
        if K == 0 and fs: out.append(patch(0, 2, "true", gx, gy))
        elif K == 0: out.append(patch(0, 2, "false", gx, gy))
        elif k4 and K <= 128 and u4: out.append(patch(1, 4, "false", gx, gy))
        elif k4 and K <= 128 and (packed or not small or dyn): out.append(patch(1, 2, "false", gx, gy, lds=dyn, attr=bool(dyn)))
        elif k4 and K <= 128: out.append(patch(1, 2, "true", gx, gy))
        elif k4 and K <= 256 and fs: out.append(patch(2, 2, "true", gx, gy))
        elif k4 and K <= 256: out.append(patch(2, 2, "false", gx, gy))
        else: return UNSUPPORTED, []
    elif pl["c128"]:
        if K == 0: out.append(direct(0, gx, vb))
        elif k4 and K <= 128: out.append(direct(1, gx, vb))
        elif k4 and K <= 256: out.append(direct(2, gx, vb))
        else: return UNSUPPORTED, []
    else:
        even, keven = (C & 1) == 0, (K & 1) == 0
        if even and C <= 128: vc = (2, 1)
        elif even and C <= 256: vc = (2, 2)
        elif C <= 64: vc = (1, 1)
        elif C <= 128: vc = (1, 2)
        else: return UNSUPPORTED, []
        if K == 0: kk = (1, 0)
        elif keven and K <= 128: kk = (2, 1)
        elif keven and K <= 256: kk = (2, 2)
        elif K <= 64: kk = (1, 1)
        elif K <= 128: kk = (1, 2)
        else: return UNSUPPORTED, []
        out.append(generic(vc[0], vc[1], "true" if grad else "false", kk[0], kk[1], gx, vb))
    if pl["frows"] != pl["rows"]:
        out.append(fold(pl["frows"], vb))
    return 0, out


MATRIX_SHAPES = ac.SHAPES + ((480, 640),)
MATRIX_BATCHES = (2, 32)
MATRIX_KS = (0, 20, 128, 256)
MATRIX_FRAMES = (1, 3, 4, 7)


def test_every_flag_set_of_the_case_table(lib):
    F = tp.dev_flags(lib)
    levels, names = [], []
    for name, (bits, sel, frames) in ac.gather_flag_sets().items():
        for H, W in MATRIX_SHAPES:
            for B in MATRIX_BATCHES:
                for K in MATRIX_KS:
                    for pairs in MATRIX_FRAMES:
                        if frames is not None and pairs == 1:
                            continue                                    # a multi-frame form
                        levels.append(level(B, H, W, K, pairs, int(bits)))
                        names.append(name)
    assert len(levels) == (10 * 4 + 3 * 3) * 4 * 2 * 4                  # ten forms at 1, 3, 4, 7 frames, three multi-frame ones
    families = {}
    for reset in (True, False):
        for name, lv, pl, (rc, steps) in zip(names, levels, plans_of(lib, levels), steps_of(lib, levels, reset_queue=reset)):
            assert pl["rc"] == 0
            want = old_launches(lv, pl, F, reset_queue=reset)
            assert (rc, steps) == want, (name, lv, steps, want)
            families.setdefault(name, set()).add([s for s in steps if "gather" in s][0].split("<")[0])
    # the table's forms reach what their names say at the table's own (small) shapes; here, with 480 x 640 among the shapes, at least that
    assert families["generic"] == {"ba_gather_kernel"} and "ba_gather128_kernel" in families["direct"]
    assert "ba_gather128p_kernel" in families["patch"] and "ba_gather128s_kernel" in families["strip"]
    assert "ba_gather128q_kernel" in families["quad"]


# ---- 3. the generic kernel's instantiation by parity and size of C and K, the [f|gx|gy] layout, the two refusals ---------------------
GENERIC_C = {63: (1, 1), 64: (2, 1), 65: (1, 2), 127: (1, 2), 128: (2, 1), 130: (2, 2), 256: (2, 2)}       # C -> (VEC, CH)
GENERIC_K = {0: (1, 0), 63: (1, 1), 64: (2, 1), 65: (1, 2), 127: (1, 2), 128: (2, 1), 130: (2, 2), 256: (2, 2)}   # K -> (KVEC, KCH)


def test_generic_kernel_by_parity_and_size(lib):
    F = tp.dev_flags(lib)
    gen = F["kDevGenericGather"] | F["kDevNoQuadGather"]
    for grad in (0, 1):
        levels = [level(2, 23, 21, K, 1, gen, C=C, grad=grad) for C in GENERIC_C for K in GENERIC_K]
        want = [[generic(v, c, "true" if grad else "false", kv, kc, 3, 2)] for (v, c) in GENERIC_C.values() for (kv, kc) in GENERIC_K.values()]
        for lv, (rc, steps), exp in zip(levels, steps_of(lib, levels), want):
            assert rc == 0 and steps == exp, (lv, steps, exp)
    # the two refusals: odd C above 128, odd K above 128 -- and nothing enqueued, not even at C = 128 where the queue would be zeroed
    for lv in (level(2, 23, 21, 20, 1, gen, C=129), level(2, 23, 21, 129, 1, gen, C=64), level(2, 23, 21, 255, 1, gen, C=128),
               level(2, 23, 21, 129, 1, 0, C=128), level(2, 23, 21, 131, 3, gen, C=255, grad=1)):
        (rc, steps), = steps_of(lib, [lv])
        assert rc == UNSUPPORTED and steps == [], lv


def test_sparse_points(lib):
    # 1000 points x 2 windows: 16 per item (4 x 32 items fit a resident round) -> 63 items, 16 groups; [f|gx|gy] map, C = 70, K = 33
    (rc, steps), = steps_of(lib, [level(2, 48, 64, 33, 1, 0, C=70, grad=1, dense=0, N=1000)])
    assert rc == 0 and steps == [generic(2, 1, "true", 1, 1, 16, 2)]
    # the C-channel map at C = 128, K % 4 == 0: the direct kernel on sparse points
    (rc, steps), = steps_of(lib, [level(2, 48, 64, 128, 1, 0, C=128, grad=0, dense=0, N=1000)])
    assert rc == 0 and [s.split(" grid")[0] for s in steps] == ["zero_iters_kernel words(16)", "ba_gather128_kernel<1>"]


# ---- 4. the patch kernel's flags and the 2 GiB limit -------------------------------------------------------------------------------
def test_patch_flags(lib):
    F = tp.dev_flags(lib)
    fpatch = F["kDevForcePatchGather"] | F["kDevNoQuadGather"]
    u4, packed, one = F["kDevPatchUnits4"], F["kDevPatchPacked"], F["kDevPatchOnePerCU"]
    Z = zero(16, 1)
    table = [   # 37 x 53 x 2, one frame: grid (16, 2)
        (0, 0, patch(0, 2, "true", 16, 2)), (0, packed, patch(0, 2, "false", 16, 2)), (0, u4, patch(0, 2, "true", 16, 2)),
        (0, one, patch(0, 2, "false", 16, 2)),                                               # the 60 KB go to <1, 2, false> alone
        (128, 0, patch(1, 2, "true", 16, 2)), (20, u4, patch(1, 4, "false", 16, 2)), (128, u4 | one, patch(1, 4, "false", 16, 2)),
        (128, packed, patch(1, 2, "false", 16, 2)), (128, one, patch(1, 2, "false", 16, 2, lds=61440, attr=True)),
        (128, packed | one, patch(1, 2, "false", 16, 2, lds=61440, attr=True)),
        (256, 0, patch(2, 2, "true", 16, 2)), (256, u4, patch(2, 2, "true", 16, 2)), (256, packed, patch(2, 2, "false", 16, 2)),
        (256, one, patch(2, 2, "false", 16, 2)),
    ]
    levels = [level(2, 37, 53, K, 1, fpatch | bits) for K, bits, _ in table]
    for (K, bits, want), (rc, steps) in zip(table, steps_of(lib, levels)):
        assert rc == 0 and steps == [Z, want], (K, bits, steps)


def test_patch_level_past_2_gib_drops_the_fixed_stride(lib):
    # 2048 x 2048 x 128 floats = 2^31 B: the strip gather declines it, 65536 tiles -> one resident round of 512 workgroups, 1024 folded rows
    for K, kv4 in ((0, 0), (128, 1), (256, 2)):
        (rc, steps), = steps_of(lib, [level(1, 2048, 2048, K, 1)])
        assert rc == 0 and steps == [zero(8, 1), patch(kv4, 2, "false", 512, 1), fold(1024, 1)], (K, steps)
    # one pixel row fewer: below the limit -- the strip gather takes the level; with it off, the fixed-stride patch
    (rc, steps), = steps_of(lib, [level(1, 2047, 2048, 128, 1, tp.dev_flags(lib)["kDevNoStripGather"])])
    assert rc == 0 and steps == [zero(8, 1), patch(1, 2, "true", 512, 1), fold(1024, 1)], steps


# ---- 5. the strip kernel: seg_h -> NCH, FP at NCH = 4 with 2 .. 7 frames, the one LDS formula -------------------------------------
def test_strip_segment_heights_and_frame_parallel_workgroups(lib):
    F = tp.dev_flags(lib)
    force = F["kDevForceStripGather"]
    # 32 x 48 x 2, one frame: 3 segment columns x 4 / 2 / 1 segment rows, two segments per 128-thread workgroup
    for bits, nch, G in ((force | F["kDevQuarterTiles"], 2, 6), (force, 4, 3), (force | F["kDevStripRows32"], 8, 2)):
        (rc, steps), = steps_of(lib, [level(2, 32, 48, 128, 1, bits)])
        assert rc == 0 and steps == [zero(16, 1), strip(1, nch, "false", G, 2)], (nch, steps)
    # 2 .. 7 frames: one workgroup of `frames` waves per segment; 8 frames and kDevStripFrameLoop: the frames looped over in one wave
    for pairs in range(2, 8):
        (rc, steps), = steps_of(lib, [level(2, 32, 48, 128, pairs, force)])
        words = 2 * pairs * 8
        assert rc == 0 and steps == [zero(words, (words + 63) // 64),
                                     strip(1, 4, "true", 6, 2, block=64 * pairs, lds=FP_LDS[pairs], attr=pairs >= 4)], (pairs, steps)
    for pairs, bits in ((8, force), (3, force | F["kDevStripFrameLoop"])):
        (rc, steps), = steps_of(lib, [level(2, 32, 48, 128, pairs, bits)])
        assert rc == 0 and steps[1] == strip(1, 4, "false", 3, 2), (pairs, steps)
    # 8- and 32-row segments are never frame-parallel
    for bits, nch in ((force | F["kDevQuarterTiles"], 2), (force | F["kDevStripRows32"], 8)):
        (rc, steps), = steps_of(lib, [level(2, 32, 48, 128, 3, bits)])
        assert rc == 0 and steps[1].startswith("ba_gather128s_kernel<1, %d, false> " % nch) and " block 128 lds 0" in steps[1]
    # what plan_gather never hands over, refused as the old launcher refused it (BANET_ERR_INVALID_ARG = -1)
    lv = _desc([level(2, 32, 48, 128, 3)])
    for seg_h, fp, rc in ((16, 0, 0), (16, 1, 0), (12, 0, -1), (8, 1, -1), (32, 1, -1)):
        assert lib.banet_test_gather_steps_of_strip(lv.ctypes.data, seg_h, fp) == rc, (seg_h, fp)
    for pairs in (1, 8):
        lv = _desc([level(2, 32, 48, 128, pairs)])
        assert lib.banet_test_gather_steps_of_strip(lv.ctypes.data, 16, 1) == -1


def test_fp_lds_formula(lib):
    """the value choose_strip divides 160 KB by, the step's LDS and the kernel's layout: one function"""
    for pairs in range(2, 8):
        by_hand = (pairs * (7 * 21 * 32 + 128) + 4 * 64 + 4) * 4
        assert lib.banet_test_strip_fp_lds_bytes(pairs, 4) == by_hand == FP_LDS[pairs]
    assert FP_LDS[4] == 78352 and FP_LDS[7] == 136336 and FP_LDS[3] < 65536 < FP_LDS[4]
    # the workgroups per CU that follow: min(8 / frames, 160 KB / LDS) = 4, 2, 2, 1, 1, 1 -- read back from a level's grid
    # (960 x 1280 x 32, 6400 segments: G = resident workgroups / 32 windows)
    for pairs, per_cu in ((2, 4), (3, 2), (4, 2), (5, 1), (6, 1), (7, 1)):
        (rc, steps), = steps_of(lib, [level(32, 960, 1280, 128, pairs)])
        assert rc == 0 and steps[1] == strip(1, 4, "true", CUS * per_cu // 32, 32, block=64 * pairs, lds=FP_LDS[pairs], attr=pairs >= 4), (pairs, steps)


# ---- 6. the sweep: every planned level has a compiled kernel, the lists are reached, capacity -----------------------------------------
def sweep_levels():
    """test_plan_cpu.sweep_levels(), and -- its channel counts are 64, 127, 128, its K all even -- one shape with odd C up to 64, even C
    above 128 and odd K on both sides of 64, which <1, 1, ..>, <2, 2, ..> and <.., 1, 1> / <.., 1, 2> of the generic kernel need"""
    levels, _ = tp.sweep_levels()
    extra = [(2, 60 * 80, C, K, 60, 80, 1, grad, 1, 0) for C in (63, 64, 127, 130) for grad in (0, 1) for K in (0, 6, 33, 65, 256)]
    return np.concatenate([levels, np.asarray(extra, np.int32)])


# reachable only by flag (or past 2 GiB: test_patch_level_past_2_gib_drops_the_fixed_stride): every level of the sweep is small, so FS
# is dropped by kDevPatchPacked / kDevPatchOnePerCU alone, and US = 4 is kDevPatchUnits4
ONLY_BY_FLAG = {"ba_gather128p_kernel<0, 2, false>", "ba_gather128p_kernel<1, 2, false>", "ba_gather128p_kernel<2, 2, false>",
                "ba_gather128p_kernel<1, 4, false>"}


def test_sweep_capacity_refusals_and_instantiations(lib):
    levels = sweep_levels()
    flags = tp.dev_flags(lib)
    compiled = lib.banet_test_gather_instantiations().decode().split("\n")[:-1]
    assert len(compiled) == len(set(compiled)) == 40 + 3 + 7 + 12 + 3
    compiled = set(compiled)
    assert ONLY_BY_FLAG <= compiled
    others = {"zero_iters_kernel", "ba_fold_kernel"}
    fpatch = flags["kDevForcePatchGather"] | flags["kDevNoQuadGather"]
    words = [(w, False) for _, w in tp.flag_words(flags)] + [(fpatch | flags[n], True) for n in ("kDevPatchUnits4", "kDevPatchPacked", "kDevPatchOnePerCU")]
    reached, by_flag, most = set(), set(), 0
    for word, patch_flag in words:
        desc = np.ascontiguousarray(np.concatenate([levels, np.full((len(levels), 1), word, np.int32)], axis=1))
        for reset in (0, 1):
            out = np.zeros((len(desc), 3), np.int32)
            names = set(lib.banet_test_gather_steps_sweep(desc.ctypes.data, len(desc), CUS, reset, out.ctypes.data).decode().split("\n")[:-1])
            (by_flag if patch_flag else reached).update(names)
            rc_plan, rc, n = out[:, 0], out[:, 1], out[:, 2]
            planned = rc_plan == 0
            # REFUSALS, from the old launchers: odd C above 128 or odd K above 128 on the generic kernel.  The sweep holds neither (odd C:
            # 63, 127; odd K: 33, 65), and use_c128 lets only K % 4 == 0, K <= 256 through to the C = 128 kernels: no planned level is refused
            assert (rc[planned] == 0).all() and (n[planned] >= 1).all() and (n[~planned] == 0).all()
            most = max(most, int(n.max()))
    assert most == 3 == lib.banet_test_gather_max_steps()      # zero, the gather kernel, fold
    assert reached - others <= compiled and by_flag - others <= compiled
    assert others <= reached
    assert reached - others == compiled - ONLY_BY_FLAG, sorted((reached - others) ^ (compiled - ONLY_BY_FLAG))
    assert ONLY_BY_FLAG <= by_flag
