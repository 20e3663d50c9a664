"""The inputs of the sparse-layout adjoint tests (adjoint_cases.py) are what they claim to be, the float32 yardstick the GPU module
(test_gpu_sparse_adjoint.py) relies on, the dispatch of launch_dense_adjoint -- asked of its own plan, csrc/adjoint_plan.hpp compiled
with g++ -- enumerated against the cases of both adjoint GPU modules, the plan's workspace totals against the loaded library, and
the shapes the sparse layout refuses -- all on the CPU.

The yardstick: the same autograd through oracle/torch_port.sparse_assemble in float32 torch against float64, on the same float32
inputs, every tensor on its own per-window max-norm scale.  It must stay below a quarter of the gate: the gate is then reachable by
plain float32 arithmetic and the inputs are not ill-posed."""
import ctypes
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

import adjoint_cases as ac

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
_IDS = [c.name for c in ac.CASES]


@pytest.mark.parametrize("name", _IDS)
def test_case_conditions_and_the_float32_yardstick(name):
    ref = ac.reference(name)
    case, inp, fwd, want = ref["case"], ref["inp"], ref["fwd"], ref["want"]
    B, N, C, K, H, W = case.B, case.N, case.C, case.K, case.H, case.W
    # float32 numbers, the declared shapes
    for k in ("conv1", "conv2", "D", "Bs", "R", "T", "Wc", "fx", "fy", "ox", "oy", "p", "G", "gb", "gabs"):
        v = inp[k]
        assert v is None or (v.dtype == torch.float64 and torch.equal(v, v.float().double())), k
    assert inp["conv1"].shape == (B, N, C) and inp["conv2"].shape == (B, H, W, 3 * C) and inp["p"].shape == (B, 3, N)
    assert (inp["Bs"] is None) == (K == 0) and inp["G"].shape == (B, 6 + K, 6 + K)
    # intrinsics differ from point to point, from window to window, and fx from fy
    if N > 1:
        for k in ("fx", "fy", "ox", "oy"):
            assert bool((inp[k].max(1).values > inp[k].min(1).values).all()), k
    assert not torch.equal(inp["fx"], inp["fy"]) and not torch.equal(inp["fx"][0], inp["fx"][1]) and not torch.equal(inp["ox"][0], inp["ox"][1])
    assert float((inp["fx"] - inp["fy"]).abs().min()) > 0.0
    # no projection near an integer coordinate
    fr = lambda v: float((v - torch.round(v)).abs().min())       # noqa: E731
    assert fr(fwd["px"]) >= ac.INT_MARGIN and fr(fwd["py"]) >= ac.INT_MARGIN
    assert inp["nudges"] <= 3
    # share of outside points per window
    inside = fwd["mask"] > 0
    out_share = 1.0 - inside.double().mean(1)
    for b in range(B):
        if case.special == "empty" and b == 1:
            assert float(out_share[b]) == 1.0
        elif name in ac.NO_OUTSIDE_SHARE and case.special != "empty":
            assert int(inside[b].sum()) >= 1, "window %d is empty by accident" % b
        else:
            assert ac.OUTSIDE_SHARE[0] <= float(out_share[b]) <= ac.OUTSIDE_SHARE[1], (name, b, float(out_share[b]))
    if case.special in ("inside", "cluster"):
        assert bool(inside.all())
    if case.special == "cluster":               # a long cell list: every point of a window in the same two cells
        key = torch.floor(fwd["py"]).long() * W + torch.floor(fwd["px"]).long()
        for b in range(B):
            cells, counts = torch.unique(key[b], return_counts=True)
            assert cells.tolist() == [9 * W + 7, 9 * W + 8] and int(counts.min()) >= 64, (cells, counts)
    # |d| away from its kink
    d = fwd["d"].abs()[inside]
    assert d.numel() == 0 or float(d.min()) >= ac.MIN_ABS_D
    # the reference: finite, no output identically zero in a window that is not empty by construction
    for k, v in want.items():
        assert bool(torch.isfinite(v).all()), k
        for b in range(B):
            empty = case.special == "empty" and b == 1
            assert (float(v[b].abs().max()) == 0.0) == empty, (name, k, b)
    assert set(want) == set(ac.OUTPUTS if K else [o for o in ac.OUTPUTS if o not in ("dbasis", "dW")])
    # the float32 yardstick
    assert ref["finite32"]
    worst = {}
    for k, errs in ref["e_ref32"].items():
        assert len(errs) == B
        worst[k] = max(errs)
        assert worst[k] <= ac.GATE[k] / 4, (name, k, errs)
        assert ac.gate_of(name, k) == ac.GATE[k]
    print("%-22s nudges %d outside %s  e_ref32 %s" % (name, inp["nudges"], ["%.2f" % float(s) for s in out_share],
                                                      " ".join("%s %.1e" % kv for kv in worst.items())))


def test_cases_are_reproducible_and_cover_the_listed_shapes():
    a, b = ac.make_case(ac.BY_NAME["bundle-C5-K3"]), ac.make_case(ac.BY_NAME["bundle-C5-K3"])
    for k, v in a.items():
        assert (v is b[k] or v == b[k]) if not torch.is_tensor(v) else torch.equal(v, b[k]), k
    assert len(set(c.name for c in ac.CASES)) == len(ac.CASES)
    shapes = {(c.C, c.K) for c in ac.CASES if c.variant == "bundle" and c.N == 500 and (c.H, c.W) == (20, 24) and c.special is None}
    assert shapes >= set(ac.SPARSE_BUNDLE_CK)
    assert {c.C for c in ac.CASES if c.variant == "bundle_camera"} == {6, 128, 131, 255}
    assert {(c.N, c.B) for c in ac.CASES if c.name.startswith("ragged")} == {(1, 2), (3, 2), (63, 2), (64, 2), (65, 3), (257, 2)}
    assert {(c.H, c.W) for c in ac.CASES if c.name.startswith("scan")} == {(4, 4), (32, 32), (25, 41)}
    assert ac.BY_NAME["N4096-8x8"].N == 4096 and ac.BY_NAME["empty-window"].B == 3 and ac.BY_NAME["cluster-two-cells"].N == 300
    for n_ in ac.ACCUMULATION_CASES + (ac.REPRODUCIBILITY_CASE,):
        assert n_ in ac.BY_NAME
    assert all(c.N <= 4096 for c in ac.CASES)
    # the forward has a kernel for every case but those with an odd C or K above 128 (plan.hpp, plan_gather_steps)
    assert set(ac.FORWARD_NOT_COMPILED) == {c.name for c in ac.CASES if (c.C > 128 and c.C % 2) or (c.K > 128 and c.K % 2)}


def test_window_errors_does_not_let_a_wrong_window_hide():
    want = torch.tensor([[1000.0, 1.0], [1e-3, 2e-3], [0.0, 0.0]])
    got = want.clone()
    got[1, 0] += 1e-3
    e = ac.window_errors(got, want)
    assert e[0] == 0.0 and abs(e[1] - 0.5) < 1e-12 and e[2] == 0.0
    got[2, 1] = 1e-30
    assert ac.window_errors(got, want)[2] == float("inf")
    got[0, 0] = float("nan")
    assert ac.window_errors(got, want)[0] == float("inf")


# ---- the dispatch, answered by plan_adjoint (csrc/adjoint_plan.hpp through tests/native/adjoint_plan_host.cpp) -------------------
def test_dispatch_mirror_on_known_shapes():
    assert ac.dispatch("dense", "bundle", 128, 128, True) == ("adj_basis6_kernel<8, false>", "adj_pixel2_kernel<1, true>", "adj_map2_kernel<3, 6>")
    assert ac.dispatch("dense", "bundle", 128, 128, False)[1] == "adj_pixel2_kernel<1, false>"
    assert ac.dispatch("dense", "bundle", 128, 128, False, ac.DEV_ADJ_PIXEL_PER_WAVE)[1] == "adj_pixel_kernel<2, 2>"
    assert ac.dispatch("dense", "bundle", 128, 128, False, ac.DEV_ADJ_FP32_MFMA)[0] == "adj_basis_kernel<8>"
    assert ac.dispatch("dense", "bundle", 128, 128, False, ac.DEV_ADJ_TEXEL_PER_WAVE)[2] == "adj_map_kernel<6>"
    assert ac.dispatch("dense", "bundle", 128, 128, False, N=1 << 24)[1] == "adj_pixel_kernel<2, 2>"
    assert ac.dispatch("sparse", "bundle", 128, 128, True) == ("adj_basis6_kernel<8, false>", "adj_pixel_kernel<2, 2, true>", "adj_map2_kernel<3, 6>")
    assert ac.dispatch("sparse", "bundle_camera", 131, 0, True) == (None, "adj_pixel_kernel<3, 1, true>", "adj_map_kernel<12>")
    assert ac.dispatch("sparse", "bundle", 130, 130, True)[1] is None            # refused before the launch (no point instantiation)
    assert ac.dispatch("dense", "bundle", 3, 1) == ("adj_basis_kernel<1>", "adj_pixel_kernel<1, 1>", "adj_map_kernel<3>")
    assert ac.dispatch("dense", "bundle", 256, 256)[:2] == ("adj_basis_wide_kernel<16, 6>", "adj_pixel_kernel<4, 4>")


def test_fold_mode_tile_dispatch_on_known_shapes():
    """BANET_ADJOINT_FOLD_TARGET: (channel chunks, vector width) by C, tile shape by BANET_ADJOINT_TILE_SHAPE"""
    assert ac.tile_dispatch(128, 0) == "adj_tile2_kernel<8, 4>"
    assert [ac.tile_dispatch(128, k) for k in range(9, 14)] == ["adj_tile2_kernel<8, 3>", "adj_tile2_kernel<8, 5>", "adj_tile2_kernel<8, 7>",
                                                                "adj_tile2_kernel<16, 3>", "adj_tile2_kernel<16, 2>"]
    assert ac.tile_dispatch(128, 3) == "adj_tile_kernel<1, 2, 8, 2>"
    assert ac.tile_dispatch(6) == "adj_tile_kernel<1, 2, 8, 4>"
    assert ac.tile_dispatch(131) == "adj_tile_kernel<4, 1, 8, 4>"
    for shape in range(8, 16):                                   # C = 130 has no two-visit kernel: a shape >= 8 is shape 0 of adj_tile_kernel
        assert ac.tile_dispatch(130, shape) == "adj_tile_kernel<2, 2, 8, 4>"
    assert ac.tile_dispatch(5) == "adj_tile_kernel<1, 1, 8, 4>"
    # every tile instantiation of the lists is some level's choice, and no level chooses another
    got = {ac.tile_dispatch(C, k) for C in (5, 6, 65, 128, 130, 131) for k in range(16)}
    assert got == set(ac.ALL_TILE_KERNELS)


# ---- the plan against the loaded library: the header the tests compile and the library cannot drift ----------------------------
SWEEP_DENSE_HW = ((4, 4), (9, 11), (48, 64), (480, 640))
SWEEP_SPARSE_N = (1, 65, 4096)
SWEEP_C, SWEEP_K, SWEEP_B = (3, 4, 128, 131, 256), (0, 1, 16, 40, 128, 130, 256), (1, 2, 32)
SWEEP_ADJ_FLAGS = (0,) + tuple(ac.ADJOINT_FOLD_TARGET | k << 4 for k in range(14))      # every layout-changing flag: fold off / on, tile shapes 0-13


def workspace_sweep_rows():
    """plan_sweep rows: dense H x W and sparse N (looking at a 20 x 24 map) x C x K x B x adjoint flags"""
    rows = []
    for C in SWEEP_C:
        for K in SWEEP_K:
            for B in SWEEP_B:
                for fl in SWEEP_ADJ_FLAGS:
                    var = "bundle" if K else "bundle_camera"
                    rows += [ac.level_row("dense", var, C, K, B=B, adj_flags=fl, HW=hw) for hw in SWEEP_DENSE_HW]
                    rows += [ac.level_row("sparse", var, C, K, N=N, B=B, adj_flags=fl, HW=(20, 24)) for N in SWEEP_SPARSE_N]
    return rows


def library_workspace_bytes(L, rows):
    """banet_dense_adjoint_workspace_bytes_ex of the loaded library for plan_sweep rows (host side, no launch)"""
    from banet_amd import _capi as capi
    one = (ctypes.c_float * 4)()
    ptr = ctypes.cast(one, ctypes.c_void_p).value                # any non-null pointer: the plan only checks presence
    out = []
    for B, N, C, K, H, W, dense, grad, pairs, variant, lv_flags, adj_flags in rows:
        lv = capi.Level()
        lv.B, lv.N, lv.C, lv.K, lv.H, lv.W = B, N, C, K, H, W
        lv.variant, lv.dense, lv.tgt_has_grad, lv.scale, lv.pairs, lv.flags = variant, dense, grad, 1.0, pairs, lv_flags
        lv.src = lv.tgt = lv.depth = lv.basis = lv.rays = lv.fx = lv.fy = lv.ox = lv.oy = ptr
        out.append(L.banet_dense_adjoint_workspace_bytes_ex(ctypes.byref(lv), adj_flags))
    return out


GOLDEN = os.path.join(ROOT, "tests", "golden", "adjoint_plan_digests.json")


def plan_digests():
    """what the golden file keeps: SHA-256 over (rc, every AdjPlan field) as int64 and over the chosen kernels' names, of the workspace
    sweep and of its unfolded rows once more under each of the three kDevAdj* switches and with BANET_ADJOINT_OVERWRITE"""
    rows = workspace_sweep_rows()
    plain = [r for r in rows if r[11] == 0]
    for bit in (ac.DEV_ADJ_FP32_MFMA, ac.DEV_ADJ_PIXEL_PER_WAVE, ac.DEV_ADJ_TEXEL_PER_WAVE):
        rows += [r[:10] + (bit, 0) for r in plain]
    rows += [r[:11] + (ac.ADJOINT_OVERWRITE,) for r in plain]
    plans, names = ac.plan_sweep(rows)
    text = "\n".join("|".join(k or "" for k in row) for row in names)
    return {"what": "tests/test_adjoint_cases_cpu.py: SHA-256 of the plan_adjoint sweep (PYTHONPATH=. python tests/test_adjoint_cases_cpu.py --regenerate)",
            "cases": len(rows), "fields": ac.plan_fields(), "plans_sha256": hashlib.sha256(plans.tobytes()).hexdigest(),
            "kernels_sha256": hashlib.sha256(text.encode()).hexdigest()}


def test_adjoint_plans_match_the_recorded_digests():
    """a changed G is a changed summation tree, a changed offset is two buffers overlapping, a changed kernel choice is other arithmetic:
    none may happen silently.  After a DELIBERATE change: PYTHONPATH=. python tests/test_adjoint_cases_cpu.py --regenerate"""
    assert plan_digests() == json.load(open(GOLDEN))


SSTATS_SWEEP = [(B, N, C, H, W) for B in SWEEP_B for N in SWEEP_SPARSE_N for C in SWEEP_C + (257,) for H, W in SWEEP_DENSE_HW]


def test_plan_bytes_equal_the_library_workspace_queries():
    from banet_amd import _capi as capi
    L = capi.lib()
    rows = workspace_sweep_rows()
    plans, _ = ac.plan_sweep(rows)
    col = {n: i for i, n in enumerate(ac.plan_fields())}
    want = [int(p[col["bytes"]]) if p[col["rc"]] == 0 else 0 for p in plans]
    got = library_workspace_bytes(L, rows)
    bad = [(r, g, w) for r, g, w in zip(rows, got, want) if g != w]
    assert not bad, "%d of %d differ, first: %s" % (len(bad), len(rows), bad[0])
    assert 0 in want and sum(1 for w in want if w > 0) > len(want) // 2          # refusals and plans both met
    ok = plans[plans[:, col["rc"]] == 0]
    refused = plans[plans[:, col["rc"]] != 0]
    assert len(refused) and (np.delete(refused, col["rc"], axis=1) == 0).all()      # a refused plan carries no layout and no kernel
    for f in [n for n in col if n.startswith("off_")] + ["bytes"]:
        assert (ok[:, col[f]] % 256 == 0).all(), f
    # the deterministic sample-stats gradient (its entry refuses B H W 3C >= 2^32 itself, before the plan)
    host = ac.host_lib()
    head, *names = host.banet_test_sstats_det_plan_fields().decode().split()
    assert head == "desc_ints=5"
    desc = np.ascontiguousarray(SSTATS_SWEEP, np.int32)
    out = np.zeros((len(desc), len(names)), np.int64)
    host.banet_test_sstats_det_plan_sweep(desc.ctypes.data_as(ctypes.c_void_p), len(desc), out.ctypes.data_as(ctypes.c_void_p))
    rc, nbytes = names.index("rc"), names.index("bytes")
    for (B, N, C, H, W), p in zip(SSTATS_SWEEP, out):
        want = int(p[nbytes]) if p[rc] == 0 and B * H * W * 3 * C < (1 << 32) else 0
        assert L.banet_sample_stats_grad_workspace_bytes(B, N, C, H, W) == want, (B, N, C, H, W)
        assert (C > 256) == (p[rc] != 0)


def _params(fn):
    """the argument tuples of a test's (single) pytest.mark.parametrize, with the names"""
    marks = [m for m in fn.pytestmark if m.name == "parametrize"]
    assert len(marks) == 1
    names = [s.strip() for s in marks[0].args[0].split(",")]
    return [dict(zip(names, row)) for row in marks[0].args[1]]


def dense_launches():
    """every (C, K, variant, overwrite) the kernel-level float64 comparisons of test_gpu_dense_backward.py launch, read from its
    parametrisations (imported, not copied): -> list of dispatch() results"""
    import test_gpu_dense_backward as tdb
    out = []
    for fn in (tdb.test_dense_adjoint_kernels_match_the_float64_statement, tdb.test_dense_adjoint_kernels_with_more_than_128_depth_coefficients):
        for q in _params(fn):
            out.append(ac.dispatch("dense", "bundle", q["C"], q["K"], False, N=q["H"] * q["W"]))
    for q in _params(tdb.test_pose_only_adjoint_kernels_match_the_float64_statement):
        out.append(ac.dispatch("dense", "bundle_camera", q["C"], 0, False, N=q["H"] * q["W"]))
    for q in _params(tdb.test_dense_adjoint_overwrite_mode_equals_accumulation_into_zeros):
        for ow in (False, True):
            out.append(ac.dispatch("dense", q["variant"], q["C"], q["K"], ow, N=q["H"] * q["W"]))
    return out


def sparse_launches():
    return [ac.dispatch("sparse", c.variant, c.C, c.K, True) for c in ac.CASES]


def test_sparse_cases_reach_every_point_instantiation_and_seed_class():
    got = sparse_launches()
    assert all(p is not None for _, p, _ in got)
    assert {p for _, p, _ in got} == {"adj_pixel_kernel<%d, %d, true>" % ck for ck in ac.SPARSE_POINT_INSTANTIATIONS}
    assert {s for s, _, _ in got} == set(ac.ALL_SEED_KERNELS) | {None}
    assert {m for _, _, m in got} == set(ac.ALL_MAP_KERNELS)
    # each (C, K) of the bundle list is there for a point instantiation of its own: the list alone reaches all 12, one each
    own = [ac.dispatch("sparse", "bundle", C, K, True)[1] for C, K in ac.SPARSE_BUNDLE_CK]
    assert len(own) == 12 and set(own) == {p for _, p, _ in got}
    assert {ac.dispatch("sparse", "bundle", C, K, True)[0] for C, K in ac.SPARSE_BUNDLE_CK} == set(ac.ALL_SEED_KERNELS)


def test_dense_cases_reach_every_pixel_seed_and_map_instantiation():
    got = dense_launches()
    assert all(p is not None for _, p, _ in got)
    want_pixel = {"adj_pixel_kernel<%d, %d>" % ck for ck in ac.DENSE_PIXEL_INSTANTIATIONS} | {"adj_pixel2_kernel<1, true>", "adj_pixel2_kernel<1, false>"}
    assert {p for _, p, _ in got} == want_pixel, sorted(want_pixel - {p for _, p, _ in got})
    assert {s for s, _, _ in got} == set(ac.ALL_SEED_KERNELS) | {None}, sorted(set(ac.ALL_SEED_KERNELS) - {s for s, _, _ in got})
    assert {m for _, _, m in got} == set(ac.ALL_MAP_KERNELS)


def test_two_pixel_kernel_edges_are_among_the_dense_cases():
    """adj_pixel2_kernel with one live lane (C = 4 / K = 4) and with C, K multiples of 4 but not of 16"""
    import test_gpu_dense_backward as tdb
    ck = {(q["C"], q["K"]) for q in _params(tdb.test_dense_adjoint_kernels_match_the_float64_statement)}
    assert {(4, 4), (100, 36), (128, 4), (4, 128)} <= ck
    for C, K in ((4, 4), (100, 36), (128, 4), (4, 128)):
        assert ac.dispatch("dense", "bundle", C, K)[1] == "adj_pixel2_kernel<1, false>"


# ---- what the sparse layout refuses (host side, no launch) --------------------------------------------------------------------
def test_sparse_layout_refusals():
    from banet_amd import _capi as capi
    L = capi.lib()
    FOLD = 4                                                     # banet_hip.h: BANET_ADJOINT_FOLD_TARGET
    one = (ctypes.c_float * 4)()
    ptr = ctypes.cast(one, ctypes.c_void_p).value                # any non-null pointer: the plan only checks presence

    def ws(C=128, K=128, flags=0, pairs=1):
        lv = capi.Level()
        lv.B, lv.N, lv.C, lv.K, lv.H, lv.W = 2, 500, C, K, 20, 24
        lv.variant, lv.dense, lv.tgt_has_grad, lv.scale, lv.pairs = capi.BUNDLE, 0, 1, 1.0, pairs
        lv.src = lv.tgt = lv.depth = lv.basis = lv.rays = lv.fx = lv.fy = lv.ox = lv.oy = ptr
        return L.banet_dense_adjoint_workspace_bytes_ex(ctypes.byref(lv), flags)

    assert ws() > 0
    assert ws(C=130, K=130) == 0                                 # no point kernel for > 2 channel chunks with > 2 coefficient chunks
    assert ws(C=130, K=128) > 0 and ws(C=128, K=130) > 0
    assert ws(flags=FOLD) == 0                                   # the tile kernels form the map's gradients themselves: dense layout only
    assert ws(pairs=2) == 0
    for c in ac.CASES:                                           # every case of the GPU module is accepted
        assert ws(C=c.C, K=max(c.K, 1)) > 0, c.name


if __name__ == "__main__":
    if sys.argv[1:] != ["--regenerate"]:
        sys.exit("usage: PYTHONPATH=. python tests/test_adjoint_cases_cpu.py --regenerate   (rewrites tests/golden/adjoint_plan_digests.json from the current tree)")
    with open(GOLDEN, "w") as f:
        json.dump(plan_digests(), f, indent=1)
        f.write("\n")
    print("wrote", GOLDEN)
