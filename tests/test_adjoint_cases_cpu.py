"""The inputs of the sparse-layout adjoint tests (adjoint_cases.py) are what they claim to be, the float32 yardstick the GPU module
(test_gpu_sparse_adjoint.py) relies on, the dispatch of launch_dense_adjoint enumerated against the cases of both adjoint GPU modules,
and the shapes the sparse layout refuses -- all on the CPU.

The yardstick: the same autograd through oracle/torch_port.sparse_assemble in float32 torch against float64, on the same float32
inputs, every tensor on its own per-window max-norm scale.  It must stay below a quarter of the gate: the gate is then reachable by
plain float32 arithmetic and the inputs are not ill-posed."""
import ctypes
import os

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
    # the forward has a kernel for every case but those with an odd C or K above 128 (gather.hip, launch_c / launch_k)
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


# ---- the dispatch mirror ---------------------------------------------------------------------------------------------------------
def _mirror_matches_the_source():
    """the line ranges adjoint_cases.dispatch cites still hold what it copies"""
    lines = open(os.path.join(ROOT, "banet_amd", "csrc", "adjoint.hip")).read().split("\n")
    seg = lambda lo, hi: "\n".join(lines[lo - 1:hi])             # noqa: E731
    return seg(2489, 2509), seg(2510, 2556), seg(2272, 2291)


def test_dispatch_mirror_cites_the_lines_it_copies():
    seed, pixel, mapk = _mirror_matches_the_source()
    assert seed.lstrip().startswith("const bool b6") and "switch ((K + 15) / 16)" in seed and seed.rstrip().endswith("}")
    for nk in range(2, 9):
        assert "case %d: b6 ? launch_adj_basis6<%d>(a, pl.Ga, s) : launch_adj_basis<%d>(a, pl.Ga, s); break;" % (nk, nk, nk) in seed
    assert "case 1: launch_adj_basis<1>" in seed and "case 9: case 10: case 11: case 12: launch_adj_basis_wide<12>" in seed
    assert "case 13: case 14: case 15: case 16: launch_adj_basis_wide<16>" in seed
    assert pixel.lstrip().startswith("if (!lv->dense)") and pixel.rstrip().endswith("}")
    point = [l for l in pixel.split("\n") if l.strip().startswith("BANET_ADJ_POINT(")]
    dense = [l for l in pixel.split("\n") if l.strip().startswith("BANET_ADJ_PIXEL(")]
    assert [tuple(int(v) for v in l.strip()[16:-2].split(",")) for l in point] == list(ac.SPARSE_POINT_INSTANTIATIONS)
    assert [tuple(int(v) for v in l.strip()[16:-2].split(",")) for l in dense] == list(ac.DENSE_PIXEL_INSTANTIATIONS)
    assert "(lv->C & 3) == 0 && (K & 3) == 0 && lv->C <= 128 && K <= 128 && !(lv->flags & kDevAdjPixelPerWave)" in pixel
    assert "adj_pixel2_kernel<1, true>" in pixel and "adj_pixel2_kernel<1, false>" in pixel
    assert mapk.startswith("static void launch_adj_map") and mapk.rstrip().endswith("}")
    for k in ac.ALL_MAP_KERNELS:
        assert k in mapk, k
    flags = open(os.path.join(ROOT, "banet_amd", "csrc", "dev_flags.hpp")).read()
    assert "kDevAdjFp32Mfma = 1u << 26" in flags and "kDevAdjPixelPerWave = 1u << 27" in flags and "kDevAdjTexelPerWave = 1u << 28" in flags


def test_dispatch_mirror_on_known_shapes():
    assert ac.dispatch("dense", "bundle", 128, 128, True) == ("adj_basis6_kernel<8, false>", "adj_pixel2_kernel<1, true>", "adj_map2_kernel<3, 6>")
    assert ac.dispatch("dense", "bundle", 128, 128, False)[1] == "adj_pixel2_kernel<1, false>"
    assert ac.dispatch("dense", "bundle", 128, 128, False, ac.DEV_ADJ_PIXEL_PER_WAVE)[1] == "adj_pixel_kernel<2, 2>"
    assert ac.dispatch("dense", "bundle", 128, 128, False, ac.DEV_ADJ_FP32_MFMA)[0] == "adj_basis_kernel<8>"
    assert ac.dispatch("dense", "bundle", 128, 128, False, ac.DEV_ADJ_TEXEL_PER_WAVE)[2] == "adj_map_kernel<6>"
    assert ac.dispatch("dense", "bundle", 128, 128, False, N=1 << 24)[1] == "adj_pixel_kernel<2, 2>"
    assert ac.dispatch("sparse", "bundle", 128, 128, True) == ("adj_basis6_kernel<8, false>", "adj_pixel_kernel<2, 2, true>", "adj_map2_kernel<3, 6>")
    assert ac.dispatch("sparse", "bundle_camera", 131, 0, True) == (None, "adj_pixel_kernel<3, 1, true>", "adj_map_kernel<12>")
    assert ac.dispatch("sparse", "bundle", 130, 130, True)[1] is None            # refused before the launch (adj_supported)
    assert ac.dispatch("dense", "bundle", 3, 1) == ("adj_basis_kernel<1>", "adj_pixel_kernel<1, 1>", "adj_map_kernel<3>")
    assert ac.dispatch("dense", "bundle", 256, 256)[:2] == ("adj_basis_wide_kernel<16, 6>", "adj_pixel_kernel<4, 4>")


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
