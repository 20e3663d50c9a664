"""The inputs of the small-step tests (small_step_cases.py) are what they claim to be, the float32 yardstick the GPU module
(test_gpu_small_step.py) gates against, and the shapes banet_small_step_adjoint_f32 accepts -- all on the CPU.

The yardstick: dense_train._small_grads -- the torch graph the kernels replaced (LU with partial pivoting, twice: the forward
solve and the implicit-function one) -- evaluated in float32 against the same graph in float64, on the same float32-rounded inputs.
A float32 kernel cannot be asked for more than the float32 evaluation of the statement delivers; how much that is depends on the
conditioning (2e-7 at l2_base = 1000, 5e-2 on the last rung), so it is computed, never written down."""
import functools
import math

import pytest
import torch

import small_step_cases as ssc

VARIANT_ID = {"bundle_camera": 2, "bundle": 3}      # banet_hip.h: BANET_BUNDLE_CAMERA, BANET_BUNDLE


# ---- helpers shared with the GPU module --------------------------------------------------------------------------------------
def workspace_bytes(variant, B, N, C, K, pairs):
    from banet_amd import _capi as capi
    return int(capi.lib().banet_small_step_adjoint_workspace_bytes(VARIANT_ID[variant], B, N, C, K, pairs))


@functools.lru_cache(maxsize=None)
def largest_supported_K(pairs, B=3, C=32):
    """bundle: scan K upward from 1 until banet_small_step_adjoint_workspace_bytes refuses"""
    K = 1
    assert workspace_bytes("bundle", B, ssc.N_POINTS, C, K, pairs) > 0
    while workspace_bytes("bundle", B, ssc.N_POINTS, C, K + 1, pairs) > 0:
        K += 1
        assert K < 4096, "no upper limit found"
    return K


def resolve(grp):
    """a group with K = MAX_K -> the same group with the number"""
    variant, B, C, K, pairs = grp
    return (variant, B, C, largest_supported_K(pairs) if K == ssc.MAX_K else K, pairs)


def graph_grads(case, dtype):
    """dense_train._small_grads on a case -> the 15 outputs of ssc.OUTPUTS (gAtA symmetrised; dL/dWc = gW is not an output of
    the kernels), as float64 CPU tensors"""
    from banet_amd import dense_train
    c = lambda x: x.to(dtype)
    flat = [c(t) for wb in case["layers"] for t in wb]
    g = dense_train._small_grads(c(case["AtA"]), c(case["Atb"]), c(case["absres"]), c(case["R"]), c(case["T"]), c(case["Wc"]),
                                 c(case["gR"]), c(case["gT"]), c(case["gW"]), flat, case["N"], case["l2_base"], case["pairs"],
                                 case["camera"])
    out = [ssc.sym(g[0]), g[1], g[2], g[3], g[4]] + list(g[6:])
    return [t.double() for t in out]


@functools.lru_cache(maxsize=2)
def group_reference(grp, rung):
    """For one (group, rung): per seed (case, the float64 graph's outputs), and the yardstick e_ref32 = per output the error of
    the float32 graph against the float64 one, the maximum over the seeds; `finite32`: every float32 output was finite.
    Also e_solve32: the error of ONE float32 LU solve of the damped system, A^-1 dL/dsol, against gAtb of the float64 graph
    (which is that vector) -- the tighter yardstick for gAtb, without the graph's own forward solve in it."""
    variant, B, C, K, pairs = resolve(grp)
    per_seed, e32, finite32, e_solve = [], dict.fromkeys(ssc.OUTPUTS, 0.0), True, 0.0
    for seed in ssc.SEEDS:
        case = ssc.make_case(variant, B, C, K, pairs, rung, seed)
        want = graph_grads(case, torch.float64)
        got32 = graph_grads(case, torch.float32)
        finite32 = finite32 and all(bool(torch.isfinite(t).all()) for t in got32)
        for name, gv, wv in zip(ssc.OUTPUTS, got32, want):
            e32[name] = max(e32[name], ssc.rel_err(gv, wv))
        rhs = torch.matmul(case["A"], want[1].reshape(B, -1, 1))                       # dL/dsol = A (A^-1 dL/dsol), float64
        x32 = torch.linalg.solve(case["A"].float(), rhs.float())
        e_solve = max(e_solve, ssc.rel_err(x32.reshape(B, -1), want[1]))
        per_seed.append((case, want))
    return dict(per_seed=per_seed, e_ref32=e32, finite32=finite32, e_solve32=e_solve)


# ---- the tests -----------------------------------------------------------------------------------------------------------------
_ALL = ssc.all_groups()


@pytest.mark.parametrize("grp,rung", _ALL, ids=[ssc.group_id(g, r) for g, r in _ALL])
def test_ladder_conditions_and_the_float32_yardstick(grp, rung):
    """Every case the GPU module feeds the kernels: the float32-rounded damped matrix is positive definite (an unpivoted
    Cholesky / LDL^T is legitimate on it), its condition number is the rung's, the float32 graph is finite on it -- and the
    yardstick is a number (finite, not below the float32 rounding of one operation)."""
    ref = group_reference(grp, rung)
    lo, hi = ssc.cond_band(grp, rung)
    for case, _ in ref["per_seed"]:
        A32 = case["A"].float().double()
        A32 = ssc.sym(A32)
        ev = torch.linalg.eigvalsh(A32)
        assert float(ev.min()) > 0.0, (ssc.group_id(grp, rung), float(ev.min()))
        cond = ev[:, -1] / ev[:, 0]
        assert lo <= float(cond.min()) and float(cond.max()) <= hi, (ssc.group_id(grp, rung), float(cond.min()), float(cond.max()), lo, hi)
        assert bool(torch.isfinite(case["delta"]).all())
    assert ref["finite32"]
    for name in ssc.OUTPUTS:
        e = ref["e_ref32"][name]
        assert math.isfinite(e) and e < 1.0, (name, e)
    assert math.isfinite(ref["e_solve32"])
    print("%-40s e_ref32 gAtA %.1e gAtb %.1e gabs %.1e dR %.1e dT %.1e weights %.1e  solve32 %.1e" % (
        ssc.group_id(grp, rung), ref["e_ref32"]["gAtA"], ref["e_ref32"]["gAtb"], ref["e_ref32"]["gabs"], ref["e_ref32"]["dR"],
        ref["e_ref32"]["dT"], max(ref["e_ref32"][k] for k in ssc.WEIGHT_OUTPUTS), ref["e_solve32"]))


def test_cases_are_float32_numbers_and_reproducible():
    a = ssc.make_case("bundle", 2, 5, 8, 1, 3, 1)
    b = ssc.make_case("bundle", 2, 5, 8, 1, 3, 1)
    for k in ("AtA", "Atb", "absres", "R", "T", "Wc", "gR", "gT", "gW"):
        assert a[k].dtype == torch.float64 and torch.equal(a[k], a[k].float().double()) and torch.equal(a[k], b[k]), k
    for (w, bb) in a["layers"]:
        assert torch.equal(w, w.float().double()) and torch.equal(bb, bb.float().double())
    assert torch.equal(a["AtA"], a["AtA"].transpose(1, 2))
    res = torch.matmul(a["A"], a["delta"].unsqueeze(-1)).squeeze(-1) - a["Atb"]
    assert float(res.abs().max()) <= 1e-9 * float(a["Atb"].abs().max())
    c = ssc.make_case("bundle_camera", 2, 5, 0, 2, 1, 1)
    assert c["Wc"].shape == (2, 0, 1) and c["P"] == 12
    lam = ssc.lambda_of(c["absres"], c["layers"], c["N"], 2, c["l2_base"], True)
    d0, d1 = torch.diagonal(c["AtA"], dim1=1, dim2=2), torch.diagonal(c["A"], dim1=1, dim2=2)
    assert torch.allclose(d1, d0 + (d0 + 1e-5) * lam.unsqueeze(-1), rtol=1e-14)          # camera: every diagonal damped
    assert torch.equal(torch.diagonal(a["A"], dim1=1, dim2=2)[:, -1], torch.diagonal(a["AtA"], dim1=1, dim2=2)[:, -1])   # bundle: not the last


def test_small_step_support_limits():
    """banet_small_step_adjoint_workspace_bytes (host side: no device needed) is non-zero exactly for C in 1 .. 256, `bundle`
    with K >= 1, `bundle_camera` with K = 0; up to a largest P (the LDS of spd_solve_kernel) that does not depend on how P
    splits into poses and depth coefficients."""
    N = ssc.N_POINTS
    for C in range(0, 260):
        assert (workspace_bytes("bundle", 3, N, C, 8, 1) > 0) == (1 <= C <= 256), C
        assert (workspace_bytes("bundle_camera", 3, N, C, 0, 1) > 0) == (1 <= C <= 256), C
    for pairs in (1, 2, 4, 7):
        assert workspace_bytes("bundle", 3, N, 32, 0, pairs) == 0
        assert workspace_bytes("bundle", 3, N, 32, -1, pairs) == 0
        assert workspace_bytes("bundle_camera", 3, N, 32, 0, pairs) > 0
        assert workspace_bytes("bundle_camera", 3, N, 32, 1, pairs) == 0
    assert workspace_bytes("bundle", 0, N, 32, 8, 1) == 0 and workspace_bytes("bundle", 3, 0, 32, 8, 1) == 0
    assert workspace_bytes("bundle", 3, N, 32, 8, 0) == 0
    for v in (0, 1, 4):                                   # the legacy variants have no lambda MLP backward
        from banet_amd import _capi as capi
        assert capi.lib().banet_small_step_adjoint_workspace_bytes(v, 3, N, 32, 8, 1) == 0
    pmax = {}
    for pairs in (1, 2, 4, 7):
        K = largest_supported_K(pairs)
        for k in range(1, K + 1):                         # no hole below the limit (P = 31 / 32 switches the solver)
            assert workspace_bytes("bundle", 3, N, 32, k, pairs) > 0, (pairs, k)
        assert workspace_bytes("bundle", 3, N, 32, K + 1, pairs) == 0
        pmax[pairs] = 6 * pairs + K
    assert len(set(pmax.values())) == 1, pmax
    P = pmax[1]
    assert P >= 134                                       # (the shapes the trainer runs: K = 128)
    for B, C in ((1, 1), (64, 256)):                      # the limit is the solve's, not the batch's or the MLP's
        assert workspace_bytes("bundle", B, N, C, P - 6, 1) > 0 and workspace_bytes("bundle", B, N, C, P - 5, 1) == 0
    # camera windows: the same largest P where 6 divides into it
    pc = P // 6
    assert workspace_bytes("bundle_camera", 3, N, 32, 0, pc) > 0 and workspace_bytes("bundle_camera", 3, N, 32, 0, pc + 1) == 0
