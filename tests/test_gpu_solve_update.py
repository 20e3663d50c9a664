"""The forward solve-and-update kernel on HIP (`-m gpu`): banet_ba_solve_update[_ws]_f32 and banet_spd_solve_f32 (csrc/solve.hip)
on synthetic normal equations (solve_cases.py) through bare banet_level_t structs -- one launch of one workgroup per window per
case, where the other modules reach this kernel only through assembled scenes at a few P.  Against the float64 statement of
lambda, damping, solve and SE(3) / W update on the same float32-rounded inputs:
  * every solver of the kernel: the one-thread QR (legacy, P = 6), the pivoted LU in registers (6 <= P <= 31, also with row orders
    that are not the identity), Jacobi-PCG + Schur step (32 <= P, all four residues of the row tail), the blocked LDL^T as the
    fallback (a family on which the CG emulation cannot converge) and on its own (DEV_SOLVE_LDLT_ONLY), the LDL^T on the matrix
    in the caller's workspace (BIG) on both sides of the LDS limit at C = 32 and C = 128 and up to P = 304;
  * the gate is relative to what float32 delivers on the case (test_solve_cases_cpu.py): e_hip <= max(1e-4, 4 e_ref32) per
    coefficient group, e_ref32 the error of one textbook float32 LU (legacy: QR) solve on the CPU (solve_cases.lu32);
  * the update arithmetic per pose slot on planted updates (theta below the clamp, 1e-3, 1, just under pi), a zero right-hand
    side, the isolation of a window from the others of its launch (NaN neighbours included), refusals before any launch, bit
    reproducibility.

What this module measured on an MI355X is kept in profiles/solve_update_ladder.txt."""
import ctypes

import numpy as np
import pytest
import torch

import solve_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL, MARGIN = 1e-4, 4.0              # the project's solve tolerance; "as accurate as the reference's algorithm in float32"
TOL_LAMBDA, TOL_UPDATE = 1e-5, 2e-6
SMALL_ANGLE = 0.05                    # rotation updates below this get _v_allowance on T'
ITERS0 = 3                            # the iteration counters start here: the call must add exactly 1
ERR_WORKSPACE, ERR_UNSUPPORTED = -2, -3      # banet_hip.h


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from banet_amd import _capi
    _capi.lib()


class _Bare:
    """what ops.ba_solve_update reads of a LevelProblem"""

    def __init__(self, c, C):
        self.c, self.C, self.device = c, C, torch.device(DEV)


_MLPS = {}


def _mlp(case):
    """device copies of the lambda layers (make_case draws them from the channel count alone: one upload per C)"""
    from banet_amd import ops
    if case["variant"] == "legacy_fixed":
        return None
    C = case["C"]
    if C not in _MLPS:
        _MLPS[C] = (ops.MlpWeights([(torch.tensor(w).float(), torch.tensor(b).float()) for w, b in case["layers"]], torch.device(DEV)),
                    case["layers"][0][0].copy())
    assert np.array_equal(_MLPS[C][1], case["layers"][0][0])
    return _MLPS[C][0]


def _dev(a, sel):
    return torch.tensor(np.ascontiguousarray(a[sel]), dtype=torch.float32, device=DEV)


def _inputs(case, sel, AtA=None, Atb=None):
    AtA = case["AtA"] if AtA is None else AtA
    Atb = case["Atb"] if Atb is None else Atb
    return _dev(AtA, sel), _dev(Atb, sel), _dev(case["absres"], sel), _dev(case["nvalid"], sel)


def _state(case, sel):
    from banet_amd import ops
    st = ops.LmState(_dev(case["R"], sel), _dev(case["T"], sel), _dev(case["Wc"], sel) if case["K"] else None, P=case["P"],
                     pairs=case["pairs"])
    st.iters.add_(ITERS0)
    st.delta.fill_(float("nan"))
    return st


def _read(st, B, pairs, K):
    torch.cuda.synchronize()
    return dict(delta=st.delta.cpu(), R=st.R.cpu().reshape(B, pairs, 3, 3), T=st.T.cpu().reshape(B, pairs, 3, 1),
                Wc=st.Wc.cpu() if K else torch.zeros(B, 0, 1), iters=st.iters.cpu(), ratio=st.ratio.cpu(), lam=st.lambda_out.cpu())


def _run(case, flags=0, sel=None, AtA=None, Atb=None):
    """one banet_ba_solve_update[_ws]_f32 call on the windows `sel` of a case (all of them by default), from the case's state"""
    from banet_amd import ops
    sel = list(range(case["B"])) if sel is None else list(sel)
    lv = _Bare(sc.bare_level(case["variant"], len(sel), case["N"], case["C"], case["K"], case["pairs"], flags), case["C"])
    st = _state(case, sel)
    ops.ba_solve_update(lv, _mlp(case), case["l2_base"], *_inputs(case, sel, AtA, Atb), st)
    return _read(st, len(sel), case["pairs"], case["K"])


def _f64(t):
    return t.double().numpy()


def _check_solve(case, out, e_hip, lam_err):
    """lambda against float64; delta against the float64 solution AT THE LAMBDA READ BACK (a rounding difference of lambda is not
    charged to the solver) -> accumulates the group errors and, under "backward", the backward error on that float64 system;
    returns finiteness"""
    lam64 = sc.lambda64(case)
    lam = _f64(out["lam"])
    lam_err[0] = max(lam_err[0], float(np.abs(lam / lam64 - 1.0).max()))
    finite = bool(torch.isfinite(out["delta"]).all())
    sc.max_merge(e_hip, sc.group_errors(case, _f64(out["delta"]), sc.solve64(case, lam)))
    if finite:
        sc.max_merge(e_hip, {"backward": sc.backward_error(sc.damped64(case, lam), _f64(out["delta"]), case["Atb"])})
    return finite


def _two_runs(spec):
    family, variant, C, P, pairs, rung = sc.resolve(spec)
    return family == "clustered" or (family == "ladder" and P >= 32)


def _fmt(e, e32):
    return " ".join("%s %.1e/%.1e" % (k, e[k], e32[k]) for k in e32)


_SOLVE = sc.all_specs(sc.SOLVE_FAMILIES)


@pytest.mark.parametrize("spec", _SOLVE, ids=[sc.spec_id(s) for s in _SOLVE])
def test_solve_against_float64(spec):
    """families a .. e, five seeds of three windows each: delta finite and e_hip <= max(1e-4, 4 e_ref32) in every coefficient group
    (pose, depth, the undamped last coefficient; each on its own max-norm scale, the maximum over seeds), lambda_out within 1e-5
    of float64; the backward error is printed beside them.  The ladder at P >= 32 and the clustered family run twice -- as in production and with DEV_SOLVE_LDLT_ONLY --
    and both results are held to the gate; the clustered family's two results are bit-identical (its CG cannot converge, so the
    production run took the fallback), the ladder's largest difference is printed.

    Rung 5 (cond ~5e5 .. 5e6, e_ref32 1e-2 .. 1.3e-1: a gate of 4 e_ref32 would accept anything) is held to its BACKWARD error
    instead, ||A x - b|| / (||A|| ||x|| + ||b||) <= max(n 2^-24, 4 x the float32 LU's own) on both runs; its forward errors are
    printed only, except at P = 7, where e_ref32 is below 1e-2 and the forward gate applies as everywhere else.

    The production run of ladder-bundle-C32-Plds32-pairs1-rung5 (P = 180) is what gave pcg_schur_solve its lower limit on the
    Schur complement: 1.9e-1 against e_ref32 4.0e-2 while CG + Schur kept a complement of 3e-6 a_PP, 4.0e-2 (the LDL^T's) since
    it hands such systems over."""
    from banet_amd import _capi as capi
    e32 = dict(sc.yardstick(spec), backward=sc.yardstick_backward(spec))
    e_hip, e_ldlt, lam_err, finite, diff, same = {}, {}, [0.0], True, 0.0, True
    for seed in sc.SEEDS:
        case = sc.make(spec, seed)
        out = _run(case)
        finite = _check_solve(case, out, e_hip, lam_err) and finite
        assert torch.equal(out["iters"], torch.full((case["B"],), ITERS0 + 1, dtype=torch.int32))
        if _two_runs(spec) or spec[0] == "camera" and case["P"] >= 32:
            alt = _run(case, flags=capi.DEV_SOLVE_LDLT_ONLY)
            finite = _check_solve(case, alt, e_ldlt, lam_err) and finite
            diff = max(diff, float((out["delta"] - alt["delta"]).abs().max() / alt["delta"].abs().max()))
            same = same and torch.equal(out["delta"], alt["delta"])
    print("\nsolve_update %-46s P %3d  lambda %.3e (err %.0e)  e_hip/e_ref32: %s%s" % (
        sc.spec_id(spec), case["P"], float(out["lam"][0]), lam_err[0], _fmt(e_hip, e32),
        "  | LDL^T only: %s | default vs LDL^T %.1e%s" % (_fmt(e_ldlt, e32), diff, " (same bits)" if same else "") if e_ldlt else ""))
    assert finite
    assert lam_err[0] <= TOL_LAMBDA
    for e in (e_hip, e_ldlt):
        for k, v in e.items():
            if k == "backward":
                assert sc.forward_gated(spec) or v <= sc.residual_gate(case["P"], e32[k]), (k, v, e32[k])
            elif max(e32[g] for g in e32 if g != "backward") <= sc.E_REF32_CAP:
                assert v <= max(TOL, MARGIN * e32[k]), (k, v, e32[k])
            else:
                assert not sc.forward_gated(spec)
    if spec[0] == "clustered":
        assert same, "the clustered family must take the LDL^T fallback"


def test_a_batch_of_64_windows():
    """P = 134 (PCG, matrix in LDS), 64 windows in one launch: the same gate, every window against its own float64 solution"""
    spec = ("ladder", "bundle", 32, 134, 1, 1)
    case = sc.make(spec, 0, 64)
    lam = sc.lambda64(case).astype(np.float32).astype(np.float64)
    x32 = sc.solve32(case, lam)
    e32 = dict(sc.group_errors(case, x32, sc.solve64(case, lam)), backward=sc.backward_error(sc.damped64(case, lam), x32, case["Atb"]))
    e_hip, lam_err = {}, [0.0]
    out = _run(case)
    assert _check_solve(case, out, e_hip, lam_err)
    want = sc.solve64(case, _f64(out["lam"]))
    per_window = max(float(np.abs(_f64(out["delta"])[b] - want[b]).max() / np.abs(want[b]).max()) for b in (0, 31, 63))
    print("\nsolve_update B = 64, P = 134: e_hip/e_ref32 %s; windows 0, 31, 63 on their own scale %.1e" % (_fmt(e_hip, e32), per_window))
    assert lam_err[0] <= TOL_LAMBDA and per_window <= TOL
    for k, v in e_hip.items():
        assert v <= max(TOL, MARGIN * e32[k]), (k, v, e32[k])           # (the backward error too: far below 1e-4 on rung 1)


# ---- the update --------------------------------------------------------------------------------------------------------------
def _cross(a, b):
    return np.cross(a, b)


def _v_allowance(case, delta):
    """What the float32 evaluation of V(w) = I + (1 - cos th) / th^2 K + (th - sin th) / th^3 K^2 (bundlenet.py:39-46, the
    kernel's statement) may add to the error of T' beyond a few ulps of O(1) products, per pose slot: 1 - cos th and th - sin th
    cancel, so an error of 2^-23 (2 ulp of a cosine just below 1; of th for the sine) in the numerators is 2^-23 / th^2 in the
    coefficients -- at most the coefficients themselves, 1/2 and 1/6 -- times |w x t| and |w x (w x t)|.  1.2e-4 |t| at
    th = 1e-3 (measured: 2.5e-5 of T's max-norm).  Only for slots with th < 0.05: from there on the term is below the 2e-6 gate
    (2^-23 / th^2 x th |t| = 2.4e-6 |t| at th = 0.05) and the plain gate holds alone.  Zero for LEGACY_FIXED, which has no V."""
    B, pairs = case["B"], case["pairs"]
    sol = np.asarray(delta, np.float64)[:, :6 * pairs].reshape(B, pairs, 6)
    w, t = sol[..., :3], sol[..., 3:]
    if case["variant"] == "legacy_fixed":
        return np.zeros((B, pairs))
    th2 = np.maximum((w * w).sum(-1), 1e-300)
    wt = _cross(w, t)
    allow = np.minimum(0.5, 2.0 ** -23 / th2) * np.abs(wt).max(-1) + np.minimum(1.0 / 6.0, 2.0 ** -23 / th2) * np.abs(_cross(w, wt)).max(-1)
    return np.where(th2 < SMALL_ANGLE ** 2, allow, 0.0)


def _check_update(case, out):
    """R, T, Wc after the call against the float64 update of the starting state by the delta THE GPU WROTE: within 2e-6 of each
    tensor's max-norm in every pose slot (T: plus _v_allowance of the slot); iters + 1; ratio as documented"""
    delta = _f64(out["delta"])
    Rn, Tn, Wn = sc.update64(case, delta)
    allow = _v_allowance(case, delta)
    eR = np.abs(_f64(out["R"]) - Rn).max(axis=(2, 3))
    eT = np.abs(_f64(out["T"]) - Tn).max(axis=(2, 3))
    assert np.all(eR <= TOL_UPDATE * np.abs(Rn).max()), (eR.max(), np.abs(Rn).max())
    assert np.all(eT <= TOL_UPDATE * np.abs(Tn).max() + allow), ((eT - allow).max(), np.abs(Tn).max())
    if case["K"]:
        assert np.abs(_f64(out["Wc"]) - Wn).max() <= TOL_UPDATE * np.abs(Wn).max()
    assert torch.equal(out["iters"], torch.full((case["B"],), ITERS0 + 1, dtype=torch.int32))
    np.testing.assert_allclose(_f64(out["ratio"]), sc.ratio64(case), rtol=3e-7)
    return float(eR.max() / np.abs(Rn).max()), float(eT.max() / np.abs(Tn).max()), float(allow.max() / np.abs(Tn).max())


@pytest.mark.parametrize("spec", sc.PLANTED, ids=[sc.spec_id(s) for s in sc.PLANTED])
def test_update_of_planted_solutions(spec):
    """family f: every pose slot b pairs + p of every window has its own R, T and its own planted update; the solve returns the
    planted x* (1e-4 of its max-norm per group) and the state moves as the float64 update says"""
    worst = (0.0, 0.0, 0.0)
    for seed in sc.SEEDS:
        case = sc.make(spec, seed)
        out = _run(case)
        assert torch.isfinite(out["delta"]).all()
        for k, v in sc.group_errors(case, _f64(out["delta"]), case["planted"]).items():
            assert v <= TOL, (k, v)
        worst = tuple(max(a, b) for a, b in zip(worst, _check_update(case, out)))
    print("\nsolve_update %-46s update errors on the tensors' max-norm: R %.1e T %.1e (largest V(w) allowance used %.1e)" % (
        (sc.spec_id(spec),) + worst))


_ONE_EACH = [("ladder", "bundle", 32, 7, 1, 1), ("ladder", "bundle", 32, 134, 1, 1), ("ladder", "bundle", 32, 304, 8, 1),
             ("camera", "bundle_camera", 32, 12, 2, 1), ("camera", "bundle_camera", 32, 48, 8, 1), ("legacy", "legacy_lm", 3, 6, 1, 1),
             ("legacy", "legacy_fixed", 8, 6, 1, 1), ("pivot", "bundle", 32, 31, 1, 1), ("clustered", "bundle", 32, 70, 1, 1)]
assert all(s_ in sc.all_specs() for s_ in _ONE_EACH)


@pytest.mark.parametrize("spec", _ONE_EACH, ids=[sc.spec_id(s) for s in _ONE_EACH])
def test_update_on_one_case_of_each_family(spec):
    case = sc.make(spec, 0)
    _check_update(case, _run(case))


_ZERO = [sc.LEGACY[0], sc.LEGACY[3], ("camera", "bundle_camera", 32, 12, 2, 1)] + \
        [("ladder", "bundle", 32, P, 1, 1) for P in (19, 38, 134, 262)]


@pytest.mark.parametrize("spec", _ZERO, ids=[sc.spec_id(s) for s in _ZERO])
def test_zero_right_hand_side_leaves_the_state_unchanged(spec):
    case = sc.make(spec, 0)
    out = _run(case, Atb=np.zeros_like(case["Atb"]))
    sel = list(range(case["B"]))
    assert torch.equal(out["delta"], torch.zeros_like(out["delta"]))
    assert torch.equal(out["R"], _dev(case["R"], sel).cpu()) and torch.equal(out["T"], _dev(case["T"], sel).cpu())
    if case["K"]:
        assert torch.equal(out["Wc"], _dev(case["Wc"], sel).cpu())
    assert torch.equal(out["iters"], torch.full((case["B"],), ITERS0 + 1, dtype=torch.int32))


# ---- one workgroup per window ---------------------------------------------------------------------------------------------------
_KEYS = ("delta", "R", "T", "Wc", "lam", "ratio", "iters")


@pytest.mark.parametrize("P", [19, 70, 262])
def test_a_window_does_not_depend_on_its_neighbours(P):
    """5 windows in one launch, a NaN in window 2's Atb and one in window 4's AtA: windows 0, 1, 3 come out bit for bit as in a
    launch of these three and as alone; the poisoned windows give a non-finite delta, never a silently wrong finite one"""
    case = sc.make(("ladder", "bundle", 32, P, 1, 1), 0, 5)
    AtA, Atb = case["AtA"].copy(), case["Atb"].copy()
    Atb[2, P // 3] = np.nan
    AtA[4, P // 2, 3] = AtA[4, 3, P // 2] = np.nan
    full = _run(case, AtA=AtA, Atb=Atb)
    three = _run(case, sel=[0, 1, 3])
    for i, b in enumerate((0, 1, 3)):
        alone = _run(case, sel=[b])
        for k in _KEYS:
            assert torch.equal(full[k][b], three[k][i]) and torch.equal(full[k][b], alone[k][0]), (b, k)
        assert torch.isfinite(full["delta"][b]).all()
    for b in (2, 4):
        assert not torch.isfinite(full["delta"][b]).all(), b


_REPRO = [("legacy", "legacy_lm", 8, 6, 1, 1), ("legacy", "legacy_fixed", 128, 6, 1, 1),                          # QR
          ("ladder", "bundle", 32, 19, 1, 1), ("pivot", "bundle", 32, 31, 1, 2),                                      # LU
          ("ladder", "bundle", 32, 65, 1, 0), ("camera", "bundle_camera", 32, 48, 8, 1),                              # PCG
          ("clustered", "bundle", 32, 38, 1, 1), ("clustered", "bundle", 32, 134, 1, 1),                              # fallback
          ("ladder", "bundle", 32, 262, 1, 1), ("ladder", "bundle", 32, sc.lds(32, 1), 1, 3)]                         # BIG
assert all(s_ in sc.all_specs() for s_ in _REPRO)


@pytest.mark.parametrize("spec", _REPRO, ids=[sc.spec_id(s) for s in _REPRO])
def test_solve_update_is_bit_reproducible(spec):
    """two cases per path (QR, LU, PCG, fallback, BIG), twice on fresh state: equal bits in every output"""
    case = sc.make(spec, 1)
    a, b = _run(case), _run(case)
    assert torch.isfinite(a["delta"]).all()
    for k in _KEYS:
        assert torch.equal(a[k], b[k]), k


# ---- refusals ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [32, 128])
def test_refusals_are_decided_before_any_launch(C):
    """above the LDS limit: banet_ba_solve_update_f32 (no workspace) -> BANET_ERR_UNSUPPORTED; the _ws_ entry with a too small or
    a misaligned workspace -> BANET_ERR_WORKSPACE; the state is untouched in all three"""
    from banet_amd import _capi as capi
    L = capi.lib()
    case = sc.make(("ladder", "bundle", C, sc.lds(C, 1), 1, 1), 0)
    sel = list(range(case["B"]))
    lv = sc.bare_level(case["variant"], case["B"], case["N"], C, case["K"], 1)
    need = int(L.banet_ba_solve_update_workspace_bytes(ctypes.byref(lv)))
    assert need > 0
    ins = _inputs(case, sel)
    st = _state(case, sel)
    before = _read(st, case["B"], 1, case["K"])
    mlp = _mlp(case)
    args = [ctypes.byref(lv), ctypes.byref(mlp.c), float(case["l2_base"])] + [capi.ptr(t) for t in ins] + [ctypes.byref(st.c)]
    ws = capi.workspace(need + 512, torch.device(DEV))
    assert L.banet_ba_solve_update_f32(*args, capi.stream()) == ERR_UNSUPPORTED
    assert L.banet_ba_solve_update_ws_f32(*args, ctypes.c_void_p(ws.data_ptr()), need - 1, capi.stream()) == ERR_WORKSPACE
    assert L.banet_ba_solve_update_ws_f32(*args, ctypes.c_void_p(ws.data_ptr() + 128), need + 256, capi.stream()) == ERR_WORKSPACE
    assert L.banet_ba_solve_update_ws_f32(*args, None, need, capi.stream()) == ERR_WORKSPACE
    after = _read(st, case["B"], 1, case["K"])
    for k in _KEYS:
        assert torch.equal(before[k], after[k]) or (k == "delta" and bool(torch.isnan(after[k]).all())), k
    assert L.banet_ba_solve_update_ws_f32(*args, ctypes.c_void_p(ws.data_ptr()), need, capi.stream()) == 0
    assert torch.isfinite(_read(st, case["B"], 1, case["K"])["delta"]).all()


# ---- banet_spd_solve_f32 -----------------------------------------------------------------------------------------------------------
def _spd_rc(P, B=1):
    """return code of banet_spd_solve_f32 at this P on an identity system (a refusal is decided before the launch)"""
    from banet_amd import _capi as capi
    A = torch.eye(P, device=DEV).repeat(B, 1, 1).contiguous()
    b = torch.ones(B, P, 1, device=DEV)
    x = torch.full((B, P, 1), 7.0, device=DEV)
    rc = capi.lib().banet_spd_solve_f32(capi.ptr(A), capi.ptr(b), capi.ptr(x), B, P, capi.stream())
    torch.cuda.synchronize()
    return rc, x.cpu()


_SPD_MAX = []


def _spd_largest_p():
    if not _SPD_MAX:
        P = 134
        assert _spd_rc(P)[0] == 0
        while _spd_rc(P + 1)[0] == 0:
            P += 1
            assert P < sc.P_MAX
        _SPD_MAX.append(P)
    return _SPD_MAX[0]


def test_spd_solve_support_limits():
    for P in (31, sc.P_MAX):
        rc, x = _spd_rc(P)
        assert rc == ERR_UNSUPPORTED and bool((x == 7.0).all())
    rc, x = _spd_rc(32, B=2)
    assert rc == 0 and torch.equal(x, torch.ones_like(x))
    assert 150 <= _spd_largest_p() <= 200


@pytest.mark.parametrize("P", sc.SPD_P + ("max",))
def test_spd_solve_against_float64(P):
    """the ladder's damped matrices (symmetric positive definite) and right-hand sides, rungs 0 .. 5, five seeds of three systems:
    x finite and e_hip <= max(1e-4, 4 e_ref32) on x's max-norm, e_ref32 one float32 LU solve (sc.lu32) of the same float32 matrix;
    where e_ref32 is above 1e-2 (rung 5) the backward error instead, <= max(n 2^-24, 4 x the float32 LU's own)"""
    from banet_amd import dense_train
    P = _spd_largest_p() if P == "max" else P
    for rung in sc.ALL_RUNGS:
        e_hip = e32 = r_hip = r32 = 0.0
        for seed in sc.SEEDS:
            case = sc.make(("ladder", "bundle", 32, P, 1, rung), seed)
            A = sc.damped64(case, sc.lambda64(case)).astype(np.float32)
            b = case["Atb"].astype(np.float32)[:, :, None]
            want = np.linalg.solve(A.astype(np.float64), b.astype(np.float64))
            x32 = sc.lu32(A, b)
            got = dense_train.spd_solve(torch.tensor(A, device=DEV), torch.tensor(b, device=DEV))
            torch.cuda.synchronize()
            assert torch.isfinite(got).all()
            e_hip = max(e_hip, float(np.abs(_f64(got.cpu()) - want).max() / np.abs(want).max()))
            e32 = max(e32, float(np.abs(x32 - want).max() / np.abs(want).max()))
            r_hip, r32 = max(r_hip, sc.backward_error(A, _f64(got.cpu()), b)), max(r32, sc.backward_error(A, x32, b))
        print("\nspd_solve    P %3d rung %d  e_hip/e_ref32 %.1e/%.1e  backward %.1e/%.1e" % (P, rung, e_hip, e32, r_hip, r32))
        if e32 <= sc.E_REF32_CAP:
            assert e_hip <= max(TOL, MARGIN * e32), (rung, e_hip, e32)
        else:
            assert rung == 5 and r_hip <= sc.residual_gate(P, r32), (rung, r_hip, r32)


def test_spd_solve_is_bit_reproducible():
    from banet_amd import dense_train
    for P, rung in ((49, 3), (134, 5)):
        case = sc.make(("ladder", "bundle", 32, P, 1, rung), 0)
        A = torch.tensor(sc.damped64(case, sc.lambda64(case)), dtype=torch.float32, device=DEV)
        b = torch.tensor(case["Atb"][:, :, None], dtype=torch.float32, device=DEV)
        x, y = dense_train.spd_solve(A, b), dense_train.spd_solve(A, b)
        assert torch.isfinite(x).all() and torch.equal(x, y)
