"""The pose prior (include/banet_hip.h (5f); csrc/pose_prior.hip) without a GPU: the float64 twin of tests/pose_prior_ref.py against
finite differences, the float32 evaluation of the same formulas against the twin (the GPU test's gate), the host plan compiled
with g++, and the entries' argument validation through the library (every call here is refused before a launch, or launches
nothing)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import pose_prior_ref as ppr
import ws_contract as wsc

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
os.environ.setdefault("BANET_NUM_CUS", "256")
OK, ERR_INVALID_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED, ERR_LAUNCH = 0, -1, -2, -3, -4
SYMBOLS = ("banet_pose_prior_apply_f32", "banet_lm_level_pose_prior_workspace_bytes", "banet_lm_level_pose_prior_f32",
           "banet_lm_solve_pose_prior_workspace_bytes", "banet_lm_solve_pose_prior_f32")
ALL_ANGLES = ppr.ANGLES + ppr.THRESHOLD_ANGLES


@pytest.fixture(scope="module")
def capi():
    from banet_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _capi


# ---- the twin against finite differences ---------------------------------------------------------------------------------------------
def pose_at(angle, seed):
    rng = np.random.RandomState(seed)
    R0 = ppr.random_rotation(rng, 0.7)
    R = ppr.random_rotation(rng, angle) @ R0
    T0 = rng.standard_normal(3)
    return R, T0 + rng.standard_normal(3) * 0.5, R0, T0


@pytest.mark.parametrize("angle", ALL_ANGLES)
def test_log_inverts_exp_and_jr_is_the_derivative_of_the_log(angle):
    """Jr = d Log(Exp(delta) E) / d delta at 0 by central differences (h = 1e-6: truncation h^2, rounding 1e-16 / h -- 1e-8 is generous
    for both up to |phi| = 3, where the log's own conditioning is 1 / sin(3) = 7)"""
    R, T, R0, T0 = pose_at(angle, 11)
    r, Jinv = ppr.log_se3(R, T, R0, T0)
    assert abs(np.linalg.norm(r[:3]) - angle) < 1e-9
    Re, te = ppr.exp_se3(r)
    assert np.abs(Re - R @ R0.T).max() < 1e-12 and np.abs(te - (T - R @ R0.T @ T0)).max() < 1e-12
    Jr = ppr.jr_block(r, Jinv)
    h, fd = 1e-6, np.zeros((6, 6))
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        plus, minus = ppr.compose(d, R, T), ppr.compose(-d, R, T)
        fd[:, k] = (ppr.log_se3(plus[0], plus[1], R0, T0)[0] - ppr.log_se3(minus[0], minus[1], R0, T0)[0]) / (2 * h)
    err = np.abs(Jr - fd).max()
    print("|phi| %.4g: |Jr - central differences| %.2e" % (angle, err))
    assert err < 1e-8
    assert np.abs(Jr[:3, 3:]).max() == 0.0                 # the rotation part of the log does not see the translation


def test_jr_is_the_identity_at_zero_exactly_in_both_precisions():
    for dt in (np.float64, np.float32):
        T0 = np.array([0.3, -0.2, 0.1], dt)
        eye = np.eye(3, dtype=dt)
        r, Jinv = ppr.log_se3(eye, T0, eye, T0, dt)       # Re = I exactly
        assert r.dtype == dt and (r == 0).all()
        assert np.array_equal(ppr.jr_block(r, Jinv, dt), np.eye(6, dtype=dt))
        r, Jinv = ppr.log_se3(eye, T0 + dt(0.5), eye, T0, dt)   # phi = 0, rho != 0: J^-1 = I, the lower left block -1/2 rho^
        Jr = ppr.jr_block(r, Jinv, dt)
        assert np.array_equal(Jr[:3, :3], eye) and np.array_equal(Jr[3:, 3:], eye)
        assert np.array_equal(Jr[3:, :3], -dt(0.5) * ppr.hat(r[3:]))


@pytest.mark.parametrize("pairs", [1, 2, 7])
def test_the_term_is_the_gradient_and_the_gauss_newton_hessian_of_the_cost(pairs):
    """-v = -scale Jr^T Lambda r is minus the gradient of scale 1/2 r^T Lambda r with respect to the left perturbation of every pose
    (central differences); H = scale Jr^T Lambda Jr is symmetric positive semi-definite with Lambda"""
    c = ppr.apply_cases(pairs, 40 + pairs, B=2)
    f = lambda x: x.astype(np.float64)

    def polar(M):                                           # the cases' rotations are rounded to float32: 3e-8 from orthonormal, which the
        u, _, vt = np.linalg.svd(M)                         # log amplifies by 1 / sin(3) and more; Jr is the derivative on SO(3) itself
        return u @ vt
    scale, h = 0.37, 1e-6
    for w in range(2):
        R, T, R0, T0, Lam = (f(c[k][w]) for k in ("R", "T", "R0", "T0", "Lambda"))
        R, R0 = polar(R), polar(R0)
        t = ppr.window_term(R, T, R0, T0, Lam, scale)
        grad = np.zeros(6 * pairs)
        for i in range(pairs):
            for k in range(6):
                vals = []
                for sgn in (1.0, -1.0):
                    d = np.zeros(6)
                    d[k] = sgn * h
                    Rp, Tp = R.copy(), T.copy()
                    Rp[i], Tp[i] = ppr.compose(d, R[i], T[i])
                    vals.append(ppr.window_term(Rp, Tp, R0, T0, Lam, scale)["cost"])
                grad[6 * i + k] = (vals[0] - vals[1]) / (2 * h)
        err = np.abs(grad - t["v"]).max() / np.abs(t["v"]).max()
        print("pairs %d window %d: |gradient - central differences| / max |gradient| %.2e" % (pairs, w, err))
        assert err < 1e-7
        assert np.abs(t["H"] - t["H"].T).max() <= 1e-12 * np.abs(t["H"]).max()
        assert np.linalg.eigvalsh(0.5 * (t["H"] + t["H"].T)).min() > -1e-10 * np.abs(t["H"]).max()
        # one Gauss-Newton step on the term alone reduces it
        step = np.linalg.solve(t["H"] + 1e-9 * np.eye(6 * pairs), -t["v"])
        Rn, Tn = R.copy(), T.copy()
        for i in range(pairs):
            Rn[i], Tn[i] = ppr.compose(step[6 * i:6 * i + 6], R[i], T[i])
        assert ppr.window_term(Rn, Tn, R0, T0, Lam, scale)["cost"] < 0.5 * t["cost"]


def test_float32_arithmetic_is_this_far_from_the_twin():
    """the GPU gate's base: the formulas in float32 numpy against float64 on the cases of test_gpu_pose_prior.py's apply test"""
    worst_A = worst_b = 0.0
    seen = set()
    for pairs, K in ppr.APPLY_SHAPES:
        c = ppr.apply_problem(pairs, K)
        seen |= set(c["angles"])
        A, b, _, _ = ppr.apply(c["AtA"], c["Atb"], c["R"], c["T"], c["R0"], c["T0"], c["Lambda"], ppr.APPLY_SCALE, np.float32)
        assert A.dtype == np.float32 and b.dtype == np.float32
        eA, eb = ppr.apply_errors(A, b, c)
        print("pairs %d K %d: float32 against the twin, AtA %.3e Atb %.3e" % (pairs, K, eA, eb))
        worst_A, worst_b = max(worst_A, eA), max(worst_b, eb)
    assert seen == set(ALL_ANGLES)                          # every angle, both sides of every threshold
    assert 0.5 * ppr.F32_ERR <= max(worst_A, worst_b) <= ppr.F32_ERR, (worst_A, worst_b)
    assert ppr.APPLY_GATE == 4 * ppr.F32_ERR


def test_outputs_are_finite_past_the_supported_range():
    rng = np.random.RandomState(5)
    for angle in (3.1, 3.14159, np.pi):
        for dt in (np.float64, np.float32):
            R0 = ppr.random_rotation(rng, 0.3)
            R = ppr.random_rotation(rng, angle) @ R0
            t = ppr.window_term(R[None].astype(dt), np.ones((1, 3), dt), R0[None].astype(dt), np.zeros((1, 3), dt), np.eye(6, dtype=dt), 1.0, dt)
            assert np.isfinite(t["H"]).all() and np.isfinite(t["v"]).all()


# ---- linkage and layout -------------------------------------------------------------------------------------------------------------
def test_the_library_exports_the_symbols_and_capi_binds_them(capi):
    L = ctypes.CDLL(capi.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "banet_hip.h")).read()
    for name in SYMBOLS:
        assert hasattr(L, name), name
        assert name in capi.EXPORTS
        assert re.search(r"\b%s\(" % name, header), name
    assert capi.lib().banet_version() == 150              # unchanged: the entries are detected by their symbols
    assert "(5f)" in header


def test_struct_layout_matches_the_header(capi, tmp_path):
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "banet_hip.h"\n'
                    'int main(){printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(banet_pose_prior_t), offsetof(banet_pose_prior_t, R0), '
                    'offsetof(banet_pose_prior_t, T0), offsetof(banet_pose_prior_t, Lambda), offsetof(banet_pose_prior_t, scale), '
                    'offsetof(banet_pose_prior_t, reserved_));return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    P = capi.PosePrior
    assert got == [ctypes.sizeof(P), P.R0.offset, P.T0.offset, P.Lambda.offset, P.scale.offset, P.reserved_.offset]
    assert [n for n, _ in P._fields_] == ["R0", "T0", "Lambda", "scale", "reserved_"]


# ---- argument validation ------------------------------------------------------------------------------------------------------------
class Host:
    """fake host pointers (compared with NULL, never dereferenced), a level, a state, an MLP and an aligned fake workspace address"""

    def __init__(self, capi, B=2, H=24, W=32, K=16, pairs=1, variant=None, scale=0.5):
        self.capi, self.L = capi, capi.lib()
        self.host = (ctypes.c_float * 64)()
        self.p = ctypes.cast(self.host, ctypes.c_void_p).value
        self.arena = (ctypes.c_char * 512)()
        self.base = (ctypes.addressof(self.arena) + 255) & ~255
        self.lv = wsc._abi_level(capi, self.p, B, H, W, K, pairs, C=16, variant=variant)
        self.pp = capi.PosePrior()
        self.pp.R0 = self.pp.T0 = self.pp.Lambda = self.p
        self.pp.scale = scale
        self.pr = capi.Prior()
        self.pr.Lambda, self.pr.scale = self.p, 0.5
        self.st = capi.State()
        self.st.R = self.st.T = self.st.Wc = self.st.iters = self.st.ratio = self.st.lambda_out = self.st.delta = self.p
        self.mlp = capi.Mlp()
        for i in range(5):
            self.mlp.w[i] = self.mlp.b[i] = self.p

    def ref(self, pp):
        return ctypes.byref(self.pp) if pp == "pp" else pp

    def q_level(self, pp="pp", pr=None):
        return self.L.banet_lm_level_pose_prior_workspace_bytes(ctypes.byref(self.lv), pr, self.ref(pp))

    def apply(self, pp="pp", R="p", T="p", AtA="p", Atb="p"):
        pick = lambda v: self.p if v == "p" else v
        return self.L.banet_pose_prior_apply_f32(ctypes.byref(self.lv), self.ref(pp), pick(R), pick(T), pick(AtA), pick(Atb), None)

    def level(self, pp="pp", pr=None, ws="base", nbytes=1 << 30, iters=2):
        return self.L.banet_lm_level_pose_prior_f32(ctypes.byref(self.lv), ctypes.byref(self.mlp), 1000.0, iters, None, pr, self.ref(pp),
                                                    ctypes.byref(self.st), self.base if ws == "base" else ws, nbytes, None)

    def schedule(self, n=2, early=0):
        c = self.capi
        self.lvs = (c.Level * n)(*([self.lv] * n))
        self.mp = (ctypes.POINTER(c.Mlp) * n)(*([ctypes.pointer(self.mlp)] * n))
        self.it = (ctypes.c_int32 * n)(*([1] * n))
        s = c.Schedule()
        s.levels, s.n_levels, s.early_termination = ctypes.cast(self.lvs, ctypes.POINTER(c.Level)), n, early
        s.mlps = ctypes.cast(self.mp, ctypes.POINTER(ctypes.POINTER(c.Mlp)))
        s.max_iters, s.l2_base = ctypes.cast(self.it, ctypes.POINTER(ctypes.c_int32)), 1000.0
        s.workspace, s.workspace_bytes = self.base, 1 << 30
        return s


def bad_pose_priors(capi, p):
    for has in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)):      # some but not all of the three pointers
        q = capi.PosePrior()
        for name, on in zip(("R0", "T0", "Lambda"), has):
            setattr(q, name, p if on else None)
        q.scale = 1.0
        yield "pointers %s" % (has,), q, True
    for scale in (-1.0, float("nan"), float("inf"), -0.5):
        q = capi.PosePrior()
        q.R0 = q.T0 = q.Lambda = p
        q.scale = scale
        yield "scale %r" % scale, q, False
    q = capi.PosePrior()
    q.R0 = q.T0 = q.Lambda = p
    q.scale, q.reserved_ = 1.0, 1
    yield "reserved_", q, False
    q = capi.PosePrior()                                    # ... also where the scale makes the prior empty
    q.R0, q.scale = p, 0.0
    yield "R0 alone, scale 0", q, True
    q = capi.PosePrior()
    q.scale, q.reserved_ = 0.0, 7
    yield "reserved_ of an empty prior", q, False


@pytest.mark.parametrize("K", [16, 0])
def test_bad_pose_priors_are_invalid_arguments_in_every_entry(capi, K):
    h = Host(capi, K=K)
    for what, q, query_zero in bad_pose_priors(capi, h.p):
        assert h.apply(pp=ctypes.byref(q)) == ERR_INVALID_ARG, what
        assert h.level(pp=ctypes.byref(q)) == ERR_INVALID_ARG, what
        s = h.schedule()
        for at in (0, 1):                                   # a bad prior on the first and on the last level
            pps = (capi.PosePrior * 2)()
            pps[at] = q
            assert h.L.banet_lm_solve_pose_prior_f32(ctypes.byref(s), None, pps, ctypes.byref(h.st), None) == ERR_INVALID_ARG, (what, at)
            if query_zero:
                assert h.L.banet_lm_solve_pose_prior_workspace_bytes(ctypes.byref(s), None, pps) == 0, what
        base = h.L.banet_lm_level_workspace_bytes(ctypes.byref(h.lv))
        assert h.q_level(ctypes.byref(q)) == (0 if query_zero else base), what       # the query reads the pointers only


def test_null_arguments_unsupported_levels_and_the_rules_of_the_coefficient_prior(capi):
    h = Host(capi)
    for name in ("R", "T", "AtA", "Atb"):
        assert h.apply(**{name: None}) == ERR_INVALID_ARG, name
        assert h.apply(pp=None, **{name: None}) == ERR_INVALID_ARG, name     # also with the empty prior
    assert h.L.banet_pose_prior_apply_f32(None, ctypes.byref(h.pp), h.p, h.p, h.p, h.p, None) == ERR_INVALID_ARG
    assert h.L.banet_lm_level_pose_prior_workspace_bytes(None, None, ctypes.byref(h.pp)) == 0
    # legacy variants: unsupported, and a query of 0 -- while the empty pose prior is accepted there
    for variant in (capi.LEGACY_FIXED, capi.LEGACY_LM):
        leg = Host(capi, K=0, variant=variant)
        assert leg.apply() == ERR_UNSUPPORTED and leg.level() == ERR_UNSUPPORTED and leg.q_level() == 0
        assert leg.q_level(None) == leg.L.banet_lm_level_workspace_bytes(ctypes.byref(leg.lv)) > 0
        assert leg.apply(pp=None) == OK
        s = leg.schedule()
        pps = (capi.PosePrior * 2)(capi.PosePrior(), leg.pp)
        assert leg.L.banet_lm_solve_pose_prior_f32(ctypes.byref(s), None, pps, ctypes.byref(leg.st), None) == ERR_UNSUPPORTED
        assert leg.L.banet_lm_solve_pose_prior_workspace_bytes(ctypes.byref(s), None, pps) == 0
    many = Host(capi, pairs=9)                              # more target frames than the kernel's LDS holds
    assert many.apply() == ERR_UNSUPPORTED
    # the camera level takes the pose prior; the coefficient prior keeps (5d)'s rules there
    cam = Host(capi, K=0)
    assert cam.lv.variant == capi.BUNDLE_CAMERA
    base = cam.L.banet_lm_level_workspace_bytes(ctypes.byref(cam.lv))
    assert cam.q_level() == base > 0
    assert cam.level(nbytes=base - 1) == ERR_WORKSPACE and cam.level(ws=None) == ERR_WORKSPACE
    assert cam.q_level(pr=ctypes.byref(cam.pr)) == 0 and cam.level(pr=ctypes.byref(cam.pr)) == ERR_UNSUPPORTED
    # the bundle level: the query is banet_lm_level_prior_workspace_bytes, with the coefficient prior and without
    for pr in (None, ctypes.byref(h.pr)):
        want = h.L.banet_lm_level_prior_workspace_bytes(ctypes.byref(h.lv), pr)
        assert h.q_level(pr=pr) == want > 0
        assert h.level(pr=pr, nbytes=want - 1) == ERR_WORKSPACE
    bad = capi.Prior()
    bad.eta, bad.scale = h.p, 1.0                           # eta without Lambda
    assert h.level(pr=ctypes.byref(bad)) == ERR_INVALID_ARG and h.q_level(pr=ctypes.byref(bad)) == 0
    # what banet_lm_level_ex_f32 refuses is refused with its code
    g = Host(capi)
    g.st.delta = None
    assert g.level() == ERR_INVALID_ARG
    assert Host(capi).level(iters=-1) == ERR_INVALID_ARG
    # the schedule: early termination is excluded, with or without priors
    s = h.schedule(early=1)
    assert h.L.banet_lm_solve_pose_prior_f32(ctypes.byref(s), None, None, ctypes.byref(h.st), None) == ERR_INVALID_ARG
    assert h.L.banet_lm_solve_pose_prior_f32(None, None, None, ctypes.byref(h.st), None) == ERR_INVALID_ARG


def test_the_empty_pose_prior_launches_nothing_and_needs_the_level_workspace(capi):
    h = Host(capi)
    zero = capi.PosePrior()
    zero.R0 = zero.T0 = zero.Lambda = h.p
    zero.scale = 0.0
    base = h.L.banet_lm_level_workspace_bytes(ctypes.byref(h.lv))
    for i, pp in enumerate([None, ctypes.byref(capi.PosePrior()), ctypes.byref(zero)]):
        assert h.apply(pp=pp) == OK, i                      # no launch: OK also without a device
        assert h.level(pp=pp, nbytes=base - 1) == ERR_WORKSPACE, i
        assert h.q_level(pp) == base, i
    s = h.schedule()
    L = h.L
    assert L.banet_lm_solve_pose_prior_workspace_bytes(ctypes.byref(s), None, None) == L.banet_lm_solve_workspace_bytes(ctypes.byref(s)) == base
    assert L.banet_lm_solve_pose_prior_workspace_bytes(ctypes.byref(s), None, (capi.PosePrior * 2)()) == base
    prs = (capi.Prior * 2)(capi.Prior(), h.pr)
    assert L.banet_lm_solve_pose_prior_workspace_bytes(ctypes.byref(s), prs, (capi.PosePrior * 2)(h.pp, h.pp)) == \
        L.banet_lm_solve_prior_workspace_bytes(ctypes.byref(s), prs) > base


# ---- pose_prior_plan.hpp, compiled with g++ ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_lib(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("pose_prior_plan")), "libpose_prior_plan_host.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", out,
                           os.path.join(ROOT, "tests", "native", "pose_prior_plan_host.cpp")])
    L = ctypes.CDLL(out)
    L.banet_test_pose_prior_plan_fields.restype = ctypes.c_char_p
    return L


def plan_rows(L, rows, scales):
    fields = L.banet_test_pose_prior_plan_fields().decode().split()
    assert fields[0] == "desc_ints=9"
    names = fields[3:]
    desc = np.ascontiguousarray(np.array(rows, np.int64))
    sc = np.ascontiguousarray(np.array(scales, np.float32))
    out = np.zeros((len(rows), len(names)), np.int64)
    L.banet_test_pose_prior_plan_sweep(desc.ctypes.data_as(ctypes.c_void_p), sc.ctypes.data_as(ctypes.c_void_p), len(rows),
                                       out.ctypes.data_as(ctypes.c_void_p))
    return [dict(zip(names, [int(v) for v in row])) for row in out]


def test_the_plan_decides_the_grid_emptiness_and_refusals(capi, plan_lib):
    BUNDLE, CAMERA, FIXED = capi.BUNDLE, capi.BUNDLE_CAMERA, capi.LEGACY_FIXED
    assert plan_lib.banet_test_pose_prior_threads() == 256 and plan_lib.banet_test_pose_prior_pairs_max() == 8
    #        B  K    pairs variant R0 T0 La res given  scale
    rows = [((3, 16, 1, BUNDLE, 1, 1, 1, 0, 1), 1.0),      # 0: on
            ((32, 128, 0, BUNDLE, 1, 1, 1, 0, 1), 0.5),    # 1: pairs = 0 counts as one target frame
            ((3, 0, 7, CAMERA, 1, 1, 1, 0, 1), 2.0),       # 2: the pose-only level
            ((3, 130, 8, BUNDLE, 1, 1, 1, 0, 1), 1.0),     # 3: the largest window
            ((3, 16, 1, BUNDLE, 1, 1, 1, 0, 1), 0.0),      # 4: empty by its scale
            ((3, 16, 1, BUNDLE, 0, 0, 0, 0, 1), 1.0),      # 5: empty by its pointers
            ((3, 16, 1, BUNDLE, 1, 1, 1, 0, 0), 1.0),      # 6: empty: NULL
            ((3, 0, 1, FIXED, 0, 0, 0, 0, 1), 1.0),        # 7: the empty prior on a legacy level
            ((3, 0, 1, FIXED, 1, 1, 1, 0, 1), 1.0),        # 8: unsupported
            ((3, 16, 9, BUNDLE, 1, 1, 1, 0, 1), 1.0),      # 9: unsupported: 9 target frames
            ((3, 0, 1, BUNDLE, 1, 1, 1, 0, 1), 1.0),       # 10: unsupported: `bundle` without a basis
            ((3, 16, 1, BUNDLE, 1, 0, 1, 0, 1), 1.0),      # 11: invalid: T0 missing
            ((3, 16, 1, BUNDLE, 1, 1, 1, 1, 1), 1.0),      # 12: invalid: reserved_
            ((3, 16, 1, BUNDLE, 1, 1, 1, 0, 1), -1.0),     # 13: invalid: scale
            ((3, 16, 1, BUNDLE, 1, 1, 1, 0, 1), float("nan")),
            ((3, 16, 1, BUNDLE, 1, 1, 1, 0, 1), float("inf")),
            ((0, 16, 1, BUNDLE, 1, 1, 1, 0, 1), 1.0),      # 16: invalid: B
            ((3, 16, 1, BUNDLE, 0, 1, 0, 0, 1), 0.0)]      # 17: invalid whatever the scale
    got = plan_rows(plan_lib, [r for r, _ in rows], [s for _, s in rows])
    on = lambda pairs, K, B: dict(rc=OK, on=1, pairs=pairs, m=6 * pairs, K=K, P=6 * pairs + K, grid=B)
    off = lambda rc: dict(rc=rc, on=0, pairs=0, m=0, K=0, P=0, grid=0)
    want = [on(1, 16, 3), on(1, 128, 32), on(7, 0, 3), on(8, 130, 3)] + [off(OK)] * 4 + [off(ERR_UNSUPPORTED)] * 3 + [off(ERR_INVALID_ARG)] * 7
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, g, w)


def test_python_entries_refuse_cpu_tensors_and_the_differentiable_solve_names_the_missing_backward(capi):
    import torch
    from banet_amd import dense, dense_train, ops
    with pytest.raises(capi.BanetError):
        ops.PosePrior(torch.zeros(1, 1, 3, 3), torch.zeros(1, 1, 3), torch.zeros(1, 6, 6))
    assert ops._pose_prior_is_empty(None) and ops._pose_prior_is_empty(ops.PosePrior())
    prior = dense.DensePrior(pose=(object(), object(), object()))
    assert prior.coef is None and prior.depth_obs is None and len(prior.pose) == 3

    class FakeBA:
        variant = "bundle"
    with pytest.raises(NotImplementedError, match="backward"):
        dense_train.solve_differentiable(FakeBA(), [], [], [1], prior=prior)
