"""The pose prior's backward (include/banet_hip.h (5g); csrc/pose_prior_grad.hip) without a GPU: the float64 twin of
tests/pose_prior_grad_ref.py against central differences of pose_prior_ref.window_term, the float32 evaluation of the same formulas
against the twin (the GPU test's gate), the host plan compiled with g++, and the entry's argument validation through the library
(every call here is refused before a launch)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import pose_prior_grad_ref as ppg
import pose_prior_ref as ppr
import ws_contract as wsc

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
os.environ.setdefault("BANET_NUM_CUS", "256")
OK, ERR_INVALID_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED, ERR_LAUNCH = 0, -1, -2, -3, -4
ALL_ANGLES = ppr.ANGLES + ppr.THRESHOLD_ANGLES

# the twin against central differences: the largest error measured here is 2.35e-9 (pairs 1; 2.02e-9 at pairs 2, 8.8e-10 at pairs 7;
# relative to the largest derivative of the window); the gate is 10 x that.  Float64 against float64: were it not <~ 1e-7 the twin
# would be wrong.
FD_MEASURED, FD_GATE = 2.35e-9, 2.35e-8
FD_STEPS = (1e-7, 2e-7, 4e-7)      # below the 1e-6 between the threshold angles (0.999 / 1.001 x 1e-3) and the threshold: no step crosses


@pytest.fixture(scope="module")
def capi():
    from banet_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _capi


# ---- the twin against finite differences ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pairs,B", [(1, 13), (2, 7), (7, 2)])
def test_the_twin_is_the_gradient_of_the_functional_by_central_differences(pairs, B):
    """d(<G, H> - <g, v>) / d(every entry of R, T, R0, T0, Lambda, scale), R and R0 as nine free entries; median of three steps"""
    seed = 13 * pairs                                        # angles[(seed + b pairs + i) % 13]: B pairs >= 13 poses see every angle
    c = ppr.apply_cases(pairs, seed, B=B)
    m = 6 * pairs
    rng = np.random.RandomState(900 + pairs)
    worst = 0.0
    f64 = lambda x: x.astype(np.float64)                     # noqa: E731
    for w in range(B):
        args = [f64(c[k][w]) for k in ("R", "T", "R0", "T0", "Lambda")] + [np.array(0.37)]
        G, g = rng.standard_normal((m, m)), rng.standard_normal(m)
        ref = ppg.window_grad(*args[:5], 0.37, G, g, with_bounds=False)
        got = [ref[k] for k in ("gR", "gT", "gR0", "gT0", "gLambda")] + [np.array(ref["gscale"])]
        top = max(np.abs(x).max() for x in got)
        for a, gx in zip(range(6), got):
            fd = np.zeros(args[a].size)
            for e in range(args[a].size):
                vals = []
                for h in FD_STEPS:
                    pm = []
                    for sgn in (1.0, -1.0):
                        q = [x.copy() for x in args]
                        q[a].reshape(-1)[e] += sgn * h
                        pm.append(ppg.functional(q[0], q[1], q[2], q[3], q[4], float(q[5]), G, g))
                    vals.append((pm[0] - pm[1]) / (2 * h))
                fd[e] = np.median(vals)
            worst = max(worst, np.abs(fd - np.asarray(gx).reshape(-1)).max() / top)
    print("pairs %d: |twin - central differences| / largest derivative %.2e (gate %.1e)" % (pairs, worst, FD_GATE))
    assert worst <= FD_GATE


def test_every_angle_is_seen_by_the_finite_difference_cases():
    angles = ALL_ANGLES
    for pairs, B in ((1, 13), (2, 7), (7, 2)):
        assert {angles[(13 * pairs + k) % len(angles)] for k in range(B * pairs)} == set(angles)


def test_gradients_at_exact_identity_are_finite_and_the_limit():
    """R = R0, T = T0 exactly (theta = 0, s = 0): finite, and equal to the value a hair away (1e-9 in the tangent) to 1e-7"""
    rng = np.random.RandomState(3)
    R0 = ppr.random_rotation(rng, 0.6)[None]
    T0 = rng.standard_normal((1, 3))
    Lam = np.eye(6) + 0.1 * rng.standard_normal((6, 6))
    G, g = rng.standard_normal((6, 6)), rng.standard_normal(6)
    at = ppg.window_grad(R0, T0, R0, T0, Lam, 0.5, G, g, with_bounds=False)
    Rn, Tn = ppr.compose(1e-9 * rng.standard_normal(6), R0[0], T0[0])
    near = ppg.window_grad(Rn[None], Tn[None], R0, T0, Lam, 0.5, G, g, with_bounds=False)
    for k in ppg.OUTPUTS:
        assert np.isfinite(at[k]).all(), k
        assert np.abs(np.asarray(at[k]) - np.asarray(near[k])).max() <= 1e-7 * max(np.abs(at[k]).max(), 1.0), k


# ---- float32 against the twin: the GPU gate ---------------------------------------------------------------------------------------------
def test_float32_arithmetic_is_this_far_from_the_twin():
    """the GPU gate's base: the formulas in float32 torch (the kernel's thresholds and series orders) against float64 on the cases of
    test_gpu_pose_prior_grad.py's main test; G is not symmetrised"""
    worst = {}
    seen = set()
    for pairs, K in ppr.APPLY_SHAPES:
        c = ppg.grad_problem(pairs, K)
        seen |= set(c["angles"])
        assert np.abs(c["gAtA"] - c["gAtA"].transpose(0, 2, 1)).max() > 0.1
        ref = ppg.batch_grad(c, c["gAtA"], c["gAtb"])
        got = ppg.batch_grad(c, c["gAtA"], c["gAtb"], mode="kernel", with_bounds=False)
        err = ppg.grad_errors(got, ref)
        print("pairs %d K %d: float32 against the twin  %s" % (pairs, K, "  ".join("%s %.3e" % kv for kv in err.items())))
        for k, v in err.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("worst per output: %s" % "  ".join("%s %.3e" % kv for kv in worst.items()))
    assert seen == set(ALL_ANGLES)
    top = max(worst.values())
    assert 0.5 * ppg.F32_GRAD_ERR <= top <= ppg.F32_GRAD_ERR, worst
    assert ppg.GRAD_GATE == 4 * ppg.F32_GRAD_ERR


# ---- linkage and layout -------------------------------------------------------------------------------------------------------------
def test_the_library_exports_the_symbol_and_capi_binds_it(capi):
    L = ctypes.CDLL(capi.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "banet_hip.h")).read()
    name = "banet_pose_prior_add_grad_f32"
    assert hasattr(L, name) and name in capi.EXPORTS and re.search(r"\b%s\(" % name, header)
    assert capi.lib().banet_version() == 150              # unchanged: the entry is detected by its symbol
    assert "(5g)" in header
    assert (capi.POSE_PRIOR_GRAD_OVERWRITE_STATE, capi.POSE_PRIOR_GRAD_OVERWRITE_PRIOR) == (1, 2)
    for macro, val in (("BANET_POSE_PRIOR_GRAD_OVERWRITE_STATE", 1), ("BANET_POSE_PRIOR_GRAD_OVERWRITE_PRIOR", 2)):
        assert re.search(r"#define %s %d\b" % (macro, val), header), macro


def test_struct_layout_matches_the_header(capi, tmp_path):
    names = ["gR", "gT", "gR0", "gT0", "gLambda", "gscale", "flags", "reserved_"]
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "banet_hip.h"\nint main(){printf("%zu", sizeof(banet_pose_prior_grad_t));\n' +
                    "".join('printf(" %%zu", offsetof(banet_pose_prior_grad_t, %s));\n' % n for n in names) + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    G = capi.PosePriorGrad
    assert got == [ctypes.sizeof(G)] + [getattr(G, n).offset for n in names]
    assert [n for n, _ in G._fields_] == names


# ---- argument validation ------------------------------------------------------------------------------------------------------------
class Host:
    """fake host pointers (compared with NULL, never dereferenced) and a level"""

    def __init__(self, capi, B=2, K=16, pairs=1, variant=None, scale=0.5):
        self.capi, self.L = capi, capi.lib()
        self.host = (ctypes.c_float * 64)()
        self.p = ctypes.cast(self.host, ctypes.c_void_p).value
        self.lv = wsc._abi_level(capi, self.p, B, 24, 32, K, pairs, C=16, variant=variant)
        self.pp = capi.PosePrior()
        self.pp.R0 = self.pp.T0 = self.pp.Lambda = self.p
        self.pp.scale = scale

    def out(self, names=("gR", "gT", "gR0", "gT0", "gLambda", "gscale"), flags=0, reserved=0):
        o = self.capi.PosePriorGrad()
        for n in names:
            setattr(o, n, self.p)
        o.flags, o.reserved_ = flags, reserved
        return o

    def call(self, pp="pp", R="p", T="p", gAtA="p", gAtb="p", out="all", lv="lv"):
        pick = lambda v: self.p if v == "p" else v                                          # noqa: E731
        o = self.out() if out == "all" else out
        return self.L.banet_pose_prior_add_grad_f32(ctypes.byref(self.lv) if lv == "lv" else lv, ctypes.byref(self.pp) if pp == "pp" else pp,
                                                    pick(R), pick(T), pick(gAtA), pick(gAtb), ctypes.byref(o) if o is not None else None, None)


@pytest.mark.parametrize("K", [16, 0])
def test_refusals_come_before_any_launch(capi, K):
    h = Host(capi, K=K)
    from test_pose_prior_cpu import bad_pose_priors
    for what, q, _ in bad_pose_priors(capi, h.p):           # the struct checks of (5f)
        assert h.call(pp=ctypes.byref(q)) == ERR_INVALID_ARG, what
    # the empty prior has no backward: NULL, no pointers, scale 0
    zero = capi.PosePrior()
    zero.R0 = zero.T0 = zero.Lambda = h.p
    zero.scale = 0.0
    for pp in (None, ctypes.byref(capi.PosePrior()), ctypes.byref(zero)):
        assert h.call(pp=pp) == ERR_INVALID_ARG
    for name in ("R", "T", "gAtA", "gAtb"):
        assert h.call(**{name: None}) == ERR_INVALID_ARG, name
    assert h.call(out=None) == ERR_INVALID_ARG and h.call(lv=None) == ERR_INVALID_ARG
    assert h.call(out=h.out(names=())) == ERR_INVALID_ARG                    # no output at all
    for flags in (4, 8, -1, 1 << 30, 3 | 16):
        assert h.call(out=h.out(flags=flags)) == ERR_INVALID_ARG, flags
    assert h.call(out=h.out(reserved=1)) == ERR_INVALID_ARG


def test_unsupported_levels_are_the_forwards(capi):
    for variant in (capi.LEGACY_FIXED, capi.LEGACY_LM):
        assert Host(capi, K=0, variant=variant).call() == ERR_UNSUPPORTED
    assert Host(capi, pairs=9).call() == ERR_UNSUPPORTED
    bad = Host(capi)
    bad.lv.B = 0
    assert bad.call() == ERR_INVALID_ARG
    # invalid arguments win over an unsupported level
    leg = Host(capi, K=0, variant=capi.LEGACY_FIXED)
    assert leg.call(out=leg.out(flags=4)) == ERR_INVALID_ARG and leg.call(R=None) == ERR_INVALID_ARG


# ---- pose_prior_grad_plan.hpp, compiled with g++ --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_lib(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("pose_prior_grad_plan")), "libpose_prior_grad_plan_host.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", out,
                           os.path.join(ROOT, "tests", "native", "pose_prior_grad_plan_host.cpp")])
    L = ctypes.CDLL(out)
    L.banet_test_pose_prior_grad_plan_fields.restype = ctypes.c_char_p
    return L


def plan_rows(L, rows, scales):
    fields = L.banet_test_pose_prior_grad_plan_fields().decode().split()
    assert fields[0] == "desc_ints=11"
    names = fields[1:]
    desc = np.ascontiguousarray(np.array(rows, np.int64))
    sc = np.ascontiguousarray(np.array(scales, np.float32))
    out = np.zeros((len(rows), len(names)), np.int64)
    L.banet_test_pose_prior_grad_plan_sweep(desc.ctypes.data_as(ctypes.c_void_p), sc.ctypes.data_as(ctypes.c_void_p), len(rows),
                                            out.ctypes.data_as(ctypes.c_void_p))
    return [dict(zip(names, [int(v) for v in row])) for row in out]


def test_the_plan_decides_the_grid_the_phases_and_the_refusals(capi, plan_lib):
    BUNDLE, CAMERA, FIXED = capi.BUNDLE, capi.BUNDLE_CAMERA, capi.LEGACY_FIXED
    assert plan_lib.banet_test_pose_prior_grad_threads() == 256 and plan_lib.banet_test_pose_prior_grad_entries() == 24
    A, X, XT, LAM, SCALE, POSE = (plan_lib.banet_test_pose_prior_grad_work_bit(i) for i in range(6))
    assert sorted((A, X, XT, LAM, SCALE, POSE)) == [1, 2, 4, 8, 16, 32]
    ALL = 63
    #        B  K    pairs variant prior res outputs flags ores lv out  scale
    rows = [((3, 16, 1, BUNDLE, 1, 0, ALL, 0, 0, 1, 1), 1.0),       # 0: everything, accumulating
            ((32, 128, 0, BUNDLE, 1, 0, ALL, 3, 0, 1, 1), 0.5),     # 1: pairs = 0 counts as one target frame; both groups written
            ((3, 0, 7, CAMERA, 1, 0, 1, 1, 0, 1, 1), 2.0),          # 2: the pose-only level, gR alone
            ((3, 130, 8, BUNDLE, 1, 0, 8, 2, 0, 1, 1), 1.0),        # 3: the largest window, gT0 alone
            ((3, 16, 2, BUNDLE, 1, 0, 16, 0, 0, 1, 1), 1.0),        # 4: gLambda alone: A only
            ((3, 16, 2, BUNDLE, 1, 0, 32, 0, 0, 1, 1), 1.0),        # 5: gscale alone: A, X
            ((3, 16, 2, BUNDLE, 1, 0, 48, 0, 0, 1, 1), 1.0),        # 6: gLambda and gscale: no pose phase
            ((3, 16, 2, BUNDLE, 1, 0, 2 | 16, 0, 0, 1, 1), 1.0),    # 7: gT and gLambda
            ((3, 16, 1, BUNDLE, 1, 0, ALL, 0, 0, 1, 1), 0.0),       # 8: invalid: empty by its scale
            ((3, 16, 1, BUNDLE, 2, 0, ALL, 0, 0, 1, 1), 1.0),       # 9: invalid: empty by its pointers
            ((3, 16, 1, BUNDLE, 0, 0, ALL, 0, 0, 1, 1), 1.0),       # 10: invalid: NULL prior
            ((3, 16, 1, BUNDLE, 3, 0, ALL, 0, 0, 1, 1), 1.0),       # 11: invalid: T0 missing
            ((3, 16, 1, BUNDLE, 1, 1, ALL, 0, 0, 1, 1), 1.0),       # 12: invalid: the prior's reserved_
            ((3, 16, 1, BUNDLE, 1, 0, ALL, 0, 0, 1, 1), -1.0),      # 13: invalid: scale
            ((3, 16, 1, BUNDLE, 1, 0, ALL, 0, 0, 1, 1), float("nan")),
            ((3, 16, 1, BUNDLE, 1, 0, ALL, 4, 0, 1, 1), 1.0),       # 15: invalid: an unknown flag bit
            ((3, 16, 1, BUNDLE, 1, 0, ALL, 0, 1, 1, 1), 1.0),       # 16: invalid: the output struct's reserved_
            ((3, 16, 1, BUNDLE, 1, 0, 0, 0, 0, 1, 1), 1.0),         # 17: invalid: no output at all
            ((3, 16, 1, BUNDLE, 1, 0, ALL, 0, 0, 0, 1), 1.0),       # 18: invalid: NULL level
            ((3, 16, 1, BUNDLE, 1, 0, ALL, 0, 0, 1, 0), 1.0),       # 19: invalid: NULL out
            ((0, 16, 1, BUNDLE, 1, 0, ALL, 0, 0, 1, 1), 1.0),       # 20: invalid: B
            ((3, 0, 1, FIXED, 1, 0, ALL, 4, 0, 1, 1), 1.0),         # 21: invalid before unsupported
            ((3, 0, 1, FIXED, 1, 0, ALL, 0, 0, 1, 1), 1.0),         # 22: unsupported: a legacy level
            ((3, 16, 9, BUNDLE, 1, 0, ALL, 0, 0, 1, 1), 1.0),       # 23: unsupported: 9 target frames
            ((3, 0, 1, BUNDLE, 1, 0, ALL, 0, 0, 1, 1), 1.0)]        # 24: unsupported: `bundle` without a basis
    got = plan_rows(plan_lib, [r for r, _ in rows], [s for _, s in rows])

    def on(pairs, K, B, work, ows=0, owp=0):
        return dict(rc=OK, on=1, pairs=pairs, m=6 * pairs, K=K, P=6 * pairs + K, grid=B, work=work, lanes=24 * pairs, overwrite_state=ows,
                    overwrite_prior=owp)
    off = lambda rc: dict(rc=rc, on=0, pairs=0, m=0, K=0, P=0, grid=0, work=0, lanes=0, overwrite_state=0, overwrite_prior=0)   # noqa: E731
    pose = POSE | X | XT
    want = [on(1, 16, 3, ALL), on(1, 128, 32, ALL, 1, 1), on(7, 0, 3, pose, 1, 0), on(8, 130, 3, pose, 0, 1), on(2, 16, 3, LAM | A),
            on(2, 16, 3, SCALE | A | X), on(2, 16, 3, LAM | SCALE | A | X), on(2, 16, 3, pose | LAM | A)] + \
        [off(ERR_INVALID_ARG)] * 14 + [off(ERR_UNSUPPORTED)] * 3
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, g, w)


def test_python_entries_and_the_keyword_of_the_differentiable_solve(capi):
    """the wrapper refuses the empty prior and unknown outputs; solve_differentiable keeps refusing a pose prior by default (the
    message names the keyword) and takes pose_prior_backward"""
    import inspect
    from banet_amd import dense, dense_train, ops
    assert ops.POSE_PRIOR_GRAD_OUTPUTS == ppg.OUTPUTS
    sig = inspect.signature(dense_train.solve_differentiable)
    assert sig.parameters["pose_prior_backward"].default is False
    assert inspect.signature(dense.DenseBA.solve_differentiable).parameters["pose_prior_backward"].default is False
    prior = dense.DensePrior(pose=(object(), object(), object()))

    class FakeBA:
        variant = "bundle"
    with pytest.raises(NotImplementedError, match="backward.*pose_prior_backward"):
        dense_train.solve_differentiable(FakeBA(), [], [], [1], prior=prior)
