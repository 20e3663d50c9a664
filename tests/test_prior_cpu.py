"""The prior term on the host (include/banet_hip.h (5d)): linkage and struct layout, argument validation and the queries of every new
entry, the workspace refusals (driven through the library in a child process without a device), the region offsets of
csrc/prior_plan.hpp pinned by hand, and the float64 twin of tests/prior_ref.py against finite differences.  No GPU: every call here
is refused by the host-side checks, launches nothing (the empty prior), or fails for lack of a device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import prior_ref as pref
import ws_contract as wsc

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
os.environ.setdefault("BANET_NUM_CUS", "256")
OK, ERR_INVALID_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED, ERR_LAUNCH = 0, -1, -2, -3, -4
SYMBOLS = ("banet_prior_workspace_bytes", "banet_prior_apply_f32", "banet_lm_level_prior_workspace_bytes", "banet_lm_level_prior_f32",
           "banet_lm_solve_prior_workspace_bytes", "banet_lm_solve_prior_f32")
up = lambda n: (n + 255) // 256 * 256


@pytest.fixture(scope="module")
def capi():
    from banet_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _capi


class Host:
    """fake host pointers (compared with NULL, never dereferenced), a level, a state, an MLP and an aligned fake workspace address"""

    def __init__(self, capi, B=2, H=24, W=32, K=16, pairs=1, variant=None, has=(1, 1, 1, 1), scale=0.5):
        self.capi, self.L = capi, capi.lib()
        self.host = (ctypes.c_float * 64)()
        self.p = ctypes.cast(self.host, ctypes.c_void_p).value
        self.arena = (ctypes.c_char * 512)()
        self.base = (ctypes.addressof(self.arena) + 255) & ~255
        self.lv = wsc._abi_level(capi, self.p, B, H, W, K, pairs, C=16, variant=variant)
        self.pr = capi.Prior()
        for name, on in zip(("Lambda", "eta", "obs_depth", "obs_weight"), has):
            setattr(self.pr, name, self.p if on else None)
        self.pr.scale = scale
        self.st = capi.State()
        self.st.R = self.st.T = self.st.Wc = self.st.iters = self.st.ratio = self.st.lambda_out = self.st.delta = self.p
        self.mlp = capi.Mlp()
        for i in range(5):
            self.mlp.w[i] = self.mlp.b[i] = self.p

    def ref(self, pr="pr"):
        return ctypes.byref(self.pr) if pr == "pr" else pr

    def q_apply(self, pr="pr"):
        return self.L.banet_prior_workspace_bytes(ctypes.byref(self.lv), self.ref(pr))

    def q_level(self, pr="pr"):
        return self.L.banet_lm_level_prior_workspace_bytes(ctypes.byref(self.lv), self.ref(pr))

    def apply(self, pr="pr", Wc="p", AtA="p", Atb="p", ws="base", nbytes=1 << 30):
        pick = lambda v: self.p if v == "p" else v
        return self.L.banet_prior_apply_f32(ctypes.byref(self.lv), self.ref(pr), pick(Wc), pick(AtA), pick(Atb),
                                            self.base if ws == "base" else ws, nbytes, None)

    def level(self, pr="pr", ws="base", nbytes=1 << 30, iters=2):
        return self.L.banet_lm_level_prior_f32(ctypes.byref(self.lv), ctypes.byref(self.mlp), 1000.0, iters, None, self.ref(pr),
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


# ---- linkage and layout -------------------------------------------------------------------------------------------------------------
def test_the_library_exports_the_symbols_and_capi_binds_them(capi):
    L = ctypes.CDLL(capi.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "banet_hip.h")).read()
    for name in SYMBOLS:
        assert hasattr(L, name), name
        assert name in capi.EXPORTS
        assert re.search(r"\b%s\(" % name, header), name
    assert capi.lib().banet_version() == 150              # unchanged: the entries are detected by their symbols
    section = header[header.index("(5d)"):header.index("/* (6) per-level preparation")]
    assert "ws_bytes" not in section and section.count("workspace_bytes") >= 5


def test_struct_layout_matches_the_header(capi, tmp_path):
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "banet_hip.h"\n'
                    'int main(){printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(banet_prior_t), offsetof(banet_prior_t, Lambda), '
                    'offsetof(banet_prior_t, eta), offsetof(banet_prior_t, obs_depth), offsetof(banet_prior_t, obs_weight), '
                    'offsetof(banet_prior_t, scale), offsetof(banet_prior_t, reserved_));return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    P = capi.Prior
    assert got == [ctypes.sizeof(P), P.Lambda.offset, P.eta.offset, P.obs_depth.offset, P.obs_weight.offset, P.scale.offset,
                   P.reserved_.offset]
    assert [n for n, _ in P._fields_] == ["Lambda", "eta", "obs_depth", "obs_weight", "scale", "reserved_"]


# ---- argument validation ------------------------------------------------------------------------------------------------------------
def test_bad_priors_are_invalid_arguments_in_every_entry(capi):
    def bad_priors(h):
        for has in ((0, 1, 0, 0), (0, 1, 1, 0), (0, 0, 0, 1), (1, 0, 0, 1)):       # eta without Lambda, obs_weight without obs_depth
            q = capi.Prior()
            for name, on in zip(("Lambda", "eta", "obs_depth", "obs_weight"), has):
                setattr(q, name, h.p if on else None)
            q.scale = 1.0
            yield "pointers %s" % (has,), q, True
        for scale in (-1.0, float("nan"), float("inf"), -0.5):
            q = capi.Prior()
            q.Lambda, q.scale = h.p, scale
            yield "scale %r" % scale, q, False
        q = capi.Prior()
        q.Lambda, q.scale, q.reserved_ = h.p, 1.0, 1
        yield "reserved_", q, False
        q = capi.Prior()                                    # ... also where the scale makes the prior empty
        q.eta, q.scale = h.p, 0.0
        yield "eta alone, scale 0", q, True
    h = Host(capi)
    for what, q, query_zero in bad_priors(h):
        assert h.apply(pr=ctypes.byref(q)) == ERR_INVALID_ARG, what
        assert h.level(pr=ctypes.byref(q)) == ERR_INVALID_ARG, what
        s = h.schedule()
        for at in (0, 1):                                   # a bad prior on the first and on the last level
            prs = (capi.Prior * 2)()
            prs[at] = q
            assert h.L.banet_lm_solve_prior_f32(ctypes.byref(s), prs, ctypes.byref(h.st), None) == ERR_INVALID_ARG, (what, at)
            if query_zero:
                assert h.L.banet_lm_solve_prior_workspace_bytes(ctypes.byref(s), prs) == 0, what
        if query_zero:                                      # the queries read the pointers only
            assert h.q_apply(ctypes.byref(q)) == 0 and h.q_level(ctypes.byref(q)) == 0, what
        else:
            assert h.q_apply(ctypes.byref(q)) > 0 and h.q_level(ctypes.byref(q)) > 0, what


def test_null_arguments_and_levels_without_a_basis(capi):
    h = Host(capi)
    assert h.apply(Wc=None) == ERR_INVALID_ARG and h.apply(AtA=None) == ERR_INVALID_ARG and h.apply(Atb=None) == ERR_INVALID_ARG
    assert h.apply(pr=None, Wc=None) == ERR_INVALID_ARG    # also with the empty prior
    assert h.L.banet_prior_apply_f32(None, ctypes.byref(h.pr), h.p, h.p, h.p, h.base, 1 << 30, None) == ERR_INVALID_ARG
    assert h.L.banet_prior_workspace_bytes(None, ctypes.byref(h.pr)) == 0
    assert h.L.banet_lm_level_prior_workspace_bytes(None, ctypes.byref(h.pr)) == 0
    for field in ("depth", "basis"):                        # the observation half reads them
        g = Host(capi)
        setattr(g.lv, field, None)
        assert g.apply() == ERR_INVALID_ARG, field
    g = Host(capi, has=(1, 1, 0, 0))                        # the coefficient half alone does not
    g.lv.depth = g.lv.basis = None
    assert g.apply(ws=None) == ERR_WORKSPACE
    # a prior that is not empty on a level without a depth basis: unsupported, and a query of 0
    cam = Host(capi, K=0)
    assert cam.lv.variant == capi.BUNDLE_CAMERA
    assert cam.q_apply() == 0 and cam.q_level() == 0
    assert cam.apply() == ERR_UNSUPPORTED and cam.level() == ERR_UNSUPPORTED
    s = cam.schedule()
    prs = (capi.Prior * 2)(capi.Prior(), cam.pr)
    assert cam.L.banet_lm_solve_prior_f32(ctypes.byref(s), prs, ctypes.byref(cam.st), None) == ERR_UNSUPPORTED
    assert cam.L.banet_lm_solve_prior_workspace_bytes(ctypes.byref(s), prs) == 0
    leg = Host(capi, K=0, variant=capi.LEGACY_FIXED)
    assert leg.q_level() == 0 and leg.level() == ERR_UNSUPPORTED and leg.apply() == ERR_UNSUPPORTED
    # ... while the EMPTY prior is accepted there: the existing entry's own checks and workspace need
    assert cam.q_level(None) == cam.L.banet_lm_level_workspace_bytes(ctypes.byref(cam.lv)) > 0
    assert cam.level(pr=None, ws=None) == ERR_WORKSPACE
    # what banet_lm_level_ex_f32 refuses is refused with its code
    h = Host(capi)
    h.st.delta = None
    assert h.level() == ERR_INVALID_ARG
    h = Host(capi)
    assert h.level(iters=-1) == ERR_INVALID_ARG
    # the schedule: early termination is excluded, with or without priors
    h = Host(capi)
    s = h.schedule(early=1)
    assert h.L.banet_lm_solve_prior_f32(ctypes.byref(s), None, ctypes.byref(h.st), None) == ERR_INVALID_ARG
    assert h.L.banet_lm_solve_prior_f32(None, None, ctypes.byref(h.st), None) == ERR_INVALID_ARG


def test_the_empty_prior_launches_nothing_and_needs_the_level_workspace(capi):
    h = Host(capi)
    empties = [None, ctypes.byref(capi.Prior())]
    zero = capi.Prior()
    zero.Lambda = zero.eta = zero.obs_depth = zero.obs_weight = h.p
    zero.scale = 0.0
    empties.append(ctypes.byref(zero))
    base = h.L.banet_lm_level_workspace_bytes(ctypes.byref(h.lv))
    for i, pr in enumerate(empties):
        assert h.apply(pr=pr, ws=None, nbytes=0) == OK, i   # no device in sight: OK means that nothing was launched
        assert h.level(pr=pr, nbytes=base - 1) == ERR_WORKSPACE, i       # the call's need is banet_lm_level_workspace_bytes exactly
    for pr in empties[:2]:                                 # the queries read the pointers, not the scale
        assert h.q_apply(pr) == 0 and h.q_level(pr) == base
    assert h.q_level(empties[2]) > base
    s = h.schedule()
    assert h.L.banet_lm_solve_prior_workspace_bytes(ctypes.byref(s), None) == h.L.banet_lm_solve_workspace_bytes(ctypes.byref(s)) == base
    assert h.L.banet_lm_solve_prior_workspace_bytes(ctypes.byref(s), (capi.Prior * 2)()) == base


# ---- the workspace: queries and refusals, through the library ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sweep(capi):
    return pref.abi_sweep_in_child()


def expected_regions(B, N, K, has):
    """DESIGN.md 2.1, by hand: Le, ee, then -- with observations -- the Gram pass's partial rows, G and g"""
    n = up(B * K * K * 4) + up(B * K * 4)
    if has[2]:
        NR = (K + 31) // 32
        rows = min((N + 255) // 256, 64)
        chunk = (-(-N // rows) + 1) // 2 * 2
        rows = -(-N // chunk)
        pstride = NR * (NR + 1) // 2 * 1024 + NR * 32 + 32
        n += up(B * rows * pstride * 4) + up(B * K * K * 4) + up(B * K * 4)
    return n


def test_the_queries_are_the_level_need_plus_the_regions(sweep):
    assert len(sweep) == 3 * len(pref.ABI_SHAPES)
    for r in sweep:
        B, N, K, pairs = r["shape"][:4]
        has = r["shape"][4:]
        assert r["bytes"] > 0 and r["bytes"] % 256 == 0, r
        if r["name"].startswith("lm_solve_prior"):
            assert r["bytes"] == r["base"] + expected_regions(B, N, K, has), r      # the maximum of an empty level and this one
        else:
            assert r["bytes"] == r["base"] + expected_regions(B, N, K, has), r
        assert r["base"] % 256 == 0 and (r["base"] > 0) == (not r["name"].startswith("prior_apply")), r


def test_exact_query_accepted_one_byte_less_misaligned_and_null_refused(sweep):
    for r in sweep:
        assert r["exact"] == ERR_LAUNCH, r                  # past every check: fails for lack of a device only
        assert r["minus1"] == ERR_WORKSPACE and r["off4"] == ERR_WORKSPACE and r["null"] == ERR_WORKSPACE, r


# ---- prior_plan.hpp, compiled with g++ --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_lib(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("prior_plan")), "libprior_plan_host.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", out,
                           os.path.join(ROOT, "tests", "native", "prior_plan_host.cpp")])
    L = ctypes.CDLL(out)
    L.banet_test_prior_plan_fields.restype = ctypes.c_char_p
    return L


def plan_rows(L, rows, scales):
    fields = L.banet_test_prior_plan_fields().decode().split()
    assert fields[0] == "desc_ints=12"
    names = fields[1:]
    desc = (ctypes.c_int64 * (12 * len(rows)))(*[v for r in rows for v in r])
    sc = (ctypes.c_float * len(rows))(*scales)
    out = (ctypes.c_int64 * (len(names) * len(rows)))()
    L.banet_test_prior_plan_sweep(desc, sc, len(rows), out)
    return [dict(zip(names, out[i * len(names):(i + 1) * len(names)])) for i in range(len(rows))]


def test_region_offsets_pinned_by_hand(plan_lib):
    BUNDLE = 3
    #        B, N,    K,   pairs, variant, L, e, o, w, reserved_, base, plan
    rows = [(2, 768, 16, 1, BUNDLE, 1, 1, 0, 0, 0, 0, 1),            # coefficients only, no base
            (3, 247, 5, 2, BUNDLE, 0, 0, 1, 1, 0, 1000192, 1),       # observations only, behind a level's carve
            (1, 768, 200, 1, BUNDLE, 1, 0, 1, 0, 0, 512, 0)]         # both halves, K = 200 (7 column blocks)
    p = plan_rows(plan_lib, rows, [1.0, 0.25, 1.0])
    a = p[0]
    assert (a["rc"], a["on"], a["coef"], a["eta"], a["obs"], a["weight"]) == (0, 1, 1, 1, 0, 0)
    assert (a["K"], a["m"], a["P"], a["add_grid"]) == (16, 6, 22, 8)                 # 32 rows of Le, 4 waves per workgroup
    assert (a["off_Le"], a["off_ee"], a["bytes"]) == (0, 2048, 2048 + 256)           # 2 x 16 x 16 x 4 = 2048; 2 x 16 x 4 = 128 -> 256
    assert (a["off_part"], a["off_G"], a["off_g"]) == (0, 0, 0)
    b = p[1]
    assert (b["rc"], b["on"], b["coef"], b["eta"], b["obs"], b["weight"]) == (0, 1, 0, 0, 1, 1)
    assert (b["m"], b["P"], b["add_grid"]) == (12, 17, 4)                            # 15 rows of Le
    assert (b["fit.NR"], b["fit.NP"], b["fit.chunk"], b["fit.rows"], b["fit.pstride"]) == (1, 1, 248, 1, 1024 + 32 + 32)
    # Le 3 x 25 x 4 = 300 -> 512; ee 60 -> 256; rows 3 x 1 x 1088 x 4 = 13056 (a multiple of 256); G 300 -> 512; g 60 -> 256
    assert b["off_Le"] == 1000192 and b["off_ee"] == 1000192 + 512 and b["off_part"] == 1000192 + 768
    assert b["off_G"] == 1000192 + 768 + 13056 and b["off_g"] == b["off_G"] + 512 and b["bytes"] == b["off_g"] + 256
    c = p[2]
    assert (c["rc"], c["on"], c["coef"], c["eta"], c["obs"], c["weight"]) == (0, 1, 1, 0, 1, 0)
    assert (c["fit.NR"], c["fit.NP"], c["fit.chunk"], c["fit.rows"], c["fit.pstride"]) == (7, 28, 256, 3, 28 * 1024 + 7 * 32 + 32)
    assert (c["m"], c["P"], c["add_grid"]) == (6, 206, 50)
    # Le 200 x 200 x 4 = 160000 -> 160000 (625 x 256); ee 800 -> 1024; rows 3 x 28928 x 4 = 347136 (1356 x 256)
    assert c["off_Le"] == 512 and c["off_ee"] == 512 + 160000 and c["off_part"] == c["off_ee"] + 1024
    assert c["off_G"] == c["off_part"] + 347136 and c["off_g"] == c["off_G"] + 160000 and c["bytes"] == c["off_g"] + 1024


def test_the_plan_decides_emptiness_and_refusals(plan_lib):
    BUNDLE, CAMERA = 3, 2
    rows = [(2, 768, 16, 1, BUNDLE, 0, 0, 0, 0, 0, 4096, 1),         # no pointers: empty
            (2, 768, 16, 1, BUNDLE, 1, 1, 1, 1, 0, 4096, 1),         # scale 0: empty for the call ...
            (2, 768, 16, 1, BUNDLE, 1, 1, 1, 1, 0, 4096, 0),         # ... not for the query
            (2, 768, 16, 1, BUNDLE, 0, 1, 0, 0, 0, 4096, 1),         # eta without Lambda
            (2, 768, 16, 1, BUNDLE, 1, 0, 0, 0, 7, 4096, 1),         # reserved_
            (2, 768, 0, 1, CAMERA, 1, 0, 0, 0, 0, 4096, 1),          # no basis
            (2, 768, 257, 1, BUNDLE, 1, 0, 0, 0, 0, 4096, 1),        # K past the Gram pass
            (2, 768, 16, 1, BUNDLE, 1, 0, 0, 0, 0, 4096, 1)]         # a negative scale
    p = plan_rows(plan_lib, rows, [1.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0, -2.0])
    assert [(r["rc"], r["on"]) for r in p] == [(0, 0), (0, 0), (0, 1), (-1, 0), (-1, 0), (-3, 0), (-3, 0), (-1, 0)]
    assert all(r["bytes"] == 4096 for i, r in enumerate(p) if i != 2) and p[2]["bytes"] > 4096


# ---- the twin ------------------------------------------------------------------------------------------------------------------------
def twin_case(seed=3, B=2, N=60, K=5):
    rng = np.random.RandomState(seed)
    depth, basis = rng.uniform(1, 3, (B, N)), rng.standard_normal((B, N, K))
    obs = depth + rng.standard_normal((B, N)) * 0.1
    weight = rng.uniform(0.5, 2.0, (B, N))
    weight[:, ::7] = 0.0
    obs[0, 3] = np.nan
    weight[1, 4] = np.inf
    M = rng.standard_normal((B, K, K))
    Lambda = np.einsum("bik,bjk->bij", M, M) + np.eye(K)
    eta = rng.standard_normal((B, K))
    return dict(depth=depth, basis=basis, obs=obs, weight=weight, Lambda=Lambda, eta=eta, W=rng.standard_normal((B, K)) * 0.3)


def test_the_twin_adds_the_gradient_and_hessian_of_the_quadratic():
    """Gauss-Newton on the term alone: what the twin adds to Atb is minus the gradient at W, what it adds to AtA the Hessian --
    checked against central differences of the value"""
    c = twin_case()
    scale, B, K, pairs = 0.7, 2, 5, 2
    G, g = pref.fit_sums(c["depth"], c["basis"], c["obs"], c["weight"])
    Le, ee = pref.terms(scale, c["Lambda"], c["eta"], G, g)
    P = 6 * pairs + K
    A, b = pref.apply(np.zeros((B, P, P)), np.zeros((B, P, 1)), c["W"][:, :, None], Le, ee, pairs)
    assert not A[:, :12].any() and not A[:, :, :12].any() and not b[:, :12].any()      # the pose rows and columns are untouched
    f = lambda W: pref.quadratic(W, scale, c["Lambda"], c["eta"], c["depth"], c["basis"], c["obs"], c["weight"])
    h = 1e-4
    grad = np.zeros((B, K))
    for k in range(K):
        e = np.zeros((B, K))
        e[:, k] = h
        grad[:, k] = (f(c["W"] + e) - f(c["W"] - e)) / (2 * h)
    assert np.abs(-grad - b[:, 12:, 0]).max() <= 1e-7 * np.abs(grad).max()              # (a quadratic: central differences are exact)
    hess = np.zeros((B, K, K))
    for i in range(K):
        for j in range(K):
            ei, ej = np.zeros((B, K)), np.zeros((B, K))
            ei[:, i], ej[:, j] = h, h
            hess[:, i, j] = (f(c["W"] + ei + ej) - f(c["W"] + ei - ej) - f(c["W"] - ei + ej) + f(c["W"] - ei - ej)) / (4 * h * h)
    assert np.abs(hess - A[:, 12:, 12:]).max() <= 1e-5 * np.abs(hess).max()
    # the Newton step of the term alone lands on its minimiser: the gradient vanishes there
    Wn = c["W"] + np.linalg.solve(A[:, 12:, 12:], b[:, 12:, 0][:, :, None])[:, :, 0]
    _, b2 = pref.apply(np.zeros((B, P, P)), np.zeros((B, P, 1)), Wn[:, :, None], Le, ee, pairs)
    assert np.abs(b2).max() <= 1e-10 * np.abs(b).max()


def test_the_observation_form_equals_the_coefficient_form_of_its_sums():
    c = twin_case(seed=5)
    G, g = pref.fit_sums(c["depth"], c["basis"], c["obs"], c["weight"])
    for b in range(2):                                      # the sums against a direct loop over the fit's point set
        Gl, gl = np.zeros((5, 5)), np.zeros(5)
        for n in range(60):
            w, t = c["weight"][b, n], c["obs"][b, n]
            if not (w > 0 and np.isfinite(w) and np.isfinite(t)):
                continue
            Gl += w * np.outer(c["basis"][b, n], c["basis"][b, n])
            gl += w * (t - c["depth"][b, n]) * c["basis"][b, n]
        assert np.allclose(G[b], Gl, rtol=1e-12) and np.allclose(g[b], gl, rtol=1e-10, atol=1e-12)
    obs_form = pref.terms(0.3, G=G, g=g)
    coef_form = pref.terms(0.3, Lambda=G, eta=g)
    assert np.array_equal(obs_form[0], coef_form[0]) and np.array_equal(obs_form[1], coef_form[1])
    # ... and as values: the two quadratics differ by a constant (1/2 sum w r^2), so their differences agree
    W0, W1 = c["W"], c["W"] + 0.1
    dv_obs = (pref.quadratic(W1, 0.3, depth=c["depth"], basis=c["basis"], obs=c["obs"], weight=c["weight"]) -
              pref.quadratic(W0, 0.3, depth=c["depth"], basis=c["basis"], obs=c["obs"], weight=c["weight"]))
    dv_coef = pref.quadratic(W1, 0.3, Lambda=G, eta=g) - pref.quadratic(W0, 0.3, Lambda=G, eta=g)
    assert np.allclose(dv_obs, dv_coef, rtol=1e-10)
    # a half that is not given is left out: eta = None is eta = 0
    L1, e1 = pref.terms(2.0, Lambda=c["Lambda"])
    assert np.array_equal(L1, 2.0 * c["Lambda"]) and not e1.any()


@pytest.mark.parametrize("pairs", [1, 2])
def test_the_schedule_scenes_are_well_posed(pairs):
    """what the GPU module's 1e-4 gate on the 3-level, 2-iteration schedule presumes: on those scenes the float32 oracle itself is
    within a quarter of the gate of the float64 one, measured the same way (the last update, the final coefficients)"""
    from oracle import banet_oracle as orc, dense as odense, synth
    B, K, C = 3, 16, 16
    trans_mag, frac = pref.SCHEDULE_MOTION
    scenes = [synth.make_window_scene(24, 32, C, K, [4, 2, 1], 31 + b, pairs, trans_mag=trans_mag) for b in range(B)]
    intr, levels = odense.batch_scene(scenes)
    mlps = [orc.he_normal_mlp_weights(C, 5 + i) for i in range(3)]
    T0 = np.stack([np.asarray(s["T_gt"]) * frac for s in scenes]).reshape(B, pairs, 3, 1).astype(np.float32)
    out = {}
    for dt in (np.float32, np.float64):
        lv = [{k: (v.astype(dt) if isinstance(v, np.ndarray) else v) for k, v in l.items()} for l in levels]
        _, _, W, hist = odense.solve_bundle_window(intr.astype(dt), lv, mlps, [2, 2, 2], dtype=dt, T0=T0.astype(dt))
        out[dt] = (hist[-1]["delta"], W)
    rel = lambda g, w: float(np.abs(g - w).max() / np.abs(w).max())
    yard = (rel(out[np.float32][0], out[np.float64][0]), rel(out[np.float32][1], out[np.float64][1]))
    print("pairs %d: float32 oracle vs float64: delta %.2e, W %.2e; last max |delta| %.3f" % (pairs, yard[0], yard[1], np.abs(out[np.float64][0]).max()))
    assert max(yard) <= 2.5e-5 and np.abs(out[np.float64][0]).max() > 0.1


def test_python_entries_refuse_cpu_tensors_and_allocate_through_capi(capi):
    import torch
    from banet_amd import ops
    with pytest.raises(capi.BanetError):
        ops.Prior(Lambda=torch.zeros(2, 4, 4))
    assert "capi.workspace(" in open(os.path.join(ROOT, "banet_amd", "ops.py")).read().split("def prior_apply")[1].split("\ndef ")[0]
