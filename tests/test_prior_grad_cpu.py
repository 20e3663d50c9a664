"""The backward of the prior term on the host (include/banet_hip.h (5e)): linkage and struct layout, the float64 twin of
tests/prior_grad_ref.py against central differences, csrc/prior_grad_plan.hpp compiled with g++ (sizes and offsets pinned by hand at
prior_ref.ABI_SHAPES), and the host-only ABI probes of the three entries in a child process that sees no device.  No GPU: every
call here is refused by the host-side checks or fails for lack of a device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import prior_grad_ref as gref
import prior_ref as pref

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
os.environ.setdefault("BANET_NUM_CUS", "256")
OK, ERR_INVALID_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED, ERR_LAUNCH = 0, -1, -2, -3, -4
SYMBOLS = ("banet_prior_terms_f32", "banet_prior_add_grad_f32", "banet_prior_terms_grad_workspace_bytes", "banet_prior_terms_grad_f32")
up = lambda n: (n + 255) // 256 * 256      # noqa: E731


@pytest.fixture(scope="module")
def capi():
    from banet_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _capi


# ---- linkage and layout -------------------------------------------------------------------------------------------------------------
def test_the_library_exports_the_symbols_and_capi_binds_them(capi):
    L = ctypes.CDLL(capi.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "banet_hip.h")).read()
    for name in SYMBOLS:
        assert hasattr(L, name), name
        assert name in capi.EXPORTS
        assert re.search(r"\b%s\(" % name, header), name
    assert capi.lib().banet_version() == 150              # unchanged: the entries are detected by their symbols
    assert header.index("(5d)") < header.index("/* (5e)") < header.index("/* (6) per-level preparation")
    assert (capi.PRIOR_GRAD_OVERWRITE, capi.PRIOR_GRAD_ACCUMULATE) == (gref.OVERWRITE, gref.ACCUMULATE)
    for name, v in (("BANET_PRIOR_GRAD_OVERWRITE", 1), ("BANET_PRIOR_GRAD_ACCUMULATE", 2)):
        assert re.search(r"#define %s %d\b" % (name, v), header), name


def test_struct_layouts_match_the_header(capi, tmp_path):
    fin = ["gLe", "gee", "Le", "ee", "flags", "reserved_"]
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "banet_hip.h"\nint main(){printf("%zu %zu", '
                    'sizeof(banet_prior_grad_in_t), sizeof(banet_prior_grad_out_t));\n'
                    + "".join('printf(" %%zu", offsetof(banet_prior_grad_in_t, %s));\n' % f for f in fin)
                    + "".join('printf(" %%zu", offsetof(banet_prior_grad_out_t, %s));\n' % f for f in gref.OUTPUTS)
                    + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    I, O = capi.PriorGradIn, capi.PriorGradOut
    assert got == [ctypes.sizeof(I), ctypes.sizeof(O)] + [getattr(I, f).offset for f in fin] + [getattr(O, f).offset for f in gref.OUTPUTS]
    assert [n for n, _ in I._fields_] == fin and [n for n, _ in O._fields_] == list(gref.OUTPUTS)


# ---- the twin against central differences -----------------------------------------------------------------------------------------------
def fd_case(K, pairs, seed, N=40, B=2):
    rng = np.random.default_rng(seed)
    m = 6 * pairs
    P = m + K
    c = dict(depth=1.0 + rng.random((B, N)), basis=rng.standard_normal((B, N, K)) * 0.4, W=rng.standard_normal((B, K)) * 0.3,
             Lambda=rng.standard_normal((B, K, K)), eta=rng.standard_normal((B, K)),          # Lambda: NOT symmetric
             AtA=rng.standard_normal((B, P, P)), Atb=rng.standard_normal((B, P, 1)))
    c["obs"] = c["depth"] + 0.2 * rng.standard_normal((B, N))
    c["weight"] = 0.3 + rng.random((B, N))
    # about a tenth of the points uncounted, by each of the three rules
    kind = rng.integers(0, 30, (B, N))
    c["weight"][kind == 0] = 0.0
    c["weight"][kind == 1] = -0.5
    c["weight"][kind == 2] = np.nan
    c["obs"][kind == 3] = np.inf
    c["cA"], c["cb"] = rng.standard_normal((B, P, P)), rng.standard_normal((B, P, 1))
    return c


@pytest.mark.parametrize("K,pairs", [(5, 1), (5, 2), (33, 1), (33, 2)])
def test_the_twin_matches_central_differences(K, pairs):
    """L = <cA, AtA'> + <cb, Atb'>: central differences along random directions in every input.  L is a polynomial of degree at most
    two along each, so the differences are exact up to rounding; the weights' perturbations stay on their side of w = 0 (counted
    weights are >= 0.3, the step 1e-3 times a direction of size <= 1) and the uncounted points are not moved."""
    c = fd_case(K, pairs, seed=100 * K + pairs)
    scale = 0.7
    ok = gref.counted(c["obs"], c["weight"])
    assert 0.03 < 1.0 - ok.mean() < 0.3
    keys = ("Lambda", "eta", "depth", "basis", "obs", "weight", "W", "AtA", "Atb")

    def loss(scale=scale, **over):
        v = dict(c, **over)
        A2, b2, _, _ = gref.forward(scale, v["Lambda"], v["eta"], v["depth"], v["basis"], v["obs"], v["weight"], v["W"], v["AtA"], v["Atb"], pairs)
        return float((c["cA"] * A2).sum() + (c["cb"] * b2).sum())

    g = gref.backward(scale, c["Lambda"], c["eta"], c["depth"], c["basis"], c["obs"], c["weight"], c["W"], c["cA"], c["cb"], pairs)
    grads = dict(Lambda=g["gLambda"], eta=g["geta"], depth=g["gdepth"], basis=g["gbasis"], obs=g["gobs"], weight=g["gweight"], W=g["gWc"],
                 AtA=g["gAtA"], Atb=g["gAtb"])
    rng = np.random.default_rng(7)
    eps = 1e-3
    ref = max(abs(loss()), 1.0)
    for k in keys:
        for _ in range(3):
            d = rng.uniform(-1, 1, c[k].shape)
            if k in ("obs", "weight"):
                d = np.where(ok, d, 0.0)
            with np.errstate(invalid="ignore"):
                fd = (loss(**{k: c[k] + eps * d}) - loss(**{k: c[k] - eps * d})) / (2 * eps)
            an = float(np.nansum(np.where(d != 0, grads[k].reshape(c[k].shape) * d, 0.0)))
            assert abs(fd - an) <= 1e-8 * max(ref, abs(an)), (k, fd, an)
    fd = (loss(scale=scale + eps) - loss(scale=scale - eps)) / (2 * eps)
    assert abs(fd - g["gscale"].sum()) <= 1e-8 * max(ref, abs(fd)), ("scale", fd, g["gscale"].sum())
    # the uncounted points get exact zeros; Lambda's gradient is the raw one (not symmetrised)
    for k in ("gobs", "gweight", "gdepth"):
        assert not g[k][~ok].any()
    assert not g["gbasis"][~ok].any()
    assert np.abs(g["gLambda"] - g["gLambda"].transpose(0, 2, 1)).max() > 1e-3


def test_the_halves_of_a_prior_each_have_their_gradients():
    c = fd_case(5, 1, seed=3)
    g = gref.backward(0.5, c["Lambda"], None, None, None, None, None, c["W"], c["cA"], c["cb"], 1)
    assert g["gLambda"] is not None and g["geta"] is None and g["gobs"] is None and g["gbasis"] is None and g["gscale"] is not None
    g = gref.backward(0.5, None, None, c["depth"], c["basis"], c["obs"], None, c["W"], c["cA"], c["cb"], 1)
    assert g["gLambda"] is None and g["gweight"] is None and g["gobs"] is not None and g["gbasis"].shape == c["basis"].shape


# ---- prior_grad_plan.hpp, compiled with g++ ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_lib(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("prior_grad_plan")), "libprior_grad_plan_host.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), "-o", out,
                           os.path.join(ROOT, "tests", "native", "prior_grad_plan_host.cpp")])
    L = ctypes.CDLL(out)
    L.banet_test_prior_grad_plan_fields.restype = ctypes.c_char_p
    return L


def plan_rows(L, rows, scales=None):
    names = L.banet_test_prior_grad_plan_fields().decode().split()
    assert names[0] == "desc_ints=12"
    names = names[1:]
    desc = (ctypes.c_int64 * (12 * len(rows)))(*[v for r in rows for v in r])
    sc = (ctypes.c_float * len(rows))(*(scales or [0.5] * len(rows)))
    out = (ctypes.c_int64 * (len(names) * len(rows)))()
    L.banet_test_prior_grad_plan_sweep(desc, sc, len(rows), out)
    return [dict(zip(names, out[i * len(names):(i + 1) * len(names)])) for i in range(len(rows))]


BUNDLE, CAMERA = 3, 2
ALL = {"gLambda": 1, "geta": 2, "gscale": 4, "gobs": 8, "gweight": 16, "gdepth": 32, "gbasis": 64}


def test_sizes_and_offsets_pinned_at_the_abi_shapes(plan_lib):
    """DESIGN.md 2.1, by hand: Gh [B,K,K] then gh [B,K], each at a 256-byte boundary; the image is NR (NR + 1) / 2 blocks of 4 KB
    plus gh padded to 32 NR floats; 2 x 256 / B workgroups per window, capped by the tiles over the kernel's waves"""
    for B, H, W, K, pairs, has in pref.ABI_SHAPES:
        N = H * W
        for which in (0, 1):
            want = (ALL["gscale"] | (ALL["gLambda"] if has[0] else 0) | (ALL["geta"] if has[1] else 0) |
                    ((ALL["gobs"] | ALL["gdepth"] | ALL["gbasis"]) if has[2] else 0) | (ALL["gweight"] if has[3] else 0))
            p = plan_rows(plan_lib, [(B, N, K, pairs, BUNDLE) + tuple(has) + (want, 0, which)])[0]
            NR = (K + 31) // 32
            assert p["rc"] == OK and p["on"] == 1 and (p["coef"], p["eta"], p["obs"], p["weight"]) == tuple(has)
            assert (p["K"], p["m"], p["P"], p["NR"], p["NP"]) == (K, 6 * pairs, 6 * pairs + K, NR, NR * (NR + 1) // 2)
            assert p["off_Gh"] == 0 and p["off_gh"] == up(B * K * K * 4) and p["bytes"] == up(B * K * K * 4) + up(B * K * 4)
            assert p["lds"] == (NR * (NR + 1) // 2 * 1024 + NR * 32) * 4 <= 160 * 1024
            assert p["add_grid"] == (B * K + 3) // 4
            waves = plan_lib.banet_test_prior_grad_threads(NR) // 64
            assert waves == (8 if K <= 128 else 4)
            if has[2]:
                tiles = (N + 31) // 32
                assert p["tiles"] == tiles and p["grid"] == max(1, min((512 + B - 1) // B, (tiles + waves - 1) // waves))
                assert p["pixel"] == which                       # (the query does not know the outputs)
            else:
                assert p["tiles"] == 0 and p["grid"] == 0 and p["pixel"] == 0
    p = plan_rows(plan_lib, [(1, 768, 256, 1, BUNDLE, 1, 1, 1, 1, 127, 0, 1)])[0]
    assert p["lds"] == 36 * 4096 + 1024 == 148480 and p["bytes"] == 262144 + 1024


def test_the_plan_decides_the_refusals(plan_lib):
    full = (1, 1, 1, 1)
    base = (2, 768, 16, 1, BUNDLE)
    rows = [base + full + (127, 0, 1),                    # 0: everything
            base + full + (127, 2, 1),                    # 1: accumulate
            base + (1, 1, 1, 0) + (16, 0, 1),             # 2: gweight without obs_weight
            base + (1, 0, 1, 1) + (2, 0, 1),              # 3: geta without eta
            base + (0, 0, 1, 1) + (1, 0, 1),              # 4: gLambda without Lambda
            base + (1, 1, 0, 0) + (8, 0, 1),              # 5: gobs without obs_depth
            base + (1, 1, 0, 0) + (32, 0, 1),             # 6: gdepth
            base + (1, 1, 0, 0) + (64, 0, 1),             # 7: gbasis
            base + full + (0, 0, 1),                      # 8: no output
            base + full + (1, 4, 1),                      # 9: unknown flag
            base + full + (1, 1, 1),                      # 10: the add's flag
            base + (0, 0, 0, 0) + (4, 0, 1),              # 11: no pointers
            (2, 768, 16, 1, CAMERA) + full + (1, 0, 1),   # 12
            (2, 768, 0, 1, BUNDLE) + full + (1, 0, 1),    # 13
            (2, 768, 257, 1, BUNDLE) + full + (1, 0, 1),  # 14
            (0, 768, 16, 1, BUNDLE) + full + (1, 0, 1),   # 15
            base + (1, 1, 0, 0) + (7, 0, 1),              # 16: coefficients only: no per-pixel launch
            base + full + (7, 0, 1),                      # 17: observations, but no per-pixel output asked for
            base + full + (0, 1, 2), base + full + (0, 0, 2), base + full + (0, 2, 2),        # 18-20: the add's plan
            (2, 768, 16, 1, CAMERA) + full + (0, 0, 2), (2, 768, 16, 2, BUNDLE) + full + (0, 0, 2)]
    p = plan_rows(plan_lib, rows)
    assert [r["rc"] for r in p[:2]] == [OK, OK] and p[0]["pixel"] == 1 and p[1]["pixel"] == 1
    assert [r["rc"] for r in p[2:12]] == [ERR_INVALID_ARG] * 10
    assert [r["rc"] for r in p[12:15]] == [ERR_UNSUPPORTED] * 3 and p[15]["rc"] == ERR_INVALID_ARG
    assert all(r["bytes"] == 0 and r["on"] == 0 for r in p[11:16])
    assert p[16]["rc"] == OK and p[16]["pixel"] == 0 and p[17]["rc"] == OK and p[17]["pixel"] == 0
    assert [r["rc"] for r in p[18:23]] == [OK, OK, ERR_INVALID_ARG, ERR_UNSUPPORTED, OK]
    assert (p[18]["m"], p[18]["P"], p[22]["m"], p[22]["P"]) == (6, 22, 12, 28)
    # scale 0: the empty prior has no backward; a negative scale is (5d)'s refusal
    q = plan_rows(plan_lib, [base + full + (1, 0, 1)] * 3 + [base + full + (1, 0, 0)], scales=[0.0, -1.0, float("nan"), 0.0])
    assert [r["rc"] for r in q] == [ERR_INVALID_ARG] * 3 + [OK] and q[3]["bytes"] > 0       # (the query does not read the scale)


# ---- the entries, through the library, without a device -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sweep(capi):
    return gref.abi_sweep_in_child()


def test_exact_query_accepted_one_byte_less_misaligned_and_null_refused(sweep):
    recs = [r for r in sweep if r["name"].startswith(("prior_terms ", "prior_terms_grad "))]
    assert len(recs) == 2 * len(pref.ABI_SHAPES)
    for r in recs:
        B, N, K = r["shape"][:3]
        has = r["shape"][4:]
        assert r["bytes"] > 0 and r["bytes"] % 256 == 0, r
        if r["name"].startswith("prior_terms_grad "):
            assert r["bytes"] == up(B * K * K * 4) + up(B * K * 4), r
        assert r["exact"] == ERR_LAUNCH, r                  # past every check: fails for lack of a device only
        assert r["minus1"] == ERR_WORKSPACE and r["off4"] == ERR_WORKSPACE and r["null"] == ERR_WORKSPACE, r
        assert len(has) == 4


def test_add_grad_needs_no_workspace_and_checks_its_arguments(sweep):
    recs = [r for r in sweep if r["name"].startswith("prior_add_grad ")]
    assert len(recs) == len(pref.ABI_SHAPES)
    for r in recs:
        assert r["accumulate"] == ERR_LAUNCH and r["overwrite"] == ERR_LAUNCH and r["off4"] == ERR_LAUNCH, r
        assert r["null_Le"] == ERR_INVALID_ARG and r["null_gWc"] == ERR_INVALID_ARG, r
        assert r["bad_flag"] == ERR_INVALID_ARG and r["accumulate_flag"] == ERR_INVALID_ARG, r


def test_every_named_refusal(sweep):
    r = [x for x in sweep if x["name"] == "refusals"][0]
    passes = ("baseline passes the checks", "accumulate passes the checks", "coefficient outputs on a level without depth")
    for what, rc in r["terms_grad"].items():
        assert rc == (ERR_LAUNCH if what in passes else ERR_INVALID_ARG), (what, rc)
    assert len(r["terms_grad"]) >= 22
    for what, d in r["unsupported"].items():
        assert d == dict(terms_grad=ERR_UNSUPPORTED, query=0, add_grad=ERR_UNSUPPORTED, terms=ERR_UNSUPPORTED), (what, d)
    t = r["terms"]
    assert t["NULL Le"] == t["NULL ee"] == t["NULL level"] == t["eta without Lambda"] == ERR_INVALID_ARG
    assert t["observations on a level without depth"] == ERR_INVALID_ARG
    assert t["empty prior"] == OK and t["scale 0"] == OK      # nothing launched, nothing written, no workspace needed
    assert r["add_null_level"] == ERR_INVALID_ARG


def test_python_entries_refuse_cpu_tensors_and_bad_requests(capi):
    import torch
    from banet_amd import ops
    assert ops.PRIOR_GRAD_OUTPUTS == gref.OUTPUTS
    with pytest.raises(capi.BanetError):
        ops.Prior(Lambda=torch.zeros(2, 4, 4))
    for name in ("prior_terms", "prior_add_grad", "prior_terms_grad", "prior_apply_diff"):
        assert callable(getattr(ops, name))
    empty = ops.Prior()
    assert ops._prior_is_empty(empty) and ops._prior_is_empty(None)
    A, b = torch.zeros(1, 8, 8), torch.zeros(1, 8)
    assert ops.prior_apply_diff(None, empty, torch.zeros(1, 2), A, b) == (A, b)      # the empty prior: the inputs themselves
