"""banet_ba_marginals_grad_f32 without a GPU: linkage, the struct mirrors, the argument contract (every refusal is decided before a
launch; the probes that pass every check run in a child process that sees no device and end in BANET_ERR_LAUNCH), the workspace
query, and the references of tests/marginals_grad_ref.py against each other: the closed form against torch autograd through the
definition and against central finite differences of marginals_ref.marginals64, the float32 yardstick, and what the gate catches
(mutations of the closed form)."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import marginals_grad_ref as gr
import marginals_ref as mr

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
os.environ.setdefault("BANET_NUM_CUS", "256")
OK, ERR_INVALID_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED, ERR_LAUNCH = 0, -1, -2, -3, -4
SYMBOLS = ("banet_ba_marginals_grad_workspace_bytes", "banet_ba_marginals_grad_f32")


@pytest.fixture(scope="module")
def capi():
    from banet_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _capi


class Call:
    """an argument set of fake host pointers (checked for NULL, never dereferenced); keyword arguments replace single ones"""

    def __init__(self, capi, B=3, N=200, K=32, pairs=1):
        self.capi, self.L = capi, capi.lib()
        self.host = (ctypes.c_float * 64)()
        self.p = ctypes.cast(self.host, ctypes.c_void_p).value
        self.lv = capi.Level()
        self.lv.B, self.lv.N, self.lv.K, self.lv.pairs, self.lv.basis = B, N, K, pairs, self.p
        self.gin = capi.MarginalsGradIn()
        self.gin.g_pose_cov = self.gin.g_depth_var = self.gin.g_logdet = self.p
        self.out = capi.MarginalsGradOut()
        self.out.gAtA = self.out.gdamping = self.out.gsigma2 = self.out.gbasis = self.out.status = self.p
        self.arena = (ctypes.c_char * 512)()
        self.base = (ctypes.addressof(self.arena) + 255) & ~255

    def query(self, want=1):
        return self.L.banet_ba_marginals_grad_workspace_bytes(ctypes.byref(self.lv), want)

    def __call__(self, lv="lv", AtA="p", gin="gin", out="out", ws="base", nbytes=None):
        return self.L.banet_ba_marginals_grad_f32(ctypes.byref(self.lv) if lv == "lv" else lv, self.p if AtA == "p" else AtA, None, None,
                                                  ctypes.byref(self.gin) if gin == "gin" else gin,
                                                  ctypes.byref(self.out) if out == "out" else out, self.base if ws == "base" else ws,
                                                  self.query() if nbytes is None else nbytes, None)


# ---- linkage ----------------------------------------------------------------------------------------------------------------------
def test_the_library_exports_both_symbols(capi):
    L = ctypes.CDLL(capi.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(L, name), name
    assert capi.lib().banet_version() == 150            # unchanged: the entry is detected by its symbol


def test_capi_exports_and_the_struct_mirrors(capi):
    for name in SYMBOLS:
        assert name in capi.EXPORTS
    assert capi.EXPORTS[SYMBOLS[0]][0] is ctypes.c_size_t and capi.EXPORTS[SYMBOLS[1]][0] is ctypes.c_int
    assert [n for n, _ in capi.MarginalsGradIn._fields_] == ["g_pose_cov", "g_depth_var", "g_logdet"]
    assert [n for n, _ in capi.MarginalsGradOut._fields_] == ["gAtA", "gdamping", "gsigma2", "gbasis", "status"]
    # five and three pointers, no padding: the layout of the header's structs
    assert ctypes.sizeof(capi.MarginalsGradIn) == 3 * ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(capi.MarginalsGradOut) == 5 * ctypes.sizeof(ctypes.c_void_p)
    header = open(os.path.join(ROOT, "include", "banet_hip.h")).read()
    body = lambda name: re.search(r"typedef struct %s \{(.*?)\} %s_t;" % (name, name), header, re.S).group(1)
    assert re.findall(r"\*\s*(\w+);", body("banet_marginals_grad_in")) == [n for n, _ in capi.MarginalsGradIn._fields_]
    assert re.findall(r"\*\s*(\w+);", body("banet_marginals_grad_out")) == [n for n, _ in capi.MarginalsGradOut._fields_]
    assert re.search(r"size_t\s+banet_ba_marginals_grad_workspace_bytes\(const banet_level_t\*\s*lv,\s*int want_gbasis\);", header)


# ---- the argument contract ----------------------------------------------------------------------------------------------------------
def test_null_and_shape_errors_are_invalid_arg(capi):
    c = Call(capi)
    assert c(lv=None) == ERR_INVALID_ARG
    assert c(AtA=None) == ERR_INVALID_ARG
    assert c(gin=None) == ERR_INVALID_ARG
    assert c(out=None) == ERR_INVALID_ARG
    c.out.status = None
    assert c() == ERR_INVALID_ARG
    for B in (0, -1):
        c = Call(capi, B=B)
        assert c(nbytes=4096) == ERR_INVALID_ARG and c.query() == 0
    for field, v in (("K", -1), ("pairs", -1)):
        c = Call(capi)
        setattr(c.lv, field, v)
        assert c(nbytes=4096) == ERR_INVALID_ARG and c.query() == 0
    # the basis and N are needed exactly when K > 0 and g_depth_var or gbasis is given
    for drop in ((), ("g_depth_var",), ("gbasis",)):
        for broken in ("basis", "N"):
            c = Call(capi)
            if broken == "basis":
                c.lv.basis = None
            else:
                c.lv.N = 0
            for name in drop:
                setattr(c.gin if name.startswith("g_") else c.out, name, None)
            assert c() == ERR_INVALID_ARG, (drop, broken)
    c = Call(capi, N=0)
    c.lv.basis = None
    c.gin.g_depth_var = c.out.gbasis = None             # neither: not needed (refused later, by the workspace)
    assert c(ws=None) == ERR_WORKSPACE
    c = Call(capi, K=0, N=0)                            # K = 0: g_depth_var / gbasis are ignored
    c.lv.basis = None
    assert c.query() > 0 and c(ws=None) == ERR_WORKSPACE


def test_unsupported_shapes_and_the_query(capi):
    for K, pairs in ((256, 1), (257, 1), (256, 8), (255, 8), (251, 9), (0, 50), (0, 51), (5, 50)):
        c = Call(capi, K=K, pairs=pairs)
        ok = K <= 256 and 6 * max(pairs, 1) + K <= 304
        for want in (0, 1):
            nb = c.query(want)
            assert (nb > 0) == ok and nb % 256 == 0, (K, pairs, want)     # 0 exactly for K > 256 or P > 304
        if not ok:
            assert c(nbytes=1 << 30) == ERR_UNSUPPORTED
    assert capi.lib().banet_ba_marginals_grad_workspace_bytes(None, 1) == 0
    assert Call(capi, K=32, pairs=0).query() == Call(capi, K=32, pairs=1).query()
    # the layout (MargGradPlan): M's partial rows and M, T when gbasis is wanted, Hinv (packed triangle) and X [P][P] in doubles,
    # Y's triangle only where it does not fit the LDS: P (P + 1) / 2 + 2 P doubles against 160 KB -> in LDS up to P = 199
    up = lambda n: (n + 255) // 256 * 256
    for B, N, K, pairs in ((3, 200, 32, 1), (2, 4801, 128, 4), (3, 77, 193, 1), (3, 77, 194, 1), (2, 100000, 256, 8), (3, 10, 0, 1)):
        c = Call(capi, B=B, N=N, K=K, pairs=pairs)
        P = 6 * pairs + K
        tri = P * (P + 1) // 2
        assert (tri * 8 + 2 * P * 8 > 160 * 1024) == (P >= 200)
        rows = min((N + 255) // 256, 64)
        chunk = ((N + rows - 1) // rows + 1) // 2 * 2
        rows = (N + chunk - 1) // chunk
        NR = (K + 31) // 32
        common = up(B * rows * NR * (NR + 1) // 2 * 1024 * 4) + up(B * K * K * 4) if K else 0
        tail = up(B * tri * 8) + up(B * P * P * 8) + (up(B * tri * 8) if P >= 200 else 0)
        assert c.query(0) == common + tail, (B, N, K, pairs)
        assert c.query(1) == common + (up(B * K * K * 4) if K else 0) + tail, (B, N, K, pairs)


PROBE = r'''
import ctypes, json, sys
sys.path[:0] = [%r, %r]
import test_marginals_grad_cpu as t
from banet_amd import _capi as capi
out = []
for B, N, K, pairs in ((3, 200, 32, 1), (1, 1, 1, 1), (2, 4801, 128, 4), (3, 77, 193, 1), (3, 77, 194, 1), (2, 63, 256, 8), (3, 10, 0, 1)):
    for drop in ((), ("g_depth_var", "gbasis"), ("g_pose_cov", "g_logdet", "gAtA", "gdamping", "gsigma2")):
        c = t.Call(capi, B, N, K, pairs)
        for name in drop:
            setattr(c.gin if name.startswith("g_") else c.out, name, None)
        nb = c.query(int("gbasis" not in drop))
        out.append(dict(shape=[B, N, K, pairs], bytes=nb, exact=c(nbytes=nb), minus1=c(nbytes=nb - 1), off4=c(ws=c.base + 4, nbytes=nb),
                        null=c(ws=None, nbytes=nb), bigger=c(nbytes=nb + 4096)))
print("PROBE " + json.dumps(out))
'''


def test_workspace_probes_without_a_device(capi):
    """exact query / one byte less / pointer off by 4 / NULL, in a child process that sees no device: a valid call passes every
    check and fails at the launch (never an argument or workspace error), the others are BANET_ERR_WORKSPACE"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="", BANET_NUM_CUS="256")
    r = subprocess.run([sys.executable, "-c", PROBE % (ROOT, os.path.join(ROOT, "tests"))], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    recs = json.loads([l for l in r.stdout.splitlines() if l.startswith("PROBE ")][-1][6:])
    assert len(recs) == 21
    for rec in recs:
        assert rec["bytes"] > 0 and rec["bytes"] % 256 == 0, rec
        assert rec["exact"] == ERR_LAUNCH and rec["bigger"] == ERR_LAUNCH, rec
        assert [rec[k] for k in ("minus1", "off4", "null")] == [ERR_WORKSPACE] * 3, rec


def test_python_entries_refuse_cpu_tensors(capi):
    import torch
    from banet_amd import ops
    holder = type("Bare", (), {})()
    holder.c = capi.Level()
    holder.c.B, holder.c.N, holder.c.K, holder.c.pairs = 2, 10, 0, 1
    with pytest.raises(capi.BanetError):
        ops.ba_marginals_grad(holder, torch.eye(6).repeat(2, 1, 1), g_logdet=torch.ones(2))
    assert ops.MarginalsGrad._fields == ("gAtA", "gdamping", "gsigma2", "gbasis", "status")
    assert "ba_marginals_grad" in open(os.path.join(ROOT, "banet_amd", "ops.py")).read()


# ---- the references -----------------------------------------------------------------------------------------------------------------
def show(tag, e, g=None):
    print(tag + ": " + "  ".join("%s %.2e%s" % (k, e[k], "" if g is None else " (gate %.2e)" % g[k]) for k in gr.ERRORS))


SUBSET = [s for s in mr.LADDER if s[3] in (1e2, 1e6) and s[4] and s[5]]          # all shapes at kappa = 1e2 and 1e6, damped, scaled


@pytest.mark.parametrize("spec", SUBSET, ids=mr.spec_id)
def test_closed_form_equals_autograd_through_the_definition(spec):
    """float64 against float64: both lose at most cond(H) 2^-53 of an entry's scale; cond(H) <= kappa e^8 = 3e9 on the ladder
    (column scales e^+-2 on both sides), so 3e-7 bounds the difference -- still forty times under the lowest gate (1.2e-5).
    Measured: 4e-11 at worst."""
    case = mr.make("ladder", spec, 0)
    ups, want, yard = gr.reference(case)
    e = gr.errors(case, ups, gr.autograd_ref(case, ups), want)
    show(mr.spec_id(spec), e)
    for k in gr.ERRORS:
        assert e[k] <= 3e-7, (k, e[k])


@pytest.mark.parametrize("spec", [(6, 1, 0, 1e2, True, True), (7, 1, 1, 1e2, True, True)], ids=mr.spec_id)
def test_closed_form_equals_central_differences_of_marginals64(spec):
    """L = <g_cov, pose_cov> + <g_dv, depth_var> + g_ld logdet through marginals_ref.marginals64, central differences with a
    relative step of 1e-6 (error ~ step^2 + 1e-16 / step ~ 1e-10 relative to the loss; asserted at 1e-6 of the gradient's scale).
    marginals64 reads the lower triangle of AtA: an off-diagonal entry of it moves both halves, d L = 2 gAtA[i,j]."""
    case = mr.make("ladder", spec, 0)
    ups, want, _ = gr.reference(case)
    B, P, K, N = case["B"], case["P"], case["K"], case["N"]

    def loss(c):
        m64 = mr.marginals64(c)
        s = (ups["g_cov"] * m64["pose_cov"]).sum((1, 2)) + ups["g_ld"] * m64["logdet"]
        return s + (ups["g_dv"] * m64["depth_var"]).sum(1) if K > 0 else s

    def fd(name, index):
        x = np.array(case[name], np.float64)
        h = 1e-6 * max(abs(x[index]), 1e-3)
        hi, lo = x.copy(), x.copy()
        hi[index] += h
        lo[index] -= h
        return (loss(dict(case, **{name: hi})) - loss(dict(case, **{name: lo})))[index[0]] / (2 * h)

    for b in range(B):
        scale = np.abs(want["gAtA"][b]).max()
        for i in range(P):
            for j in range(i + 1):
                d = fd("AtA", (b, i, j))
                w = want["gAtA"][b, i, j] * (1.0 if i == j else 2.0)
                assert abs(d - w) <= 1e-6 * scale, (b, i, j, d, w)
        assert abs(fd("damping", (b,)) - want["gdamping"][b]) <= 1e-6 * want["scale_damping"][b]
        assert abs(fd("sigma2", (b,)) - want["gsigma2"][b]) <= 1e-6 * want["scale_sigma2"][b]
        for n in range(0, N, 37) if K > 0 else ():
            for k in range(K):
                assert abs(fd("basis", (b, n, k)) - want["gbasis"][b, n, k]) <= 1e-6 * max(np.abs(want["gbasis"][b]).max(), 1e-30)


@pytest.mark.parametrize("shape", mr.LADDER_SHAPES, ids=lambda s: "P%d-pairs%d-K%d" % s)
def test_the_yardstick_stays_finite_on_every_ladder_case(shape):
    for spec in mr.LADDER:
        if spec[:3] != shape:
            continue
        case = mr.make("ladder", spec, 0)
        ups, want, yard = gr.reference(case)
        assert all(np.isfinite(yard[k]) for k in gr.ERRORS), (spec, yard)
        assert all(np.all(np.isfinite(want[k])) for k in gr.OUTPUTS)
        assert list(want["status"]) == [0] * case["B"]


@pytest.mark.parametrize("shape", mr.LADDER_SHAPES, ids=lambda s: "P%d-pairs%d-K%d" % s)
def test_the_gate_catches_each_mutation_of_the_closed_form(shape):
    """no (1 + mu) on the diagonal / g_cov not symmetrised / the factor 2 of gbasis dropped / the logdet term dropped / M from
    |g| / one 32 x 32 block of M zeroed: each exceeds the gate of some output (kappa = 1e2, damped, scaled; the last four need K > 0)"""
    case = mr.make("ladder", shape + (1e2, True, True), 0)
    ups, want, yard = gr.reference(case)
    gate = gr.gates(case, yard)
    for mut in gr.MUTATIONS:
        if case["K"] == 0 and mut in ("gbasis_no2", "abs_g", "zero_block"):
            continue
        e = gr.errors(case, ups, gr.closed_form(case, ups, mutate=mut), want)
        worst = max(e[k] / gate[k] for k in gr.ERRORS)
        print("%s %s: worst error / gate %.3g" % (mr.spec_id(case["spec"]), mut, worst))
        assert worst > 1.0, (mut, e, gate)


def test_gates_never_fall_below_the_dot_product_bound():
    case = mr.make("ladder", (38, 1, 32, 1e2, True, True), 0)
    g = gr.gates(case, dict.fromkeys(gr.ERRORS, 0.0))
    assert all(v == (38 + 200) * 2.0 ** -24 for v in g.values())
    g = gr.gates(case, dict.fromkeys(gr.ERRORS, 1.0))
    assert all(v == 4.0 for v in g.values())
