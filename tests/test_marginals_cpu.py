"""banet_ba_marginals_f32 / banet_ba_marginals_workspace_bytes on the host (include/banet_hip.h (3d)) and the references of
tests/marginals_ref.py.  No GPU: every call is refused by the host-side checks before anything could be launched -- except the
probe with the exact workspace size, which runs in a child process that sees no device (as tests/ws_contract.py does) and fails
there for lack of one.

The conditions the GPU module relies on, for every ladder / indefinite case and seed:
  * the float32 yardstick (marginals32) succeeds on every window expected to succeed and raises LinAlgError on the indefinite one;
  * lambda_min(H) <= -1e-3 lambda_max (float64) on the indefinite window;
  * lambda_min >= 1e-8 lambda_max (float64) on every other window -- of H with the family's column scales D taken out again,
    D^-1 H D^-1 = Q diag(s) Q^T (+ damping).  On H itself the bound cannot hold for the family as specified: D = exp(U(-2, 2))
    alone spreads the spectrum by up to e^8, and the kappa = 1e6 cases measure lambda_min / lambda_max = 3e-9 .. 2e-8 (printed by
    the test).  What a Cholesky factorisation's success and the scaled error measures of the GPU module depend on is the
    conditioning after diagonal equilibration (the factorisation commutes with a diagonal scaling up to rounding), which is what
    taking D out measures.
"""
import ctypes
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import marginals_ref as mr
import ws_contract as wsc

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
os.environ.setdefault("BANET_NUM_CUS", "256")
OK, ERR_INVALID_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED, ERR_LAUNCH = 0, -1, -2, -3, -4
SYMBOLS = ("banet_ba_marginals_workspace_bytes", "banet_ba_marginals_f32")


@pytest.fixture(scope="module")
def capi():
    from banet_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _capi


def bare_level(capi, B, N, K, pairs, basis=None):
    """the fields the entry reads and nothing else (tests/solve_cases.bare_level plus the basis pointer)"""
    lv = capi.Level()
    lv.B, lv.N, lv.K, lv.pairs = B, N, K, pairs
    lv.basis = basis
    return lv


class Call:
    """an argument set of fake host pointers (checked for NULL, never dereferenced); keyword arguments replace single ones"""

    def __init__(self, capi, B=3, N=200, K=32, pairs=1):
        self.capi, self.L = capi, capi.lib()
        self.host = (ctypes.c_float * 64)()
        self.p = ctypes.cast(self.host, ctypes.c_void_p).value
        self.lv = bare_level(capi, B, N, K, pairs, self.p)
        self.out = capi.MarginalsOut()
        self.out.pose_cov = self.out.depth_var = self.out.wfactor = self.out.logdet = self.out.status = self.p
        self.arena = (ctypes.c_char * 512)()
        self.base = (ctypes.addressof(self.arena) + 255) & ~255

    def query(self, want=1):
        return self.L.banet_ba_marginals_workspace_bytes(ctypes.byref(self.lv), want)

    def __call__(self, lv="lv", AtA="p", out="out", ws="base", nbytes=None):
        return self.L.banet_ba_marginals_f32(ctypes.byref(self.lv) if lv == "lv" else lv, self.p if AtA == "p" else AtA, None, None,
                                             ctypes.byref(self.out) if out == "out" else out, self.base if ws == "base" else ws,
                                             self.query() if nbytes is None else nbytes, None)


# ---- linkage ----------------------------------------------------------------------------------------------------------------------
def test_the_library_exports_both_symbols(capi):
    L = ctypes.CDLL(capi.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(L, name), name
    assert capi.lib().banet_version() == 150            # unchanged: the entry is detected by its symbol


def test_capi_exports_and_the_struct_mirror(capi):
    for name in SYMBOLS:
        assert name in capi.EXPORTS
    assert capi.EXPORTS[SYMBOLS[0]][0] is ctypes.c_size_t and capi.EXPORTS[SYMBOLS[1]][0] is ctypes.c_int
    assert [n for n, _ in capi.MarginalsOut._fields_] == ["pose_cov", "depth_var", "wfactor", "logdet", "status"]


def test_the_header_declares_them_and_compiles_as_c99(capi, tmp_path):
    """a C99 translation unit sizes a workspace, is refused on the host, and the struct layout equals the ctypes mirror"""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    header = open(os.path.join(ROOT, "include", "banet_hip.h")).read()
    assert re.search(r"size_t\s+banet_ba_marginals_workspace_bytes\(const banet_level_t\*\s*lv,\s*int want_depth_var\);", header)
    assert re.search(r"int\s+banet_ba_marginals_f32\(", header) and "size_t workspace_bytes, banet_stream_t stream);" in header
    fields = [n for n, _ in capi.MarginalsOut._fields_]
    src = tmp_path / "t.c"
    src.write_text('''#include <stdio.h>
#include <stddef.h>
#include <string.h>
#include "banet_hip.h"
int main(void) {
  static float dummy[4];
  static int32_t status[4];
  banet_level_t lv;
  banet_marginals_out_t out;
  size_t need;
  memset(&lv, 0, sizeof lv); memset(&out, 0, sizeof out);
  lv.B = 2; lv.N = 100; lv.K = 32; lv.pairs = 1; lv.basis = dummy;
  out.pose_cov = dummy; out.status = status;
  need = banet_ba_marginals_workspace_bytes(&lv, 1);
  if (need == 0 || need % 256 != 0) return 1;
  if (banet_ba_marginals_f32(&lv, 0, 0, 0, &out, 0, need, 0) != BANET_ERR_INVALID_ARG) return 2;
  if (banet_ba_marginals_f32(&lv, dummy, 0, 0, &out, 0, need, 0) != BANET_ERR_WORKSPACE) return 3;
  lv.K = 257;
  if (banet_ba_marginals_workspace_bytes(&lv, 1) != 0) return 4;
  if (banet_version() != BANET_VERSION) return 5;
  printf("%zu''' + "".join(" %zu" for _ in fields) + '''\\n", sizeof(banet_marginals_out_t)''' +
                   "".join(", offsetof(banet_marginals_out_t, %s)" % n for n in fields) + ''');
  return 0;
}
''')
    libdir = os.path.join(ROOT, "banet_amd", "lib")
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-lbanet_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    got = [int(v) for v in subprocess.check_output([str(exe)], env=dict(os.environ, BANET_NUM_CUS="256")).split()]
    assert got == [ctypes.sizeof(capi.MarginalsOut)] + [getattr(capi.MarginalsOut, n).offset for n in fields]


# ---- the argument contract ----------------------------------------------------------------------------------------------------------
def test_null_and_shape_errors_are_invalid_arg(capi):
    c = Call(capi)
    assert c(lv=None) == ERR_INVALID_ARG
    assert c(AtA=None) == ERR_INVALID_ARG
    assert c(out=None) == ERR_INVALID_ARG
    for field in ("pose_cov", "status"):
        c = Call(capi)
        setattr(c.out, field, None)
        assert c() == ERR_INVALID_ARG, field
    c = Call(capi)
    c.lv.basis = None                                   # depth_var requested, K > 0, no basis
    assert c() == ERR_INVALID_ARG
    c.out.depth_var = None                              # ... not requested: the basis is not needed (refused later, by the workspace)
    assert c(ws=None) == ERR_WORKSPACE
    c = Call(capi, N=0)                                 # N < 1 with depth_var requested
    assert c() == ERR_INVALID_ARG
    c.out.depth_var = None
    assert c(ws=None) == ERR_WORKSPACE
    for B in (0, -1):
        c = Call(capi, B=B)
        assert c(nbytes=4096) == ERR_INVALID_ARG and c.query() == 0
    # K = 0: depth_var / wfactor are ignored, so neither the basis nor N is looked at
    c = Call(capi, K=0, N=0)
    c.lv.basis = None
    assert c.query() > 0 and c(ws=None) == ERR_WORKSPACE


def test_unsupported_shapes_and_the_query(capi):
    for K, pairs, ok in ((256, 1, True), (257, 1, False), (256, 8, True), (255, 8, True), (251, 9, False), (0, 50, True), (0, 51, False),
                         (5, 50, False)):
        c = Call(capi, K=K, pairs=pairs)
        P = 6 * max(pairs, 1) + K
        assert ok == (K <= 256 and P <= 304)
        for want in (0, 1):
            assert (c.query(want) > 0) == ok, (K, pairs, want)
        if not ok:                                       # (supported shapes: probed in the child process below)
            assert c(nbytes=1 << 30) == ERR_UNSUPPORTED
    assert Call(capi, K=257, pairs=1).query() == 0       # K = 257
    assert Call(capi, K=251, pairs=9).query() == 0       # P = 305
    assert Call(capi, K=32, pairs=0).query() == Call(capi, K=32, pairs=1).query()   # pairs 0 = the two-frame case
    assert capi.lib().banet_ba_marginals_workspace_bytes(None, 1) == 0
    # the query: 256-byte multiples, never 0 for a supported shape; T [B,K,K] only when depth_var is wanted; the matrix only where
    # it does not fit the LDS (P = 262, 298, 304 of the project's shapes)
    up = lambda n: (n + 255) // 256 * 256
    for B, K, pairs in ((3, 32, 1), (2, 128, 4), (3, 184, 1), (3, 193, 1), (3, 194, 1), (3, 256, 1), (2, 256, 7), (2, 256, 8), (3, 0, 1)):
        c = Call(capi, B=B, K=K, pairs=pairs)
        with_dv, without = c.query(1), c.query(0)
        P = 6 * pairs + K
        big = up(B * (P * (P + 1) // 2) * 8) if P >= 200 else 0       # the packed triangle in doubles: in LDS up to P = 199
        assert without == max(big, 256), (B, K, pairs)
        assert with_dv == max(up(B * K * K * 4) + big, 256), (B, K, pairs)


PROBE = r'''
import ctypes, json, sys
sys.path[:0] = [%r, %r]
import test_marginals_cpu as t
from banet_amd import _capi as capi
out = []
for B, N, K, pairs in ((3, 200, 32, 1), (1, 1, 1, 1), (2, 4801, 128, 4), (3, 77, 184, 1), (3, 1000, 256, 1), (2, 63, 256, 8), (3, 10, 0, 1), (2, 10, 0, 8)):
    c = t.Call(capi, B, N, K, pairs)
    nb = c.query()
    out.append(dict(shape=[B, N, K, pairs], bytes=nb, exact=c(), minus1=c(nbytes=nb - 1), off4=c(ws=c.base + 4), null=c(ws=None),
                    bigger=c(nbytes=nb + 4096)))
print("PROBE " + json.dumps(out))
'''


def test_workspace_probes_without_a_device(capi):
    """exact query / one byte less / pointer off by 4 / NULL, in a child process that sees no device: the exact size passes every
    check and fails at the launch, the others are BANET_ERR_WORKSPACE"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="", BANET_NUM_CUS="256")
    r = subprocess.run([sys.executable, "-c", PROBE % (ROOT, os.path.join(ROOT, "tests"))], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    recs = json.loads([l for l in r.stdout.splitlines() if l.startswith("PROBE ")][-1][6:])
    assert len(recs) == 8
    for rec in recs:
        assert rec["bytes"] > 0 and rec["bytes"] % 256 == 0, rec
        assert rec["exact"] == wsc.ERR_LAUNCH and rec["bigger"] == wsc.ERR_LAUNCH, rec
        assert [rec[k] for k in ("minus1", "off4", "null")] == [wsc.ERR_WORKSPACE] * 3, rec


def test_python_entry_refuses_cpu_tensors(capi):
    import torch
    from banet_amd import ops
    holder = type("Bare", (), {})()
    holder.c = bare_level(capi, 2, 10, 0, 1)
    with pytest.raises(capi.BanetError):
        ops.ba_marginals(holder, torch.eye(6).repeat(2, 1, 1))


# ---- the references -----------------------------------------------------------------------------------------------------------------
WELL = [s for s in mr.LADDER if s[3] <= 1e2 and s[0] in (6, 7, 38, 152, 304)]


@pytest.mark.parametrize("spec", WELL, ids=mr.spec_id)
def test_marginals64_is_the_blocks_of_the_inverse(spec):
    """pose_cov = sigma2 inv(H)[:m,:m]; depth_var = b^T Sigma_WW b with Sigma_WW = sigma2 T^T T = the trailing block of Sigma;
    logdet = slogdet(H): to 1e-9 on the scales of marginals_ref.errors"""
    case = mr.make("ladder", spec, mr.SEEDS[0])
    got = mr.marginals64(case)
    H = mr.damped(case)
    m, K = 6 * case["pairs"], case["K"]
    want = dict(pose_cov=[], depth_var=[], wfactor=[], logdet=[])
    for b in range(case["B"]):
        s2 = 1.0 if case["sigma2"] is None else case["sigma2"][b]
        S = s2 * np.linalg.inv(H[b])
        want["pose_cov"].append(S[:m, :m])
        want["depth_var"].append(np.einsum("nk,kl,nl->n", case["basis"][b], S[m:, m:], case["basis"][b]))
        want["logdet"].append(np.linalg.slogdet(H[b])[1])
        if K:
            T = got["wfactor"][b]
            assert np.all(np.triu(T, 1) == 0)
            assert np.abs(s2 * T.T @ T - S[m:, m:]).max() <= 1e-9 * np.abs(S[m:, m:]).max()
    want["wfactor"] = got["wfactor"]
    assert np.all(got["status"] == 0)
    e = mr.errors(case, got, {k: np.stack(v) if isinstance(v, list) else v for k, v in want.items()})
    print(mr.spec_id(spec), e)
    assert max(e.values()) <= 1e-9, e


UNIQUE = sorted({s[:5] for s in mr.LADDER})     # the conditions do not depend on sigma2


@pytest.mark.parametrize("shape", mr.LADDER_SHAPES, ids=lambda s: "P%d-pairs%d-K%d" % s)
def test_ladder_conditions(shape):
    worst_raw = 1.0
    for spec5 in UNIQUE:
        if spec5[:3] != shape:
            continue
        spec = spec5 + (True,)
        for seed in mr.SEEDS:
            case = mr.make("ladder", spec, seed)
            rs = mr._rng(spec, seed)
            H = mr.damped(case)
            for b in range(case["B"]):
                # the generator's own draws again, for D (same stream as marginals_ref._ladder_matrix)
                P, kappa = spec[0], spec[3]
                rs.standard_normal((P, P)); rs.uniform(0.0, 1.0, P)
                D = np.exp(rs.uniform(-2.0, 2.0, P))
                w = np.linalg.eigvalsh(H[b])
                worst_raw = min(worst_raw, w[0] / w[-1])
                we = np.linalg.eigvalsh(H[b] / np.outer(D, D))
                assert we[0] >= 1e-8 * we[-1], (mr.spec_id(spec), seed, b, we[0] / we[-1])
                out = mr.marginals32_window(case, b)      # raises LinAlgError if the float32 factorisation fails
                assert out["status"] == 0 and np.all(np.isfinite(out["pose_cov"])) and np.all(out["depth_var"] >= 0)
    print("P%d pairs%d K%d" % shape, "smallest lambda_min / lambda_max of H itself: %.2e" % worst_raw)


@pytest.mark.parametrize("spec", mr.INDEFINITE, ids=mr.spec_id)
def test_indefinite_conditions(spec):
    for seed in mr.SEEDS:
        case = mr.make("indefinite", spec, seed)
        w = mr.spectrum(case)
        for b in range(case["B"]):
            if case["expect_fail"][b]:
                assert b == 1 and w[b, 0] <= -1e-3 * w[b, -1]
                with pytest.raises(np.linalg.LinAlgError):
                    mr.marginals32_window(case, b)
            else:
                assert w[b, 0] > 0
                assert mr.marginals32_window(case, b)["status"] == 0
        ref = mr.marginals64(case)
        assert list(ref["status"]) == [0, 1, 0]
        assert np.all(np.isinf(ref["depth_var"][1])) and ref["logdet"][1] == -np.inf and np.all(ref["wfactor"][1] == 0)
        assert np.all(np.isinf(np.diag(ref["pose_cov"][1]))) and np.count_nonzero(ref["pose_cov"][1]) == 6 * case["pairs"]


def test_gates_never_fall_below_the_dot_product_bound():
    case = mr.make("ladder", (38, 1, 32, 10.0, False, False), 0)
    g = mr.gates(case, dict.fromkeys(mr.OUTPUTS, 0.0))
    assert all(v == 38 * 2.0 ** -24 for v in g.values())
    g = mr.gates(case, dict.fromkeys(mr.OUTPUTS, 1e-5))
    assert all(v == 4e-5 for v in g.values())
