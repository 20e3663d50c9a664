"""EquationConstruction / EquationConstructionGrad on the GPU through the C ABI, entry by entry against the float64 oracle on the
table of eqcon_cases.py (`-m gpu`; the table's own conditions: test_eqcon_cases_cpu.py).

Every case, both ops: the outputs are NaN-filled before the call (the forward's whole P x P matrix, lower triangle included) and
the workspace holds NaN bit patterns; after it every entry is finite, within GATE[output] = 4 x the float32 twin's worst err of
its own scale, and exactly 0 where the scale is 0; AtA is bit-symmetric; a second call gives the same bits.  The backward runs
twice: with its workspace (the matrix-pipe kernels of eqcon_grad.hip) and with ws = NULL (eq_construction_grad_kernel, eqcon.hip),
both under the same gate.  The two environment forms of the forward (BANET_EQ_LDS_KERNEL=1, BANET_EQ_FOUR_PASS=1) are read once
into statics, so each runs in one fresh child process that saves its outputs; the parent gates them with the same function.

P = 305: the forward's workspace query is 0 and the call is BANET_ERR_UNSUPPORTED with its outputs untouched.  The backward's query
is 0 as well, which by the header selects the first-generation kernel: that one runs while its J and U tiles fit the LDS (P <= 313)
and is gated here at 305; at P = 314 the call is BANET_ERR_UNSUPPORTED with its outputs untouched.

Every figure is printed as an `EQCON` line (pytest -s); profiles/eqcon_entrywise.txt is such a run, next to the twin's figures
of test_eqcon_cases_cpu.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import eqcon_cases as ec

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
IDS = [ec.case_id(c) for c in ec.TABLE]
ERR_UNSUPPORTED = -3
FOUR_PASS_CASES = tuple(c for c in ec.TABLE if ec.fwd_class(c.P) == 17)
CHILD_TIMEOUT = 600
_child_died = []          # a child process that ended by signal or at its timeout: the other child is not started


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from banet_amd import _capi
    _capi.lib()                                   # fail loudly if the HIP library is missing


def _dev(x):
    return torch.from_numpy(np.array(x, order="C")).to(DEV)       # (a copy: the table's arrays are read-only)


def _nan(shape):
    return torch.full(tuple(shape), float("nan"), dtype=torch.float32, device=DEV)


def _nan_ws(nbytes):
    from banet_amd import _capi as capi
    ws = capi.workspace(nbytes, DEV)
    ws.fill_(0xFF)                                # every float of it a NaN
    return ws


def gpu_forward(c, calls=2):
    """-> list of (AtA, Atb) numpy pairs, one per call; every call into NaN-filled outputs and a NaN-filled workspace"""
    from banet_amd import _capi as capi
    L = capi.lib()
    inp = ec.make(c)
    J, G, d = _dev(inp["J"]), _dev(inp["G"]), _dev(inp["d"])
    nb = L.banet_equation_construction_workspace_bytes(c.B, c.N, c.C, c.P)
    assert nb > 0
    outs = []
    for _ in range(calls):
        AtA, Atb, ws = _nan((c.B, c.P, c.P)), _nan((c.B, c.P, 1)), _nan_ws(nb)
        capi.check(L.banet_equation_construction_f32(capi.ptr(J), capi.ptr(G), capi.ptr(d), capi.ptr(AtA), capi.ptr(Atb), c.B, c.N, c.C,
                                                     c.P, ctypes.c_void_p(ws.data_ptr()), ws.numel(), capi.stream()))
        outs.append((AtA, Atb))
    torch.cuda.synchronize()
    return [(a.cpu().numpy(), b.cpu().numpy()) for a, b in outs]


def gpu_backward(c, use_ws, calls=2):
    """-> list of (dJ, dG, dd) numpy triples; use_ws: the matrix-pipe kernels, else ws = NULL: the first-generation kernel"""
    from banet_amd import _capi as capi
    L = capi.lib()
    inp = ec.make(c)
    J, G, d, g0, g1 = (_dev(inp[k]) for k in ("J", "G", "d", "g0", "g1"))
    nb = L.banet_equation_construction_grad_workspace_bytes(c.B, c.N, c.C, c.P)
    assert nb > 0
    outs = []
    for _ in range(calls):
        o = [_nan(x.shape) for x in (J, G, d)]
        ws = _nan_ws(nb) if use_ws else None
        capi.check(L.banet_equation_construction_grad_f32(capi.ptr(J), capi.ptr(G), capi.ptr(d), capi.ptr(g0), capi.ptr(g1),
                                                          capi.ptr(o[0]), capi.ptr(o[1]), capi.ptr(o[2]), c.B, c.N, c.C, c.P,
                                                          ctypes.c_void_p(ws.data_ptr()) if use_ws else None,
                                                          ws.numel() if use_ws else 0, capi.stream()))
        outs.append(o)
    torch.cuda.synchronize()
    return [tuple(x.cpu().numpy() for x in o) for o in outs]


def _same_bits(a, b):
    return np.array_equal(a.view(np.int32), b.view(np.int32))


def _report(form, c, errors, op=None):
    print("\nEQCON %-14s %-30s %s" % (form, ec.case_id(c), "  ".join(
        "%s gpu %.3e at %s gate %.3e" % (k, e.worst, "/".join(map(str, e.index)), ec.GATE[k]) for k, e in errors.items())))


def check_forward(form, c, AtA, Atb):
    """the assertions of one forward result (this process's, or a child's)"""
    errors = ec.forward_errors(c, AtA, Atb)
    _report(form, c, errors, "fwd")
    blocks = ec.block_errors(AtA, ec.want_forward(c)["AtA"], ec.scale_forward(c)["AtA"])
    bi, bj = np.unravel_index(int(np.argmax(blocks)), blocks.shape)
    print("EQCON %-14s %-30s AtA worst 16x16 block (%d, %d) of %d x %d: %.3e" % (form, ec.case_id(c), bi, bj, blocks.shape[0], blocks.shape[1],
                                                                                 blocks[bi, bj]))
    assert np.isfinite(AtA).all() and np.isfinite(Atb).all()
    assert ec.gate_failures(errors) == []
    assert _same_bits(AtA, np.ascontiguousarray(np.swapaxes(AtA, 1, 2)))              # bit-symmetric
    assert blocks.max() == errors["AtA"].worst


# ---- this process: the library's own dispatch ------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ec.TABLE, ids=IDS)
def test_forward_entry_by_entry(c):
    (A1, b1), (A2, b2) = gpu_forward(c)
    assert A1.shape == (c.B, c.P, c.P) and b1.shape == (c.B, c.P, 1)
    check_forward("fwd", c, A1, b1)
    assert _same_bits(A1, A2) and _same_bits(b1, b2)                                  # two calls: equal bits


@pytest.mark.parametrize("use_ws", (True, False), ids=("ws", "null"))
@pytest.mark.parametrize("c", ec.TABLE, ids=IDS)
def test_backward_entry_by_entry(c, use_ws):
    assert ec.null_form_lds(c.P) <= ec.LDS_BYTES                                      # (every table case fits the first-generation kernel)
    first, second = gpu_backward(c, use_ws)
    errors = ec.backward_errors(c, *first)
    _report("bwd-ws" if use_ws else "bwd-null", c, errors, "bwd")
    for x in first:
        assert np.isfinite(x).all()
    assert ec.gate_failures(errors) == []
    for x, y in zip(first, second):
        assert _same_bits(x, y)


def test_p_305_is_unsupported_and_leaves_the_outputs_untouched():
    from banet_amd import _capi as capi
    L = capi.lib()
    B, N, C = 1, 33, 4
    rng = np.random.RandomState(305)
    for P, ops_ in ((ec.UNSUPPORTED_P, ("fwd",)), (ec.NULL_FORM_UNSUPPORTED_P, ("fwd", "bwd"))):
        J, G, d = (_dev(rng.standard_normal(s).astype(np.float32)) for s in ((B, N, 2, P), (B, N, C, 2), (B, N, C, 1)))
        g0, g1 = _dev(rng.standard_normal((B, P, P)).astype(np.float32)), _dev(rng.standard_normal((B, P, 1)).astype(np.float32))
        assert L.banet_equation_construction_workspace_bytes(B, N, C, P) == 0
        assert L.banet_equation_construction_grad_workspace_bytes(B, N, C, P) == 0
        ws = _nan_ws(1 << 20)
        if "fwd" in ops_:
            AtA, Atb = _nan((B, P, P)), _nan((B, P, 1))
            rc = L.banet_equation_construction_f32(capi.ptr(J), capi.ptr(G), capi.ptr(d), capi.ptr(AtA), capi.ptr(Atb), B, N, C, P,
                                                   ctypes.c_void_p(ws.data_ptr()), ws.numel(), capi.stream())
            torch.cuda.synchronize()
            assert rc == ERR_UNSUPPORTED
            assert bool(torch.isnan(AtA).all()) and bool(torch.isnan(Atb).all())
        if "bwd" in ops_:
            for wsp, wsn in ((ctypes.c_void_p(ws.data_ptr()), ws.numel()), (None, 0)):
                o = [_nan(x.shape) for x in (J, G, d)]
                rc = L.banet_equation_construction_grad_f32(capi.ptr(J), capi.ptr(G), capi.ptr(d), capi.ptr(g0), capi.ptr(g1), capi.ptr(o[0]),
                                                            capi.ptr(o[1]), capi.ptr(o[2]), B, N, C, P, wsp, wsn, capi.stream())
                torch.cuda.synchronize()
                assert rc == ERR_UNSUPPORTED
                assert all(bool(torch.isnan(x).all()) for x in o)


def test_backward_at_p_305_runs_the_first_generation_kernel_under_the_same_gate():
    """the backward's workspace query is 0 beyond P = 304, which selects the kernel that needs none (banet_hip.h): gated like the table"""
    from banet_amd import _capi as capi
    L = capi.lib()
    c = ec.Case(1, 33, 4, ec.UNSUPPORTED_P, "scaled")
    assert L.banet_equation_construction_grad_workspace_bytes(c.B, c.N, c.C, c.P) == 0 and ec.null_form_lds(c.P) <= ec.LDS_BYTES
    inp = ec.make(c)
    J, G, d, g0, g1 = (_dev(inp[k]) for k in ("J", "G", "d", "g0", "g1"))
    o = [_nan(x.shape) for x in (J, G, d)]
    capi.check(L.banet_equation_construction_grad_f32(capi.ptr(J), capi.ptr(G), capi.ptr(d), capi.ptr(g0), capi.ptr(g1), capi.ptr(o[0]),
                                                      capi.ptr(o[1]), capi.ptr(o[2]), c.B, c.N, c.C, c.P, None, 0, capi.stream()))
    torch.cuda.synchronize()
    errors = ec.backward_errors(c, *(x.cpu().numpy() for x in o))
    _report("bwd-null", c, errors, "bwd")
    assert ec.gate_failures(errors) == []


# ---- ops.equation_construction(symmetric_grad=...) -------------------------------------------------------------------------------
SYM_CASES = (ec.Case(2, 21, 5, 6, "scaled"), ec.Case(1, 33, 3, 165, "scaled"), ec.Case(2, 80, 5, 298, "degenerate"))


@pytest.mark.parametrize("c", SYM_CASES, ids=[ec.case_id(c) for c in SYM_CASES])
def test_symmetric_grad(c):
    """symmetric_grad=True with a NON-symmetric g0 is the oracle's gradient at (g0 + g0^T) / 2, under the table's gate (the scale: the same
    function on |(g0 + g0^T) / 2|); symmetric_grad=False with a symmetric g0 is the plain call bit for bit"""
    from banet_amd import ops
    assert c in ec.TABLE
    inp = ec.make(c)
    rng = np.random.RandomState(c.P)
    skew = rng.standard_normal((c.B, c.P, c.P)).astype(np.float32)
    g0n = (inp["g0"] * (1 + 0.5 * np.tanh(skew))).astype(np.float32)                 # every entry of the table's g0 off by up to 50 %, its scale kept
    assert not np.array_equal(g0n, np.swapaxes(g0n, 1, 2))
    g0s = (0.5 * (g0n.astype(np.float64) + np.swapaxes(g0n.astype(np.float64), 1, 2)))
    J64, G64, d64, g164 = (inp[k].astype(np.float64) for k in ("J", "G", "d", "g1"))
    want = ec.grad64(J64, G64, d64, g0s, g164)
    scale = ec.grad64(np.abs(J64), np.abs(G64), np.abs(d64), np.abs(g0s), np.abs(g164))

    def run(g0, symmetric_grad, plain=False):
        J, G, d = (_dev(inp[k]).requires_grad_() for k in ("J", "G", "d"))
        AtA, Atb = ops.equation_construction(J, G, d) if plain else ops.equation_construction(J, G, d, symmetric_grad=symmetric_grad)
        ((AtA * _dev(g0)).sum() + (Atb * _dev(inp["g1"])).sum()).backward()
        return [x.grad.cpu().numpy() for x in (J, G, d)]

    got = run(g0n, True)
    errors = {k: ec.entry_errors(g, w, s) for k, g, w, s in zip(ec.BWD_OUTPUTS, got, want, scale)}
    print("\nEQCON %-14s %-30s %s" % ("symmetric_grad", ec.case_id(c), "  ".join("%s gpu %.3e gate %.3e" % (k, e.worst, ec.GATE[k])
                                                                                for k, e in errors.items())))
    assert ec.gate_failures(errors) == []
    # and the reference's own pairing is NOT that gradient for this g0 (the switch does something)
    ref = run(g0n, False)
    assert ec.gate_failures({"dJ": ec.entry_errors(ref[0], want[0], scale[0])}) != []
    for a, b in zip(run(inp["g0"], False), run(inp["g0"], None, plain=True)):
        assert _same_bits(a, b)


# ---- the two environment forms: one fresh child process each ---------------------------------------------------------------------
def child_main(out, which):
    """(in the child) the forward over `which` cases of the table -> out (.npz): A<i>, b<i>"""
    cases = ec.TABLE if which == "all" else FOUR_PASS_CASES
    res = {}
    for i, c in enumerate(cases):
        (A, b), = gpu_forward(c, calls=1)
        res["A%d" % i], res["b%d" % i] = A, b
    np.savez(out, **res)


def _run_child(tmp_path, env_name, which):
    if _child_died:
        pytest.fail("not started: the child process of %s ended by a signal or at its timeout" % _child_died[0])
    torch.cuda.synchronize()                      # raises if this process's own GPU context has faulted: no child after that
    here = os.path.dirname(os.path.abspath(__file__))
    out = str(tmp_path / ("%s.npz" % env_name))
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_eqcon_entrywise as m; m.child_main(%r, %r); print('EQCON_CHILD done')"
            % (os.path.dirname(here), here, out, which))
    env = {k: v for k, v in os.environ.items() if k not in ("BANET_EQ_LDS_KERNEL", "BANET_EQ_FOUR_PASS")}
    env[env_name] = "1"
    try:
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        _child_died.append(env_name)
        pytest.fail("the child process of %s did not end within %d s" % (env_name, CHILD_TIMEOUT))
    if r.returncode < 0:
        _child_died.append(env_name)
    assert r.returncode == 0 and "EQCON_CHILD done" in r.stdout, "child of %s ended with %s:\n%s" % (env_name, r.returncode,
                                                                                                   (r.stdout + r.stderr)[-3000:])
    return np.load(out)


def _gate_child(form, cases, res):
    failed = []
    for i, c in enumerate(cases):
        try:
            check_forward(form, c, res["A%d" % i], res["b%d" % i])
        except AssertionError as e:
            failed.append("%s: %s" % (ec.case_id(c), str(e).splitlines()[0] if str(e) else "assertion"))
    assert failed == [], "\n".join(failed)


def test_the_lds_operand_kernel_under_the_same_gate(tmp_path):
    """BANET_EQ_LDS_KERNEL=1: eq_construction_kernel<NB>, every class, the whole forward table"""
    assert "BANET_EQ_LDS_KERNEL" not in os.environ and "BANET_EQ_FOUR_PASS" not in os.environ
    res = _run_child(tmp_path, "BANET_EQ_LDS_KERNEL", "all")
    c = ec.TABLE[10]
    (A, b), = gpu_forward(c, calls=1)
    assert not _same_bits(A, res["A10"])                          # the switch reached the library: another kernel, other bits
    _gate_child("fwd-lds", ec.TABLE, res)


def test_the_four_launch_form_under_the_same_gate(tmp_path):
    """BANET_EQ_FOUR_PASS=1: the four jobs of 144 < P <= 272 as four launches of eq_syrk_kernel"""
    assert "BANET_EQ_LDS_KERNEL" not in os.environ and "BANET_EQ_FOUR_PASS" not in os.environ
    assert {c.P for c in FOUR_PASS_CASES} >= {145, 272} and any(c.family == "degenerate" for c in FOUR_PASS_CASES)
    res = _run_child(tmp_path, "BANET_EQ_FOUR_PASS", "17")
    _gate_child("fwd-four-pass", FOUR_PASS_CASES, res)
