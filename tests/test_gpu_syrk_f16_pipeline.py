"""The fp16 two-piece SYRK (syrk.hip, ba_syrk_bf16x6_kernel<.., .., 16>) keeps its loads ahead of the split: two sets of raw registers
at K = 64, a piecewise refill of the one set at K = 128 with one target frame, the refill after the split elsewhere.  None of it may
change a bit of the arithmetic, so the gate is the one tests/test_gpu_round4.py uses for this kernel (every entry of AtA / Atb within
3e-5 of its own scale against the float64 twin), at shapes chosen by HOW MANY 32-pixel steps a wave gets: 0, 1, 2, 4 and 5 (odd and
even in the loop unrolled by two), a last step that is partly or wholly past the window, and the window-wide fallback to the exact form
after the prologue of the pipelined loop.  Plus the first pass of a level (T0 = 1), whose column maxima are kept as bit patterns.

The CPU test at the end checks the inputs of every case (finite twin, no empty system) and the step counts the cases were chosen for.
"""
import functools
import math

import numpy as np
import pytest
import torch

from banet_amd import _capi as F     # the DEV_* names of banet_level_t.flags
from oracle import banet_oracle as orc, torch_port

DEV = "cuda:0"
C = 128
CANONICAL_BATCH = 32                 # banet_hip.h: BANET_CANONICAL_BATCH, the batch BANET_POLICY_BATCH_INVARIANT decides from
SYRK_F16, NO_SYRK_F16 = F.DEV_SYRK_F16, F.DEV_NO_SYRK_F16

# name -> (H, W, B, batch_invariant, the set of steps per wave the shape is there for, with 256 CUs)
SHAPES = {
    "4x4": (4, 4, 2, False, {0, 1}),            # N = 16: one step in all; both prologue batches of most waves lie past their run
    "30x20": (30, 20, 2, False, {1, 2}),        # N = 600: 19 steps on 12 waves
    "40x30bi": (40, 30, 2, True, {1, 2}),       # decisions as for batch 32: Gs = 5, 38 steps on 20 waves
    "60x80bi": (60, 80, 2, True, {4, 5}),       # Gs = 8, 150 steps on 32 waves: odd and even runs in the unrolled loop
    "7x9": (7, 9, 1, False, {0, 1}),            # N = 63: the last step is partly beyond N
    "30x21": (30, 21, 1, False, {1, 2}),        # N = 630, no multiple of 32: the last wave's last step is ragged
}
# (shape, K, target frames): one target frame is the pipelined form (two sets at K = 64, piecewise refill at K = 128); K = 128 with
# 2 and 3 target frames refills after the split as before -- both sides of the `if constexpr`
CASES = [(s, K, 1) for s in SHAPES for K in (128, 64)] + [(s, 128, p) for s in ("30x20", "60x80bi") for p in (2, 3)]
CASE_IDS = ["%s-K%d-p%d" % c for c in CASES]


def wave_runs(N, Bsel, cus):
    """steps per wave of the bf16x6 SYRK launch (plan_syrk + the kernel's own split): ns 32-pixel steps over 4 Gs waves"""
    ns = (N + 31) // 32
    Gs = max(1, min((N + 255) // 256, (cus + Bsel - 1) // Bsel))
    waves = 4 * Gs
    return [ns * (g + 1) // waves - ns * g // waves for g in range(waves)], Gs, ns


def case_runs(shape, cus):
    H, W, B, bi, _ = SHAPES[shape]
    return wave_runs(H * W, CANONICAL_BATCH if bi else B, cus)


def n(x):
    return x.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def make_case(shape, K, pairs, device):
    """levels, state and the float64 twin of one case; computed once per device and shared (nothing below writes into it)"""
    from banet_amd import synth as bsynth
    H, W, B, bi, _ = SHAPES[shape]
    intr, levels, gt = bsynth.make_dense_windows(B, H, W, C, K, [1], 700 + H + K + pairs, device, trans_mag=0.06, pairs=pairs)
    lv = levels[0]
    R = torch.eye(3, device=device).repeat(B, pairs, 1, 1) if pairs > 1 else torch.eye(3, device=device).repeat(B, 1, 1)
    T = (gt["T"] * 0.7).reshape(B, pairs, 3, 1).to(device) if pairs > 1 else (gt["T"] * 0.7).reshape(B, 3, 1).to(device)
    Wc = torch.zeros(B, K, 1, device=device)
    tg = lv.tgt if lv.tgt.dim() == 5 else lv.tgt.unsqueeze(1)
    twin = []
    for b in range(B):
        sl = slice(b, b + 1)
        A64, b64, _, _ = torch_port.window_assemble(intr[sl], lv.scale, lv.src[sl], tg[sl], lv.depth[sl], lv.basis[sl],
                                                    R.reshape(B, pairs, 3, 3)[sl], T.reshape(B, pairs, 3, 1)[sl], Wc[sl])
        twin.append((n(A64[0]), n(b64[0])))
    return dict(intr=intr, levels=levels, R=R, T=T, Wc=Wc, twin=twin, B=B, K=K, pairs=pairs, bi=bi, N=H * W)


def _entry_errors(AtA, Atb, absres, A64, b64):
    """as tests/test_gpu_round4.py: every entry against its own scale, sqrt(A_ii A_jj) resp. sqrt(A_ii) |r|"""
    dg = np.sqrt(np.maximum(np.diag(A64), 1e-300))
    eA = np.abs(n(AtA).astype(np.float64) - A64) / np.outer(dg, dg)
    rs = float(np.sqrt((n(absres).astype(np.float64) ** 2).sum()))
    eb = np.abs(n(Atb).astype(np.float64) - b64) / (dg * max(rs, 1e-30))
    return eA, eb, dg


def _gpu():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    F.lib()
    return torch.cuda.get_device_properties(0).multi_processor_count


def _problem(case, levels=None):
    from banet_amd import dense as bdense
    ba = bdense.DenseBA(case["intr"], levels if levels is not None else case["levels"], [orc.he_normal_mlp_weights(C, 5)], "bundle", 1000.0,
                        batch_invariant=case["bi"])
    return ba, ba.problems[0]


def _assemble(p, case, flags):
    from banet_amd import ops
    p.c.flags = flags
    out = [x.clone() for x in ops.ba_assemble(p, case["R"], case["T"], case["Wc"])]
    p.c.flags = 0
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("shape,K,pairs", CASES, ids=CASE_IDS)
def test_f16_syrk_by_steps_per_wave(shape, K, pairs):
    """The single assembly pass with DEV_SYRK_F16 (ba_colmax_kernel up front, then the fp16 form) against the float64 twin, entry by
    entry; pose block and sum|d| are the gather's and equal the exact form's bits; symmetric; two calls give equal bits.  The single
    pass never launches the lambda-MLP role workgroup, so Gs is the plan's own here (the role's Gs - 1 is the LM loop's, below)."""
    cus = _gpu()
    runs, Gs, ns = case_runs(shape, cus)
    want = SHAPES[shape][4]
    if set(runs) != want:
        pytest.skip("%d CUs give Gs = %d and runs of %s steps per wave, not the intended %s" % (cus, Gs, sorted(set(runs)), sorted(want)))
    case = make_case(shape, K, pairs, DEV)
    ba, p = _problem(case)
    exact = _assemble(p, case, NO_SYRK_F16)
    f16 = _assemble(p, case, SYRK_F16)
    again = _assemble(p, case, SYRK_F16)
    assert all(torch.equal(a, b) for a, b in zip(f16, again))                  # bit-reproducible
    o = 6 * pairs
    assert torch.equal(exact[0][:, :o, :o], f16[0][:, :o, :o]) and torch.equal(exact[2], f16[2])
    assert torch.equal(f16[0], f16[0].transpose(1, 2))
    if case["N"] >= 600:
        assert not torch.equal(exact[0], f16[0])                               # another kernel ran
    for b in range(case["B"]):
        A64, b64 = case["twin"][b]
        eA, eb, dg = _entry_errors(f16[0][b], f16[1][b], f16[2][b], A64, b64)
        xA, xb, _ = _entry_errors(exact[0][b], exact[1][b], exact[2][b], A64, b64)
        print("%s K=%d pairs=%d Gs=%d steps/wave %s window %d: fp16 two-piece AtA %.2e Atb %.2e | bf16x6 AtA %.2e Atb %.2e" % (
            shape, K, pairs, Gs, sorted(set(runs)), b, eA.max(), eb.max(), xA.max(), xb.max()))
        assert eA.max() < 3e-5, (b, eA.max(), np.unravel_index(eA.argmax(), eA.shape))
        assert eb.max() < 3e-5, (b, eb.max())


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["30x20", "60x80bi"])
@pytest.mark.parametrize("K", [128, 64])
def test_fallback_to_the_exact_form_after_the_pipelined_prologue(shape, K):
    """One Inf in window 1's basis: that window's scales cannot be formed and all of its waves run the exact loop -- from step s0,
    which the prologue must have left in the set that loop reads -- bit-identical to the exact kernel; window 0 runs the fp16 form.
    tests/test_gpu_round4.py covers this at 2 steps per wave only; here batch-invariant, B = 2: runs of 1 / 2 and of 4 / 5."""
    from banet_amd import dense as bdense
    _gpu()
    case = dict(make_case(shape, K, 1, DEV), bi=True)
    lv = case["levels"][0]
    B, N = case["B"], case["N"]
    basis = lv.basis.clone()
    basis.reshape(B, N, K)[1, N // 2 + 3, 5] = float("inf")
    ba, p = _problem(case, [bdense.DenseLevel(lv.scale, lv.src, lv.tgt, lv.depth, basis)])
    exact = _assemble(p, case, NO_SYRK_F16)
    mixed = _assemble(p, case, SYRK_F16)
    assert torch.equal(mixed[0][1].nan_to_num(1.0, 2.0, 3.0), exact[0][1].nan_to_num(1.0, 2.0, 3.0))     # window 1: the exact form's bits
    assert torch.equal(mixed[1][1].nan_to_num(1.0, 2.0, 3.0), exact[1][1].nan_to_num(1.0, 2.0, 3.0))
    assert not torch.equal(mixed[0][0], exact[0][0]) and torch.isfinite(mixed[0][0]).all()                # window 0: the fp16 form
    A64, b64 = case["twin"][0]
    eA, eb, _ = _entry_errors(mixed[0][0], mixed[1][0], mixed[2][0], A64, b64)
    assert eA.max() < 3e-5 and eb.max() < 3e-5, (eA.max(), eb.max())


def _lm(ba, case, iters, flags, state=None):
    for prob in ba.problems:
        prob.c.flags = flags
    st = state if state is not None else ba.new_state(T=case["T"].clone())
    st, _ = ba.solve([iters], st)
    torch.cuda.synchronize()
    for prob in ba.problems:
        prob.c.flags = 0
    return st


@pytest.mark.gpu
def test_lm_level_with_the_pipelined_f16_syrk():
    """banet_lm_level_f32 through DenseBA.solve at 60x80, B = 2, batch-invariant, three iterations: the first pass is T0 = 1 (exact
    form + column maxima as bit patterns), the other two the fp16 form with them; here the role workgroup takes one of the 8 SYRK
    workgroups per window where the plan says so.  Two runs agree bit for bit; within 1e-4 (relative, as
    test_lm_loop_with_the_f16_syrk_*) of the same loop on the exact form."""
    _gpu()
    case = make_case("60x80bi", 128, 1, DEV)
    ba, _ = _problem(case)
    a = _lm(ba, case, 3, SYRK_F16)
    b = _lm(ba, case, 3, SYRK_F16)
    e = _lm(ba, case, 3, NO_SYRK_F16)
    for x, y in ((a.R, b.R), (a.T, b.T), (a.Wc, b.Wc)):
        assert torch.equal(x, y)

    def rel(x, y):
        return float((x - y).abs().max() / y.abs().max())
    print("fp16 LM level vs exact: R %.2e T %.2e W %.2e" % (rel(a.R, e.R), rel(a.T, e.T), rel(a.Wc, e.Wc)))
    assert rel(a.R, e.R) < 1e-4 and rel(a.T, e.T) < 1e-4 and rel(a.Wc, e.Wc) < 1e-4
    assert not torch.equal(a.Wc, e.Wc)                                         # the fp16 form really ran


@pytest.mark.gpu
def test_first_pass_column_maxima_equal_the_colmax_kernel():
    """Column maxima of the first pass (T0 = 1) on bit patterns, end to end: a basis whose columns span 2^24, with zero entries and a
    column that is zero but for one pixel, 30x20, B = 2.  A two-iteration LM level with DEV_SYRK_F16 runs [exact form + maxima in the
    kernel, fp16 form with them]; the comparison run takes its maxima from ba_colmax_kernel: a one-iteration call on the exact form
    (DEV_NO_SYRK_F16: the same bits as the first pass, which only adds the maxima) followed by a one-iteration call with DEV_SYRK_F16
    from that state (one iteration: ba_colmax_kernel up front, then the fp16 form).  Equal bits of R, T and W mean equal scales, i.e.
    equal exponents of every column's maximum.  (Two one-iteration fp16 calls would not do as the comparison: their FIRST iteration
    is the fp16 form where the two-iteration level runs the exact one.)  The workspace has no accessor for off_colmax, so the
    maxima are compared through the results only."""
    from banet_amd import dense as bdense
    _gpu()
    K = 128
    case = make_case("30x20", K, 1, DEV)
    lv = case["levels"][0]
    B, N = case["B"], case["N"]
    g = torch.Generator().manual_seed(17)
    scale = torch.pow(2.0, 24.0 * torch.arange(K, dtype=torch.float64) / (K - 1) - 12.0).to(torch.float32)
    basis = lv.basis.reshape(B, N, K).cpu() * scale[torch.randperm(K, generator=g)]
    basis[torch.rand(B, N, K, generator=g) < 0.1] = 0.0
    keep = basis[:, 123, 7].clone()
    basis[:, :, 7] = 0.0
    basis[:, 123, 7] = keep
    basis = basis.reshape(lv.basis.shape).contiguous().to(DEV)
    ba, _ = _problem(case, [bdense.DenseLevel(lv.scale, lv.src, lv.tgt, lv.depth, basis)])
    two = _lm(ba, case, 2, SYRK_F16)
    one = _lm(ba, case, 1, NO_SYRK_F16)
    ref = _lm(ba, case, 1, SYRK_F16, state=one)
    assert torch.isfinite(two.Wc).all()
    for name, x, y in (("R", two.R, ref.R), ("T", two.T, ref.T), ("W", two.Wc, ref.Wc)):
        assert torch.equal(x, y), (name, float((x - y).abs().max()))


def test_inputs_of_every_case_on_the_cpu():
    """No GPU: every case's float64 twin is finite and no diagonal entry is zero, so that the gate cannot be met by an empty system;
    every shape gives the steps per wave it was chosen for on a 256-CU device; no case is missing from the parametrisation."""
    assert len(CASES) == 2 * len(SHAPES) + 4 and len(set(CASES)) == len(CASES)
    assert {c[0] for c in CASES} == set(SHAPES) and {(c[1], c[2]) for c in CASES} == {(128, 1), (64, 1), (128, 2), (128, 3)}
    for shape, (H, W, B, bi, want) in SHAPES.items():
        runs, Gs, ns = case_runs(shape, 256)
        assert set(runs) == want and sum(runs) == ns == math.ceil(H * W / 32), (shape, runs)
    assert case_runs("40x30bi", 256)[1:] == (5, 38) and case_runs("60x80bi", 256)[1:] == (8, 150) and case_runs("30x20", 256)[1:] == (3, 19)
    for shape, K, pairs in CASES:
        case = make_case(shape, K, pairs, "cpu")
        for A64, b64 in case["twin"]:
            assert np.isfinite(A64).all() and np.isfinite(b64).all(), (shape, K, pairs)
            assert np.diag(A64).min() > 0, (shape, K, pairs, float(np.diag(A64).min()))
