"""The workspace contract on the GPU (`-m gpu`; include/banet_hip.h, DESIGN.md "Workspace regions", tests/ws_contract.py):

  * on entry a workspace holds arbitrary bytes -- no call reads a workspace byte it did not write itself
    (BANET_ADJOINT_REUSE_DEPTH_SEED is the one documented exception, tested as a pair of calls);
  * no call touches a byte outside [ws, ws + workspace_bytes).

Every case runs the same call four times with banet_amd._capi.workspace replaced by the guarded allocator: body zero-filled,
`stale` (the leftovers of a call of another shape / kernel selection in the same bytes), NaN words (0x7FC00000) and 1.0 words
(0x3F800000) -- benign fills first.  All outputs must be bit-equal across the four runs, finite where the existing tests expect
finite, and every guard band intact.  Bit equality is the bar because every path below is documented as bit-reproducible (the only
float-atomic entry point, banet_sample_stats_grad_f32, takes no workspace).
"""
import ctypes

import numpy as np
import pytest
import torch

import ws_contract as wsc
from banet_amd import _capi as F     # the DEV_* names of banet_level_t.flags

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# development bits of banet_level_t.flags that force a kernel (test_gpu_round4.py)
GENERIC, DIRECT, PATCH = (F.DEV_GENERIC_GATHER | F.DEV_NO_QUAD_GATHER, F.DEV_DIRECT_GATHER | F.DEV_NO_STRIP_GATHER | F.DEV_NO_QUAD_GATHER,
                          F.DEV_FORCE_PATCH_GATHER | F.DEV_NO_QUAD_GATHER)
STRIP, STRIP_PAIR_LOOP, QUAD = F.DEV_FORCE_STRIP_GATHER, F.DEV_FORCE_STRIP_GATHER | F.DEV_STRIP_FRAME_LOOP, F.DEV_FORCE_QUAD_GATHER
SYRK_F16, SYRK_FP32_OR_LDS, MLP_IN_SOLVE = F.DEV_SYRK_F16, F.DEV_SYRK_NO_BF16X6, F.DEV_MLP_IN_SOLVE
GATHER_OF = {GENERIC: 0, DIRECT: 1, PATCH: 2, STRIP: 3, STRIP_PAIR_LOOP: 3, QUAD: 4}

_ARENA = []


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from banet_amd import _capi
    _capi.lib()
    yield
    _ARENA.clear()


def arena():
    """one 768 MB buffer for the whole module: every run carves its workspaces from its first bytes (ws_contract.Arena)"""
    if not _ARENA:
        _ARENA.append(wsc.Arena(768 << 20, DEV))
    return _ARENA[0]


def lambda_weights(C, seed):
    from banet_amd.bundlenet import he_normal_lambda_weights
    return he_normal_lambda_weights(C, seed)


_PRIMER = {}


def primer():
    """What leaves the `stale` bytes: an LM level on the strip gather with K = 64 (another partial-row layout, queue heads and SYRK
    partials in other places than any case below) followed by a generic-gather assembly with sum|d| rows of C = 70."""
    from banet_amd import dense as bdense, ops, synth as bsynth
    if not _PRIMER:
        intr, levels, gt = bsynth.make_dense_windows(3, 37, 53, 128, 64, [1], 901, torch.device(DEV), trans_mag=0.06)
        _PRIMER["lm"] = (intr, levels, [lambda_weights(128, 31)], (gt["T"] * 0.7).reshape(3, 3, 1).to(DEV))
        intr2, levels2, gt2 = bsynth.make_dense_windows(2, 41, 57, 70, 33, [1], 902, torch.device(DEV), trans_mag=0.06)
        _PRIMER["asm"] = (intr2, levels2, [lambda_weights(70, 32)], (gt2["T"] * 0.7).reshape(2, 3, 1).to(DEV))
    intr, levels, mlps, T0 = _PRIMER["lm"]
    ba = bdense.DenseBA(intr, levels, mlps, "bundle", 1000.0)
    ba.problems[0].c.flags = STRIP
    ba.solve([2], ba.new_state(T=T0.clone()))
    intr, levels, mlps, T0 = _PRIMER["asm"]
    ba = bdense.DenseBA(intr, levels, mlps, "bundle", 1000.0)
    ops.ba_assemble(ba.problems[0], torch.eye(3, device=DEV).repeat(2, 1, 1), T0, torch.zeros(2, 33, 1, device=DEV))
    torch.cuda.synchronize()


def check(run, names=None, finite=True, min_workspaces=1):
    """run under zero / stale / nan / one; guards are checked on leaving each run (ws_contract.patched_workspace)"""
    outs, seen = wsc.run_under_every_fill(run, arena(), primer=primer)
    assert list(outs) == ["zero", "stale", "nan", "one"]
    for fill, handles in seen.items():
        assert len(handles) >= min_workspaces, (fill, len(handles))      # the call really took its scratch from the patched allocator
    wsc.assert_same_bits_across_fills(outs, names=names, finite=finite)
    return outs


def test_the_guarded_allocator_works_on_the_device():
    """the harness on the GPU: exact length, alignment, the fills, and a one-byte overrun written by a device kernel is reported"""
    for fill in ("zero", "nan", "one"):
        ws, h = wsc.guarded_workspace(1000, DEV, fill)
        assert ws.is_cuda and ws.numel() == 1000 and ws.data_ptr() % 256 == 0
        assert int(ws.view(torch.int32)[7]) == wsc.FILL_WORDS[fill]
        wsc.assert_guards_intact(h)
    ws.fill_(3)
    wsc.assert_guards_intact(h)
    h.block[wsc.GUARD_BYTES + 1000:wsc.GUARD_BYTES + 1001].fill_(0)
    with pytest.raises(AssertionError, match="after the body.*offset 0 "):
        wsc.assert_guards_intact(h)


# ======================================================================================================================
# EquationConstruction (+Grad)
# ======================================================================================================================
@pytest.mark.parametrize("P", [6, 38, 143, 144, 145, 200, 304])
def test_equation_construction_and_its_gradient(P):
    """the matrix-pipe fast path up to P = 144 and above it (partials + per-pixel records), the fast gradient workspace (two
    record arrays), ragged N and C"""
    from banet_amd import ops
    B, N, C = 2, 777, 70
    g = torch.Generator().manual_seed(P)
    J = torch.randn(B, N, 2, P, generator=g).to(DEV)
    G = torch.randn(B, N, C, 2, generator=g).to(DEV)
    d = torch.randn(B, N, C, 1, generator=g).to(DEV)
    g0 = torch.randn(B, P, P, generator=g).to(DEV)
    g1 = torch.randn(B, P, 1, generator=g).to(DEV)

    def run():
        return list(ops.equation_construction_forward(J, G, d)) + list(ops.equation_construction_grad(J, G, d, g0, g1))
    check(run, names=["AtA", "Atb", "gJ", "gG", "gd"], min_workspaces=2)


# ======================================================================================================================
# one assembly pass
# ======================================================================================================================
def _window_inputs(B, H, W, K, pairs, seed, C=128, trans_mag=0.06):
    from banet_amd import synth as bsynth
    intr, levels, gt = bsynth.make_dense_windows(B, H, W, C, K, [1], seed, torch.device(DEV), trans_mag=trans_mag, pairs=pairs)
    shape = (B, pairs) if pairs > 1 else (B,)
    R = torch.eye(3, device=DEV).repeat(B * pairs, 1, 1).reshape(*shape, 3, 3).contiguous()
    T = (gt["T"] * 0.7).reshape(*shape, 3, 1).to(DEV).contiguous()
    g = torch.Generator().manual_seed(seed)
    Wc = (0.01 * torch.randn(B, K, 1, generator=g)).to(DEV) if K else None
    return intr, levels, R, T, Wc


@pytest.mark.parametrize("H,W,K,pairs", [(41, 57, 0, 1), (37, 53, 0, 3), (41, 57, 32, 1), (37, 53, 32, 3), (41, 57, 128, 1), (37, 53, 128, 3),
                                         (10, 13, 32, 1), (35, 45, 256, 1), (30, 40, 128, 5), (37, 53, 256, 3)])
def test_ba_assemble_with_every_gather_kernel(H, W, K, pairs):
    """banet_ba_assemble_f32 / _mask_f32 under the default selection and every forced gather kernel (generic, direct, patch, strip,
    strip with the frames looped, 4x4 items): partial rows, the fold region, the tile-queue heads, the records and the SYRK
    partials of K = 0 / 32 / 128 / 256 (LDS-tiled, bf16x6, wide jobs with their per-pixel aux sums for > 1 frame)."""
    from banet_amd import dense as bdense, ops
    B = 2
    intr, levels, R, T, Wc = _window_inputs(B, H, W, K, pairs, 500 + K + pairs)
    mlps = [lambda_weights(128, 9)]
    # (the strip and patch kernels at the sizes the existing parity tests force them at: not on the 10x13 map)
    kinds = [0, GENERIC, DIRECT, QUAD] + ([PATCH, STRIP] if W >= 21 else []) + ([STRIP_PAIR_LOOP] if pairs > 1 and W >= 21 else [])
    for bits in kinds:
        for with_mask in (False, True):
            def run():
                ba = bdense.DenseBA(intr, levels, mlps, "bundle" if K else "bundle_camera", 1000.0)
                ba.problems[0].c.flags = bits
                if bits:
                    assert ops.gather_selection(ba.problems[0]) == GATHER_OF[bits], (bits, ops.gather_selection(ba.problems[0]))
                return list(ops.ba_assemble(ba.problems[0], R, T, Wc, return_mask=with_mask))
            outs = check(run, names=["AtA", "Atb", "absres", "nvalid", "mask"], min_workspaces=2)
            if with_mask:
                assert int(outs["zero"][4].max()) <= 1                   # every mask entry written (the buffer starts at 255)


def test_ba_assemble_with_every_syrk_kernel():
    """SyrkPlan::direct 0 (LDS-tiled), 1 (fp32 MFMA), 2 (bf16x6), 3 (wide jobs; with off_aux for multi-frame windows) and the fp16
    two-piece form of 2 and 3 in a single pass (colmax / recmax regions, f16_stats = 0)"""
    from banet_amd import dense as bdense, ops
    B, seen_sel, aux = 2, set(), 0
    for H, W, K, pairs, bits in ((41, 57, 32, 1, 0), (41, 57, 128, 1, 0), (41, 57, 128, 1, SYRK_FP32_OR_LDS), (37, 53, 64, 3, 0),
                                 (37, 53, 64, 3, SYRK_FP32_OR_LDS), (30, 40, 128, 5, 0), (35, 45, 256, 1, 0), (37, 53, 256, 3, 0),
                                 (35, 45, 256, 1, SYRK_FP32_OR_LDS), (41, 57, 128, 1, SYRK_F16), (37, 53, 64, 3, SYRK_F16),
                                 (30, 40, 128, 5, SYRK_F16), (37, 53, 256, 3, SYRK_F16)):
        intr, levels, R, T, Wc = _window_inputs(B, H, W, K, pairs, 600 + K + pairs)
        mlps = [lambda_weights(128, 9)]
        sel = []

        def run():
            ba = bdense.DenseBA(intr, levels, mlps, "bundle", 1000.0)
            ba.problems[0].c.flags = bits
            sel.append(ops.syrk_selection(ba.problems[0]))
            return list(ops.ba_assemble(ba.problems[0], R, T, Wc))
        check(run, names=["AtA", "Atb", "absres", "nvalid"], min_workspaces=2)
        assert len(set(sel)) == 1
        want = 4 if bits == SYRK_F16 else (0 if K == 32 or (bits and K == 256) else 1 if bits else 3 if (K == 256 or pairs > 4) else 2)
        assert sel[0] == want, (H, W, K, pairs, bits, sel[0], want)
        seen_sel.add((sel[0], K == 256 or pairs > 4))
        aux += int((K == 256 or pairs > 4) and pairs > 1 and bits != SYRK_FP32_OR_LDS)
    assert {s for s, _ in seen_sel} == {0, 1, 2, 3, 4} and (4, True) in seen_sel and (4, False) in seen_sel and aux >= 3


@pytest.mark.parametrize("B,N,C,K", [(2, 777, 128, 128), (1, 4096, 128, 0), (2, 777, 70, 33), (1, 4096, 70, 33)])
def test_ba_assemble_on_sparse_points(B, N, C, K):
    """the reference's own layout (sampled points, rays + per-point intrinsics, [f|gx|gy] target map): ba_gather_kernel with 16- and
    64-point items -- one partial row per workgroup -- ragged N"""
    from banet_amd import ops
    g = torch.Generator().manual_seed(B * 1000 + N + C)
    H, W = 48, 64
    img = torch.randn(B, H, W, C, generator=g).to(DEV)
    conv2 = ops.target_map(img)
    pts = torch.stack([torch.rand(B, N, generator=g) * (W + 2) - 1.5, torch.rand(B, N, generator=g) * (H + 2) - 1.5], dim=-1).to(DEV)
    conv1 = ops.resample(img, pts.clamp(min=0.0)) + 0.05 * torch.randn(B, N, C, generator=g).to(DEV)
    fx = torch.full((B, N), 0.8 * W, device=DEV)
    ox, oy = torch.full((B, N), W / 2.0, device=DEV), torch.full((B, N), H / 2.0, device=DEV)
    ray = torch.stack([(pts[..., 0] - ox) / fx, (pts[..., 1] - oy) / fx, torch.ones(B, N, device=DEV)], dim=1)
    p = (ray / ray.norm(dim=1, keepdim=True)).contiguous()
    D = (2.5 + torch.rand(B, N, generator=g)).to(DEV)
    Bs = (torch.randn(B, N, K, generator=g) / max(K, 1) ** 0.5).to(DEV) if K else None
    R = torch.eye(3, device=DEV).repeat(B, 1, 1)
    T = (0.02 * torch.randn(B, 3, 1, generator=g)).to(DEV)
    Wc = (0.01 * torch.randn(B, K, 1, generator=g)).to(DEV) if K else None
    for bits in (0, F.DEV_SPARSE_ITEMS64):                              # 16-point items where the launch is latency-bound / always 64
        def run():
            prob = ops.LevelProblem("bundle" if K else "bundle_camera", conv1, conv2, D, H, W, C, basis=Bs, rays=p, fx=fx, fy=fx.clone(),
                                    ox=ox, oy=oy, dense=False, tgt_has_grad=True)
            prob.c.flags = bits
            assert ops.gather_selection(prob) == 0
            return list(ops.ba_assemble(prob, R, T, Wc))
        outs = check(run, names=["AtA", "Atb", "absres", "nvalid"])
        assert 0 < float(outs["zero"][3].min()) and float(outs["zero"][3].max()) < N      # some points are outside the image


# ======================================================================================================================
# the LM loop of a level
# ======================================================================================================================
def _lm_case(B, H, W, K, pairs, scales, seed, variant="bundle", C=128, normalize_rays=True):
    from banet_amd import synth as bsynth
    intr, levels, gt = bsynth.make_dense_windows(B, H, W, C, K, scales, seed, torch.device(DEV), trans_mag=0.06, pairs=pairs,
                                                 normalize_rays=normalize_rays)
    mlps = [lambda_weights(C, 100 + i) for i in range(len(scales))]
    T0 = (gt["T"] * 0.7).reshape(B * pairs, 3, 1).to(DEV)
    return intr, levels, mlps, T0


def _lm_run(case, variant, iters, flags=0, batch_invariant=False, early=False, l2=1000.0, expect=None):
    from banet_amd import dense as bdense, ops
    intr, levels, mlps, T0 = case

    def run():
        ba = bdense.DenseBA(intr, levels, mlps, variant, l2, batch_invariant=batch_invariant)
        for prob in ba.problems:
            prob.c.flags = flags
        if expect is not None:
            got = (ops.gather_selection(ba.problems[-1]), ops.syrk_selection(ba.problems[-1]))
            assert got == expect, (got, expect)
        st, counts = ba.solve(iters, ba.new_state(T=T0.clone()), early_termination=early)
        return [st.R, st.T] + ([st.Wc] if st.Wc is not None else []) + [st.iters, st.ratio, st.lambda_out, st.delta] + list(counts)
    return run


@pytest.mark.parametrize("max_iters", [1, 3])
@pytest.mark.parametrize("flags,policy", [(SYRK_F16, False), (SYRK_F16 | MLP_IN_SOLVE, False), (SYRK_F16, True), (0, False), (0, True),
                                          (SYRK_F16 | STRIP, False), (SYRK_F16 | DIRECT, False), (GENERIC, False)])
def test_lm_level_fixed_count(max_iters, flags, policy):
    """banet_lm_level_f32 on a level where the fp16 two-piece SYRK is eligible (pl.s.f16): one iteration (f16_stats 0: column maxima
    up front) and three (2, then 1, 1: the exact form leaves them, the later passes read them in place); the lambda MLP as a role
    workgroup of the SYRK launch (mlp_y) and inside the solve kernel (flags bit 15); BANET_POLICY_BATCH_INVARIANT (Gs from the
    canonical batch, one SYRK workgroup given up for the role); queue heads reset once per level and left zeroed by the solve."""
    case = _lm_case(2, 48, 64, 128, 1, [1], 611)
    check(_lm_run(case, "bundle", [max_iters], flags, policy), min_workspaces=1)


@pytest.mark.parametrize("H,W,K,pairs,flags", [(35, 45, 256, 1, 0), (35, 45, 256, 1, SYRK_F16), (37, 53, 256, 3, SYRK_F16), (37, 53, 128, 3, SYRK_F16),
                                               (30, 40, 128, 5, SYRK_F16), (41, 57, 32, 1, 0), (37, 53, 0, 2, 0), (10, 13, 32, 1, 0),
                                               (41, 57, 188, 1, 0)])
def test_lm_level_other_shapes(H, W, K, pairs, flags):
    """K = 256 and P = 194 (the solve's matrix in the workspace: bigA), the wide SYRK jobs in the LM loop (their own column-maxima
    pass, off_aux), multi-frame windows, the LDS-tiled SYRK, pose only, a map of a few items"""
    case = _lm_case(2, H, W, K, pairs, [1], 620 + K + pairs)
    check(_lm_run(case, "bundle" if K else "bundle_camera", [3], flags))


def test_lm_level_with_no_iterations_leaves_the_state_alone():
    from banet_amd import dense as bdense
    intr, levels, mlps, T0 = _lm_case(2, 41, 57, 128, 1, [1], 630)
    outs = check(_lm_run((intr, levels, mlps, T0), "bundle", [0]))
    ba = bdense.DenseBA(intr, levels, mlps, "bundle", 1000.0)
    st = ba.new_state(T=T0.clone())
    for got, want in zip(outs["one"][:3], (st.R, st.T, st.Wc)):
        assert torch.equal(got, want.cpu())
    assert int(outs["one"][3].abs().max()) == 0


@pytest.mark.parametrize("flags", [0, STRIP, GENERIC])
def test_legacy_early_terminated_lm(flags):
    """legacy/ba.py's early-terminated LM: the per-window loop state (LmCtl) lives in the workspace; the iteration counts are part of
    the outputs compared.  Three levels, coarse to fine, in ONE workspace (DenseBA.ws)."""
    case = _lm_case(3, 48, 64, 0, 1, [4, 2, 1], 51, C=128 if flags == STRIP else 8, normalize_rays=False)
    outs = check(_lm_run(case, "legacy_lm", [3, 5, 7], flags, early=True, l2=1.0))
    counts = [c.tolist() for c in outs["zero"][-3:]]
    assert all(0 <= v <= m for c, m in zip(counts, (3, 5, 7)) for v in c), counts


def test_ba_solve_update_with_a_workspace():
    """banet_ba_solve_update_ws_f32 (K = 256: the damped matrix lives in the workspace)"""
    from banet_amd import dense as bdense, ops
    B, K = 2, 256
    intr, levels, R, T, Wc = _window_inputs(B, 35, 45, K, 1, 640)
    mlps = [lambda_weights(128, 9)]

    def run():
        ba = bdense.DenseBA(intr, levels, mlps, "bundle", 1000.0)
        prob = ba.problems[0]
        AtA, Atb, absres, nvalid = ops.ba_assemble(prob, R, T, Wc)
        st = ba.new_state(R=R.clone(), T=T.clone(), Wc=Wc.clone())
        ws = ops.ba_solve_update(prob, ba.mlps[0], ba.l2_base, AtA, Atb, absres, nvalid, st)
        assert ws is not None
        return [st.R, st.T, st.Wc, st.lambda_out, st.delta]
    check(run, min_workspaces=3)


# ======================================================================================================================
# gradients of the per-level preparation, deterministic sample-stats gradient
# ======================================================================================================================
@pytest.mark.parametrize("clamp", [False, True])
@pytest.mark.parametrize("overwrite", [True, False])
@pytest.mark.parametrize("B,N,C,H,W", [(2, 777, 70, 41, 57), (1, 4096, 128, 37, 53), (2, 130, 3, 10, 13)])
def test_resampler_gradient(B, N, C, H, W, clamp, overwrite):
    """banet_resample_grad_f32: sort keys / values (ping-pong), histograms, cell bounds -- both sampling modes, overwrite
    (NaN-filled outputs: every entry written) and accumulate"""
    from test_gpu_prep_grad import make_warp, resample_grad
    rng = np.random.RandomState(N + C)
    data = torch.from_numpy(rng.standard_normal((B, H, W, C)).astype(np.float32)).to(DEV)
    warp = torch.from_numpy(make_warp(rng, B, N, H, W, "mixed")).to(DEV)
    gout = torch.from_numpy(rng.standard_normal((B, N, C)).astype(np.float32)).to(DEV)
    base = torch.from_numpy(rng.standard_normal((B, H, W, C)).astype(np.float32)).to(DEV)

    def run():
        ddata = torch.full_like(data, float("nan")) if overwrite else base.clone()
        dwarp = torch.full((B, N, 2), float("nan"), device=DEV)
        return list(resample_grad(data, warp, gout, clamp, ddata=ddata, dwarp=dwarp, overwrite=overwrite))
    check(run, names=["ddata", "dwarp"])


@pytest.mark.parametrize("B,N,K", [(2, 2337, 128), (1, 777, 32), (3, 130, 256)])
def test_depth_output_gradient(B, N, K):
    from banet_amd import prep_grad
    g = torch.Generator().manual_seed(N)
    basis = torch.randn(B, N, K, generator=g).to(DEV)
    Wc = torch.randn(B, K, 1, generator=g).to(DEV)
    gout = torch.randn(B, N, generator=g).to(DEV)
    check(lambda: list(prep_grad.depth_output_grad_forward(basis, Wc, gout)), names=["dinit", "dbasis", "dWc"])


@pytest.mark.parametrize("B,N,C,H,W", [(2, 777, 128, 41, 57), (1, 4096, 70, 37, 53)])
def test_deterministic_sample_stats_gradient(B, N, C, H, W):
    from banet_amd import ops
    g = torch.Generator().manual_seed(5)
    conv1 = torch.randn(B, N, C, generator=g).to(DEV)
    conv2 = torch.randn(B, H, W, 3 * C, generator=g).to(DEV)
    px = (torch.rand(B, N, generator=g) * (W + 3) - 2).to(DEV)
    py = (torch.rand(B, N, generator=g) * (H + 3) - 2).to(DEV)
    px[:, 16:48], py[:, 16:48] = 5.25, 7.5                # 32 points in one cell
    dstats = torch.randn(B, N, 8, generator=g).to(DEV)
    dabs = torch.randn(B, C, generator=g).to(DEV)
    check(lambda: list(ops.sample_stats_grad(conv1, conv2, px, py, dstats, dabs, deterministic=True)), names=["dconv1", "dconv2", "dpos"])


# ======================================================================================================================
# backward of the dense assembly
# ======================================================================================================================
ADJOINT_MODES = ("accumulate", "overwrite", "overwrite_map", "fold", "fold_overwrite")     # flags 0, OVERWRITE, OVERWRITE | OVERWRITE_MAP, FOLD_TARGET (+ both)


def _adjoint_run(intr, level, variant, R, T, Wc, G, gb, gabs, mode):
    from banet_amd import dense as bdense, dense_train

    def run():
        ba = bdense.DenseBA(intr, [level], [lambda_weights(level.C, 5)], variant, 1000.0)
        prob = ba.problems[0]
        B, H, W, C, K = level.B, level.H, level.W, level.C, prob.K
        fold = mode.startswith("fold")
        ow = mode in ("overwrite", "overwrite_map", "fold_overwrite")
        owm = mode in ("overwrite_map", "fold_overwrite")
        nan = float("nan")                                  # overwrite modes: every entry is written, nothing is read
        dsrc = torch.full((B, H * W, C), nan if ow else 0.0, device=DEV)
        dmap = torch.full((B, H, W, C if fold else 3 * C), nan if owm else 0.0, device=DEV)
        ddepth = torch.full((B, H * W), nan if ow else 0.0, device=DEV)
        dbasis = torch.full((B, H * W, K), nan if ow else 0.0, device=DEV)
        dpose, _ = dense_train.dense_adjoint(prob, R, T, Wc, G, gb, gabs, dsrc, dmap, ddepth, dbasis, overwrite=ow, overwrite_map=owm, fold=fold)
        return [dsrc, dmap, ddepth, dbasis, dpose]
    return run


def _adjoint_inputs(B, H, W, C, K, seed, pairs=1):
    from banet_amd import synth as bsynth
    intr, levels, gt = bsynth.make_dense_windows(B, H, W, C, K, [1], seed, torch.device(DEV), trans_mag=0.06, pairs=pairs)
    g = torch.Generator().manual_seed(seed)
    P = 6 + K
    R = torch.eye(3, device=DEV).repeat(B, 1, 1)
    T = (gt["T"].reshape(B, pairs, 3)[:, 0] * 0.7).reshape(B, 3, 1).to(DEV).contiguous()
    Wc = (0.02 * torch.randn(B, K, 1, generator=g)).to(DEV)
    G = torch.randn(B, P, P, generator=g).to(DEV)
    gb = torch.randn(B, P, generator=g).to(DEV)
    gabs = (0.1 * torch.randn(B, C, generator=g)).to(DEV)
    return intr, levels[0], R, T, Wc, G, gb, gabs


@pytest.mark.parametrize("mode", ADJOINT_MODES)
@pytest.mark.parametrize("H,W,C,K,variant", [(41, 57, 128, 128, "bundle"), (37, 53, 70, 33, "bundle"), (10, 13, 16, 8, "bundle"),
                                             (20, 24, 128, 256, "bundle"), (18, 22, 70, 200, "bundle"), (37, 53, 128, 0, "bundle_camera")])
def test_dense_adjoint(H, W, C, K, variant, mode):
    """banet_dense_adjoint_ex_f32 through dense_train.dense_adjoint: S, z2, the per-pixel records, the 3C rows (or, with
    BANET_ADJOINT_FOLD_TARGET, the sorted cell lists and the big-cell queue), the cell counts / starts / cursors, the per-wave
    partial rows of dpose; K <= 128 (two pixels per wave), K > 128 (wide seed blocks), pose only (the zeroed record array stands in
    for basis / z2)."""
    intr, level, R, T, Wc, G, gb, gabs = _adjoint_inputs(2, H, W, C, K, 700 + K)
    check(_adjoint_run(intr, level, variant, R, T, Wc, G, gb, gabs, mode), names=["dsrc", "dmap", "ddepth", "dbasis", "dpose"],
          min_workspaces=2)


@pytest.mark.parametrize("mode", ["accumulate", "fold", "fold_overwrite"])
def test_dense_adjoint_with_a_collapsed_warp(mode):
    """the scene of test_target_tile_adjoint_with_a_collapsed_warp: hundreds of pixels per target cell (big-cell queue, rank sort)"""
    from banet_amd import dense as bdense
    from test_gpu_dense_backward import _scene, t
    H, W, C, K = 24, 32, 16, 8
    intr, levels, R, T, Wc, rng = _scene(H, W, C, K, 21)
    lv = levels[0]
    T = T.copy()
    T[:, 2, 0] += 60.0
    B, P = 2, 6 + K
    G, gb, gabs = rng.standard_normal((B, P, P)), rng.standard_normal((B, P)), rng.standard_normal((B, C)) * 0.1
    level = bdense.DenseLevel(lv["scale"], t(lv["src"]), t(lv["tgt"]), t(lv["D0"]), t(lv["basis"]))
    outs = check(_adjoint_run(t(intr), level, "bundle", t(R), t(T), t(Wc), t(G), t(gb), t(gabs), mode),
                 names=["dsrc", "dmap", "ddepth", "dbasis", "dpose"], min_workspaces=2)
    if mode != "accumulate":
        hit = (outs["zero"][1].abs().amax(dim=-1) > 0).reshape(B, -1).sum(dim=1)
        assert 0 < int(hit.max()) <= 64, hit                        # the window's footprint really is a handful of texels


@pytest.mark.parametrize("K", [32, 128])
def test_dense_adjoint_reusing_the_depth_seed_is_the_one_documented_exception(K):
    """BANET_ADJOINT_REUSE_DEPTH_SEED reads z2 / zeta / e of the PREVIOUS call from the workspace -- tested as a pair: the workspace is
    poisoned before the first call only, the second call (the window's second target frame) reuses it.  The pair's results are equal
    across the fills, and equal to the pair that recomputes everything."""
    from banet_amd import dense as bdense, dense_train, synth as bsynth
    B, H, W, C, pairs = 2, 37, 53, 32, 2
    intr, levels, gt = bsynth.make_dense_windows(B, H, W, C, K, [1], 711, torch.device(DEV), trans_mag=0.06, pairs=pairs)
    g = torch.Generator().manual_seed(K)
    P = 6 + K
    R = torch.eye(3, device=DEV).repeat(B, 1, 1)
    Ts = [(gt["T"][:, i] * 0.7).reshape(B, 3, 1).to(DEV).contiguous() for i in range(pairs)]
    Wc = (0.02 * torch.randn(B, K, 1, generator=g)).to(DEV)
    Gs = [torch.randn(B, P, P, generator=g).to(DEV) for _ in range(pairs)]
    gbs = [torch.randn(B, P, generator=g).to(DEV) for _ in range(pairs)]
    for i in range(1, pairs):                                  # the flag's premise: the depth block of gAtA and the depth part of gAtb
        Gs[i][:, 6:, 6:] = Gs[0][:, 6:, 6:]                    # are those of the previous call
        gbs[i][:, 6:] = gbs[0][:, 6:]
    gabs = (0.1 * torch.randn(B, C, generator=g)).to(DEV)

    def pair(reuse):
        def run():
            ba = bdense.DenseBA(intr, levels, [lambda_weights(C, 5)], "bundle", 1.0)
            probs = dense_train._pair_problems(ba, 0)
            nan = float("nan")
            dsrc, ddepth, dbasis = torch.full((B, H * W, C), nan, device=DEV), torch.full((B, H * W), nan, device=DEV), torch.full((B, H * W, K), nan, device=DEV)
            dmap = [torch.full((B, H, W, C), nan, device=DEV) for _ in range(pairs)]
            ws, out = None, []
            for i in range(pairs):
                dpose, ws2 = dense_train.dense_adjoint(probs[i], R, Ts[i], Wc, Gs[i], gbs[i], gabs, dsrc, dmap[i], ddepth, dbasis, ws,
                                                      overwrite=i == 0, overwrite_map=True, fold=True,
                                                      extra_flags=dense_train.ADJOINT_REUSE_DEPTH_SEED if (reuse and i > 0) else 0)
                assert ws is None or ws2 is ws                 # the second call runs in the first call's workspace
                ws = ws2
                out.append(dpose)
            return [dsrc, ddepth, dbasis] + dmap + out
        return run
    reused = check(pair(True), min_workspaces=2)
    fresh = check(pair(False), min_workspaces=2)
    for x, y in zip(reused["nan"], fresh["nan"]):
        assert torch.equal(x, y)


# (variant, B, C, K, pairs): one rung of a group each -- P < 32 (in-kernel factorisation), P >= 32 (LDS solve), pairs > 1, camera
@pytest.mark.parametrize("grp", [("bundle", 3, 32, 8, 1), ("bundle", 3, 32, 33, 1), ("bundle", 3, 32, 7, 2), ("bundle_camera", 3, 32, 0, 3),
                                 ("bundle", 3, 32, 128, 1), ("bundle", 37, 32, 8, 1), ("bundle", 3, 255, 33, 1)])
def test_small_step_adjoint(grp):
    """banet_small_step_adjoint_f32 (SmallStepHip, two accumulating calls): the damped matrix, right-hand side, its adjoint, the
    per-window scalars and the MLP activations / deltas all live in the workspace"""
    import small_step_cases as ssc
    from test_gpu_small_step import _run_hip
    case = ssc.make_case(*grp, 1, 3)
    check(lambda: _run_hip(case), names=list(ssc.OUTPUTS))


# ======================================================================================================================
# end to end
# ======================================================================================================================
def test_dense_solve_over_three_levels_in_one_shared_workspace():
    """DenseBA sizes ONE workspace for all its levels and runs them one after another in it: each level starts on the previous
    level's leftovers, laid out by another kernel selection (4x4 items -> direct tiles -> strip segments forced on the finest)"""
    from banet_amd import dense as bdense, ops
    intr, levels, mlps, T0 = _lm_case(2, 96, 128, 128, 1, [4, 2, 1], 651)

    def make(order):
        def run():
            lv = [levels[i] for i in order]
            ba = bdense.DenseBA(intr, lv, [mlps[i] for i in order], "bundle", 1000.0)
            for prob, bits in zip(ba.problems, [(QUAD, DIRECT, STRIP | SYRK_F16)[i] for i in order]):
                prob.c.flags = bits
            sizes = [ops.lm_level_workspace_bytes(p) for p in ba.problems]
            assert len(set(sizes)) == 3 and [s_ for _, s_ in sorted(zip([l.H for l in lv], sizes))] == sorted(sizes)
            st, counts = ba.solve([3, 3, 3], ba.new_state(T=T0.clone()))
            return [st.R, st.T, st.Wc, st.lambda_out, st.delta] + list(counts)
        return run
    check(make([0, 1, 2]))          # coarse to fine: ascending sizes
    check(make([2, 1, 0]))          # descending sizes: the small levels run inside the big level's leftovers


@pytest.mark.parametrize("frames,variant,K", [(2, "bundle", 16), (3, "bundle", 16), (2, "bundle_camera", 0), (2, "bundle", 136)])
def test_solve_differentiable_forward_and_backward(frames, variant, K):
    """DenseBA.solve_differentiable, two levels x two iterations, forward plus backward: gradients to the feature maps, depth, basis
    and the lambda weights (assembly, solve with and without its workspace, dense adjoint with the depth-seed reuse, small step)"""
    from banet_amd import dense as bdense, synth as bsynth
    B, H, W, C = 2, 48, 64, 32
    scales = [2, 1]
    intr, levels, gt = bsynth.make_dense_windows(B, H, W, C, K, scales, 7, torch.device(DEV), trans_mag=0.06, pairs=frames - 1)
    base = [lambda_weights(C, 100 + i) for i in range(len(scales))]
    T0 = (gt["T"] * 0.7).reshape(B * (frames - 1), 3, 1).to(DEV)
    names = ("src", "tgt", "depth") + (("basis",) if K else ())

    def run():
        mlps = [[(w.clone().to(DEV).requires_grad_(True), b.clone().to(DEV).requires_grad_(True)) for w, b in lw] for lw in base]
        lvs = [bdense.DenseLevel(lv.scale, *[getattr(lv, nm).detach().clone().requires_grad_(True) if getattr(lv, nm) is not None else None
                                             for nm in ("src", "tgt", "depth", "basis")]) for lv in levels]
        ba = bdense.DenseBA(intr, lvs, mlps, variant, 1.0)
        leaves = [getattr(lv, nm) for lv in lvs for nm in names] + [x for lw in mlps for wb in lw for x in wb]
        Rr, Tt, Ww = ba.solve_differentiable([2, 2], T=T0)
        loss = (Rr * torch.arange(Rr.numel(), device=DEV).reshape(Rr.shape).float().cos()).sum() + Tt.sum()
        if K:
            loss = loss + (Ww * 0.5).sum()
        return [Rr, Tt] + ([Ww] if K else []) + list(torch.autograd.grad(loss, leaves))
    check(run, min_workspaces=4)


@pytest.mark.parametrize("B,N,C,K,H,W", [(1, 777, 70, 33, 40, 56), (2, 4096, 128, 128, 96, 128)])
def test_fused_sparse_training_iteration(B, N, C, K, H, W):
    """the fused sparse training iteration of test_fused_sparse_training_iteration_equals_the_lean_graph (BundleIteration and
    CameraIteration with gradients, training_graph "fused"), updates and every gradient"""
    from banet_amd import ops
    from banet_amd.bundlenet import BundleNet
    g = torch.Generator().manual_seed(1000 + N)
    img = torch.randn(B, H, W, C, generator=g).to(DEV)
    conv2 = ops.target_map(img)
    pts = torch.stack([torch.rand(B, N, generator=g) * (W - 1.5) + 0.25, torch.rand(B, N, generator=g) * (H - 1.5) + 0.25], dim=-1).to(DEV)
    conv1 = ops.resample(img, pts) + 0.05 * torch.randn(B, N, C, generator=g).to(DEV)
    fx = torch.full((B, N), 0.8 * W, device=DEV)
    fy = fx.clone()
    ox, oy = torch.full((B, N), W / 2.0, device=DEV), torch.full((B, N), H / 2.0, device=DEV)
    ray = torch.stack([(pts[..., 0] - ox) / fx, (pts[..., 1] - oy) / fy, torch.ones(B, N, device=DEV)], dim=1)
    p = ray / ray.norm(dim=1, keepdim=True)
    D = (2.5 + torch.rand(B, N, 1, generator=g)).to(DEV)
    Bs = (torch.randn(B, N, K, generator=g) / K ** 0.5).to(DEV)
    R = torch.eye(3, device=DEV).repeat(B, 1, 1)
    T = (0.02 * torch.randn(B, 3, 1, generator=g)).to(DEV)
    Wc = (0.01 * torch.randn(B, K, 1, generator=g)).to(DEV)
    cR, cT, cW = [torch.randn(x.shape, generator=g).to(DEV) for x in (R, T, Wc)]
    base = lambda_weights(C, 7)

    def run():
        lw = [(w.clone().to(DEV).requires_grad_(True), b.clone().to(DEV).requires_grad_(True)) for w, b in base]
        leaves = [x.clone().requires_grad_(True) for x in (conv1, conv2, D, Bs, R, T, Wc)]
        net = BundleNet(lambda_weights={"0": lw})
        net.training_graph = "fused"
        R2, T2, W2 = net.BundleIteration(leaves[0], leaves[1], fx, fy, ox, oy, p, leaves[2], leaves[3], leaves[4], leaves[5], leaves[6], 1000.0, "0")
        Rc, Tc = net.CameraIteration(leaves[0], leaves[1], fx, fy, ox, oy, p, leaves[2], leaves[4], leaves[5], 1.0, "0")
        loss = (R2 * cR).sum() + (T2 * cT).sum() + (W2 * cW).sum()
        grads = torch.autograd.grad(loss, leaves + [x for wb in lw for x in wb])
        gc = torch.autograd.grad((Rc * cR).sum() + (Tc * cT).sum(), [leaves[0], leaves[1], leaves[2], leaves[4], leaves[5]] + [x for wb in lw for x in wb])
        return [R2, T2, W2, Rc, Tc] + list(grads) + list(gc)
    check(run, min_workspaces=2)


# ======================================================================================================================
# one arena, two problems: X, Y, X
# ======================================================================================================================
def test_arena_reuse_by_two_lm_levels_with_different_kernel_selections():
    """A C caller's arena, sized for the larger of two problems: X = a strip-gather level with K = 128 (fp16 SYRK in the loop), Y = a
    4x4-item pose-only level with two target frames.  X, Y, X in the same bytes: X equals X, Y equals Y on a fresh zeroed buffer."""
    from banet_amd import dense as bdense, ops
    cx = _lm_case(2, 48, 64, 128, 1, [1], 661)
    cy = _lm_case(3, 37, 53, 0, 2, [1], 662)

    def solve(case, variant, flags, expect, ws):
        intr, levels, mlps, T0 = case
        ba = bdense.DenseBA(intr, levels, mlps, variant, 1000.0)
        prob = ba.problems[0]
        prob.c.flags = flags
        assert (ops.gather_selection(prob), ops.syrk_selection(prob)) == expect
        st = ba.new_state(T=T0.clone())
        nb = ops.lm_level_workspace_bytes(prob)
        assert ws is None or ws.numel() >= nb
        used = ops.lm_level(prob, ba.mlps[0], ba.l2_base, 3, False, st, ws=ws)
        assert ws is None or used is ws
        torch.cuda.synchronize()
        return nb, [x.clone() for x in (st.R, st.T, st.iters, st.lambda_out, st.delta)] + ([st.Wc.clone()] if st.Wc is not None else [])
    X = (cx, "bundle", STRIP | SYRK_F16, (3, 4))
    Y = (cy, "bundle_camera", QUAD, (4, -1000))
    nbx, _ = solve(*X, None)
    nby, _ = solve(*Y, None)
    _, y_fresh = solve(*Y, wsc.guarded_workspace(nby, DEV, "zero")[0])
    assert nbx != nby
    for fill in ("zero", "nan", "one"):
        ws, h = wsc.guarded_workspace(max(nbx, nby), DEV, fill)
        _, x1 = solve(*X, ws)
        _, y = solve(*Y, ws)
        _, x2 = solve(*X, ws)
        _, y2 = solve(*Y, ws)
        wsc.assert_guards_intact(h)
        for a, b in zip(x1, x2):
            assert torch.equal(a, b), fill
        for a, b, c in zip(y, y_fresh, y2):
            assert torch.equal(a, b) and torch.equal(a, c), fill
        assert all(bool(torch.isfinite(a).all()) for a in x1 + y if a.dtype.is_floating_point)


def test_arena_reuse_by_two_dense_adjoints():
    """the same for the backward: X = the tile-kernel adjoint of a K = 128 level, Y = the row-gather adjoint of a pose-only level"""
    from banet_amd import dense as bdense, dense_train
    ax = _adjoint_inputs(2, 41, 57, 128, 128, 671)
    ay = _adjoint_inputs(3, 37, 53, 70, 0, 672)

    def adjoint(a, variant, fold, ws):
        intr, level, R, T, Wc, G, gb, gabs = a
        ba = bdense.DenseBA(intr, [level], [lambda_weights(level.C, 5)], variant, 1000.0)
        prob = ba.problems[0]
        B, H, W, C, K = level.B, level.H, level.W, level.C, prob.K
        nan = float("nan")
        outs = [torch.full((B, H * W, C), nan, device=DEV), torch.full((B, H, W, C if fold else 3 * C), nan, device=DEV),
                torch.full((B, H * W), nan, device=DEV), torch.full((B, H * W, K), nan, device=DEV)]
        dpose, used = dense_train.dense_adjoint(prob, R, T, Wc, G, gb, gabs, *outs, ws, overwrite=True, overwrite_map=True, fold=fold)
        assert ws is None or used is ws
        torch.cuda.synchronize()
        return used.numel(), outs + [dpose]
    nbx, _ = adjoint(ax, "bundle", True, None)
    nby, _ = adjoint(ay, "bundle_camera", False, None)
    _, y_fresh = adjoint(ay, "bundle_camera", False, wsc.guarded_workspace(nby, DEV, "zero")[0])
    for fill in ("zero", "nan", "one"):
        ws, h = wsc.guarded_workspace(max(nbx, nby), DEV, fill)
        _, x1 = adjoint(ax, "bundle", True, ws)
        _, y = adjoint(ay, "bundle_camera", False, ws)
        _, x2 = adjoint(ax, "bundle", True, ws)
        wsc.assert_guards_intact(h)
        for a, b in zip(x1, x2):
            assert torch.equal(a, b) and bool(torch.isfinite(a).all()), fill
        for a, b in zip(y, y_fresh):
            assert torch.equal(a, b) and bool(torch.isfinite(a).all()), fill


# ======================================================================================================================
# output extents: the outputs carved out of guard-banded buffers, straight over ctypes
# ======================================================================================================================
class _Out:
    """output tensors inside guard bands; NaN-filled (float) / 0x7F-filled (bytes) so that an entry left unwritten shows"""

    def __init__(self):
        self.handles = []

    def f32(self, *shape, fill=float("nan")):
        n = int(np.prod(shape)) * 4
        body, h = wsc.guarded_workspace(n, DEV, "zero")
        self.handles.append(h)
        assert n > 0
        out = body[:n].view(torch.float32).reshape(shape)
        out.fill_(fill)
        if n < body.numel():
            body[n:].fill_(wsc.GUARD_BYTE)             # the rounding of tiny outputs up to 256 bytes belongs to the guard
        return out

    def i32(self, *shape):
        return self.f32(*shape, fill=0.0).view(torch.int32)


def _tail_intact(out_tensor, handle):
    n = out_tensor.numel() * out_tensor.element_size()
    return bool((handle.body[n:] == wsc.GUARD_BYTE).all())


@pytest.mark.parametrize("H,W,K,pairs,bits", [(41, 57, 128, 1, 0), (37, 53, 32, 3, STRIP), (10, 13, 32, 1, QUAD), (37, 53, 0, 2, DIRECT),
                                              (41, 57, 128, 1, PATCH), (37, 53, 128, 3, GENERIC)])
def test_output_extents_of_the_assembly_with_mask(H, W, K, pairs, bits):
    from banet_amd import _capi as capi, dense as bdense
    B = 2
    intr, levels, R, T, Wc = _window_inputs(B, H, W, K, pairs, 800 + K + pairs)
    ba = bdense.DenseBA(intr, levels, [lambda_weights(128, 9)], "bundle" if K else "bundle_camera", 1000.0)
    prob = ba.problems[0]
    prob.c.flags = bits
    P, C, N = prob.P, prob.C, prob.N
    o = _Out()
    AtA, Atb, absres, nvalid = o.f32(B, P, P), o.f32(B, P), o.f32(B, C), o.f32(B)
    mbody, mh = wsc.guarded_workspace(B * pairs * N, DEV, "zero")
    mbody.fill_(wsc.GUARD_BYTE)
    mask = mbody[:B * pairs * N]
    L = capi.lib()
    nb = L.banet_ba_assemble_workspace_bytes(ctypes.byref(prob.c))
    ws, wh = wsc.guarded_workspace(nb, DEV, "nan")
    capi.check(L.banet_ba_assemble_mask_f32(ctypes.byref(prob.c), capi.ptr(R), capi.ptr(T), capi.ptr(Wc), capi.ptr(AtA), capi.ptr(Atb),
                                            capi.ptr(absres), capi.ptr(nvalid), ctypes.c_void_p(mask.data_ptr()),
                                            ctypes.c_void_p(ws.data_ptr()), ws.numel(), capi.stream()))
    torch.cuda.synchronize()
    for h in o.handles + [mh, wh]:
        wsc.assert_guards_intact(h)
    for x, h in zip((AtA, Atb, absres, nvalid), o.handles):
        assert bool(torch.isfinite(x).all()) and _tail_intact(x, h)                  # every entry written, nothing behind the last one
    assert int(mask.max()) <= 1 and bool((mbody[B * pairs * N:] == wsc.GUARD_BYTE).all())
    assert float(mask.reshape(B, -1).sum(1).float().sub(nvalid).abs().max()) == 0.0


@pytest.mark.parametrize("H,W,K,pairs,variant,early", [(41, 57, 128, 1, "bundle", False), (37, 53, 32, 3, "bundle", False), (37, 53, 0, 2, "bundle_camera", False),
                                                       (35, 45, 256, 1, "bundle", False), (41, 57, 0, 1, "legacy_lm", True)])
def test_output_extents_of_the_lm_level_state(H, W, K, pairs, variant, early):
    """banet_lm_level_ex_f32 writes R, T, Wc, iters, ratio, lambda_out, delta of exactly B windows"""
    from banet_amd import _capi as capi, dense as bdense, ops
    B = 3
    C = 8 if early else 128
    intr, levels, mlps, T0 = _lm_case(B, H, W, K, pairs, [1], 810 + K + pairs, C=C, normalize_rays=not early)
    ba = bdense.DenseBA(intr, levels, mlps, variant, 1000.0 if variant == "bundle" else 1.0)
    prob = ba.problems[0]
    P = prob.P
    o = _Out()
    R, T = o.f32(B, pairs, 3, 3), o.f32(B, pairs, 3, 1)
    R.copy_(torch.eye(3, device=DEV).expand(B, pairs, 3, 3))
    T.copy_(T0.reshape(B, pairs, 3, 1))
    Wc = o.f32(B, K, 1, fill=0.0) if K else None
    iters, ratio, lam, delta = o.i32(B), o.f32(B, fill=0.0), o.f32(B, fill=0.0), o.f32(B, P, fill=0.0)
    st = capi.State()
    st.R, st.T, st.Wc = R.data_ptr(), T.data_ptr(), Wc.data_ptr() if K else None
    st.iters, st.ratio, st.lambda_out, st.delta = iters.data_ptr(), ratio.data_ptr(), lam.data_ptr(), delta.data_ptr()
    L = capi.lib()
    nb = L.banet_lm_level_workspace_bytes(ctypes.byref(prob.c))
    ws, wh = wsc.guarded_workspace(nb, DEV, "one")
    mlp = ba.mlps[0]
    capi.check(L.banet_lm_level_ex_f32(ctypes.byref(prob.c), ctypes.byref(mlp.c), float(ba.l2_base), 3, int(early), None, ctypes.byref(st),
                                       ctypes.c_void_p(ws.data_ptr()), ws.numel(), capi.stream()))
    torch.cuda.synchronize()
    for h in o.handles + [wh]:
        wsc.assert_guards_intact(h)
    outs = [R, T] + ([Wc] if K else []) + [iters, ratio, lam, delta]
    for x, h in zip(outs, o.handles):
        assert _tail_intact(x, h)
        if x.dtype.is_floating_point:
            assert bool(torch.isfinite(x).all())
    assert int(iters.min()) >= (0 if early else 3) and int(iters.max()) <= 3


@pytest.mark.parametrize("H,W,C,K,variant,fold", [(41, 57, 128, 128, "bundle", True), (41, 57, 128, 128, "bundle", False), (37, 53, 70, 33, "bundle", True),
                                                  (10, 13, 16, 8, "bundle", False), (20, 24, 128, 256, "bundle", True), (37, 53, 128, 0, "bundle_camera", True),
                                                  (37, 53, 70, 0, "bundle_camera", False)])
def test_output_extents_of_the_dense_adjoint(H, W, C, K, variant, fold):
    """banet_dense_adjoint_ex_f32 with OVERWRITE | OVERWRITE_MAP (+ FOLD_TARGET): every entry of dsrc / dmap3 / ddepth / dbasis / dpose
    written, nothing outside them"""
    from banet_amd import _capi as capi, dense as bdense
    B = 2
    intr, level, R, T, Wc, G, gb, gabs = _adjoint_inputs(B, H, W, C, K, 820 + K)
    ba = bdense.DenseBA(intr, [level], [lambda_weights(C, 5)], variant, 1000.0)
    prob = ba.problems[0]
    N = H * W
    o = _Out()
    dsrc, dmap, ddepth = o.f32(B, N, C), o.f32(B, H, W, C if fold else 3 * C), o.f32(B, N)
    dbasis = o.f32(B, N, K) if K else None
    dpose = o.f32(B, 12 + K)
    flags = 1 | 2 | (4 if fold else 0)
    L = capi.lib()
    nb = L.banet_dense_adjoint_workspace_bytes_ex(ctypes.byref(prob.c), flags)
    assert nb > 0
    ws, wh = wsc.guarded_workspace(nb, DEV, "nan")
    capi.check(L.banet_dense_adjoint_ex_f32(ctypes.byref(prob.c), capi.ptr(R), capi.ptr(T), capi.ptr(Wc) if K else None, capi.ptr(G), capi.ptr(gb),
                                            capi.ptr(gabs), capi.ptr(dsrc), capi.ptr(dmap), capi.ptr(ddepth), capi.ptr(dbasis) if K else None,
                                            capi.ptr(dpose), flags, ctypes.c_void_p(ws.data_ptr()), ws.numel(), capi.stream()))
    torch.cuda.synchronize()
    for h in o.handles + [wh]:
        wsc.assert_guards_intact(h)
    for x, h in zip([dsrc, dmap, ddepth] + ([dbasis] if K else []) + [dpose], o.handles):
        assert bool(torch.isfinite(x).all()) and _tail_intact(x, h)


@pytest.mark.parametrize("grp", [("bundle", 3, 32, 8, 1), ("bundle", 3, 32, 33, 1), ("bundle", 3, 32, 7, 2), ("bundle_camera", 3, 32, 0, 3),
                                 ("bundle", 2, 255, 128, 1)])
def test_output_extents_of_the_small_step_adjoint(grp):
    """banet_small_step_adjoint_f32: gAtA / gAtb / gabs / dR / dT written (every entry), the ten weight gradients accumulated in
    place, nothing outside them"""
    import small_step_cases as ssc
    from banet_amd import _capi as capi, ops
    variant, B, C, K, pairs = grp
    case = ssc.make_case(variant, B, C, K, pairs, 1, 4)
    N, P = case["N"], case["P"]
    dev = torch.device(DEV)
    mlp = ops.MlpWeights([(w.float(), b.float()) for w, b in case["layers"]], dev)
    c = lambda x: x.float().to(dev).contiguous()
    ins = [c(case[k]) for k in ("AtA", "Atb", "absres", "delta", "R", "T", "gR", "gT")] + [c(case["gW"]) if K else None]
    o = _Out()
    gAtA, gAtb, gabs, dR, dT = o.f32(B, P, P), o.f32(B, P), o.f32(B, C), o.f32(B, pairs, 3, 3), o.f32(B, pairs, 3, 1)
    dims = [C, 2 * C, 4 * C, 2 * C, C, 1]
    gl = []
    gm = capi.Mlp()
    for i in range(5):
        gl += [o.f32(dims[i], dims[i + 1], fill=0.0), o.f32(dims[i + 1], fill=0.0)]
        gm.w[i], gm.b[i] = gl[-2].data_ptr(), gl[-1].data_ptr()
    L = capi.lib()
    v = ops._VARIANT_OF[variant]
    nb = L.banet_small_step_adjoint_workspace_bytes(v, B, N, C, K, pairs)
    assert nb > 0
    ws, wh = wsc.guarded_workspace(nb, DEV, "nan")
    capi.check(L.banet_small_step_adjoint_f32(v, B, N, C, K, pairs, float(case["l2_base"]), ctypes.byref(mlp.c),
                                              *[capi.ptr(x) if x is not None else None for x in ins], capi.ptr(gAtA), capi.ptr(gAtb),
                                              capi.ptr(gabs), capi.ptr(dR), capi.ptr(dT), ctypes.byref(gm), ctypes.c_void_p(ws.data_ptr()),
                                              ws.numel(), capi.stream()))
    torch.cuda.synchronize()
    for h in o.handles + [wh]:
        wsc.assert_guards_intact(h)
    for x, h in zip([gAtA, gAtb, gabs, dR, dT] + gl, o.handles):
        assert bool(torch.isfinite(x).all()) and _tail_intact(x, h)
