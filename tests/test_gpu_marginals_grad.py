"""banet_ba_marginals_grad_f32 on the GPU (csrc/marginals_grad.hip) against tests/marginals_grad_ref.py: the float64 closed form as
the reference, the same closed form in float32 (np.linalg.cholesky on the float32 matrix) as the yardstick.

Gate per case and error (marginals_grad_ref.gates): max(4 x the yardstick's error on the same case, (P + N) 2^-24), on the scales of
marginals_grad_ref.errors -- gAtA per block relative to the block's largest entry, gbasis per pixel relative to the row's largest
entry (rows with g_depth_var = 0 exactly 0), gdamping / gsigma2 relative to the sums of the magnitudes of their terms.  Every case
prints its figures before it asserts; with BANET_MARGINALS_GRAD_REPORT set to a file name the per-family maxima are written there
at the end of the module (profiles/marginals_grad.txt quotes such a run).  Three windows and N <= 3072 throughout."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import marginals_grad_ref as gr
import marginals_ref as mr
import ws_contract as wsc
from test_gpu_marginals import Bare, same_bits, t32, tail_case      # the forward module's helpers: the same levels, the same tail matrices

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
OUT_NAMES = ("gAtA", "gdamping", "gsigma2", "gbasis", "status")
IN_NAMES = ("g_pose_cov", "g_depth_var", "g_logdet")
UPS_OF = dict(g_pose_cov="g_cov", g_depth_var="g_dv", g_logdet="g_ld")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from banet_amd import _capi
    _capi.lib()
    return torch.device("cuda:0")


REPORT = {}


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    path = os.environ.get("BANET_MARGINALS_GRAD_REPORT")
    if path and REPORT:
        with open(path, "w") as f:
            f.write("family error cases max_error max_yardstick max_error_over_gate\n")
            for (family, k), (n, e, y, r) in sorted(REPORT.items()):
                f.write("%s %s %d %.3e %.3e %.3f\n" % (family, k, n, e, y, r))


def record(family, err, yard, gate):
    for k in err:
        n, e, y, r = REPORT.get((family, k), (0, 0.0, 0.0, 0.0))
        REPORT[(family, k)] = (n + 1, max(e, err[k]), max(y, yard.get(k, 0.0)), max(r, err[k] / gate[k]))


def new_outs(B, N, K, pairs, dev, names=OUT_NAMES):
    P = 6 * max(pairs, 1) + K
    shapes = dict(gAtA=(B, P, P), gdamping=(B,), gsigma2=(B,), gbasis=(B, N, K), status=(B,))
    return {k: torch.full(shapes[k], -7, dtype=torch.int32 if k == "status" else torch.float32, device=dev) for k in names}


def raw_call(lv, AtA, damping, sigma2, ins, outs, fill=None, arena=None):
    """the C entry with caller-owned tensors (dicts by field name; missing = NULL) -> the guarded workspace's handle, or None"""
    from banet_amd import _capi as capi
    L = capi.lib()
    gin, gout = capi.MarginalsGradIn(), capi.MarginalsGradOut()
    for k, v in ins.items():
        setattr(gin, k, v.data_ptr())
    for k, v in outs.items():
        setattr(gout, k, v.data_ptr())
    nb = L.banet_ba_marginals_grad_workspace_bytes(ctypes.byref(lv.c), int("gbasis" in outs))
    assert nb > 0
    handle = None
    if fill is None:
        ws = capi.workspace(nb, AtA.device)
    else:
        ws, handle = wsc.guarded_workspace(nb, AtA.device, fill, arena)
        assert ws.numel() == nb
    capi.check(L.banet_ba_marginals_grad_f32(ctypes.byref(lv.c), capi.ptr(AtA), capi.ptr(damping), capi.ptr(sigma2), ctypes.byref(gin),
                                             ctypes.byref(gout), ctypes.c_void_p(ws.data_ptr()), ws.numel(), capi.stream()))
    return handle


def run_case(case, ups, dev, windows=None, names=OUT_NAMES, ins=IN_NAMES, fill=None, arena=None, zero_for_missing=False, basis=None):
    """the case (or the given windows of it, in that order) through the C entry -> dict of numpy arrays.  ins: the upstream
    gradients passed (the others NULL, or zero-filled tensors with zero_for_missing)"""
    idx = list(range(case["B"])) if windows is None else list(windows)
    if basis is None:
        basis = t32(case["basis"][idx], dev) if case["K"] > 0 else None
    lv = Bare(len(idx), case["N"], case["K"], case["pairs"], basis)
    outs = new_outs(len(idx), case["N"], case["K"], case["pairs"], dev, names)
    gin = {}
    for k in IN_NAMES:
        if k in ins:
            gin[k] = t32(ups[UPS_OF[k]][idx], dev)
        elif zero_for_missing:
            gin[k] = torch.zeros_like(t32(ups[UPS_OF[k]][idx], dev))
    h = raw_call(lv, t32(case["AtA"][idx], dev), t32(None if case["damping"] is None else case["damping"][idx], dev),
                 t32(None if case["sigma2"] is None else case["sigma2"][idx], dev), gin, outs, fill=fill, arena=arena)
    torch.cuda.synchronize()
    if h is not None:
        wsc.assert_guards_intact(h)
    return {k: v.cpu().numpy() for k, v in outs.items()}


def check_parity(case, got, family, ref=None):
    ups, want, yard = ref if ref is not None else gr.reference(case)
    gate = gr.gates(case, yard)
    err = gr.errors(case, ups, got, want)
    print("%s %s seed %d: " % (family, mr.spec_id(case["spec"]), case["seed"]) +
          "  ".join("%s %.2e (yardstick %.2e, gate %.2e)" % (k, err[k], yard[k], gate[k]) for k in gr.ERRORS))
    record(family, err, yard, gate)
    if "status" in got:
        assert list(got["status"]) == [int(f) for f in case["expect_fail"]]
    for k in gr.ERRORS:
        assert err[k] <= gate[k], (k, err[k], gate[k])


# ---- 1. parity --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", mr.LADDER, ids=mr.spec_id)
def test_parity_ladder(dev, spec):
    for seed in mr.SEEDS:
        case = mr.make("ladder", spec, seed)
        ups = gr.reference(case)[0]
        got = run_case(case, ups, dev)
        assert np.array_equal(got["gAtA"], got["gAtA"].transpose(0, 2, 1))          # exactly symmetric
        check_parity(case, got, "ladder")


@pytest.mark.parametrize("spec", mr.ASSEMBLED, ids=mr.spec_id)
def test_parity_assembled(dev, spec):
    case = mr.make("assembled", spec, 0)
    ref = gr.reference(case)
    check_parity(case, run_case(case, ref[0], dev), "assembled", ref)


# ---- 2. tails of the two basis passes ---------------------------------------------------------------------------------------------
TAILS = [(N, K) for N in (31, 33, 200) for K in (1, 31, 32, 33, 130, 256)]


@pytest.mark.parametrize("N,K", TAILS, ids=lambda v: str(v))
def test_tails_against_float64_aligned_and_offset_basis_with_guards(dev, N, K):
    case = tail_case(N, K)
    B = case["B"]
    ref = gr.reference(case)
    got = run_case(case, ref[0], dev, fill="nan")
    check_parity(case, got, "tails", ref)
    # the same with the basis a view offset by one float (4-byte aligned only) between NaNs, gbasis offset likewise inside a guard
    flat = torch.zeros(B * N * K + 1 + 64, dtype=torch.float32, device=dev)
    flat[-64:] = float("nan")                                       # read past the tensor's end: poisons the result
    flat[0] = float("nan")
    view = flat[1:1 + B * N * K].view(B, N, K)
    view.copy_(t32(case["basis"], dev))
    assert view.data_ptr() % 16 == 4
    lv = Bare(B, N, K, 1, view)
    outs = new_outs(B, N, K, 1, dev)
    gb = torch.full((B * N * K + 1 + 1024,), -7.0, dtype=torch.float32, device=dev)
    outs["gbasis"] = gb[1:]
    gin = {k: t32(ref[0][UPS_OF[k]], dev) for k in IN_NAMES}
    h = raw_call(lv, t32(case["AtA"], dev), t32(case["damping"], dev), t32(case["sigma2"], dev), gin, outs, fill="one")
    torch.cuda.synchronize()
    wsc.assert_guards_intact(h)
    assert float(gb[0]) == -7.0 and bool((gb[1 + B * N * K:] == -7.0).all()), "written outside gbasis"
    assert same_bits(gb[1:1 + B * N * K].cpu().numpy().reshape(B, N, K), got["gbasis"])
    for k in ("gAtA", "gdamping", "gsigma2", "status"):
        assert same_bits(outs[k].cpu().numpy(), got[k]), k


@pytest.mark.parametrize("K", [193, 194])
def test_the_last_triangle_in_lds_and_the_first_in_the_workspace(dev, K):
    """Y's packed triangle and two vectors in doubles: P (P + 1) / 2 * 8 + 2 P * 8 bytes against 163840 of LDS.  P = 199 (K = 193):
    159200 + 3184 = 162384 fits; P = 200 (K = 194): 160800 + 3200 = 164000 does not -- the triangle moves to the workspace, whose
    query grows by exactly B such triangles (rounded up to 256) beyond Hinv and X"""
    from banet_amd import _capi as capi
    case = tail_case(65, K)
    P, B = 6 + K, case["B"]
    assert (P * (P + 1) // 2 * 8 + 2 * P * 8 <= 160 * 1024) == (K == 193)
    up = lambda n: (n + 255) // 256 * 256
    lv = Bare(B, 0, 0, 1, None)
    lv.c.pairs, lv.c.K = 1, K
    lv.c.N = 65
    nb = capi.lib().banet_ba_marginals_grad_workspace_bytes(ctypes.byref(lv.c), 0)
    tri = up(B * P * (P + 1) // 2 * 8)
    rest = up(B * 1 * 28 * 1024 * 4) + up(B * K * K * 4) + tri + up(B * P * P * 8)      # one partial row of 28 blocks, M, Hinv, X
    assert nb == rest + (tri if K == 194 else 0)
    ref = gr.reference(case)
    check_parity(case, run_case(case, ref[0], dev, fill="nan"), "tails", ref)


# ---- 3. an indefinite window ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", mr.INDEFINITE, ids=mr.spec_id)
def test_indefinite_window_gets_zeros_and_leaves_its_neighbours_alone(dev, spec):
    case = mr.make("indefinite", spec, 0)
    ups = {k: v.copy() for k, v in gr.reference(case)[0].items()}
    for v in ups.values():
        v[1] = np.nan                                               # the failed window's upstream values are not used
    got = run_case(case, ups, dev)
    assert list(got["status"]) == [0, 1, 0]
    for k in ("gAtA", "gdamping", "gsigma2", "gbasis"):
        assert np.all(got[k][1] == 0), k
        assert np.all(np.isfinite(got[k])), k
    alone = run_case(case, ups, dev, windows=[0, 2])
    for k in OUT_NAMES:
        assert same_bits(alone[k], got[k][[0, 2]]), k
    check_parity(case, got, "indefinite")


# ---- 4. bit equality --------------------------------------------------------------------------------------------------------------
BITS = [(38, 1, 32, 1e2, True, True), (152, 4, 128, 1e4, True, True), (304, 8, 256, 1e2, True, True)]


@pytest.mark.parametrize("spec", BITS, ids=mr.spec_id)
def test_a_windows_bits_do_not_depend_on_the_batch_nor_on_the_run(dev, spec):
    case = mr.make("ladder", spec, 0)
    ups = gr.reference(case)[0]
    three = run_case(case, ups, dev)
    again = run_case(case, ups, dev)
    for k in OUT_NAMES:
        assert same_bits(again[k], three[k]), k
    for b in range(case["B"]):
        one = run_case(case, ups, dev, windows=[b])
        for k in OUT_NAMES:
            assert same_bits(one[k][0], three[k][b]), (k, b)
    eight = run_case(case, ups, dev, windows=[0, 1, 2, 2, 1, 0, 0, 1])
    for k in OUT_NAMES:
        assert same_bits(eight[k][:3], three[k]), k


def test_subsets_of_the_outputs_and_null_upstreams(dev):
    for spec in ((38, 1, 32, 1e2, True, True), (262, 1, 256, 1e2, False, True)):
        case = mr.make("ladder", spec, 0)
        ups = gr.reference(case)[0]
        full = run_case(case, ups, dev)
        for names in (("status",), ("gAtA", "status"), ("gbasis", "status"), ("gdamping", "gsigma2", "status"), ("gAtA", "gbasis", "status")):
            part = run_case(case, ups, dev, names=names)
            for k in names:
                assert same_bits(part[k], full[k]), (spec, names, k)
        # a NULL upstream gives the bits of a zero-filled one
        for ins in ((), ("g_pose_cov",), ("g_depth_var",), ("g_logdet",), ("g_pose_cov", "g_logdet")):
            null = run_case(case, ups, dev, ins=ins)
            zero = run_case(case, ups, dev, ins=ins, zero_for_missing=True)
            for k in OUT_NAMES:
                assert same_bits(null[k], zero[k]), (spec, ins, k)
            if "g_depth_var" not in ins:
                assert np.all(null["gbasis"] == 0)
        assert np.all(run_case(case, ups, dev, ins=())["gAtA"] == 0)


def test_workspace_contents_do_not_matter(dev):
    """zeros / another call's leftovers / NaN / ones in the workspace (ws_contract's fills, one arena): the same bits"""
    case = mr.make("ladder", (262, 1, 256, 1e2, False, True), 0)
    primer = mr.make("ladder", (152, 4, 128, 1e4, True, True), 0)
    ups, pups = gr.reference(case)[0], gr.reference(primer)[0]
    arena = wsc.Arena(64 << 20, dev)
    outs = {}
    for fill in wsc.FILLS:
        if fill == "stale":
            arena.reset()
            run_case(primer, pups, dev, fill="zero", arena=arena)
        arena.reset()
        outs[fill] = run_case(case, ups, dev, fill=fill, arena=arena)
    for fill in wsc.FILLS:
        for k in OUT_NAMES:
            assert same_bits(outs[fill][k], outs["zero"][k]), (fill, k)
            assert np.all(np.isfinite(outs[fill][k])), (fill, k)


def test_pose_only_level(dev):
    """K = 0: gAtA comes from g_pose_cov and g_logdet only; g_depth_var / gbasis are accepted and ignored, gbasis is untouched"""
    case = mr.make("ladder", (6, 1, 0, 1e2, True, True), 0)
    ref = gr.reference(case)
    B = case["B"]
    lv = Bare(B, 0, 0, 1, None)
    outs = new_outs(B, 16, 4, 1, dev)
    outs["gAtA"] = torch.full((B, 6, 6), -7.0, device=dev)
    gin = {k: t32(ref[0][UPS_OF[k]], dev) for k in IN_NAMES}
    raw_call(lv, t32(case["AtA"], dev), t32(case["damping"], dev), t32(case["sigma2"], dev), gin, outs)
    torch.cuda.synchronize()
    assert bool((outs["gbasis"] == -7).all())
    got = {k: v.cpu().numpy() for k, v in outs.items() if k != "gbasis"}
    check_parity(case, got, "pose_only", ref)


# ---- 5. the forward's bits are unchanged ------------------------------------------------------------------------------------------
def test_forward_marginals_bits_equal_the_recorded_ones(dev):
    """ops.ba_marginals against tests/golden/marginals_forward_bits.npz, recorded (tools/record_marginals_forward_bits.py) from the
    build before marg_factor_kernel's factorisation moved into the function it shares with marg_grad_factor_kernel"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import record_marginals_forward_bits as rec
    finally:
        sys.path.pop(0)
    gold = np.load(os.path.join(ROOT, "tests", "golden", "marginals_forward_bits.npz"))
    assert len(gold.files) == 5 * len(rec.CASES)
    for family, spec, seed in rec.CASES:
        for name, v in rec.run(family, spec, seed, dev).items():
            assert same_bits(v, gold[rec.key(family, spec, seed, name)]), (family, spec, name)


# ---- 6. the Python layers ---------------------------------------------------------------------------------------------------------
def test_ops_entry_equals_the_c_entry(dev):
    from banet_amd import ops
    case = mr.make("ladder", (134, 1, 128, 1e2, True, True), 0)
    ups = gr.reference(case)[0]
    raw = run_case(case, ups, dev)
    lv = Bare(case["B"], case["N"], case["K"], 1, t32(case["basis"], dev))
    with wsc.patched_workspace("nan"):
        g = ops.ba_marginals_grad(lv, t32(case["AtA"], dev), damping=t32(case["damping"], dev), sigma2=t32(case["sigma2"], dev),
                                  g_pose_cov=t32(ups["g_cov"], dev), g_depth_var=t32(ups["g_dv"], dev), g_logdet=t32(ups["g_ld"], dev),
                                  want=ops.MARGINALS_GRAD_OUTPUTS)
    for k in OUT_NAMES:
        assert same_bits(getattr(g, k).cpu().numpy(), raw[k]), k
    g2 = ops.ba_marginals_grad(lv, t32(case["AtA"], dev), damping=1e-3, sigma2=t32(case["sigma2"], dev), g_depth_var=t32(ups["g_dv"], dev))
    assert g2.gdamping is None and g2.gsigma2 is None and g2.gAtA.shape == (3, 134, 134) and g2.gbasis.shape == (3, 200, 128)
    assert same_bits(g2.gbasis.cpu().numpy(), raw["gbasis"])            # (gbasis depends on T, sigma2 and g_depth_var only)
    with pytest.raises(ops.capi.BanetError):
        ops.ba_marginals_grad(lv, torch.tensor(case["AtA"], dtype=torch.float32), g_logdet=t32(ups["g_ld"], dev))


@pytest.mark.parametrize("spec", [(38, 1, 32, 1e2, True, True), (152, 4, 128, 1e2, True, True)], ids=mr.spec_id)
def test_marginals_diff_against_float64_entrywise_and_along_a_direction(dev, spec):
    """ops.ba_marginals_diff: L = <g_cov, pose_cov> + <g_dv, depth_var> + <g_ld, logdet>, backward.  The gradients pass the parity
    gates entry by entry, and along a random direction d of each input |<got - want, d>| stays within the bound those gates imply,
    sum over the blocks of gate x the block's scale x sum |d| (gbasis: per row)."""
    from banet_amd import ops
    case = mr.make("ladder", spec, 0)
    ups, want, yard = gr.reference(case)
    gate = gr.gates(case, yard)
    lv = Bare(case["B"], case["N"], case["K"], case["pairs"], t32(case["basis"], dev).requires_grad_(True))
    AtA = t32(case["AtA"], dev).requires_grad_(True)
    damping, sigma2 = t32(case["damping"], dev).requires_grad_(True), t32(case["sigma2"], dev).requires_grad_(True)
    m = ops.ba_marginals_diff(lv, AtA, damping=damping, sigma2=sigma2, want=ops.MARGINALS_OUTPUTS)
    assert not m.wfactor.requires_grad and not m.status.requires_grad and m.pose_cov.requires_grad
    loss = (t32(ups["g_cov"], dev) * m.pose_cov).sum() + (t32(ups["g_dv"], dev) * m.depth_var).sum() + (t32(ups["g_ld"], dev) * m.logdet).sum()
    loss.backward()
    got = dict(gAtA=AtA.grad.cpu().numpy(), gbasis=lv.basis.grad.cpu().numpy(), gdamping=damping.grad.cpu().numpy(),
               gsigma2=sigma2.grad.cpu().numpy())
    check_parity(case, got, "autograd")
    rs = np.random.RandomState(7)
    mP = 6 * case["pairs"]
    for b in range(case["B"]):
        d = rs.standard_normal(want["gAtA"][b].shape)
        diff = abs(((got["gAtA"][b].astype(np.float64) - want["gAtA"][b]) * d).sum())
        bound = 0.0
        for name, r, c in (("gAtA_pp", slice(0, mP), slice(0, mP)), ("gAtA_pd", slice(0, mP), slice(mP, None)),
                           ("gAtA_pd", slice(mP, None), slice(0, mP)), ("gAtA_dd", slice(mP, None), slice(mP, None))):
            bound += gate[name] * np.abs(want["gAtA"][b][r, c]).max() * np.abs(d[r, c]).sum()
        print("window %d: |<gAtA - want, d>| = %.3e, bound %.3e" % (b, diff, bound))
        assert diff <= bound
        d = rs.standard_normal(want["gbasis"][b].shape)
        diff = abs(((got["gbasis"][b].astype(np.float64) - want["gbasis"][b]) * d).sum())
        bound = float((gate["gbasis"] * np.abs(want["gbasis"][b]).max(1) * np.abs(d).sum(1)).sum())
        print("window %d: |<gbasis - want, d>| = %.3e, bound %.3e" % (b, diff, bound))
        assert diff <= bound


def test_depth_nll_loss_with_an_indefinite_window(dev):
    from banet_amd import dense_train, ops
    case = mr.make("indefinite", mr.INDEFINITE[0], 0)
    B, N = case["B"], case["N"]
    lv = Bare(B, N, case["K"], case["pairs"], t32(case["basis"], dev).requires_grad_(True))
    AtA = t32(case["AtA"], dev).requires_grad_(True)
    m = ops.ba_marginals_diff(lv, AtA, damping=None, sigma2=t32(case["sigma2"], dev))
    rs = np.random.RandomState(3)
    d_np, gt_np, keep = mr._r32(rs.uniform(1.0, 2.0, (B, N))), mr._r32(rs.uniform(1.0, 2.0, (B, N))), rs.uniform(0, 1, (B, N)) > 0.2
    depth = t32(d_np, dev).requires_grad_(True)
    gt = t32(gt_np, dev)
    loss = dense_train.depth_nll_loss(depth, m.depth_var, gt, mask=t32(keep, dev))
    assert loss.shape == (B,) and bool(torch.isfinite(loss).all()) and float(loss.detach()[1]) == 0.0
    loss.sum().backward()
    assert list(m.status.cpu().numpy()) == [0, 1, 0]
    for name, g in (("AtA", AtA.grad), ("basis", lv.basis.grad), ("depth", depth.grad)):
        assert bool(torch.isfinite(g).all()), name
        assert bool((g[1] == 0).all()), name
        assert bool((g[0] != 0).any()) and bool((g[2] != 0).any()), name
    # the loss itself: 0.5 (log var + err^2 / var), masked mean
    var = m.depth_var.detach().cpu().numpy().astype(np.float64)
    for b in (0, 2):
        want = (0.5 * (np.log(var[b]) + (d_np[b] - gt_np[b]) ** 2 / var[b]))[keep[b]].mean()
        assert abs(float(loss.detach()[b]) - want) <= 1e-5 * max(abs(want), 1.0), (b, float(loss.detach()[b]), want)


# ---- 7. the chain: DenseBA.marginals(differentiable=True) -------------------------------------------------------------------------
def _chain_scene(pairs, dev):
    """24 x 32, C = 32, K = 32, three windows: pairs = 1 the generator of marginals_ref's `assembled` family, pairs = 3 its
    multi-frame sibling; the state: R = I, T = 0.7 T_gt, Wc = 0"""
    from oracle import dense as odense, synth
    H, W, C, K, B = 24, 32, 32, 32, 3
    if pairs == 1:
        scenes = [synth.make_pair_scene(H, W, C, K, [1], 11 + b, normalize_rays=True, w_gt=[0.01, -0.008, 0.006], t_gt=[0.06, -0.04, 0.03])
                  for b in range(B)]
    else:
        scenes = [synth.make_window_scene(H, W, C, K, [1], 41 + b, pairs, normalize_rays=True) for b in range(B)]
    intr, levels = odense.batch_scene(scenes)
    lv = levels[0]
    T0 = np.stack([np.asarray(s["T_gt"], np.float64).reshape(pairs, 3) * 0.7 for s in scenes]).reshape(B, pairs, 3, 1)
    R0 = np.tile(np.eye(3), (B, pairs, 1, 1))
    if pairs == 1:
        T0, R0 = T0[:, 0], R0[:, 0]
    gt = lv["D0"].reshape(B, H * W) + np.einsum("bnk,bk->bn", lv["basis"].reshape(B, H * W, K), np.stack([np.asarray(s["W_gt"]).reshape(K) for s in scenes]))
    vals = dict(src=lv["src"], tgt=lv["tgt"], depth=lv["D0"], basis=lv["basis"], R=R0, T=T0, Wc=np.zeros((B, K, 1)))
    return dict(B=B, H=H, W=W, C=C, K=K, pairs=pairs, intr=mr._r32(intr), scale=lv["scale"], vals={k: mr._r32(v) for k, v in vals.items()},
                gt=mr._r32(gt.reshape(B, H, W)), gcov=mr._r32(np.random.RandomState(17 + pairs).standard_normal((B, 6 * pairs, 6 * pairs))))


LEAVES = ("src", "tgt", "depth", "basis", "R", "T", "Wc")


def _chain_gpu(sc, dev):
    from banet_amd import dense as bdense, dense_train
    from oracle import banet_oracle as orc
    leaves = {k: t32(v, dev).requires_grad_(True) for k, v in sc["vals"].items()}
    tl = [bdense.DenseLevel(sc["scale"], leaves["src"], leaves["tgt"], leaves["depth"], leaves["basis"])]
    ba = bdense.DenseBA(t32(sc["intr"], dev), tl, [orc.he_normal_mlp_weights(sc["C"], 5)], "bundle", 1000.0)
    return ba, leaves, dense_train


def _chain_loss(dense_train, m, depth_map, gt, gcov):
    return dense_train.depth_nll_loss(depth_map, m.depth_var, gt).sum() + m.logdet.sum() + (gcov * m.pose_cov).sum()


@pytest.mark.parametrize("pairs", [1, 3])
def test_chain_equals_the_manual_composition_bit_for_bit(dev, pairs):
    """DenseBA.marginals(differentiable=True), damping 1e-2, loss = NLL + logdet + a random contraction of pose_cov (the NLL's depth
    map and ground truth constants, so that every gradient passes through the marginals) against ops.ba_assemble ->
    ops.ba_marginals -> (torch: the loss's gradients of the three outputs) -> ops.ba_marginals_grad -> dense_adjoint per frame"""
    from banet_amd import ops
    sc = _chain_scene(pairs, dev)
    ba, leaves, dense_train = _chain_gpu(sc, dev)
    B, H, W, C, K = sc["B"], sc["H"], sc["W"], sc["C"], sc["K"]
    gt, gcov = t32(sc["gt"], dev), t32(sc["gcov"], dev)
    dmap = (gt * 1.03).detach()
    m = ba.marginals(0, R=leaves["R"], T=leaves["T"], Wc=leaves["Wc"], damping=1e-2, sigma2=None, want=("pose_cov", "depth_var", "logdet"),
                     differentiable=True)
    assert m.depth_var.shape == (B, H, W) and m.depth_var.requires_grad and list(m.status.cpu().numpy()) == [0] * B
    _chain_loss(dense_train, m, dmap, gt, gcov).backward()
    # the manual composition
    p = ba.problems[0]
    R, T, Wc = (leaves[k].detach() for k in ("R", "T", "Wc"))
    AtA = ops.ba_assemble(p, R, T, Wc)[0]
    f = ops.ba_marginals(p, AtA, damping=1e-2, sigma2=None, want=("pose_cov", "depth_var", "logdet"))
    assert same_bits(f.depth_var.cpu().numpy().reshape(B, H, W), m.depth_var.detach().cpu().numpy())
    outs = [t.detach().clone().requires_grad_(True) for t in (f.pose_cov, f.depth_var, f.logdet)]
    fm = ops.Marginals(outs[0], outs[1].reshape(B, H, W), None, outs[2], f.status)
    _chain_loss(dense_train, fm, dmap, gt, gcov).backward()
    g = ops.ba_marginals_grad(p, AtA, damping=1e-2, sigma2=None, g_pose_cov=outs[0].grad, g_depth_var=outs[1].grad, g_logdet=outs[2].grad,
                              want=("gAtA", "gbasis"))
    N, P = H * W, 6 * pairs + K
    pprobs = [p] if pairs == 1 else dense_train._pair_problems(ba, 0)
    dsrc, ddepth, dbasis = torch.empty(B, N, C, device=dev), torch.empty(B, N, device=dev), torch.empty(B, N, K, device=dev)
    dtgt = [torch.empty(B, H, W, C, device=dev) for _ in range(pairs)]
    gR, gT, gW = torch.empty(B, pairs, 3, 3, device=dev), torch.empty(B, pairs, 3, 1, device=dev), torch.zeros(B, K, 1, device=dev)
    zb, za = torch.zeros(B, P, device=dev), torch.zeros(B, C, device=dev)
    Rv, Tv = R.reshape(B, pairs, 3, 3), T.reshape(B, pairs, 3, 1)
    ws = None
    for i in range(pairs):
        idx = torch.cat([torch.arange(6 * i, 6 * i + 6, device=dev), torch.arange(6 * pairs, P, device=dev)])
        gA_i = g.gAtA.index_select(1, idx).index_select(2, idx).contiguous()
        dpose, ws = dense_train.dense_adjoint(pprobs[i], Rv[:, i].contiguous(), Tv[:, i].contiguous(), Wc, gA_i, zb[:, :6 + K].contiguous(), za,
                                              dsrc, dtgt[i], ddepth, dbasis, ws, overwrite=i == 0, overwrite_map=True, fold=True)
        gR[:, i], gT[:, i] = dpose[:, 0:9].reshape(B, 3, 3), dpose[:, 9:12].reshape(B, 3, 1)
        gW += dpose[:, 12:].reshape(B, K, 1)
    man = dict(src=dsrc, tgt=dtgt[0] if pairs == 1 else torch.stack(dtgt, 1), depth=ddepth, basis=dbasis + g.gbasis, R=gR, T=gT, Wc=gW)
    for k in LEAVES:
        a, b = leaves[k].grad, man[k].reshape(leaves[k].shape)
        assert bool(torch.isfinite(a).all()), k
        assert bool((a != 0).any()) == (k != "src"), k          # (AtA = J^T J does not depend on the source features: exactly 0)
        assert wsc.bits_equal(a.cpu(), b.cpu()), k


@pytest.mark.parametrize("pairs", [1, 3])
def test_chain_against_the_float64_twin(dev, pairs):
    """the same chain (the NLL on the solved depth map depth + basis . Wc, attached) against oracle/torch_port.window_assemble ->
    torch marginals by the definition -> autograd, float64, evaluated on the kernel's own mask.  Per gradient and window the error
    relative to the gradient's largest float64 entry; the gate: 4 x the error of the same twin run in float32.  No case or pixel is
    left out."""
    from banet_amd import ops
    from oracle import torch_port
    sc = _chain_scene(pairs, dev)
    ba, leaves, dense_train = _chain_gpu(sc, dev)
    B, H, W, C, K = sc["B"], sc["H"], sc["W"], sc["C"], sc["K"]
    N, P, mP = H * W, 6 * pairs + K, 6 * pairs

    def depth_of(lv):
        return (lv["depth"].reshape(B, N) + torch.matmul(lv["basis"].reshape(B, N, K), lv["Wc"].reshape(B, K, 1))[..., 0]).reshape(B, H, W)

    m = ba.marginals(0, R=leaves["R"], T=leaves["T"], Wc=leaves["Wc"], damping=1e-2, sigma2=None, want=("pose_cov", "depth_var", "logdet"),
                     differentiable=True)
    _chain_loss(dense_train, m, depth_of(leaves), t32(sc["gt"], dev), t32(sc["gcov"], dev)).backward()
    mask = ops.ba_assemble(ba.problems[0], leaves["R"].detach(), leaves["T"].detach(), leaves["Wc"].detach(), return_mask=True)[4].cpu()

    def twin(dtype):
        lv = {k: torch.tensor(v, dtype=dtype).requires_grad_(True) for k, v in sc["vals"].items()}
        tg = lv["tgt"].reshape(B, pairs, H, W, C)
        AtA = torch_port.window_assemble(torch.tensor(sc["intr"], dtype=dtype), sc["scale"], lv["src"], tg, lv["depth"], lv["basis"],
                                         lv["R"].reshape(B, pairs, 3, 3), lv["T"].reshape(B, pairs, 3, 1), lv["Wc"], True, dtype, None, mask)[0]
        As = 0.5 * (AtA + AtA.transpose(1, 2))
        Hm = As + 1e-2 * torch.diag_embed(torch.diagonal(As, dim1=1, dim2=2) + 1e-5)
        L = torch.linalg.cholesky(Hm)
        Y = torch.linalg.solve_triangular(L, torch.eye(P, dtype=dtype).expand(B, P, P), upper=False)
        y = torch.matmul(lv["basis"].reshape(B, N, K), Y[:, mP:, mP:].transpose(1, 2))
        mm = ops.Marginals(torch.matmul(Y.transpose(1, 2), Y)[:, :mP, :mP], (y * y).sum(-1).reshape(B, H, W), None,
                           2.0 * torch.log(torch.diagonal(L, dim1=1, dim2=2)).sum(1), None)
        _chain_loss(dense_train, mm, depth_of(lv), torch.tensor(sc["gt"], dtype=dtype), torch.tensor(sc["gcov"], dtype=dtype)).backward()
        return {k: (torch.zeros_like(lv[k]) if lv[k].grad is None else lv[k].grad).numpy().astype(np.float64) for k in LEAVES}

    w64, w32 = twin(torch.float64), twin(torch.float32)
    worst = {}
    for k in LEAVES:
        g = leaves[k].grad.cpu().numpy().astype(np.float64)
        for b in range(B):
            scale = np.abs(w64[k][b]).max()
            if k == "src":                                          # AtA does not depend on the source features: exactly 0 on both sides
                assert scale == 0 and np.all(g[b] == 0)
                continue
            err, yard = np.abs(g[b] - w64[k][b]).max() / scale, np.abs(w32[k][b] - w64[k][b]).max() / scale
            print("chain pairs %d window %d d%s: gpu %.3e, float32 twin %.3e" % (pairs, b, k, err, yard))
            worst[k] = max(worst.get(k, 0.0), err / (4 * yard))
            REPORT[("chain_pairs%d" % pairs, "d" + k)] = (B, max(REPORT.get(("chain_pairs%d" % pairs, "d" + k), (0, 0, 0, 0))[1], err),
                                                          max(REPORT.get(("chain_pairs%d" % pairs, "d" + k), (0, 0, 0, 0))[2], yard), worst[k])
    for k in worst:
        assert worst[k] <= 1.0, (k, worst[k])


def test_sigma2_from_the_residual_is_differentiable(dev):
    """sigma2="residual": the torch sums over ops.ba_residual_diff's maps equal the kernel's sums to rounding, and the gradient
    that reaches the features through sigma2 alone is the residual backward's"""
    sc = _chain_scene(1, dev)
    ba, leaves, dense_train = _chain_gpu(sc, dev)
    m = ba.marginals(0, R=leaves["R"], T=leaves["T"], Wc=leaves["Wc"], damping=1e-2, differentiable=True)
    plain = ba.marginals(0, R=leaves["R"].detach(), T=leaves["T"].detach(), Wc=leaves["Wc"].detach(), damping=1e-2)
    assert m.sigma2.requires_grad and torch.allclose(m.sigma2, plain.sigma2, rtol=1e-5)
    assert torch.allclose(m.depth_var, plain.depth_var, rtol=1e-4)
    m.sigma2.sum().backward()
    for k in ("src", "tgt", "R", "T"):
        assert bool(torch.isfinite(leaves[k].grad).all()) and bool((leaves[k].grad != 0).any()), k
