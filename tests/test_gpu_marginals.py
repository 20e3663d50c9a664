"""banet_ba_marginals_f32 on the GPU (csrc/marginals.hip) against tests/marginals_ref.py: synthetic SPD normal matrices whose
conditioning the test chooses, the float64 definition as the reference and the float32 LAPACK route as the yardstick.

Gate per case and output (marginals_ref.gates): max(4 x the yardstick's error on the same case, P 2^-24) on the scales of
marginals_ref.errors -- depth_var relative per pixel, pose_cov[i,j] relative to sqrt(Sigma_ii Sigma_jj), wfactor relative to its
largest entry per window, logdet absolute over P.  Every case prints its figures before it asserts; with BANET_MARGINALS_REPORT
set to a file name the per-family maxima are written there at the end of the module (profiles/marginals.txt quotes such a run).
Three windows and N <= 5000 throughout."""
import ctypes
import os

import numpy as np
import pytest
import torch

import marginals_ref as mr
import ws_contract as wsc

pytestmark = pytest.mark.gpu
OUT_NAMES = ("pose_cov", "depth_var", "wfactor", "logdet", "status")


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
    path = os.environ.get("BANET_MARGINALS_REPORT")
    if path and REPORT:
        with open(path, "w") as f:
            f.write("family output cases max_error max_yardstick max_error_over_gate\n")
            for (family, k), (n, e, y, r) in sorted(REPORT.items()):
                f.write("%s %s %d %.3e %.3e %.3f\n" % (family, k, n, e, y, r))


def record(family, err, yard, gate):
    for k in mr.OUTPUTS:
        n, e, y, r = REPORT.get((family, k), (0, 0.0, 0.0, 0.0))
        REPORT[(family, k)] = (n + 1, max(e, err[k]), max(y, yard[k]), max(r, err[k] / gate[k]))


class Bare:
    """a banet_level_t with the fields the entry reads (B, N, K, pairs, basis) and nothing else"""

    def __init__(self, B, N, K, pairs, basis):
        from banet_amd import _capi as capi
        self.basis = basis
        self.c = capi.Level()
        self.c.B, self.c.N, self.c.K, self.c.pairs = B, N, K, pairs
        self.c.basis = basis.data_ptr() if basis is not None else None


def t32(x, dev):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32))).to(dev)


def raw_call(lv, AtA, damping, sigma2, outs, ws=None, fill=None):
    """the C entry with caller-owned outputs (a dict by name; missing = NULL); -> the workspace handle when `fill` is given"""
    from banet_amd import _capi as capi
    L = capi.lib()
    c = capi.MarginalsOut()
    for k, v in outs.items():
        setattr(c, k, v.data_ptr())
    nb = L.banet_ba_marginals_workspace_bytes(ctypes.byref(lv.c), int("depth_var" in outs))
    assert nb > 0
    handle = None
    if ws is None:
        if fill is None:
            ws = capi.workspace(nb, AtA.device)
        else:
            ws, handle = wsc.guarded_workspace(nb, AtA.device, fill)
            assert ws.numel() == nb
    capi.check(L.banet_ba_marginals_f32(ctypes.byref(lv.c), capi.ptr(AtA), capi.ptr(damping), capi.ptr(sigma2), ctypes.byref(c),
                                        ctypes.c_void_p(ws.data_ptr()), ws.numel(), capi.stream()))
    return handle


def new_outs(B, N, K, pairs, dev, names=OUT_NAMES):
    m = 6 * max(pairs, 1)
    shapes = dict(pose_cov=(B, m, m), depth_var=(B, N), wfactor=(B, K, K), logdet=(B,), status=(B,))
    return {k: torch.full(shapes[k], -7, dtype=torch.int32 if k == "status" else torch.float32, device=dev) for k in names}


def run_case(case, dev, windows=None, names=OUT_NAMES, fill=None):
    """the case (or the given windows of it, in that order) through the C entry -> dict of numpy arrays"""
    idx = list(range(case["B"])) if windows is None else list(windows)
    basis = t32(case["basis"][idx], dev) if case["K"] > 0 else None
    lv = Bare(len(idx), case["N"], case["K"], case["pairs"], basis)
    outs = new_outs(len(idx), case["N"], case["K"], case["pairs"], dev, names)
    h = raw_call(lv, t32(case["AtA"][idx], dev), t32(None if case["damping"] is None else case["damping"][idx], dev),
                 t32(None if case["sigma2"] is None else case["sigma2"][idx], dev), outs, fill=fill)
    torch.cuda.synchronize()
    if h is not None:
        wsc.assert_guards_intact(h)
    return {k: v.cpu().numpy() for k, v in outs.items()}


def same_bits(a, b):
    return wsc.bits_equal(torch.from_numpy(np.ascontiguousarray(a)), torch.from_numpy(np.ascontiguousarray(b)))


def check_parity(case, got, family):
    want = mr.marginals64(case)
    yard = mr.errors(case, mr.marginals32(case), want)      # (mr.yardstick(case), with the reference computed once)
    gate = mr.gates(case, yard)
    err = mr.errors(case, got, want)
    print("%s %s seed %d: " % (family, mr.spec_id(case["spec"]), case["seed"]) +
          "  ".join("%s %.2e (yardstick %.2e, gate %.2e)" % (k, err[k], yard[k], gate[k]) for k in mr.OUTPUTS))
    record(family, err, yard, gate)
    assert list(got["status"]) == [int(f) for f in case["expect_fail"]]
    for k in mr.OUTPUTS:
        assert err[k] <= gate[k], (k, err[k], gate[k])


# ---- 1. parity --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", mr.LADDER, ids=mr.spec_id)
def test_parity_ladder(dev, spec):
    for seed in mr.SEEDS:
        case = mr.make("ladder", spec, seed)
        check_parity(case, run_case(case, dev), "ladder")


@pytest.mark.parametrize("spec", mr.ASSEMBLED, ids=mr.spec_id)
def test_parity_assembled(dev, spec):
    case = mr.make("assembled", spec, 0)
    w = mr.spectrum(case)
    print("assembled %s: lambda_min / lambda_max = %s" % (mr.spec_id(spec), w[:, 0] / w[:, -1]))
    assert np.all(w[:, 0] >= 1e-8 * w[:, -1])
    check_parity(case, run_case(case, dev), "assembled")


# ---- 2. tails of the depth-variance kernel ----------------------------------------------------------------------------------------
def tail_case(N, K, seed=5):
    """a hand-made SPD matrix: G G^T / cols + I on column scales 0.5 .. 2 (condition ~ 50), a random basis of N points"""
    rs = np.random.RandomState(1000 * K + N + seed)
    P, B = 6 + K, mr.B_WINDOWS
    G = rs.standard_normal((B, P, 2 * P))
    d = np.exp(rs.uniform(-0.7, 0.7, (B, P)))
    A = mr._r32((G @ G.transpose(0, 2, 1) / (2 * P) + np.eye(P)) * d[:, :, None] * d[:, None, :])
    A = np.tril(A) + np.tril(A, -1).transpose(0, 2, 1)
    return dict(family="tails", spec=(P, 1, K, 50.0, True, True), seed=seed, B=B, N=N, K=K, pairs=1, P=P, AtA=A,
                basis=mr._r32(rs.standard_normal((B, N, K))), damping=mr._r32(np.full(B, 1e-3)), sigma2=mr._r32(rs.uniform(0.5, 2.0, B)),
                expect_fail=[False] * B)


TAILS = [(N, K) for N in (1, 63, 65, 1000, 4801) for K in (1, 7, 32, 33, 128, 255, 256)]


@pytest.mark.parametrize("N,K", TAILS, ids=lambda v: str(v))
def test_tails_against_float64_aligned_and_offset_basis_with_guards(dev, N, K):
    case = tail_case(N, K)
    B, P = case["B"], case["P"]
    got = run_case(case, dev)
    check_parity(case, got, "tails")
    # the same with the basis a view offset by one float (4-byte aligned only), depth_var followed by a guard region, and a
    # poisoned workspace between guard bands
    flat = torch.zeros(B * N * K + 1 + 64, dtype=torch.float32, device=dev)
    flat[-64:] = float("nan")                                       # read past the tensor's end: poisons the result
    flat[0] = float("nan")
    view = flat[1:1 + B * N * K].view(B, N, K)
    view.copy_(t32(case["basis"], dev))
    assert view.data_ptr() % 16 == 4
    lv = Bare(B, N, K, 1, view)
    outs = new_outs(B, N, K, 1, dev)
    dv = torch.full((B * N + 1024,), -7.0, dtype=torch.float32, device=dev)
    outs["depth_var"] = dv
    h = raw_call(lv, t32(case["AtA"], dev), t32(case["damping"], dev), t32(case["sigma2"], dev), outs, fill="nan")
    torch.cuda.synchronize()
    wsc.assert_guards_intact(h)
    assert bool((dv[B * N:] == -7.0).all()), "written past depth_var"
    assert same_bits(dv[:B * N].cpu().numpy().reshape(B, N), got["depth_var"])
    for k in ("pose_cov", "wfactor", "logdet", "status"):
        assert same_bits(outs[k].cpu().numpy(), got[k]), k


@pytest.mark.parametrize("K", [193, 194])
def test_the_last_matrix_in_lds_and_the_first_in_the_workspace(dev, K):
    """P = 199: the largest packed triangle of doubles the LDS holds; P = 200: the first that lives in the workspace (the host-side
    query says which: test_marginals_cpu.py compares its value with the layout)"""
    from banet_amd import _capi as capi
    case = tail_case(65, K)
    lv = Bare(case["B"], case["N"], K, 1, None)
    nb = capi.lib().banet_ba_marginals_workspace_bytes(ctypes.byref(lv.c), 0)
    assert (nb > 256) == (K == 194)
    check_parity(case, run_case(case, dev, fill="nan"), "tails")


# ---- 3. an indefinite window ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", mr.INDEFINITE, ids=mr.spec_id)
def test_indefinite_window_gets_the_sentinels_and_leaves_its_neighbours_alone(dev, spec):
    case = mr.make("indefinite", spec, 0)
    got = run_case(case, dev)
    m, K = 6 * case["pairs"], case["K"]
    assert list(got["status"]) == [0, 1, 0]
    assert np.all(got["depth_var"][1] == np.inf)
    assert np.array_equal(got["pose_cov"][1], np.diag(np.full(m, np.inf, np.float32)))
    assert np.all(got["wfactor"][1] == 0) and got["logdet"][1] == -np.inf
    alone = run_case(case, dev, windows=[0, 2])
    for k in OUT_NAMES:
        assert same_bits(alone[k], got[k][[0, 2]]), k
    check_parity(case, got, "indefinite")


# ---- 4. batch invariance ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", [(38, 1, 32, 1e2, True, True), (152, 4, 128, 1e4, True, True), (304, 8, 256, 1e2, True, True)],
                         ids=mr.spec_id)
def test_a_windows_bits_do_not_depend_on_the_batch(dev, spec):
    case = mr.make("ladder", spec, 0)
    three = run_case(case, dev)
    for b in range(case["B"]):
        one = run_case(case, dev, windows=[b])
        for k in OUT_NAMES:
            assert same_bits(one[k][0], three[k][b]), (k, b)
    eight = run_case(case, dev, windows=[0, 1, 2, 2, 1, 0, 0, 1])     # 3 + 5 padding windows
    for k in OUT_NAMES:
        assert same_bits(eight[k][:3], three[k]), k


# ---- 5. subsets of the optional outputs -------------------------------------------------------------------------------------------
def test_subsets_of_the_optional_outputs_give_the_same_bits(dev):
    for spec in ((38, 1, 32, 1e2, True, True), (262, 1, 256, 1e2, False, True)):
        case = mr.make("ladder", spec, 0)
        full = run_case(case, dev)
        for names in (("pose_cov", "status"), ("pose_cov", "status", "depth_var"), ("pose_cov", "status", "wfactor"),
                      ("pose_cov", "status", "logdet"), ("pose_cov", "status", "depth_var", "logdet")):
            part = run_case(case, dev, names=names)
            for k in names:
                assert same_bits(part[k], full[k]), (spec, names, k)


def test_pose_only_level_leaves_depth_outputs_unwritten(dev):
    case = mr.make("ladder", (6, 1, 0, 1e2, True, True), 0)
    B = case["B"]
    lv = Bare(B, 0, 0, 1, None)
    outs = new_outs(B, 16, 4, 1, dev)                                # depth_var / wfactor given although K = 0: accepted, ignored
    raw_call(lv, t32(case["AtA"], dev), t32(case["damping"], dev), t32(case["sigma2"], dev), outs)
    torch.cuda.synchronize()
    assert bool((outs["depth_var"] == -7).all()) and bool((outs["wfactor"] == -7).all())
    assert list(outs["status"].cpu().numpy()) == [0] * B
    got = {k: v.cpu().numpy() for k, v in outs.items()}
    want = mr.marginals64(case)
    err = mr.errors(case, got, want)
    gate = mr.gates(case, mr.yardstick(case))
    assert err["pose_cov"] <= gate["pose_cov"] and err["logdet"] <= gate["logdet"], (err, gate)


# ---- 6. properties ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", [(39, 1, 33, 1e4, True, True), (152, 4, 128, 1e6, False, True), (304, 8, 256, 1e4, True, True)],
                         ids=mr.spec_id)
def test_symmetry_sign_and_exact_scaling(dev, spec):
    case = dict(mr.make("ladder", spec, 1))
    got = run_case(case, dev)
    assert np.array_equal(got["pose_cov"], got["pose_cov"].transpose(0, 2, 1))
    assert np.all(got["status"] == 0) and np.all(np.isfinite(got["depth_var"])) and np.all(got["depth_var"] >= 0)
    case["sigma2"] = case["sigma2"] * 4.0
    four = run_case(case, dev)
    assert same_bits(four["pose_cov"], got["pose_cov"] * np.float32(4)) and same_bits(four["depth_var"], got["depth_var"] * np.float32(4))
    assert same_bits(four["wfactor"], got["wfactor"]) and same_bits(four["logdet"], got["logdet"])


# ---- 7. the Python layers ---------------------------------------------------------------------------------------------------------
def test_ops_entry_equals_the_c_entry(dev):
    from banet_amd import ops
    case = mr.make("ladder", (134, 1, 128, 1e2, True, True), 0)
    raw = run_case(case, dev)
    lv = Bare(case["B"], case["N"], case["K"], 1, t32(case["basis"], dev))
    with wsc.patched_workspace("nan"):
        m = ops.ba_marginals(lv, t32(case["AtA"], dev), damping=t32(case["damping"], dev), sigma2=t32(case["sigma2"], dev),
                             want=ops.MARGINALS_OUTPUTS)
    for k in OUT_NAMES:
        assert same_bits(getattr(m, k).cpu().numpy(), raw[k]), k
    m2 = ops.ba_marginals(lv, t32(case["AtA"], dev), damping=1e-3, sigma2=None)          # floats are broadcast; default outputs
    assert m2.wfactor is None and m2.logdet is None and m2.depth_var.shape == (case["B"], case["N"])
    case1 = dict(case, sigma2=None)
    assert same_bits(m2.depth_var.cpu().numpy(), run_case(case1, dev)["depth_var"])
    with pytest.raises(ops.capi.BanetError):
        ops.ba_marginals(lv, torch.tensor(case["AtA"], dtype=torch.float32))             # a CPU tensor


def test_dense_ba_marginals(dev):
    from banet_amd import dense as bdense, ops
    from oracle import banet_oracle as orc, dense as odense, synth
    B, C, K = 3, 32, 32
    scenes = [synth.make_pair_scene(24, 32, C, K, [2, 1], 21 + b, normalize_rays=True, w_gt=[0.01, -0.008, 0.006],
                                    t_gt=[0.06, -0.04, 0.03]) for b in range(B)]
    intr, levels = odense.batch_scene(scenes)
    mlps = [orc.he_normal_mlp_weights(C, 5 + i) for i in range(2)]
    tl = [bdense.DenseLevel(lv["scale"], *(torch.from_numpy(lv[k]).to(dev) for k in ("src", "tgt", "D0", "basis"))) for lv in levels]
    ba = bdense.DenseBA(torch.from_numpy(intr).to(dev), tl, mlps, "bundle", 1000.0)
    T0 = torch.from_numpy(np.stack([np.asarray(s["T_gt"]) * 0.7 for s in scenes]).reshape(B, 3, 1).astype(np.float32)).to(dev)
    st = ba.new_state(T=T0)
    ba.solve([2, 2], st)
    H, W = levels[1]["H"], levels[1]["W"]
    p = ba.problems[1]
    m = ba.marginals(1, state=st, damping="lambda", want=ops.MARGINALS_OUTPUTS)
    assert m.depth_var.shape == (B, H, W) and m.pose_cov.shape == (B, 6, 6)
    assert same_bits(m.damping.cpu().numpy(), st.lambda_out.cpu().numpy())
    # sigma2 = sum_f sum sq / max(C sum_f count - P, 1), from residual().sums on the host
    sums = ba.residual(1, state=st).sums.cpu().numpy().astype(np.float64)
    s2 = sums[:, :, 0].sum(1) / np.maximum(C * sums[:, :, 2].sum(1) - (6 + K), 1.0)
    assert np.all(s2 > 0) and np.abs(m.sigma2.cpu().numpy() - s2).max() <= 4 * 2.0 ** -24 * s2.max()
    # the manual composition
    AtA = ops.ba_assemble(p, st.R, st.T, st.Wc)[0]
    man = ops.ba_marginals(p, AtA, damping=st.lambda_out, sigma2=m.sigma2, want=ops.MARGINALS_OUTPUTS)
    assert same_bits(man.depth_var.cpu().numpy().reshape(B, H, W), m.depth_var.cpu().numpy())
    for k in ("pose_cov", "wfactor", "logdet", "status"):
        assert same_bits(getattr(man, k).cpu().numpy(), getattr(m, k).cpu().numpy()), k
    assert list(m.status.cpu().numpy()) == [0] * B and bool(torch.isfinite(m.depth_var).all()) and bool((m.depth_var >= 0).all())
    # the other settings: sigma2 None = 1, a float damping
    u = ba.marginals(1, state=st, damping=0.5, sigma2=None)
    man = ops.ba_marginals(p, AtA, damping=0.5, sigma2=None)
    assert u.sigma2 is None and same_bits(man.pose_cov.cpu().numpy(), u.pose_cov.cpu().numpy())
    assert same_bits(man.depth_var.cpu().numpy().reshape(B, H, W), u.depth_var.cpu().numpy())
