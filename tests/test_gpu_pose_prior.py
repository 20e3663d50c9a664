"""The pose prior inside the LM loop (include/banet_hip.h (5f); csrc/pose_prior.hip) on the GPU through the C ABI, against the float64
twin of tests/pose_prior_ref.py (the oracle's iteration with the term added before its damping).

Bounds:
  * banet_pose_prior_apply_f32: everything outside the pose block bit-unchanged; the block and Atb[0:m] entrywise within
    pose_prior_ref.APPLY_GATE = 4 x 4.72e-7 of the twin, relative to |AtA_ij| + scale (|Jr|^T |Lambda| |Jr|)_ij (4.72e-7 is how far
    a float32 numpy evaluation of the twin's formulas lies from the twin on the same cases, test_pose_prior_cpu.py); at identity
    poses the block is AtA + Lambda bit for bit;
  * solves: delta, R, T, Wc within the project's 1e-4 (max |got - want| / max |want|, as test_gpu_prior.py) of the twin, with the
    same scene WITHOUT a prior as a control;
  * everything else is bit equality."""
import ctypes

import numpy as np
import pytest
import torch

import pose_prior_ref as ppr
import prior_ref as pref
import ws_contract as wsc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = 16
L2 = 1000.0
STATE = ("R", "T", "Wc", "iters", "ratio", "lambda_out", "delta")
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from banet_amd import _capi
    _capi.lib()
    yield
    _CACHE.clear()


def t32(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32))).to(DEV)


def f64(x):
    return np.asarray(x, np.float32).astype(np.float64)


def n64(x):
    return x.detach().double().cpu().numpy()


def relerr(got, want):
    want, got = np.asarray(want, np.float64), np.asarray(got, np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))


def state_bits_equal(a, b):
    return all(getattr(a, n) is None and getattr(b, n) is None or wsc.bits_equal(getattr(a, n), getattr(b, n)) for n in STATE)


# ======================================================================================================================
# banet_pose_prior_apply_f32 on synthetic normal equations
# ======================================================================================================================
class BareLevel:
    """a level with only what banet_pose_prior_apply_f32 reads"""

    def __init__(self, B, K, pairs):
        from banet_amd import _capi as capi
        self.c = capi.Level()
        self.c.B, self.c.K, self.c.pairs = B, K, pairs
        self.c.variant = capi.BUNDLE if K else capi.BUNDLE_CAMERA


def apply_on_gpu(c, scale, windows=None):
    from banet_amd import ops
    sel = (lambda x: t32(x)) if windows is None else (lambda x: t32(x[list(windows)]))
    A, b = sel(c["AtA"]), sel(c["Atb"])
    pairs, K = c["R"].shape[1], c["AtA"].shape[1] - 6 * c["R"].shape[1]
    pp = ops.PosePrior(sel(c["R0"]), sel(c["T0"]), sel(c["Lambda"]), scale)
    ops.pose_prior_apply(BareLevel(A.shape[0], K, pairs), pp, sel(c["R"]), sel(c["T"]), A, b)
    torch.cuda.synchronize()
    return A, b


@pytest.mark.parametrize("pairs,K", ppr.APPLY_SHAPES)
def test_pose_prior_apply_against_the_twin(pairs, K):
    c = ppr.apply_problem(pairs, K)
    m = 6 * pairs
    A, b = apply_on_gpu(c, ppr.APPLY_SCALE)
    A0, b0 = t32(c["AtA"]), t32(c["Atb"])
    assert not torch.equal(A[:, :m, :m], A0[:, :m, :m])
    A0[:, :m, :m], b0[:, :m] = A[:, :m, :m], b[:, :m]
    assert torch.equal(A, A0) and torch.equal(b, b0)       # everything outside the pose block and Atb[0:m]
    eA, eb = ppr.apply_errors(A.cpu().numpy(), b.cpu().numpy(), c)
    print("pose_prior_apply pairs %d K %d (|phi| %s): AtA %.3e Atb %.3e of the bound, gate %.3e (float32 numpy: %.3e)"
          % (pairs, K, ", ".join("%.3g" % a for a in sorted(set(c["angles"]))), eA, eb, ppr.APPLY_GATE, ppr.F32_ERR))
    assert bool(torch.isfinite(A).all()) and bool(torch.isfinite(b).all())
    assert eA <= ppr.APPLY_GATE and eb <= ppr.APPLY_GATE   # 4 x 4.72e-7 (pose_prior_ref.F32_ERR; profiles/pose_prior.txt)


@pytest.mark.parametrize("pairs,K", ppr.APPLY_SHAPES)
def test_identity_poses_add_lambda_bit_for_bit(pairs, K):
    c = ppr.apply_problem(pairs, K)
    m = 6 * pairs
    c["R"] = np.ascontiguousarray(np.broadcast_to(np.eye(3, dtype=np.float32), c["R"].shape))
    c["R0"], c["T"] = c["R"].copy(), c["T0"].copy()
    A, b = apply_on_gpu(c, 1.0)
    want = t32(c["AtA"])
    want[:, :m, :m] += t32(c["Lambda"])
    assert wsc.bits_equal(A, want) and wsc.bits_equal(b, t32(c["Atb"]))


def test_apply_a_window_alone_and_in_the_batch_and_the_empty_prior():
    from banet_amd import ops
    for pairs, K in ((2, 5), (7, 130), (1, 0)):
        c = ppr.apply_problem(pairs, K)
        A, b = apply_on_gpu(c, ppr.APPLY_SCALE)
        for w in range(3):
            A1, b1 = apply_on_gpu(c, ppr.APPLY_SCALE, [w])
            assert wsc.bits_equal(A1[0], A[w]) and wsc.bits_equal(b1[0], b[w]), (pairs, K, w)
        # the empty pose prior launches nothing
        A, b = t32(c["AtA"]), t32(c["Atb"])
        lvl = BareLevel(3, K, pairs)
        for pp in (None, ops.PosePrior(), ops.PosePrior(t32(c["R0"]), t32(c["T0"]), t32(c["Lambda"]), scale=0.0)):
            ops.pose_prior_apply(lvl, pp, t32(c["R"]), t32(c["T"]), A, b)
        torch.cuda.synchronize()
        assert wsc.bits_equal(A, t32(c["AtA"])) and wsc.bits_equal(b, t32(c["Atb"]))


def test_apply_past_the_supported_range_is_finite():
    c = ppr.apply_problem(2, 5)
    rng = np.random.RandomState(8)
    for b, ang in enumerate((3.1, 3.1415, np.pi)):
        for i in range(2):
            c["R"][b, i] = (ppr.random_rotation(rng, ang) @ c["R0"][b, i].astype(np.float64)).astype(np.float32)
    A, b = apply_on_gpu(c, ppr.APPLY_SCALE)
    assert bool(torch.isfinite(A).all()) and bool(torch.isfinite(b).all())


# ======================================================================================================================
# scenes, solvers and the twin
# ======================================================================================================================
def scene(key, B, H, W, K, scales, pairs, seed, channels=C):
    """-> dict(intr, levels (numpy, tgt [B,pairs,H,W,C]), mlps, T0 [B,pairs,3,1], T_gt, W_gt [B,K]), built once per module: the
    scenes of test_gpu_prior.py (prior_ref.SCHEDULE_MOTION for the schedules, so that the last update is not a small one)"""
    if key not in _CACHE:
        from oracle import banet_oracle as orc, dense as odense, synth
        trans_mag, frac = pref.SCHEDULE_MOTION if len(scales) > 1 else (0.03, 0.7)
        scenes = [synth.make_window_scene(H, W, channels, K, scales, seed + b, pairs, trans_mag=trans_mag) for b in range(B)]
        intr, levels = odense.batch_scene(scenes)
        T_gt = np.stack([np.asarray(s["T_gt"]) for s in scenes]).reshape(B, pairs, 3, 1)
        _CACHE[key] = dict(intr=intr, levels=levels, mlps=[orc.he_normal_mlp_weights(channels, 5 + i) for i in range(len(levels))],
                           T0=(T_gt * frac).astype(np.float32), T_gt=T_gt, W_gt=np.stack([s["W_gt"] for s in scenes]), B=B, K=K, pairs=pairs)
    return _CACHE[key]


def dense_ba(sc, windows=None, batch_invariant=False, variant="bundle"):
    from banet_amd import dense as bdense
    idx = list(range(sc["B"])) if windows is None else list(windows)
    tl = [bdense.DenseLevel(lv["scale"], *(t32(lv[k][idx]) for k in ("src", "tgt", "D0", "basis"))) for lv in sc["levels"]]
    return bdense.DenseBA(t32(sc["intr"][idx]), tl, sc["mlps"], variant, L2, batch_invariant=batch_invariant)


def start(ba, sc, windows=None):
    idx = list(range(sc["B"])) if windows is None else list(windows)
    T0 = sc["T0"][idx]
    return ba.new_state(T=t32(T0 if sc["pairs"] > 1 else T0[:, 0]))


def pose_inputs(sc, seed, strength=1.0):
    """a prior pose away from the truth (a rotation of 0.02 about a random axis, half the true translation) and a random symmetric
    positive definite Lambda with a mean diagonal of `strength`"""
    rng = np.random.RandomState(seed)
    B, pairs = sc["B"], sc["pairs"]
    m = 6 * pairs
    R0 = np.stack([[ppr.random_rotation(rng, 0.02) for _ in range(pairs)] for _ in range(B)])
    T0 = sc["T_gt"][:, :, :, 0] * 0.5 + rng.standard_normal((B, pairs, 3)) * 0.002
    M = rng.standard_normal((B, m, m))
    Lam = np.einsum("bik,bjk->bij", M, M) / m + np.eye(m)
    Lam = strength * Lam / np.mean([np.diag(Lam[b]).mean() for b in range(B)])
    f = lambda x: np.ascontiguousarray(x.astype(np.float32))
    return dict(R0=f(R0), T0=f(T0), Lambda=f(0.5 * (Lam + Lam.transpose(0, 2, 1))))


def dense_prior(po, scales, windows=None, pi=None):
    from banet_amd import dense as bdense
    sel = (lambda x: t32(x)) if windows is None else (lambda x: t32(x[list(windows)]))
    return bdense.DensePrior(coef=(sel(pi["Lambda"]), sel(pi["eta"])) if pi is not None else None, level_scale=scales,
                             pose=(sel(po["R0"]), sel(po["T0"]), sel(po["Lambda"])) if po is not None else None)


def coef_inputs(sc, seed, strength):
    rng = np.random.RandomState(seed)
    B, K = sc["B"], sc["K"]
    M = rng.standard_normal((B, K, K))
    Lambda = (strength * (np.einsum("bik,bjk->bij", M, M) / K + np.eye(K))).astype(np.float32)
    eta = np.einsum("bij,bj->bi", Lambda.astype(np.float64), sc["W_gt"] + rng.standard_normal((B, K)) * 0.01).astype(np.float32)
    return dict(Lambda=Lambda, eta=eta)


def twin_solve(sc, iters, po=None, scales=None, pi=None, camera=False, R=None, T=None, W=None):
    """the float64 twin over the schedule -> dict(R [B,pairs,3,3], T [B,pairs,3,1], W [B,K], delta [B,P], first = the first
    iteration's record).  po / pi: pose_inputs / coef_inputs, each scaled by scales[l]; camera: the pose-only level (one frame)"""
    from oracle import banet_oracle as orc, dense as odense
    B, K, pairs = sc["B"], sc["K"], sc["pairs"]
    Rs = [np.tile(np.eye(3)[None], (B, 1, 1)) for _ in range(pairs)] if R is None else [np.array(R[:, i]) for i in range(pairs)]
    Ts = [f64(sc["T0"][:, i]) for i in range(pairs)] if T is None else [np.array(T[:, i]) for i in range(pairs)]
    Wv = np.zeros((B, K, 1)) if W is None else np.array(W).reshape(B, K, 1)
    first = dbg = None
    for li, (lv, n_it) in enumerate(zip(sc["levels"], iters)):
        lv64 = {k: (f64(v) if isinstance(v, np.ndarray) else v) for k, v in lv.items()}
        a = odense.level_inputs(f64(sc["intr"]), dict(lv64, tgt=lv64["tgt"][:, 0]), True, np.float64)
        conv2s = [orc.target_map(lv64["tgt"][:, i]) for i in range(pairs)]
        s = float(np.float32(scales[li])) if scales is not None else 1.0
        pose = (f64(po["R0"]), f64(po["T0"]), f64(po["Lambda"]), s) if po is not None else None
        coef = pref.terms(s, f64(pi["Lambda"]), f64(pi["eta"])) if pi is not None else None
        for _ in range(n_it):
            if camera:
                Rs[0], Ts[0], dbg = ppr.camera_iteration(a, conv2s[0], Rs[0], Ts[0], sc["mlps"][li], pose)
            else:
                Rs, Ts, Wv, dbg = ppr.window_iteration(a, conv2s, Rs, Ts, Wv, sc["mlps"][li], L2, pose, coef)
            first = first or dbg
    return dict(R=np.stack(Rs, 1), T=np.stack(Ts, 1), W=Wv[:, :, 0], delta=dbg["solution"], first=first)


def check_against_twin(name, st, want, sc):
    B, pairs = sc["B"], sc["pairs"]
    errs = dict(delta=relerr(n64(st.delta), want["delta"]), R=relerr(n64(st.R).reshape(B, pairs, 3, 3), want["R"]),
                T=relerr(n64(st.T).reshape(B, pairs, 3, 1), want["T"]))
    if st.Wc is not None:
        errs["Wc"] = relerr(n64(st.Wc).reshape(B, -1), want["W"])
    print("%s: " % name + "  ".join("%s %.2e" % kv for kv in errs.items()))
    return errs


PARITY = {  # name: (B, H, W, K, scales, pairs, iters, variant)
    "schedule": (3, 24, 32, 16, [4, 2, 1], 1, [2, 2, 2], "bundle"),
    "schedule two frames": (3, 24, 32, 16, [4, 2, 1], 2, [2, 2, 2], "bundle"),
    "13x19 two frames": (1, 13, 19, 16, [1], 2, [2], "bundle"),
    # the pose-only solve (lambda = 1e-3) converges in one iteration per level: a second one updates by 1e-4, and a gate relative to
    # the last update needs one that is not small (prior_ref.SCHEDULE_MOTION) -- in the twin 7e-3 (control) and 1e-2 with [1, 1, 1]
    "camera schedule": (3, 24, 32, 16, [4, 2, 1], 1, [1, 1, 1], "bundle_camera"),
}


def parity_scene(name):
    B, H, W, K, scales, pairs, iters, variant = PARITY[name]
    key = "schedule" if name == "camera schedule" else name                 # (the camera level ignores the scene's basis)
    return scene(key, B, H, W, K, scales, pairs, 31), iters, variant


@pytest.mark.parametrize("name", list(PARITY))
def test_solves_with_a_pose_prior_against_the_float64_twin(name):
    sc, iters, variant = parity_scene(name)
    camera = variant == "bundle_camera"
    B, pairs, m = sc["B"], sc["pairs"], 6 * sc["pairs"]
    ba = dense_ba(sc, variant=variant)
    # control: the same scene without a prior
    control = twin_solve(sc, iters, camera=camera)
    st, _ = ba.solve(iters, start(ba, sc))
    torch.cuda.synchronize()
    errs = {"control": check_against_twin(name + ", control", st, control, sc)}
    # the pose prior: as strong as the data -- its scale from the control twin's first normal matrix -- at a pose away from the truth
    po = pose_inputs(sc, 7)
    data = np.mean([np.diag(control["first"]["AtA"][b, :m, :m]).mean() for b in range(B)])
    scales_l = [float(np.float32(data))] * len(iters)
    want = twin_solve(sc, iters, po, scales_l, camera=camera)
    assert relerr(want["T"], control["T"]) > 1e-3, "the pose prior does not move the solution"
    st, _ = ba.solve(iters, start(ba, sc), prior=dense_prior(po, scales_l))
    torch.cuda.synchronize()
    errs["pose prior"] = check_against_twin(name + ", pose prior (scale %.3g)" % scales_l[0], st, want, sc)
    if not camera:                                          # together with a coefficient prior of (5d)
        pi = coef_inputs(sc, 9, strength=np.mean([np.diag(control["first"]["AtA"][b, m:, m:]).mean() for b in range(B)]) / data)
        both = twin_solve(sc, iters, po, scales_l, pi)
        assert relerr(both["W"], want["W"]) > 1e-3, "the coefficient prior does not move the solution"
        st, _ = ba.solve(iters, start(ba, sc), prior=dense_prior(po, scales_l, pi=pi))
        torch.cuda.synchronize()
        errs["both priors"] = check_against_twin(name + ", pose and coefficient prior", st, both, sc)
    for what, e in errs.items():
        assert max(e.values()) < 1e-4, (what, e)


def test_a_strong_pose_prior_holds_the_poses():
    """Lambda = s I, s = 1e6 x the largest pose-block diagonal: |Log(T o T0^-1)| ends below the run without a prior by the factor
    the twin shows -- the two final norms, each relative to the no-prior norm, agree within the project's 1e-4"""
    from banet_amd import dense as bdense, ops
    sc = scene("one level 24x32", 3, 24, 32, 16, [1], 1, 31)
    B = sc["B"]
    iters = [3]
    ba = dense_ba(sc)
    st0 = start(ba, sc)
    AtA = ops.ba_assemble(ba.problems[0], st0.R, st0.T, st0.Wc)[0]
    s = 1e6 * torch.diagonal(AtA[:, :6, :6], dim1=1, dim2=2).max(dim=1).values
    po = pose_inputs(sc, 7)
    Lam = (s[:, None, None] * torch.eye(6, device=DEV)[None]).contiguous()
    po["Lambda"] = Lam.cpu().numpy()
    norms = {}
    for what, prior in (("plain", None), ("prior", bdense.DensePrior(pose=(t32(po["R0"]), t32(po["T0"]), Lam)))):
        st, _ = ba.solve(iters, start(ba, sc), prior=prior)
        torch.cuda.synchronize()
        tw = twin_solve(sc, iters, po if prior is not None else None)
        norms[what] = (ppr.log_norm(n64(st.R).reshape(B, 1, 3, 3), n64(st.T).reshape(B, 1, 3), f64(po["R0"]), f64(po["T0"]))[:, 0],
                       ppr.log_norm(tw["R"], tw["T"], f64(po["R0"]), f64(po["T0"]))[:, 0])
    gpu, twin = norms["prior"][0] / norms["plain"][0], norms["prior"][1] / norms["plain"][1]
    print("strong pose prior: |Log| with / without, GPU %s, twin %s" % (gpu, twin))
    assert (twin < 0.5).all(), "the twin's strong prior does not hold the poses"
    assert (np.abs(gpu - twin) < 1e-4).all()


# ======================================================================================================================
# the empty pose prior, and bit equalities
# ======================================================================================================================
def schedule_case(batch_invariant=True, windows=None, name="schedule"):
    sc, iters, variant = parity_scene(name)
    return sc, dense_ba(sc, windows, batch_invariant, variant)


def level_calls(ba, sc, iters, priors, pose_priors, windows=None):
    from banet_amd import ops
    st = start(ba, sc, windows)
    for prob, mlp, its, pr, pp in zip(ba.problems, ba.mlps, iters, priors, pose_priors):
        ops.lm_level(prob, mlp, ba.l2_base, its, False, st, ws=ba.ws, prior=pr, pose_prior=pp)
    return st


def pose_priors_of(po, scales, windows=None):
    """level 0 none, levels 1 and 2 the pose prior"""
    from banet_amd import ops
    sel = (lambda x: t32(x)) if windows is None else (lambda x: t32(x[list(windows)]))
    return [None] + [ops.PosePrior(sel(po["R0"]), sel(po["T0"]), sel(po["Lambda"]), scale=s) for s in scales[1:]]


@pytest.mark.parametrize("name", ["schedule two frames", "camera schedule"])
def test_the_empty_pose_prior_is_the_existing_entry_bit_for_bit(name):
    from banet_amd import _capi as capi, ops
    sc, ba = schedule_case(name=name)
    camera = ba.variant == "bundle_camera"
    iters = [2, 2, 2]
    po = pose_inputs(sc, 7)
    pi = None if camera else coef_inputs(sc, 9, 30.0)
    coef = [None] * 3 if camera else [None, ops.Prior(t32(pi["Lambda"]), t32(pi["eta"]), scale=2.0), None]
    existing = level_calls(ba, sc, iters, coef, [None] * 3)                  # banet_lm_level_prior_f32 / _ex_f32
    L = capi.lib()
    for what, make in (("no pointers", lambda: ops.PosePrior()),
                       ("scale 0", lambda: ops.PosePrior(t32(po["R0"]), t32(po["T0"]), t32(po["Lambda"]), scale=0.0))):
        pps = [make() for _ in range(3)]
        assert state_bits_equal(level_calls(ba, sc, iters, coef, pps), existing), what
        st = start(ba, sc)
        ops.lm_solve(ba.problems, ba.mlps, ba.l2_base, iters, False, st, priors=None if camera else coef, pose_priors=pps)
        assert state_bits_equal(st, existing), what
        # on a guarded workspace of exactly the existing entry's size
        prob, pr = ba.problems[1], coef[1]
        prc = ctypes.byref(pr.c) if pr is not None else None
        nb = L.banet_lm_level_prior_workspace_bytes(ctypes.byref(prob.c), prc)
        assert L.banet_lm_level_pose_prior_workspace_bytes(ctypes.byref(prob.c), prc, ctypes.byref(pps[1].c)) == nb
        assert L.banet_lm_level_pose_prior_workspace_bytes(ctypes.byref(prob.c), prc, None) == nb
        ws, handle = wsc.guarded_workspace(nb, DEV, "nan")
        st = start(ba, sc)
        capi.check(L.banet_lm_level_pose_prior_f32(ctypes.byref(prob.c), ctypes.byref(ba.mlps[1].c), ba.l2_base, 2, None, prc,
                                                   ctypes.byref(pps[1].c), ctypes.byref(st.c), ctypes.c_void_p(ws.data_ptr()), nb, capi.stream()))
        wsc.assert_guards_intact(handle)
        ref = start(ba, sc)
        ops.lm_level(prob, ba.mlps[1], ba.l2_base, 2, False, ref, ws=ba.ws, prior=pr)
        assert state_bits_equal(st, ref), what


@pytest.mark.parametrize("name", ["schedule two frames", "camera schedule"])
def test_schedule_entry_equals_the_level_calls_alone_and_in_a_batch_and_refuses_before_any_launch(name):
    from banet_amd import _capi as capi, ops
    sc, ba = schedule_case(batch_invariant=True, name=name)
    camera = ba.variant == "bundle_camera"
    iters, scales = [2, 2, 2], [1.0, 4000.0, 9000.0]
    po = pose_inputs(sc, 7)
    pps = pose_priors_of(po, scales)
    coef = None
    if not camera:
        pi = coef_inputs(sc, 9, 30.0)
        coef = [ops.Prior(t32(pi["Lambda"]), t32(pi["eta"]), scale=2.0), None, ops.Prior(t32(pi["Lambda"]), t32(pi["eta"]), scale=3.0)]
    per_level = level_calls(ba, sc, iters, coef or [None] * 3, pps)
    plain = level_calls(ba, sc, iters, coef or [None] * 3, [None] * 3)
    assert not wsc.bits_equal(per_level.T, plain.T)
    runs = []
    for _ in range(2):
        st = start(ba, sc)
        trace = ops.SolveTrace(3, st)
        ops.lm_solve(ba.problems, ba.mlps, ba.l2_base, iters, False, st, priors=coef, pose_priors=pps, trace=trace)
        runs.append((st, trace))
    torch.cuda.synchronize()
    assert state_bits_equal(runs[0][0], per_level) and state_bits_equal(runs[1][0], per_level)
    assert wsc.bits_equal(runs[0][1].T, runs[1][1].T) and wsc.bits_equal(runs[0][1].T[2], per_level.T)
    # a window alone and in the batch of 3, BANET_POLICY_BATCH_INVARIANT
    b = 1
    ba1 = dense_ba(sc, [b], batch_invariant=True, variant=ba.variant)
    st1 = start(ba1, sc, [b])
    coef1 = None
    if not camera:
        coef1 = [ops.Prior(t32(pi["Lambda"][[b]]), t32(pi["eta"][[b]]), scale=2.0), None, ops.Prior(t32(pi["Lambda"][[b]]), t32(pi["eta"][[b]]), scale=3.0)]
    ops.lm_solve(ba1.problems, ba1.mlps, ba1.l2_base, iters, False, st1, priors=coef1, pose_priors=pose_priors_of(po, scales, [b]))
    for n in STATE:
        if getattr(st1, n) is not None:
            assert wsc.bits_equal(getattr(st1, n)[0], getattr(per_level, n)[b]), n
    # every refusal is decided before any launch: a bad pose prior on the LAST level enqueues nothing, the state keeps its bits
    bads = []
    for has in ((1, 0, 1), (0, 0, 1)):
        q = capi.PosePrior()
        for field, on in zip(("R0", "T0", "Lambda"), has):
            setattr(q, field, getattr(pps[2].c, field) if on else None)
        q.scale = 1.0
        bads.append(("pointers %s" % (has,), q))
    for scale in (-1.0, float("nan"), float("inf")):
        q = capi.PosePrior()
        q.R0, q.T0, q.Lambda, q.scale = pps[2].c.R0, pps[2].c.T0, pps[2].c.Lambda, scale
        bads.append(("scale %r" % scale, q))
    q = capi.PosePrior()
    q.R0, q.T0, q.Lambda, q.scale, q.reserved_ = pps[2].c.R0, pps[2].c.T0, pps[2].c.Lambda, 1.0, 3
    bads.append(("reserved_", q))
    st = start(ba, sc)
    names = [n for n in STATE if getattr(st, n) is not None]
    for n in names:
        getattr(st, n).fill_(3)
    before = [getattr(st, n).clone() for n in names]
    ws = capi.workspace(64 << 20, DEV)
    L = capi.lib()
    for what, q in bads:
        s, keep = ops._schedule(ba.problems, ba.mlps, ba.l2_base, iters, False, None, None)
        arr = (capi.PosePrior * 3)()
        arr[1], arr[2] = pps[1].c, q
        s.workspace, s.workspace_bytes = ws.data_ptr(), ws.numel()
        assert L.banet_lm_solve_pose_prior_f32(ctypes.byref(s), None, arr, ctypes.byref(st.c), capi.stream()) == ppr.ERR_INVALID_ARG, what
        assert L.banet_lm_level_pose_prior_f32(ctypes.byref(ba.problems[2].c), ctypes.byref(ba.mlps[2].c), ba.l2_base, 2, None, None,
                                               ctypes.byref(q), ctypes.byref(st.c), ctypes.c_void_p(ws.data_ptr()), ws.numel(),
                                               capi.stream()) == ppr.ERR_INVALID_ARG, what
    s, keep = ops._schedule(ba.problems, ba.mlps, ba.l2_base, iters, True, None, None)      # early termination
    s.workspace, s.workspace_bytes = ws.data_ptr(), ws.numel()
    arr = (capi.PosePrior * 3)()
    assert L.banet_lm_solve_pose_prior_f32(ctypes.byref(s), None, arr, ctypes.byref(st.c), capi.stream()) == ppr.ERR_INVALID_ARG
    # ... and banet_pose_prior_apply_f32 on a NULL pointer or a bad struct leaves AtA / Atb alone
    c = ppr.apply_problem(2, 5)
    A, bb = t32(c["AtA"]), t32(c["Atb"])
    good = ops.PosePrior(t32(c["R0"]), t32(c["T0"]), t32(c["Lambda"]), 1.0)
    lvl = BareLevel(3, 5, 2)
    Rt, Tt = t32(c["R"]), t32(c["T"])
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    assert L.banet_pose_prior_apply_f32(ctypes.byref(lvl.c), ctypes.byref(good.c), None, ptr(Tt), ptr(A), ptr(bb), capi.stream()) == ppr.ERR_INVALID_ARG
    assert L.banet_pose_prior_apply_f32(ctypes.byref(lvl.c), ctypes.byref(good.c), ptr(Rt), ptr(Tt), ptr(A), None, capi.stream()) == ppr.ERR_INVALID_ARG
    half = capi.PosePrior()
    half.R0, half.Lambda, half.scale = good.c.R0, good.c.Lambda, 1.0
    assert L.banet_pose_prior_apply_f32(ctypes.byref(lvl.c), ctypes.byref(half), ptr(Rt), ptr(Tt), ptr(A), ptr(bb), capi.stream()) == ppr.ERR_INVALID_ARG
    lvl.c.variant = capi.LEGACY_FIXED
    assert L.banet_pose_prior_apply_f32(ctypes.byref(lvl.c), ctypes.byref(good.c), ptr(Rt), ptr(Tt), ptr(A), ptr(bb), capi.stream()) == ppr.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert all(wsc.bits_equal(getattr(st, n), x) for n, x in zip(names, before))
    assert wsc.bits_equal(A, t32(c["AtA"])) and wsc.bits_equal(bb, t32(c["Atb"]))
    with pytest.raises(capi.BanetError):
        ops.lm_solve(ba.problems, ba.mlps, ba.l2_base, iters, False, st, pose_priors=[None, pps[1], ops.PosePrior(Lambda=t32(po["Lambda"]))])


def test_dense_ba_solve_with_a_pose_prior_one_call_and_per_level():
    sc, ba = schedule_case(batch_invariant=False, name="schedule two frames")
    po, pi = pose_inputs(sc, 7), coef_inputs(sc, 9, 30.0)
    prior = dense_prior(po, [1000.0, 4000.0, 16000.0], pi=pi)
    snaps = []
    one, counts = ba.solve([2, 2, 2], start(ba, sc), prior=prior, snapshots=snaps)
    ba.c_schedule = False
    per, counts2 = ba.solve([2, 2, 2], start(ba, sc), prior=prior)
    torch.cuda.synchronize()
    assert state_bits_equal(one, per) and len(snaps) == 3 and wsc.bits_equal(snaps[2]["T"], one.T)
    assert [int(c[0]) for c in counts] == [int(c[0]) for c in counts2] == [2, 2, 2]
    coef_only, _ = ba.solve([2, 2, 2], start(ba, sc), prior=dense_prior(None, [1000.0, 4000.0, 16000.0], pi=pi))
    assert not wsc.bits_equal(coef_only.T, one.T)
    with pytest.raises(NotImplementedError, match="backward"):
        ba.solve_differentiable([1, 1, 1], prior=prior)


def test_workspace_contents_are_arbitrary_and_its_bounds_hold():
    sc, iters, _ = parity_scene("schedule two frames")
    other, _, _ = parity_scene("13x19 two frames")
    po, pi = pose_inputs(sc, 7), coef_inputs(sc, 9, 30.0)
    arena = wsc.Arena(96 << 20, DEV)

    def run():
        ba = dense_ba(sc)                                   # (owns a workspace: built inside)
        st, _ = ba.solve(iters, start(ba, sc), prior=dense_prior(po, [1000.0, 4000.0, 16000.0], pi=pi))
        cam = dense_ba(parity_scene("camera schedule")[0], variant="bundle_camera")
        sc_c = parity_scene("camera schedule")[0]
        st_c, _ = cam.solve(iters, start(cam, sc_c), prior=dense_prior(pose_inputs(sc_c, 7), [1000.0, 4000.0, 16000.0]))
        return tuple(getattr(st, n) for n in STATE) + (st_c.R, st_c.T, st_c.delta)

    def primer():                                           # another shape's leftovers in the same bytes
        ba = dense_ba(other)
        ba.solve([2], start(ba, other), prior=dense_prior(pose_inputs(other, 3), [500.0]))

    outs, seen = wsc.run_under_every_fill(run, arena, primer=primer)
    assert all(len(h) >= 2 for h in seen.values())
    wsc.assert_same_bits_across_fills(outs, names=list(STATE) + ["camera R", "camera T", "camera delta"])


# ======================================================================================================================
# marginals -> pose prior -> solve
# ======================================================================================================================
def test_pose_prior_of_the_solved_state_holds_it():
    """DenseBA.pose_prior(0, state) then solve(prior=) from the solved state: the state after it within the project's 1e-4 of the
    twin's (the twin builds its own Lambda from its float64 normal matrix at the same state), and closer to the start than the
    solve without the prior"""
    from banet_amd import dense as bdense
    sc = scene("one level 24x32", 3, 24, 32, 16, [1], 1, 31)
    B, K = sc["B"], sc["K"]
    ba = dense_ba(sc)
    solved, _ = ba.solve([4], start(ba, sc))
    prior = ba.pose_prior(0, solved)
    torch.cuda.synchronize()
    assert isinstance(prior, bdense.DensePrior) and prior.level_scale == [1.0] and prior.coef is None
    R0, T0, Lam = prior.pose
    assert R0.shape == (B, 1, 3, 3) and T0.shape == (B, 1, 3) and Lam.shape == (B, 6, 6) and Lam.dtype == torch.float32
    assert wsc.bits_equal(R0.reshape(-1), solved.R.reshape(-1)) and wsc.bits_equal(T0.reshape(-1), solved.T.reshape(-1))
    assert R0.data_ptr() != solved.R.data_ptr()
    Rs, Ts, Ws = n64(solved.R).reshape(B, 1, 3, 3), n64(solved.T).reshape(B, 1, 3, 1), n64(solved.Wc).reshape(B, K)
    # Lambda against float64 on the SAME float32 normal matrix: (the pose block of its inverse)^-1.  pose_cov comes back rounded to
    # float32, 2^-24 per entry, at most 6 x that in norm, and the inverse multiplies a relative perturbation by cond(cov): 8 cond 2^-24
    # leaves a quarter for the kernel's own factorisation (doubles) and the final cast
    from banet_amd import ops
    A = n64(ops.ba_assemble(ba.problems[0], solved.R, solved.T, solved.Wc)[0])
    for q, got in ((0.0, Lam), (1e-6, ba.pose_prior(0, solved, process_noise=1e-6).pose[2])):
        for b in range(B):
            cov = np.linalg.inv(A[b])[:6, :6] + q * np.eye(6)
            bound = 8 * np.linalg.cond(cov) * 2.0 ** -24
            err = relerr(n64(got)[b], np.linalg.inv(cov))
            print("pose_prior Q = %g window %d: |Lambda - float64| / max %.2e, bound %.2e" % (q, b, err, bound))
            assert err <= bound
    po = dict(R0=Rs[:, :, :, :].astype(np.float32), T0=Ts[:, :, :, 0].astype(np.float32), Lambda=n64(Lam).astype(np.float32))
    want = twin_solve(sc, [2], po, [1.0], R=Rs, T=Ts, W=Ws)
    moved = {}
    for what, pr in (("prior", prior), ("plain", None)):
        st = ba.new_state(R=solved.R.clone(), T=solved.T.clone(), Wc=solved.Wc.clone())
        ba.solve([2], st, prior=pr)
        torch.cuda.synchronize()
        moved[what] = ppr.log_norm(n64(st.R).reshape(B, 1, 3, 3), n64(st.T).reshape(B, 1, 3), Rs, Ts[:, :, :, 0])[:, 0]
        if pr is not None:
            e = dict(R=relerr(n64(st.R).reshape(B, 1, 3, 3), want["R"]), T=relerr(n64(st.T).reshape(B, 1, 3, 1), want["T"]),
                     Wc=relerr(n64(st.Wc).reshape(B, K), want["W"]))
            print("pose_prior then solve: against the twin %s" % e)
            assert max(e.values()) < 1e-4
    twin_moved = ppr.log_norm(want["R"], want["T"], Rs, Ts[:, :, :, 0])[:, 0]
    print("pose_prior then solve: |Log| moved with the prior %s (twin %s), without %s" % (moved["prior"], twin_moved, moved["plain"]))
    assert (moved["prior"] < moved["plain"]).all()
