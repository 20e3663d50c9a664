"""The pose prior's backward on the GPU (include/banet_hip.h (5g); csrc/pose_prior_grad.hip): banet_pose_prior_add_grad_f32 against the
float64 twin of tests/pose_prior_grad_ref.py, its accumulate / overwrite / partial-output / batch contracts and refusals,
ops.pose_prior_apply_diff, and DenseBA.solve_differentiable(prior=DensePrior(pose=...), pose_prior_backward=True) against
DenseBA.solve(prior=), the float64 chain of pose_prior_ref and its central differences."""
import functools

import numpy as np
import pytest
import torch

import pose_prior_grad_ref as ppg
import pose_prior_ref as ppr
import prior_ref as pref
import ws_contract as wsc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ppg.OUTPUTS
STATE_NAMES, PRIOR_NAMES = ("gR", "gT"), ("gR0", "gT0", "gLambda", "gscale")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from banet_amd import _capi
    _capi.lib()
    yield
    problem.cache_clear()


def t32(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32))).to(DEV)


def n64(x):
    return x.detach().double().cpu().numpy()


def f64(x):
    return np.asarray(x, np.float32).astype(np.float64)


class BareLevel:
    """a level with only what banet_pose_prior_add_grad_f32 reads"""

    def __init__(self, B, K, pairs):
        from banet_amd import _capi as capi
        self.c = capi.Level()
        self.c.B, self.c.K, self.c.pairs = B, K, pairs
        self.c.variant = capi.BUNDLE if K else capi.BUNDLE_CAMERA
        self.B, self.K, self.pairs = B, K, pairs


@functools.lru_cache(maxsize=None)
def problem(pairs, K):
    """the case and the twin's outputs and bounds, computed once and shared (read-only)"""
    c = ppg.grad_problem(pairs, K)
    return c, ppg.batch_grad(c, c["gAtA"], c["gAtb"])


def shapes(B, pairs):
    m = 6 * pairs
    return dict(gR=(B, pairs, 3, 3), gT=(B, pairs, 3), gR0=(B, pairs, 3, 3), gT0=(B, pairs, 3), gLambda=(B, m, m), gscale=(B,))


def run(c, want=NAMES, into=None, overwrite=None, windows=None, scale=ppr.APPLY_SCALE):
    from banet_amd import ops
    sel = (lambda x: t32(x)) if windows is None else (lambda x: t32(x[list(windows)]))
    pairs, K = c["R"].shape[1], c["gAtA"].shape[1] - 6 * c["R"].shape[1]
    gA, gb = sel(c["gAtA"]), sel(c["gAtb"])
    keep = (gA.clone(), gb.clone())
    pp = ops.PosePrior(sel(c["R0"]), sel(c["T0"]), sel(c["Lambda"]), scale)
    got = ops.pose_prior_add_grad(BareLevel(gA.shape[0], K, pairs), pp, sel(c["R"]), sel(c["T"]), gA, gb, want=want, into=into,
                                  overwrite=overwrite)
    torch.cuda.synchronize()
    assert wsc.bits_equal(gA, keep[0]) and wsc.bits_equal(gb, keep[1]), "gAtA / gAtb were written"
    return got


def as_dict(got):
    return {n: (None if getattr(got, n) is None else n64(getattr(got, n))) for n in NAMES}


# ======================================================================================================================
# banet_pose_prior_add_grad_f32 on synthetic gradients
# ======================================================================================================================
@pytest.mark.parametrize("pairs,K", ppr.APPLY_SHAPES)
def test_pose_prior_add_grad_against_the_twin(pairs, K):
    """B = 3, scale 0.37, every angle; K = 0 is the camera level, K = 130 makes gAtA's row stride differ from m, pairs = 7 spreads
    the poses of phase 3 over three waves.  Every output within 4 x F32_GRAD_ERR of its bound; gAtA / gAtb keep their bits (run)"""
    c, ref = problem(pairs, K)
    got = run(c)
    for n in NAMES:
        assert bool(torch.isfinite(getattr(got, n)).all()), n
    err = ppg.grad_errors(as_dict(got), ref)
    print("pose_prior_add_grad pairs %d K %d: %s  (gate %.3e, float32 torch %.3e)"
          % (pairs, K, "  ".join("%s %.3e" % kv for kv in err.items()), ppg.GRAD_GATE, ppg.F32_GRAD_ERR))
    assert set(err) == set(NAMES)
    for n, e in err.items():
        assert e <= ppg.GRAD_GATE, (n, e)


def _axis_rotations():
    """the 24 rotations whose entries are 0 and +-1: Re = R R^T = I and te = T - Re T bit for bit, in float32 as in float64"""
    import itertools
    out = []
    for p in itertools.permutations(range(3)):
        for sg in itertools.product((1.0, -1.0), repeat=3):
            M = np.zeros((3, 3))
            M[np.arange(3), p] = sg
            if np.linalg.det(M) > 0:
                out.append(M)
    return out


@pytest.mark.parametrize("pairs,K", [(1, 0), (2, 5), (7, 130)])
def test_exact_identity_is_finite_and_within_the_gate(pairs, K):
    """R = R0 and T = T0 with Re = I and te = 0 exactly (theta = 0, s = 0, rho = 0; R0 = I in the first pose of every window, the
    other axis-aligned rotations after it): every 0 / 0 of the chain is taken analytically -- finite, and every output within the
    gate of the twin, which evaluates the limit"""
    c = dict(ppg.grad_problem(pairs, K))
    rots = _axis_rotations()
    assert np.array_equal(rots[0], np.eye(3))
    c["R0"] = np.stack([[rots[(7 * b + 5 * i) * (i > 0) % 24] for i in range(pairs)] for b in range(3)]).astype(np.float32)
    c["R"], c["T"] = c["R0"].copy(), c["T0"].copy()
    ref = ppg.batch_grad(c, c["gAtA"], c["gAtb"])
    got = run(c)
    for n in NAMES:
        assert bool(torch.isfinite(getattr(got, n)).all()), n
    err = ppg.grad_errors(as_dict(got), ref)
    print("identity pairs %d K %d: %s" % (pairs, K, "  ".join("%s %.3e" % kv for kv in err.items())))
    assert set(err) == set(NAMES)
    for n, e in err.items():
        assert e <= ppg.GRAD_GATE, (n, e)


def test_equal_float32_poses_that_are_not_orthonormal_to_the_last_bit():
    """R = R0 and T = T0 bit for bit at rotations rounded to float32 (pairs 7, K 130): w = 0 and theta = 0 exactly, but Re = R0 R0^T
    is I only to 6e-8 and te = (I - Re) T0 is of that size.  Everything is finite and the pose outputs and gscale meet the gate.
    gLambda is not gated here: r and the off-diagonal of Jr ARE that rounding of the forward's float32 Re (absolute 6e-8, where the
    float64 value is 1e-8), they multiply entries of G of order 1, and the bound of an entry is as small as |G_kl| -- 4.8e-5 at the
    smallest of these 5292.  The float32 evaluation of the formulas on the host is 4.36e-4 of the bound there, and so is the kernel
    (the forward's bits, which the backward recomputes); the test above gates gLambda where the identity is exact."""
    c = dict(ppg.grad_problem(7, 130))
    c["R"], c["T"] = c["R0"].copy(), c["T0"].copy()
    ref = ppg.batch_grad(c, c["gAtA"], c["gAtb"])
    got = run(c)
    for n in NAMES:
        assert bool(torch.isfinite(getattr(got, n)).all()), n
    err = ppg.grad_errors(as_dict(got), ref)
    print("equal float32 poses, pairs 7 K 130: %s" % "  ".join("%s %.3e" % kv for kv in err.items()))
    for n in ("gR", "gT", "gR0", "gT0", "gscale"):
        assert err[n] <= ppg.GRAD_GATE, (n, err[n])
    host = ppg.grad_errors(ppg.batch_grad(c, c["gAtA"], c["gAtb"], mode="kernel", with_bounds=False), ref)
    assert err["gLambda"] <= 4 * host["gLambda"], (err["gLambda"], host["gLambda"])   # no further than the same 4 x from float32 on the host


@pytest.mark.parametrize("pairs,K", [(2, 5), (7, 130), (1, 0)])
def test_accumulate_is_overwrite_plus_the_previous_contents(pairs, K):
    """one rounding per element: |acc - fl(prev + written)| = 0, i.e. the accumulated value is the float32 sum of the two"""
    c, _ = problem(pairs, K)
    written = run(c)
    rng = np.random.RandomState(11)
    prev = {n: t32(rng.standard_normal(s)) for n, s in shapes(3, pairs).items()}
    for groups in (dict(state=False, prior=False), dict(state=True, prior=False), dict(state=False, prior=True)):
        into = {n: p.clone() for n, p in prev.items()}
        got = run(c, into=into, overwrite=groups)
        for n in NAMES:
            acc = not groups["state" if n in STATE_NAMES else "prior"]
            want = prev[n] + getattr(written, n).reshape(prev[n].shape) if acc else getattr(written, n).reshape(prev[n].shape)
            assert getattr(got, n) is into[n]
            assert wsc.bits_equal(into[n], want), (n, groups)


def test_outputs_not_asked_for_keep_their_bits_and_a_partial_want_gives_the_bits_of_the_full_call():
    pairs, K = 2, 5
    c, _ = problem(pairs, K)
    full = run(c)
    nan = {n: torch.full(s, float("nan"), device=DEV) for n, s in shapes(3, pairs).items()}
    for want in (("gLambda",), ("gscale",), ("gLambda", "gscale"), ("gR",), ("gT0",), ("gT", "gLambda"), ("gR0", "gT0", "gscale"),
                 ("gR", "gT", "gR0", "gT0")):
        got = run(c, want=want)
        for n in NAMES:
            if n in want:
                assert wsc.bits_equal(getattr(got, n), getattr(full, n)), (want, n)
            else:
                assert getattr(got, n) is None
        # the C entry with every pointer it is not given left out: the buffers it is not given are not touched (they are not passed),
        # and those it is given in accumulate mode over NaN stay NaN only where they are asked for
        bufs = {n: nan[n].clone() for n in NAMES}
        run(c, want=want, into={n: bufs[n] for n in want}, overwrite=dict(state=True, prior=True))
        for n in NAMES:
            if n in want:
                assert wsc.bits_equal(bufs[n], getattr(full, n).reshape(bufs[n].shape)), (want, n)
            else:
                assert bool(torch.isnan(bufs[n]).all())


def test_a_window_alone_has_the_bits_it_has_in_the_batch():
    for pairs, K in ((2, 5), (7, 130), (1, 0)):
        c, _ = problem(pairs, K)
        full = run(c)
        for w in range(3):
            one = run(c, windows=[w])
            for n in NAMES:
                assert wsc.bits_equal(getattr(one, n)[0], getattr(full, n)[w]), (pairs, K, w, n)


def test_refusals_return_their_codes_and_touch_nothing():
    import ctypes
    from banet_amd import _capi as capi, ops
    pairs, K, B = 2, 5, 3
    c, _ = problem(pairs, K)
    m, P = 6 * pairs, 6 * pairs + K
    R, T, gA, gb = t32(c["R"]), t32(c["T"]), t32(c["gAtA"]), t32(c["gAtb"])
    pp = ops.PosePrior(t32(c["R0"]), t32(c["T0"]), t32(c["Lambda"]), 0.37)
    bufs = {n: torch.full(s, float("nan"), device=DEV) for n, s in shapes(B, pairs).items()}
    L = capi.lib()

    def call(lv=None, q=pp.c, out_names=NAMES, flags=3, reserved=0, null=None, no_out=False):
        lv = BareLevel(B, K, pairs).c if lv is None else lv
        o = capi.PosePriorGrad()
        for n in out_names:
            setattr(o, n, bufs[n].data_ptr())
        o.flags, o.reserved_ = flags, reserved
        args = dict(R=R.data_ptr(), T=T.data_ptr(), gAtA=gA.data_ptr(), gAtb=gb.data_ptr())
        if null:
            args[null] = None
        return L.banet_pose_prior_add_grad_f32(ctypes.byref(lv), None if q is None else ctypes.byref(q), args["R"], args["T"], args["gAtA"],
                                               args["gAtb"], None if no_out else ctypes.byref(o), capi.stream())

    INV, UNS = -1, -3
    zero = capi.PosePrior()
    zero.R0, zero.T0, zero.Lambda, zero.scale = pp.c.R0, pp.c.T0, pp.c.Lambda, 0.0
    part = capi.PosePrior()
    part.R0, part.Lambda, part.scale = pp.c.R0, pp.c.Lambda, 1.0
    neg = capi.PosePrior()
    neg.R0, neg.T0, neg.Lambda, neg.scale = pp.c.R0, pp.c.T0, pp.c.Lambda, -1.0
    assert [call(q=q) for q in (None, capi.PosePrior(), zero, part, neg)] == [INV] * 5
    assert [call(flags=f) for f in (4, 7, 1 << 20)] == [INV] * 3 and call(reserved=2) == INV
    assert [call(null=k) for k in ("R", "T", "gAtA", "gAtb")] == [INV] * 4
    assert call(out_names=()) == INV and call(no_out=True) == INV
    legacy = BareLevel(B, 0, 1).c
    legacy.variant = capi.LEGACY_FIXED
    assert call(lv=legacy) == UNS and call(lv=BareLevel(B, K, 9).c) == UNS
    nobasis = BareLevel(B, 0, pairs).c
    nobasis.variant = capi.BUNDLE
    assert call(lv=nobasis) == UNS
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(b).all()) for b in bufs.values())
    assert call() == 0                                      # ... and the same arguments without a fault run
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(b).all()) for b in bufs.values())


def test_no_workspace_and_nothing_outside_the_outputs_changes_over_nan_filled_memory():
    """the entry takes no workspace.  One arena pre-filled with NaN holds the six outputs with guard words between them; in overwrite
    mode every output element is written (no NaN leaks into it) and every guard word keeps its bits"""
    from banet_amd import ops
    pairs, K, B = 7, 130, 3
    c, ref = problem(pairs, K)
    GUARD = 64
    sizes = {n: int(np.prod(s)) for n, s in shapes(B, pairs).items()}
    arena = torch.full((sum(sizes.values()) + GUARD * (len(NAMES) + 1),), float("nan"), device=DEV)
    into, off = {}, GUARD
    for n in NAMES:
        into[n] = arena[off:off + sizes[n]].view(shapes(B, pairs)[n])
        off += sizes[n] + GUARD
    before = arena.clone()
    got = run(c, into=into, overwrite=dict(state=True, prior=True))
    mask = torch.ones_like(arena, dtype=torch.bool)
    off = GUARD
    for n in NAMES:
        mask[off:off + sizes[n]] = False
        off += sizes[n] + GUARD
    assert wsc.bits_equal(arena[mask], before[mask])
    assert bool(torch.isfinite(arena[~mask]).all())
    err = ppg.grad_errors(as_dict(got), ref)
    assert max(err.values()) <= ppg.GRAD_GATE, err
    assert not hasattr(ops, "pose_prior_grad_workspace_bytes")


# ======================================================================================================================
# ops.pose_prior_apply_diff: torch.autograd through it against the twin
# ======================================================================================================================
@pytest.mark.parametrize("pairs,K", [(2, 5), (1, 0)])
def test_pose_prior_apply_diff_gradients_match_the_twin(pairs, K):
    from banet_amd import ops
    c, _ = problem(pairs, K)
    B, m, P = 3, 6 * pairs, 6 * pairs + K
    scale = ppr.APPLY_SCALE
    rng = np.random.RandomState(21)
    src = dict(R=c["R"], T=c["T"], R0=c["R0"], T0=c["T0"], Lambda=c["Lambda"], AtA=c["AtA"], Atb=c["Atb"])
    leaves = {k: t32(v).requires_grad_(True) for k, v in src.items()}
    lvl = BareLevel(B, K, pairs)
    pp = ops.PosePrior(leaves["R0"], leaves["T0"], leaves["Lambda"], scale)
    A0, b0 = leaves["AtA"].detach().clone(), leaves["Atb"].detach().clone()
    A2, b2 = ops.pose_prior_apply_diff(lvl, pp, leaves["R"], leaves["T"], leaves["AtA"], leaves["Atb"])
    assert torch.equal(leaves["AtA"], A0) and torch.equal(leaves["Atb"], b0)                    # out of place
    Ar, br = A0.clone(), b0.clone()
    ops.pose_prior_apply(lvl, ops.PosePrior(t32(c["R0"]), t32(c["T0"]), t32(c["Lambda"]), scale), t32(c["R"]), t32(c["T"]), Ar, br)
    assert torch.equal(A2, Ar) and torch.equal(b2, br)
    cA, cb = np.float32(rng.standard_normal((B, P, P))), np.float32(rng.standard_normal((B, P)))
    ((t32(cA) * A2).sum() + (t32(cb) * b2).sum()).backward()
    torch.cuda.synchronize()
    ref = ppg.batch_grad(c, cA, cb, scale)
    got = dict(gR=n64(leaves["R"].grad), gT=n64(leaves["T"].grad), gR0=n64(leaves["R0"].grad), gT0=n64(leaves["T0"].grad),
               gLambda=n64(leaves["Lambda"].grad))
    err = ppg.grad_errors(got, ref)
    print("pose_prior_apply_diff pairs %d K %d: %s" % (pairs, K, "  ".join("%s %.3e" % kv for kv in err.items())))
    for n, e in err.items():
        assert e <= ppg.GRAD_GATE, (n, e)
    assert torch.equal(leaves["AtA"].grad, t32(cA)) and torch.equal(leaves["Atb"].grad, t32(cb))   # they pass through
    # only what some input needs is asked for: with Lambda alone, gLambda -- the bits of the full call
    lone = t32(c["Lambda"]).requires_grad_(True)
    A3, b3 = ops.pose_prior_apply_diff(lvl, ops.PosePrior(t32(c["R0"]), t32(c["T0"]), lone, scale), t32(c["R"]), t32(c["T"]), t32(c["AtA"]),
                                       t32(c["Atb"]))
    ((t32(cA) * A3).sum() + (t32(cb) * b3).sum()).backward()
    assert torch.equal(lone.grad, leaves["Lambda"].grad)
    # the empty pose prior returns its arguments
    A4, b4 = ops.pose_prior_apply_diff(lvl, ops.PosePrior(), leaves["R"], leaves["T"], leaves["AtA"], leaves["Atb"])
    assert A4 is leaves["AtA"] and b4 is leaves["Atb"]


# ======================================================================================================================
# end to end: DenseBA.solve_differentiable(prior=DensePrior(pose=...), pose_prior_backward=True)
# ======================================================================================================================
def _e2e_scene(pairs, K):
    """the scenes of test_gpu_prior_grad._e2e_scene, with their ground-truth poses"""
    from oracle import banet_oracle as orc, dense as odense, synth
    C, B = 16, 2
    if pairs == 1:
        H, W = 48, 64
        scenes = [synth.make_pair_scene(H, W, C, K, [2, 1], 21 + b, normalize_rays=True, w_gt=[0.01, -0.008, 0.006], t_gt=[0.06, -0.04, 0.03])
                  for b in range(B)]
        intr, levels = odense.batch_scene(scenes)
        for lv in levels:
            lv["tgt"] = lv["tgt"][:, None]
    else:
        H, W = 40, 48
        scenes = [synth.make_window_scene(H, W, C, K, [2, 1], 61 + b, pairs, rot_mag=0.012, trans_mag=0.04) for b in range(B)]
        intr, levels = odense.batch_window_scene(scenes)
    R_gt = np.stack([np.asarray(s["R_gt"], np.float64).reshape(pairs, 3, 3) for s in scenes])
    T_gt = np.stack([np.asarray(s["T_gt"], np.float64).reshape(pairs, 3) for s in scenes])
    mlps = [orc.he_normal_mlp_weights(C, 40 + i, np.float64) for i in range(2)]
    return intr, levels, R_gt, T_gt, mlps, B, C


def _e2e(pairs, K, camera=False, with_coef=False, steps=(1, 3, 10)):
    """steps: the central differences are taken at these multiples of the step and their median is used"""
    from banet_amd import dense as bdense
    from oracle import banet_oracle as orc, dense as odense
    intr, levels, R_gt, T_gt, mlps, B, C = _e2e_scene(pairs, K)
    iters, m = [2, 2], 6 * pairs
    Kv = 0 if camera else K
    rng = np.random.RandomState(5)
    f32 = lambda v: np.asarray(v, np.float32).astype(np.float64)        # noqa: E731
    n = lambda x: x.detach().cpu().numpy().astype(np.float64)           # noqa: E731
    lv64 = [{k: (f32(v) if isinstance(v, np.ndarray) else v) for k, v in lv.items()} for lv in levels]
    Tstart = f32((T_gt * 0.7).reshape(B, pairs, 3, 1))
    W0 = f32(0.01 * rng.standard_normal((B, Kv, 1)))
    cR, cT, cW = rng.standard_normal((B, pairs, 3, 3)), rng.standard_normal((B, pairs, 3, 1)), rng.standard_normal((B, Kv, 1))

    # the pose prior: the ground-truth poses perturbed by a few 1e-2 in the tangent, Lambda seeded, symmetric positive definite
    R0, T0 = np.zeros((B, pairs, 3, 3)), np.zeros((B, pairs, 3))
    for b in range(B):
        for i in range(pairs):
            R0[b, i], T0[b, i] = ppr.compose(0.03 * rng.standard_normal(6), R_gt[b, i], T_gt[b, i])
    M = rng.standard_normal((B, m, m))
    Lam = np.einsum("bik,bjk->bij", M, M) / m + np.eye(m)
    Lam = Lam / np.mean([np.diag(Lam[b]).mean() for b in range(B)])
    pose = dict(R0=f32(R0), T0=f32(T0), Lambda=f32(0.5 * (Lam + Lam.transpose(0, 2, 1))))
    pri, k = None, 1.0
    if with_coef:       # the coefficient prior of test_gpu_prior_grad._e2e: (Lambda, eta) and weighted depth observations on both levels
        Mk = rng.standard_normal((B, K, K))
        pri = dict(Lambda=np.einsum("bik,bjk->bij", Mk, Mk) / K + np.eye(K), eta=rng.standard_normal((B, K)) * 0.05, obs=[], weight=[])
        for lv in lv64:
            Nl = lv["D0"].reshape(B, -1).shape[1]
            w = rng.uniform(0.5, 2.0, (B, Nl))
            w[:, ::4] = 0.0
            pri["obs"].append(f32(lv["D0"].reshape(B, Nl) * (1.0 + 0.02 * rng.standard_normal((B, Nl)))))
            pri["weight"].append(w)

    def chain(levels_, mlps_, pose_, pri_, W0_, T_, scale):
        Rs = [np.tile(np.eye(3)[None], (B, 1, 1)) for _ in range(pairs)]
        Ts = [T_[:, i].astype(np.float64).copy() for i in range(pairs)]
        Wn = W0_.copy()
        first = None
        for li, lv in enumerate(levels_):
            a = odense.level_inputs(np.asarray(intr, np.float64), dict(lv, tgt=lv["tgt"][:, 0]), True, np.float64)
            conv2s = [orc.target_map(lv["tgt"][:, i].astype(np.float64)) for i in range(pairs)]
            po = term = None
            if scale is not None:
                po = (pose_["R0"], pose_["T0"], pose_["Lambda"], scale)
                if pri_ is not None:
                    G, g = pref.fit_sums(a["D"][:, :, 0], a["Bs"], pri_["obs"][li], pri_["weight"][li])
                    term = pref.terms(scale, pri_["Lambda"], pri_["eta"], G, g)
            for _ in range(iters[li]):
                if camera:
                    Rs[0], Ts[0], dbg = ppr.camera_iteration(a, conv2s[0], Rs[0], Ts[0], mlps_[li], po)
                else:
                    Rs, Ts, Wn, dbg = ppr.window_iteration(a, conv2s, Rs, Ts, Wn, mlps_[li], 1000.0, po, term)
                first = first or dbg
        return np.stack(Rs, 1), np.stack(Ts, 1), Wn, first

    # as strong as the data term: the scale from the pose block's diagonal of the first iteration without the prior (Lambda's mean
    # diagonal is 1); the coefficient prior, which shares level_scale, is brought to the depth block's diagonal by its own size
    Rc, Tc, Wc_, first = chain(lv64, mlps, pose, None, W0, Tstart, None)
    data = np.mean([np.diag(first["AtA"][b, :m, :m]).mean() for b in range(B)])
    scale = float(np.float32(data))
    if with_coef:
        G0, _ = pref.fit_sums(lv64[0]["D0"].reshape(B, -1), lv64[0]["basis"].reshape(B, -1, K), pri["obs"][0], pri["weight"][0])
        own = np.mean([np.diag(G0[b] + pri["Lambda"][b]).mean() for b in range(B)])
        k = float(np.mean([np.diag(first["AtA"][b, m:, m:]).mean() for b in range(B)]) / (own * scale))
        pri = dict(Lambda=f32(k * pri["Lambda"]), eta=f32(k * pri["eta"]), obs=pri["obs"], weight=[f32(k * w) for w in pri["weight"]])

    def loss64(levels_=lv64, mlps_=mlps, pose_=pose, pri_=pri, W0_=W0, T_=Tstart):
        R, T, Wn, _ = chain(levels_, mlps_, pose_, pri_, W0_, T_, scale)
        return float((cR * R).sum() + (cT * T).sum() + (cW * Wn).sum())

    t = t32
    sq = (lambda x: x[:, 0]) if pairs == 1 else (lambda x: x)
    tl = [bdense.DenseLevel(lv["scale"], t(lv["src"]).requires_grad_(True), t(sq(lv["tgt"])).requires_grad_(True),
                            t(lv["D0"]).requires_grad_(True), None if camera else t(lv["basis"]).requires_grad_(True)) for lv in lv64]
    tm = [[(t(w).requires_grad_(True), t(b).requires_grad_(True)) for w, b in lw] for lw in mlps]
    ba = bdense.DenseBA(t(intr), tl, tm, "bundle_camera" if camera else "bundle", 1000.0)
    assert ba.pairs == pairs
    tpose = {k: t(v).requires_grad_(True) for k, v in pose.items()}
    coef = depth_obs = None
    if with_coef:
        tp = dict(Lambda=t(pri["Lambda"]).requires_grad_(True), eta=t(pri["eta"]).requires_grad_(True),
                  obs=[t(o.reshape(lv["D0"].shape)).requires_grad_(True) for o, lv in zip(pri["obs"], lv64)],
                  weight=[t(w.reshape(lv["D0"].shape)).requires_grad_(True) for w, lv in zip(pri["weight"], lv64)])
        coef, depth_obs = (tp["Lambda"], tp["eta"]), list(zip(tp["obs"], tp["weight"]))
    dp = bdense.DensePrior(coef=coef, depth_obs=depth_obs, level_scale=[scale, scale], pose=(tpose["R0"], tpose["T0"], tpose["Lambda"]))
    Tst = t(Tstart if pairs > 1 else Tstart[:, 0]).requires_grad_(True)
    W0t = t(W0).requires_grad_(True)
    kw = {} if camera else dict(Wc=W0t)

    # without the keyword the refusal stands
    with pytest.raises(NotImplementedError, match="backward"):
        ba.solve_differentiable(iters, T=Tst, prior=dp, **kw)
    # the control: the same scene without a prior meets the forward gates
    Rn, Tn, Wn0 = ba.solve_differentiable(iters, T=Tst, pose_prior_backward=True, **kw)
    for got, want in ((Rn, Rc), (Tn, Tc)) + (() if camera else ((Wn0, Wc_),)):
        assert np.abs(n(got).reshape(want.shape) - want).max() <= 1e-4 * max(np.abs(want).max(), 1e-6), "the prior-less control misses the gate"

    R, T, Wn = ba.solve_differentiable(iters, T=Tst, prior=dp, pose_prior_backward=True, **kw)
    st = ba.new_state(T=t(Tstart.reshape(B * pairs, 3, 1)) if pairs > 1 else Tst.detach().clone(), **({} if camera else dict(Wc=t(W0))))
    ba.solve(iters, st, prior=dp)
    assert torch.allclose(R, st.R.reshape(R.shape), atol=1e-6) and torch.allclose(T, st.T.reshape(T.shape), atol=1e-6)
    if not camera:
        assert torch.allclose(Wn, st.Wc.reshape(Wn.shape), atol=1e-6)
    Ro, To, Wo, _ = chain(lv64, mlps, pose, pri, W0, Tstart, scale)
    assert np.abs(To - Tc).max() > 1e-3 * np.abs(Tc).max(), "the pose prior does not move T"
    for got, want in ((R, Ro), (T, To)) + (() if camera else ((Wn, Wo),)):
        assert np.abs(n(got).reshape(want.shape) - want).max() <= 1e-4 * max(np.abs(want).max(), 1e-6)
    loss = (t(cR) * R.reshape(B, pairs, 3, 3)).sum() + (t(cT) * T.reshape(B, pairs, 3, 1)).sum() + (t(cW) * Wn).sum()
    loss.backward()
    torch.cuda.synchronize()

    def fd(apply, shape, eps, mask=None):
        dd = rng.standard_normal(shape)
        if mask is not None:
            dd = dd * mask
        dd /= np.linalg.norm(dd)
        vals = sorted((apply(e * dd) - apply(-e * dd)) / (2 * e) for e in [k * eps for k in steps])
        return dd, vals[len(vals) // 2]

    checks = []
    for key in ("R0", "T0", "Lambda"):                      # R0 along its nine free entries, Lambda as the full matrix
        def apply(dl, key=key):
            return loss64(pose_=dict(pose, **{key: pose[key] + dl}))
        dd, num = fd(apply, pose[key].shape, 1e-5)
        checks.append(("pose " + key, num, float((n(tpose[key].grad) * dd).sum())))
    dd, num = fd(lambda dl: loss64(T_=Tstart + dl), Tstart.shape, 1e-5)
    checks.append(("T start", num, float((n(Tst.grad).reshape(dd.shape) * dd).sum())))
    if not camera:
        dd, num = fd(lambda dl: loss64(W0_=W0 + dl), W0.shape, 1e-5)
        checks.append(("Wc0", num, float((n(W0t.grad) * dd).sum())))
    for li in range(2):
        for key, tens in (("src", tl[li].src), ("tgt", tl[li].tgt), ("D0", tl[li].depth)) + (() if camera else (("basis", tl[li].basis),)):
            def apply(dl, li=li, key=key):
                l2 = [dict(x) for x in lv64]
                l2[li][key] = lv64[li][key] + dl
                return loss64(levels_=l2)
            dd, num = fd(apply, lv64[li][key].shape, 1e-5)
            checks.append(("%s[%d]" % (key, li), num, float((n(tens.grad).reshape(dd.shape) * dd).sum())))
    if with_coef:
        for key in ("Lambda", "eta"):
            def apply(dl, key=key):
                return loss64(pri_=dict(pri, **{key: pri[key] + dl}))
            dd, num = fd(apply, pri[key].shape, 1e-5 * k)   # (the step that test takes on tensors of order 1, on tensors of order k)
            checks.append(("coef " + key, num, float((n(tp[key].grad) * dd).sum())))
        for key in ("obs", "weight"):
            def apply(dl, key=key):
                return loss64(pri_=dict(pri, **{key: [x + (dl if i == 0 else 0.0) for i, x in enumerate(pri[key])]}))
            live = (pri["weight"][0] > 0).astype(np.float64)
            dd, num = fd(apply, pri[key][0].shape, 1e-5 * (k if key == "weight" else 1.0), live)
            checks.append(("coef %s[0]" % key, num, float((n(tp[key][0].grad).reshape(dd.shape) * dd).sum())))

    def apply(dl):
        m2 = [[(w.copy(), b.copy()) for w, b in lw] for lw in mlps]
        m2[1][0] = (m2[1][0][0] + dl, m2[1][0][1])
        return loss64(mlps_=m2)
    dd, num = fd(apply, mlps[1][0][0].shape, 1e-4)
    checks.append(("mlp[1][0]", num, float((n(tm[1][0][0].grad) * dd).sum())))
    big = max(abs(c[1]) for c in checks)
    tag = "camera" if camera else "pairs %d K %d%s" % (pairs, K, " with the coefficient prior" if with_coef else "")
    for name, num, ana in checks:
        print("e2e %s: %-14s fd %+.6e  gpu %+.6e" % (tag, name, num, ana))
    for name, num, ana in checks:
        assert abs(num - ana) <= 2e-2 * max(abs(num), abs(ana)) + 1e-4 * big, (name, num, ana)


def test_solve_differentiable_with_a_pose_prior_matches_the_fused_forward_and_finite_differences():
    _e2e(pairs=1, K=8)


def test_solve_differentiable_with_a_pose_and_a_coefficient_prior_two_target_frames():
    _e2e(pairs=2, K=8, with_coef=True)


def test_solve_differentiable_with_a_pose_prior_on_the_camera_level():
    _e2e(pairs=1, K=8, camera=True)


# ======================================================================================================================
# unchanged behaviour
# ======================================================================================================================
def test_the_keyword_without_a_pose_prior_is_the_call_without_it():
    from banet_amd import dense as bdense
    intr, levels, R_gt, T_gt, mlps, B, C = _e2e_scene(1, 8)
    T0 = (T_gt * 0.7).reshape(B, 3, 1)
    iters = [2, 2]
    rng = np.random.RandomState(9)
    cR, cT, cW = (t32(rng.standard_normal(s)) for s in ((B, 3, 3), (B, 3, 1), (B, 8, 1)))
    eye = torch.eye(3, device=DEV).repeat(B, 1, 1, 1)
    empty_pose = (eye, torch.zeros(B, 1, 3, device=DEV), torch.ones(B, 6, 6, device=DEV))
    results = []
    for kw in ({}, dict(pose_prior_backward=True), dict(prior=None, pose_prior_backward=True),
               dict(prior=bdense.DensePrior(), pose_prior_backward=True),
               dict(prior=bdense.DensePrior(pose=empty_pose, level_scale=[0.0, 0.0]), pose_prior_backward=True)):
        tl = [bdense.DenseLevel(lv["scale"], t32(lv["src"]).requires_grad_(True), t32(lv["tgt"][:, 0]).requires_grad_(True),
                                t32(lv["D0"]).requires_grad_(True), t32(lv["basis"]).requires_grad_(True)) for lv in levels]
        tm = [[(t32(w).requires_grad_(True), t32(b).requires_grad_(True)) for w, b in lw] for lw in mlps]
        ba = bdense.DenseBA(t32(intr), tl, tm, "bundle", 1000.0)
        R, T, Wn = ba.solve_differentiable(iters, T=t32(T0), **kw)
        ((cR * R).sum() + (cT * T).sum() + (cW * Wn).sum()).backward()
        torch.cuda.synchronize()
        results.append([R.detach(), T.detach(), Wn.detach()] + [x.grad for lv in tl for x in (lv.src, lv.tgt, lv.depth, lv.basis)] +
                       [w.grad for lw in tm for w, _ in lw])
    for other in results[1:]:
        assert len(other) == len(results[0])
        for a, b in zip(results[0], other):
            assert torch.equal(a, b)
