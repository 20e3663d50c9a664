"""The backward of the prior term (include/banet_hip.h (5e); csrc/prior_grad.hip) on the GPU through the C ABI, against the float64
twin of tests/prior_grad_ref.py evaluated on the float32 inputs.

Bounds (each from the arithmetic, none from what the kernels give):
  * banet_prior_terms_f32: bit equality with the two float32 roundings of basis_fit's normal / rhs, and of prior_apply with the
    formed terms against prior_apply with the original prior;
  * banet_prior_add_grad_f32: gLe elementwise within 4 2^-24 (|gAtA| + |gAtb| |Wc| + |previous|) (one fma, one addition), gWc within
    (K + 2) 2^-24 sum_i |Le_ij| |gAtb_i| (a K-term fma chain, the butterfly, the subtraction);
  * banet_prior_terms_grad_f32: every output element within (K + 4) 2^-24 times the sum of the absolute values of the terms that
    make it up (the fp32 MFMA products are exact fmas in fixed chains: the standard bound of a K-term chain plus the roundings of
    Gh, gh and the final combination).  Each case prints the largest observed fraction of its bound (profiles/prior_grad.txt);
  * end to end: the gates of test_gpu_dense_backward.py's solve_differentiable test -- forward atol 1e-6 against DenseBA.solve(prior=),
    1e-4 relative against the float64 chain, gradients 2e-2 relative plus 1e-4 of the largest check against central differences;
  * everything else is bit equality."""
import numpy as np
import pytest
import torch

import prior_grad_ref as gref
import prior_ref as pref
import ws_contract as wsc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -24


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from banet_amd import _capi
    _capi.lib()


def t32(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32))).to(DEV)


def d(x):
    return None if x is None else x.detach().double().cpu().numpy()


def offset_view(x):
    """x as a view that starts 4 bytes past a 16-byte boundary, NaN before and after it"""
    flat = torch.full((x.numel() + 1 + 64,), float("nan"), dtype=torch.float32, device=x.device)
    view = flat[1:1 + x.numel()].view(x.shape)
    view.copy_(x)
    assert view.data_ptr() % 16 == 4
    return view


class BareLevel:
    """a level with only what the prior entries read (B, N, K, pairs, variant, depth, basis); dense or the sparse layout's N points"""

    def __init__(self, depth, basis, pairs, dense=True):
        from banet_amd import _capi as capi
        self.keep = [None, None, depth, basis]
        self.c = capi.Level()
        B, N, K = basis.shape
        self.c.B, self.c.N, self.c.K, self.c.pairs, self.c.variant = B, N, K, pairs, capi.BUNDLE
        self.c.dense, self.c.tgt_has_grad = int(dense), 0 if dense else 1
        self.c.depth, self.c.basis = depth.data_ptr(), basis.data_ptr()
        self.B, self.N, self.K, self.pairs, self.device = B, N, K, pairs, basis.device


def synthetic(K, N, B, seed, pairs=1):
    """float32 inputs; a tenth of the points uncounted by each of the three rules (w <= 0, NaN weight, inf observation)"""
    rng = np.random.RandomState(seed)
    P = 6 * pairs + K
    depth = rng.uniform(1, 3, (B, N))
    basis = rng.standard_normal((B, N, K)) / np.sqrt(K)
    obs = depth + rng.standard_normal((B, N)) * 0.1
    weight = rng.uniform(0.5, 2.0, (B, N))
    kind = rng.randint(0, 10, (B, N))
    weight[kind == 0] = np.where(rng.rand(int((kind == 0).sum())) < 0.5, 0.0, -0.7)
    weight[kind == 1] = np.nan
    obs[kind == 2] = np.where(rng.rand(int((kind == 2).sum())) < 0.5, np.inf, -np.inf)
    if N >= 96:
        obs[:, 32:64] = np.inf                              # a whole 32-pixel tile without a counted point: the kernel's short path
    s = dict(depth=depth, basis=basis, obs=obs, weight=weight, Lambda=rng.standard_normal((B, K, K)), eta=rng.standard_normal((B, K)),
             Le=rng.standard_normal((B, K, K)), ee=rng.standard_normal((B, K)), gLe=rng.standard_normal((B, K, K)),
             gee=rng.standard_normal((B, K)), Wc=rng.standard_normal((B, K)) * 0.3, gAtA=rng.standard_normal((B, P, P)),
             gAtb=rng.standard_normal((B, P)), AtA=rng.standard_normal((B, P, P)), Atb=rng.standard_normal((B, P)))
    return {k: t32(v) for k, v in s.items()}


def make_prior(s, has, scale, sel=None):
    from banet_amd import ops
    pick = (lambda x: x) if sel is None else (lambda x: x[sel].contiguous())
    return ops.Prior(*[pick(s[k]) if on else None for k, on in zip(("Lambda", "eta", "obs", "weight"), has)], scale=scale)


def allowed(has):
    return tuple(n for n, on in zip(gref.OUTPUTS, (has[0], has[1], 1, has[2], has[3], has[2], has[2])) if on)


# ======================================================================================================================
# banet_prior_terms_f32
# ======================================================================================================================
@pytest.mark.parametrize("K", [5, 32, 130])
def test_prior_terms_are_the_bits_prior_apply_forms(K):
    from banet_amd import ops
    B, N, pairs, scale = 3, 247, 1, 0.37
    s = synthetic(K, N, B, 40 + K)
    sym = 0.5 * (s["Lambda"] + s["Lambda"].transpose(1, 2))
    lvl = BareLevel(s["depth"], s["basis"], pairs)
    fit = ops.basis_fit(s["depth"], s["basis"], s["obs"], weight=s["weight"], want=("normal", "rhs"))
    sc = torch.tensor(scale, dtype=torch.float32, device=DEV)
    for has in ((1, 1, 1, 1), (0, 0, 1, 1), (1, 1, 0, 0), (1, 0, 0, 0)):
        prior = ops.Prior(sym if has[0] else None, s["eta"] if has[1] else None, s["obs"] if has[2] else None, s["weight"] if has[3] else None, scale)
        Le, ee = ops.prior_terms(lvl, prior)
        L0 = (fit.normal + sym) if (has[0] and has[2]) else fit.normal if has[2] else sym
        e0 = (fit.rhs + s["eta"]) if (has[1] and has[2]) else fit.rhs if has[2] else s["eta"] if has[1] else torch.zeros_like(s["eta"])
        assert wsc.bits_equal(Le, sc * L0) and wsc.bits_equal(ee, sc * e0), (K, has)             # two roundings each
        out = []
        for p in (prior, ops.Prior(Lambda=Le, eta=ee, scale=1.0)):                            # fl(1 x) = x
            A, b = s["AtA"].clone(), s["Atb"].clone()
            ops.prior_apply(lvl, p, s["Wc"], A, b)
            out.append((A, b))
        torch.cuda.synchronize()
        assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]), (K, has)
        assert not torch.equal(out[0][0], s["AtA"])
    assert ops.prior_terms(lvl, ops.Prior(sym, scale=0.0)) == (None, None) and ops.prior_terms(lvl, None) == (None, None)


# ======================================================================================================================
# banet_prior_add_grad_f32
# ======================================================================================================================
@pytest.mark.parametrize("pairs", [1, 2])
@pytest.mark.parametrize("K", [1, 5, 32, 130, 200, 256])
def test_prior_add_grad_against_the_twin(K, pairs):
    from banet_amd import ops
    B, m = 3, 6 * pairs
    s = synthetic(K, 8, B, 7 * K + pairs, pairs)
    lvl = BareLevel(s["depth"], s["basis"], pairs)
    (wLe, wee, wWc), (aLe, aWc) = gref.add_grad(d(s["Le"]), d(s["Wc"]), d(s["gAtA"]), d(s["gAtb"]), pairs)
    results = []
    for offset in (False, True):                           # aligned; Wc and gAtb offset by 4 bytes
        Wc, gAtb = ((offset_view(s[k]) if offset else s[k]) for k in ("Wc", "gAtb"))
        gLe, gee, gWc = ops.prior_add_grad(lvl, s["Le"], Wc, s["gAtA"], gAtb)                  # overwrite
        zLe, zee, _ = ops.prior_add_grad(lvl, s["Le"], Wc, s["gAtA"], gAtb, torch.zeros_like(gLe), torch.zeros_like(gee))
        assert torch.equal(zLe, gLe) and torch.equal(zee, gee)                                 # overwrite == accumulation into zeros
        assert torch.equal(gee, s["gAtb"][:, m:])
        err = np.abs(d(gLe) - wLe)
        bound = 4 * EPS * aLe
        fr1 = float((err / np.maximum(bound, 1e-300)).max())
        assert (err <= bound).all(), (K, pairs, offset, fr1)
        errW = np.abs(d(gWc) - wWc)
        boundW = (K + 2) * EPS * aWc
        frW = float((errW / np.maximum(boundW, 1e-300)).max())
        assert (errW <= boundW).all(), (K, pairs, offset, frW)
        # a second iteration accumulates into the first one's results (here: the same upstream again)
        prevLe, prevee, prevW = gLe.clone(), gee.clone(), gWc.clone()
        aLe2, aee2, aWc2 = ops.prior_add_grad(lvl, s["Le"], Wc, s["gAtA"], gAtb, gLe, gee, gWc)
        assert aLe2 is gLe and aWc2 is gWc
        err = np.abs(d(gLe) - (d(prevLe) + wLe))
        assert (err <= 4 * EPS * (aLe + np.abs(d(prevLe)))).all(), (K, pairs, offset)
        assert torch.equal(gee, prevee + s["gAtb"][:, m:])
        assert (np.abs(d(gWc) - (d(prevW) + wWc)) <= (K + 2) * EPS * aWc + EPS * np.abs(d(gWc))).all()
        print("PRIOR_GRAD_FRACTION add_grad K %d pairs %d offset %d: gLe %.3f gWc %.3f" % (K, pairs, offset, fr1, frW))
        results.append((gLe, gee, gWc))
    torch.cuda.synchronize()
    for a, b in zip(*results):
        assert wsc.bits_equal(a, b)                          # 16-byte and 4-byte accesses


# ======================================================================================================================
# banet_prior_terms_grad_f32
# ======================================================================================================================
FULL = (1, 1, 1, 1)
CASES = [  # K, N, B, halves (Lambda, eta, obs, weight), basis / gbasis offset by 4 bytes
    (1, 247, 3, FULL, False), (5, 5, 1, (0, 0, 1, 1), False), (5, 247, 3, (1, 0, 1, 0), False), (32, 768, 3, FULL, False),
    (32, 247, 3, FULL, True), (33, 247, 3, FULL, False), (33, 768, 1, (0, 0, 1, 0), False), (64, 5, 3, FULL, False),
    (128, 768, 3, FULL, False), (130, 247, 3, FULL, False), (130, 768, 1, (1, 1, 1, 0), False), (132, 247, 1, FULL, True),
    (200, 247, 3, (0, 0, 1, 1), False), (200, 768, 1, FULL, False), (256, 247, 3, FULL, False), (256, 768, 1, (1, 0, 1, 1), True),
    (16, 247, 3, (1, 1, 0, 0), False), (16, 247, 1, (1, 0, 0, 0), False)]


def run_terms_grad(s, lvl, prior, want, accumulate=False, into=None, gbasis_view=None):
    from banet_amd import ops
    into = dict(into or {})
    if gbasis_view is not None:
        into["gbasis"] = gbasis_view
    return ops.prior_terms_grad(lvl, prior, s["gLe"], s["gee"], s["Le"], s["ee"], want=want, accumulate=accumulate, into=into)


@pytest.mark.parametrize("K,N,B,has,offset", CASES)
def test_prior_terms_grad_against_the_twin(K, N, B, has, offset):
    scale = 0.37
    s = synthetic(K, N, B, 1000 + 10 * K + N % 7 + B)
    if offset:
        s["basis"] = offset_view(s["basis"])
    lvl = BareLevel(s["depth"], s["basis"], 1)
    prior = make_prior(s, has, scale)
    want = allowed(has)
    view = (lambda: offset_view(torch.empty(B, N, K, device=DEV))) if offset else (lambda: None)
    g = run_terms_grad(s, lvl, prior, want, gbasis_view=view() if has[2] else None)
    torch.cuda.synchronize()
    ref, mag = gref.terms_grad(np.float32(scale), d(s["gLe"]), d(s["gee"]), d(s["Le"]), d(s["ee"]), d(s["depth"]), d(s["basis"]),
                               d(s["obs"]) if has[2] else None, d(s["weight"]) if has[3] else None)
    ok = gref.counted(d(s["obs"]), d(s["weight"]) if has[3] else None) if has[2] else None
    if has[2]:
        frac = 1.0 - ok.mean()
        assert (0.15 < frac < 0.5 if has[3] else 0.03 < frac < 0.3) or N < 32, frac
    fr = {}
    for name in gref.OUTPUTS:
        got = getattr(g, name)
        if name not in want:
            assert got is None
            continue
        err = np.abs(d(got) - ref[name])
        bound = (K + 4) * EPS * mag[name]
        fr[name] = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
        assert np.isfinite(d(got)).all() and (err <= bound).all(), (name, fr[name])
        if name in ("gobs", "gweight", "gdepth", "gbasis"):                        # exact zeros at the points that are not counted
            assert not d(got)[~ok].any(), name
    print("PRIOR_GRAD_FRACTION terms_grad K %d N %d B %d has %s offset %d: %s" % (K, N, B, "".join(map(str, has)), offset,
                                                                                  " ".join("%s %.3f" % kv for kv in fr.items())))
    # two runs: the same bits
    g2 = run_terms_grad(s, lvl, prior, want, gbasis_view=view() if has[2] else None)
    for name in want:
        assert wsc.bits_equal(getattr(g, name), getattr(g2, name)), name
    # a subset of the outputs: the same bits
    for sub in [(n,) for n in want] + ([("gobs", "gbasis")] if has[2] else []):
        gs = run_terms_grad(s, lvl, prior, sub, gbasis_view=view() if (has[2] and "gbasis" in sub) else None)
        for name in sub:
            assert wsc.bits_equal(getattr(gs, name), getattr(g, name)), (sub, name)
    if has[2]:
        # accumulate into zeros == the written result; into a pattern: the uncounted points bit-untouched, the others pattern + value
        zb = view()
        zb = torch.zeros(B, N, K, device=DEV) if zb is None else zb.zero_()
        ga = run_terms_grad(s, lvl, prior, ("gdepth", "gbasis"), accumulate=True, into=dict(gdepth=torch.zeros(B, N, device=DEV), gbasis=zb))
        assert torch.equal(ga.gdepth, g.gdepth) and torch.equal(ga.gbasis, g.gbasis)
        rng = np.random.RandomState(5)
        pd, pb = t32(rng.standard_normal((B, N))), t32(rng.standard_normal((B, N, K)))
        pd[:, ::3], pb[:, ::3] = float("nan"), float("nan")                                   # a pattern a stray store or read-back would show in
        okt = torch.from_numpy(ok).to(DEV)
        pd[okt & torch.isnan(pd)] = 0.25
        pb[(okt[..., None] & torch.isnan(pb))] = -0.5
        bd, bb = pd.clone(), pb.clone()
        if offset:
            bb = offset_view(bb)
        run_terms_grad(s, lvl, prior, ("gdepth", "gbasis"), accumulate=True, into=dict(gdepth=bd, gbasis=bb))
        torch.cuda.synchronize()
        assert wsc.bits_equal(bd[~okt], pd[~okt]) and wsc.bits_equal(bb[~okt], pb[~okt])
        assert torch.equal(bd[okt], pd[okt] + g.gdepth[okt]) and torch.equal(bb[okt], pb[okt] + g.gbasis[okt])
    if B == 3:
        # a window alone: the bits it has in the batch
        one = {k: v[1:2].contiguous() for k, v in s.items()}
        if offset:
            one["basis"] = offset_view(one["basis"])
        g1 = run_terms_grad(one, BareLevel(one["depth"], one["basis"], 1), make_prior(one, has, scale), want,
                            gbasis_view=offset_view(torch.empty(1, N, K, device=DEV)) if (offset and has[2]) else None)
        for name in want:
            assert wsc.bits_equal(getattr(g1, name), getattr(g, name)[1:2]), name


def test_terms_and_terms_grad_keep_the_workspace_contract():
    """stale contents, NaN words, 1.0 words and another call's leftovers in the body, guard bands around it"""
    from banet_amd import ops
    K, N, B = 130, 247, 3
    s = synthetic(K, N, B, 77)
    lvl = BareLevel(s["depth"], s["basis"], 1)
    prior = make_prior(s, FULL, 0.37)
    s2 = synthetic(32, 768, 2, 78)
    lvl2 = BareLevel(s2["depth"], s2["basis"], 1)
    prior2 = make_prior(s2, FULL, 1.5)
    arena = wsc.Arena(64 << 20, DEV)

    def run():
        Le, ee = ops.prior_terms(lvl, prior)
        g = ops.prior_terms_grad(lvl, prior, s["gLe"], s["gee"], s["Le"], s["ee"])
        return (Le, ee) + tuple(g)

    def primer():
        ops.prior_terms(lvl2, prior2)
        ops.prior_terms_grad(lvl2, prior2, s2["gLe"], s2["gee"], s2["Le"], s2["ee"])

    outs, seen = wsc.run_under_every_fill(run, arena, primer)
    assert all(len(h) == 2 for h in seen.values())            # both workspaces came from the guarded allocator, at the exact query
    wsc.assert_same_bits_across_fills(outs, names=("Le", "ee") + gref.OUTPUTS)


# ======================================================================================================================
# ops.prior_apply_diff: torch.autograd through it against the twin
# ======================================================================================================================
@pytest.mark.parametrize("dense", [True, False])
def test_prior_apply_diff_gradients_match_the_twin(dense):
    from banet_amd import ops
    K, N, B, pairs, scale = 33, 247, 2, 2, 0.6
    s = synthetic(K, N, B, 5 + dense, pairs)
    leaves = {k: s[k].clone().requires_grad_(True) for k in ("Lambda", "eta", "obs", "weight", "depth", "basis", "Wc", "AtA", "Atb")}
    lvl = BareLevel(leaves["depth"], leaves["basis"], pairs, dense=dense)
    prior = ops.Prior(leaves["Lambda"], leaves["eta"], leaves["obs"], leaves["weight"], scale)
    A0, b0 = leaves["AtA"].detach().clone(), leaves["Atb"].detach().clone()
    A2, b2 = ops.prior_apply_diff(lvl, prior, leaves["Wc"], leaves["AtA"], leaves["Atb"])
    assert torch.equal(leaves["AtA"], A0) and torch.equal(leaves["Atb"], b0)                    # out of place
    Ar, br = A0.clone(), b0.clone()
    ops.prior_apply(lvl, ops.Prior(s["Lambda"], s["eta"], s["obs"], s["weight"], scale), s["Wc"], Ar, br)
    assert torch.equal(A2, Ar) and torch.equal(b2, br)
    rng = np.random.RandomState(3)
    cA, cb = rng.standard_normal(tuple(A2.shape)), rng.standard_normal(tuple(b2.shape))
    ((t32(cA) * A2).sum() + (t32(cb) * b2).sum()).backward()
    torch.cuda.synchronize()
    f = lambda k: d(s[k])                                                                       # noqa: E731
    want = gref.backward(np.float32(scale), f("Lambda"), f("eta"), f("depth"), f("basis"), f("obs"), f("weight"), f("Wc"),
                         np.float32(cA).astype(np.float64), np.float32(cb).astype(np.float64), pairs)
    names = dict(Lambda="gLambda", eta="geta", obs="gobs", weight="gweight", depth="gdepth", basis="gbasis", Wc="gWc", AtA="gAtA", Atb="gAtb")
    ok = gref.counted(f("obs"), f("weight"))
    for k, n in names.items():
        got, w = d(leaves[k].grad), want[n].reshape(tuple(leaves[k].shape))
        err = np.abs(got - w).max() / np.abs(w).max()
        print("prior_apply_diff dense %d: %s %.2e" % (dense, k, err))
        assert err < 1e-5, (k, err)                         # float32 against float64, K = 33 chains of O(1) terms: ~1e-6
        if k in ("obs", "weight", "depth", "basis"):
            assert not got[~ok].any()
    # only what some input needs is asked for: without any leaf, no backward call is made; with Lambda alone, only gLambda
    lone = s["Lambda"].clone().requires_grad_(True)
    A3, _ = ops.prior_apply_diff(BareLevel(s["depth"], s["basis"], pairs, dense), ops.Prior(lone, s["eta"], s["obs"], s["weight"], scale),
                                 s["Wc"], s["AtA"], s["Atb"])
    (t32(cA) * A3).sum().backward()
    m = 6 * pairs                                           # gAtb' = 0: gLe is the depth block of gAtA', gLambda = scale gLe
    assert np.abs(d(lone.grad) - np.float64(np.float32(scale)) * np.float32(cA).astype(np.float64)[:, m:, m:]).max() < 1e-6


# ======================================================================================================================
# end to end: DenseBA.solve_differentiable(prior=)
# ======================================================================================================================
def _e2e_scene(pairs, K):
    from oracle import banet_oracle as orc, dense as odense, synth
    C, B = 16, 2
    if pairs == 1:      # the scene of test_solve_differentiable_matches_the_fused_forward_and_oracle_finite_differences
        H, W = 48, 64
        scenes = [synth.make_pair_scene(H, W, C, K, [2, 1], 21 + b, normalize_rays=True, w_gt=[0.01, -0.008, 0.006], t_gt=[0.06, -0.04, 0.03])
                  for b in range(B)]
        intr, levels = odense.batch_scene(scenes)
        for lv in levels:
            lv["tgt"] = lv["tgt"][:, None]
    else:               # ... and of its multi-frame companion
        H, W = 40, 48
        scenes = [synth.make_window_scene(H, W, C, K, [2, 1], 61 + b, pairs, rot_mag=0.012, trans_mag=0.04) for b in range(B)]
        intr, levels = odense.batch_window_scene(scenes)
    T0 = (np.stack([np.asarray(s["T_gt"]) for s in scenes]) * 0.7).reshape(B, pairs, 3, 1)
    mlps = [orc.he_normal_mlp_weights(C, 40 + i, np.float64) for i in range(2)]
    return intr, levels, T0, mlps, B, C


def _e2e(pairs, K, steps=(1, 3, 10)):
    """steps: the central differences are taken at these multiples of the step and their median is used"""
    from banet_amd import dense as bdense
    from oracle import banet_oracle as orc, dense as odense
    intr, levels, T0, mlps, B, C = _e2e_scene(pairs, K)
    iters, m = [2, 2], 6 * pairs
    rng = np.random.RandomState(5)
    f32 = lambda v: np.asarray(v, np.float32).astype(np.float64)        # noqa: E731
    n = lambda x: x.detach().cpu().numpy().astype(np.float64)           # noqa: E731
    lv64 = [{k: (f32(v) if isinstance(v, np.ndarray) else v) for k, v in lv.items()} for lv in levels]
    W0 = f32(0.01 * rng.standard_normal((B, K, 1)))
    cR, cT, cW = rng.standard_normal((B, pairs, 3, 3)), rng.standard_normal((B, pairs, 3, 1)), rng.standard_normal((B, K, 1))

    # the prior: noisy observations of the depth on both levels with weights (a quarter of them zero), and (Lambda, eta)
    M = rng.standard_normal((B, K, K))
    pri = dict(Lambda=f32(np.einsum("bik,bjk->bij", M, M) / K + np.eye(K)), eta=f32(rng.standard_normal((B, K)) * 0.05), obs=[], weight=[])
    for lv in lv64:
        Nl = lv["D0"].reshape(B, -1).shape[1]
        w = rng.uniform(0.5, 2.0, (B, Nl))
        w[:, ::4] = 0.0
        pri["obs"].append(f32(lv["D0"].reshape(B, Nl) * (1.0 + 0.02 * rng.standard_normal((B, Nl)))))
        pri["weight"].append(f32(w))

    def chain(levels_, mlps_, pri_, W0_, scale):
        Rs = [np.tile(np.eye(3)[None], (B, 1, 1)) for _ in range(pairs)]
        Ts = [T0[:, i].astype(np.float64).copy() for i in range(pairs)]
        Wn = W0_.copy()
        first = None
        for li, lv in enumerate(levels_):
            a = odense.level_inputs(np.asarray(intr, np.float64), dict(lv, tgt=lv["tgt"][:, 0]), True, np.float64)
            conv2s = [orc.target_map(lv["tgt"][:, i].astype(np.float64)) for i in range(pairs)]
            term = None
            if scale is not None:
                G, g = pref.fit_sums(a["D"][:, :, 0], a["Bs"], pri_["obs"][li], pri_["weight"][li])
                term = pref.terms(scale, pri_["Lambda"], pri_["eta"], G, g)
            for _ in range(iters[li]):
                Rs, Ts, Wn, dbg = pref.window_iteration(a, conv2s, Rs, Ts, Wn, mlps_[li], 1000.0, term)
                first = first or dbg
        return np.stack(Rs, 1), np.stack(Ts, 1), Wn, first

    # as strong as the data term: the scale from the depth block's diagonal of the first iteration without the prior
    Rc, Tc, Wc_, first = chain(lv64, mlps, pri, W0, None)
    G0, _ = pref.fit_sums(lv64[0]["D0"].reshape(B, -1), lv64[0]["basis"].reshape(B, -1, K), pri["obs"][0], pri["weight"][0])
    data = np.mean([np.diag(first["AtA"][b, m:, m:]).mean() for b in range(B)])
    own = np.mean([np.diag(G0[b] + pri["Lambda"][b]).mean() for b in range(B)])
    scale = float(np.float32(data / own))

    def loss64(levels_=lv64, mlps_=mlps, pri_=pri, W0_=W0):
        R, T, Wn, _ = chain(levels_, mlps_, pri_, W0_, scale)
        return float((cR * R).sum() + (cT * T).sum() + (cW * Wn).sum())

    t = t32
    sq = (lambda x: x[:, 0]) if pairs == 1 else (lambda x: x)
    tl = [bdense.DenseLevel(lv["scale"], t(lv["src"]).requires_grad_(True), t(sq(lv["tgt"])).requires_grad_(True),
                            t(lv["D0"]).requires_grad_(True), t(lv["basis"]).requires_grad_(True)) for lv in lv64]
    tm = [[(t(w).requires_grad_(True), t(b).requires_grad_(True)) for w, b in lw] for lw in mlps]
    ba = bdense.DenseBA(t(intr), tl, tm, "bundle", 1000.0)
    assert ba.pairs == pairs
    tp = dict(Lambda=t(pri["Lambda"]).requires_grad_(True), eta=t(pri["eta"]).requires_grad_(True),
              obs=[t(o.reshape(lv["D0"].shape)).requires_grad_(True) for o, lv in zip(pri["obs"], lv64)],
              weight=[t(w.reshape(lv["D0"].shape)).requires_grad_(True) for w, lv in zip(pri["weight"], lv64)])
    dp = bdense.DensePrior(coef=(tp["Lambda"], tp["eta"]), depth_obs=list(zip(tp["obs"], tp["weight"])), level_scale=[scale, scale])
    Tst = t(T0 if pairs > 1 else T0[:, 0])
    W0t = t(W0).requires_grad_(True)

    # the control: the same scene without a prior meets the forward gates (its gradients: test_gpu_dense_backward.py)
    Rn, Tn, Wn0 = ba.solve_differentiable(iters, T=Tst, Wc=W0t)
    for got, want in ((Rn, Rc), (Tn, Tc), (Wn0, Wc_)):
        assert np.abs(n(got).reshape(want.shape) - want).max() <= 1e-4 * max(np.abs(want).max(), 1e-6), "the prior-less control misses the gate"

    R, T, Wn = ba.solve_differentiable(iters, T=Tst, Wc=W0t, prior=dp)
    st = ba.new_state(T=t(T0.reshape(B * pairs, 3, 1)) if pairs > 1 else Tst, Wc=t(W0))
    ba.solve(iters, st, prior=dp)
    assert torch.allclose(R, st.R.reshape(R.shape), atol=1e-6) and torch.allclose(T, st.T.reshape(T.shape), atol=1e-6)
    assert torch.allclose(Wn, st.Wc.reshape(Wn.shape), atol=1e-6)
    Ro, To, Wo, _ = chain(lv64, mlps, pri, W0, scale)
    assert np.abs(Wo - Wc_).max() > 1e-3 * np.abs(Wc_).max(), "the prior does not move the solution"
    for got, want in ((R, Ro), (T, To), (Wn, Wo)):
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
    for li in range(2):
        for key, tens in (("src", tl[li].src), ("tgt", tl[li].tgt), ("D0", tl[li].depth), ("basis", tl[li].basis)):
            def apply(dl, li=li, key=key):
                l2 = [dict(x) for x in lv64]
                l2[li][key] = lv64[li][key] + dl
                return loss64(levels_=l2)
            dd, num = fd(apply, lv64[li][key].shape, 1e-5)
            checks.append(("%s[%d]" % (key, li), num, float((n(tens.grad).reshape(dd.shape) * dd).sum())))
        for key in ("obs", "weight"):
            def apply(dl, li=li, key=key):
                p2 = dict(pri, **{key: [x + (dl if i == li else 0.0) for i, x in enumerate(pri[key])]})
                return loss64(pri_=p2)
            live = (pri["weight"][li] > 0).astype(np.float64)          # the perturbation does not cross w = 0: the zero weights stay
            dd, num = fd(apply, pri[key][li].shape, 1e-5, live)
            checks.append(("%s[%d]" % (key, li), num, float((n(tp[key][li].grad).reshape(dd.shape) * dd).sum())))
    for key in ("Lambda", "eta"):
        def apply(dl, key=key):
            return loss64(pri_=dict(pri, **{key: pri[key] + dl}))
        dd, num = fd(apply, pri[key].shape, 1e-5)
        checks.append((key, num, float((n(tp[key].grad) * dd).sum())))
    dd, num = fd(lambda dl: loss64(W0_=W0 + dl), W0.shape, 1e-5)
    checks.append(("Wc0", num, float((n(W0t.grad) * dd).sum())))

    def apply(dl):
        m2 = [[(w.copy(), b.copy()) for w, b in lw] for lw in mlps]
        m2[1][0] = (m2[1][0][0] + dl, m2[1][0][1])
        return loss64(mlps_=m2)
    dd, num = fd(apply, mlps[1][0][0].shape, 1e-4)
    checks.append(("mlp[1][0]", num, float((n(tm[1][0][0].grad) * dd).sum())))
    big = max(abs(c[1]) for c in checks)
    for name, num, ana in checks:
        print("e2e pairs %d K %d: %-10s fd %+.6e  gpu %+.6e" % (pairs, K, name, num, ana))
    for name, num, ana in checks:
        assert abs(num - ana) <= 2e-2 * max(abs(num), abs(ana)) + 1e-4 * big, (name, num, ana)
    # the zero weights are not counted: no gradient reaches them or their observations
    for li in range(2):
        dead = torch.from_numpy(pri["weight"][li] == 0).to(DEV).reshape(tp["weight"][li].shape)
        assert not tp["weight"][li].grad[dead].any() and not tp["obs"][li].grad[dead].any()


def test_solve_differentiable_with_a_prior_matches_the_fused_forward_and_finite_differences():
    _e2e(pairs=1, K=8)


def test_solve_differentiable_with_a_prior_two_target_frames_below_32_unknowns():
    """P = 20: the backward's solves run on the factorisation inside small_post_kernel"""
    _e2e(pairs=2, K=8)


def test_solve_differentiable_with_a_prior_two_target_frames_K40():
    _e2e(pairs=2, K=40, steps=(3,))                         # (one step: the float64 chain costs five times the K = 8 one)


def test_solve_differentiable_with_a_prior_K200_against_float64_autograd_of_one_level():
    """K = 200 (P = 206: the wide small step, the 4-wave per-pixel kernel), one level, one iteration, no finite differences: the
    gradients of the prior's own tensors against torch float64 autograd of the twin's level -- the term in float64 on the float32
    inputs, added to the level's assembled AtA / Atb (constants here: the prior's tensors reach the output through the term
    alone), then dense_train.solve_update_graph in float64.  Gates: the forward within 1e-4 and every gradient tensor within
    2e-2 of its largest entry, the end-to-end gates of the cases above."""
    from banet_amd import dense as bdense, dense_train, ops
    from oracle import banet_oracle as orc, dense as odense, synth
    H, W, C, K, B = 24, 32, 16, 200, 2
    scenes = [synth.make_pair_scene(H, W, C, K, [1], 21 + b, normalize_rays=True, w_gt=[0.01, -0.008, 0.006], t_gt=[0.06, -0.04, 0.03])
              for b in range(B)]
    intr, levels = odense.batch_scene(scenes)
    rng = np.random.RandomState(12)
    lv = levels[0]
    N = H * W
    lv["basis"] = (rng.standard_normal(lv["basis"].shape) / np.sqrt(K)).astype(np.float32)    # (the DCT basis has numerically zero columns at K = 200)
    mlps = [orc.he_normal_mlp_weights(C, 40, np.float64)]
    T0 = t32((np.stack([np.asarray(s["T_gt"]) for s in scenes]) * 0.7).reshape(B, 3, 1))
    W0 = t32(0.01 * rng.standard_normal((B, K, 1)))
    cR, cT, cW = (t32(rng.standard_normal(s)) for s in ((B, 3, 3), (B, 3, 1), (B, K, 1)))
    M = rng.standard_normal((B, K, K))
    w = rng.uniform(0.5, 2.0, (B, N))
    w[:, ::4] = 0.0
    leaves = dict(Lambda=t32(np.einsum("bik,bjk->bij", M, M) / K + np.eye(K)), eta=t32(rng.standard_normal((B, K)) * 0.05),
                  obs=t32(lv["D0"].reshape(B, N) * (1.0 + 0.02 * rng.standard_normal((B, N)))), weight=t32(w))
    for v in leaves.values():
        v.requires_grad_(True)
    tl = [bdense.DenseLevel(lv["scale"], t32(lv["src"]), t32(lv["tgt"]), t32(lv["D0"]), t32(lv["basis"]))]
    ba = bdense.DenseBA(t32(intr), tl, mlps, "bundle", 1000.0)
    prob = ba.problems[0]
    R0 = torch.eye(3, device=DEV).repeat(B, 1, 1)
    AtA0, Atb0, absres, _ = ops.ba_assemble(prob, R0, T0, W0)
    depth, basis = prob.keep[2].reshape(B, N).double(), prob.keep[3].reshape(B, N, K).double()
    # as strong as the data term
    G0 = torch.einsum("bn,bni,bnj->bij", leaves["weight"].detach().double(), basis, basis)
    scale = float(np.float32((torch.diagonal(AtA0[:, 6:, 6:], dim1=1, dim2=2).mean() /
                              torch.diagonal(G0 + leaves["Lambda"].detach().double(), dim1=1, dim2=2).mean()).item()))
    dp = bdense.DensePrior(coef=(leaves["Lambda"], leaves["eta"]), depth_obs=[(leaves["obs"].reshape(B, H, W), leaves["weight"].reshape(B, H, W))],
                           level_scale=[scale])
    R, T, Wn = ba.solve_differentiable([1], T=T0, Wc=W0, prior=dp)
    ((cR * R).sum() + (cT * T).sum() + (cW * Wn).sum()).backward()
    torch.cuda.synchronize()

    l64 = {k: v.detach().double().requires_grad_(True) for k, v in leaves.items()}
    wv = torch.where(l64["weight"] > 0, l64["weight"], torch.zeros_like(l64["weight"]))
    G = torch.einsum("bn,bni,bnj->bij", wv, basis, basis)
    g = torch.einsum("bn,bni->bi", wv * (l64["obs"] - depth), basis)
    s64 = float(np.float32(scale))
    Le, ee = s64 * (G + l64["Lambda"]), s64 * (g + l64["eta"])
    A2 = AtA0.double() + torch.nn.functional.pad(Le, (6, 0, 6, 0))
    b2 = Atb0.double().reshape(B, -1) + torch.nn.functional.pad(ee - torch.einsum("bij,bj->bi", Le, W0.double()[:, :, 0]), (6, 0))
    layers = [(torch.as_tensor(wt, dtype=torch.float64, device=DEV).reshape(wt.shape[-2], wt.shape[-1]),
               torch.as_tensor(bt, dtype=torch.float64, device=DEV).reshape(-1)) for wt, bt in mlps[0]]
    R6, T6, W6 = dense_train.solve_update_graph(A2, b2, absres.double(), N, R0.double(), T0.double(), W0.double(), layers, 1000.0)
    for got, want in ((R, R6), (T, T6), (Wn, W6)):
        got, want = got.detach().double(), want.detach().reshape(got.shape)
        assert float((got - want).abs().max()) <= 1e-4 * max(float(want.abs().max()), 1e-6)
    ((cR.double() * R6).sum() + (cT.double() * T6).sum() + (cW.double() * W6.reshape(B, K, 1)).sum()).backward()
    for k in leaves:
        got, want = leaves[k].grad.double(), l64[k].grad
        err = float((got - want).abs().max() / want.abs().max())
        print("e2e K 200, one level: %-7s max error / max |gradient| %.2e" % (k, err))
        assert err <= 2e-2, (k, err)
    assert not leaves["weight"].grad[leaves["weight"] == 0].any()


# ======================================================================================================================
# unchanged behaviour
# ======================================================================================================================
def test_no_prior_and_the_empty_prior_are_the_call_without_the_argument():
    from banet_amd import dense as bdense
    intr, levels, T0, mlps, B, C = _e2e_scene(1, 8)
    iters = [2, 2]
    rng = np.random.RandomState(9)
    cR, cT, cW = (t32(rng.standard_normal(s)) for s in ((B, 3, 3), (B, 3, 1), (B, 8, 1)))
    results = []
    for kw in ({}, dict(prior=None), dict(prior=bdense.DensePrior()), dict(prior=bdense.DensePrior(
            coef=(torch.ones(B, 8, 8, device=DEV), None), level_scale=[0.0, 0.0]))):
        tl = [bdense.DenseLevel(lv["scale"], t32(lv["src"]).requires_grad_(True), t32(lv["tgt"][:, 0]).requires_grad_(True),
                                t32(lv["D0"]).requires_grad_(True), t32(lv["basis"]).requires_grad_(True)) for lv in levels]
        tm = [[(t32(w).requires_grad_(True), t32(b).requires_grad_(True)) for w, b in lw] for lw in mlps]
        ba = bdense.DenseBA(t32(intr), tl, tm, "bundle", 1000.0)
        R, T, Wn = ba.solve_differentiable(iters, T=t32(T0[:, 0]), **kw)
        ((cR * R).sum() + (cT * T).sum() + (cW * Wn).sum()).backward()
        torch.cuda.synchronize()
        results.append([R.detach(), T.detach(), Wn.detach()] + [x.grad for lv in tl for x in (lv.src, lv.tgt, lv.depth, lv.basis)] +
                       [w.grad for lw in tm for w, _ in lw])
    for other in results[1:]:
        assert len(other) == len(results[0])
        for a, b in zip(results[0], other):
            assert torch.equal(a, b)


def test_solve_differentiable_refuses_a_prior_without_a_depth_basis():
    from banet_amd import _capi as capi, dense as bdense
    intr, levels, T0, mlps, B, C = _e2e_scene(1, 8)
    tl = [bdense.DenseLevel(lv["scale"], t32(lv["src"]), t32(lv["tgt"][:, 0]), t32(lv["D0"]), None) for lv in levels]
    ba = bdense.DenseBA(t32(intr), tl, mlps, "bundle_camera", 1000.0)
    with pytest.raises(capi.BanetError):
        ba.solve_differentiable([1, 1], T=t32(T0[:, 0]), prior=bdense.DensePrior(coef=(torch.ones(B, 8, 8, device=DEV), None)))
