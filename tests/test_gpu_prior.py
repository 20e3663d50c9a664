"""Depth observations and coefficient priors inside the LM loop (include/banet_hip.h (5d); csrc/prior.hip) on the GPU through the C
ABI, against the float64 twin of tests/prior_ref.py (the oracle's iteration with the term added before its damping).

Shapes: 24 x 32 and a ragged 13 x 19, C = 16 with one C = 128 case, B in {1, 3}.  Bounds:
  * banet_prior_apply_f32: the depth block of AtA bit-equal to AtA + Le with Le built in float32 torch from the two roundings, every
    other entry bit-unchanged; Atb's depth rows within (K + 2) 2^-24 (|Atb_i| + |ee_i| + sum_j |Le_ij| |Wc_j|) of float64 -- one
    rounding per fma of the K-term chain and butterfly, one for the subtraction, one for the addition;
  * solves: delta, R, T, Wc within the project's 1e-4 (max |got - want| / max |want|, as test_gpu_parity.py) of the twin; the same
    scene WITHOUT a prior is run as a control and must meet 1e-4 too, so that a miss is attributable to the prior;
  * everything else is bit equality."""
import ctypes

import numpy as np
import pytest
import torch

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


def relerr(got, want):
    want, got = np.asarray(want, np.float64), np.asarray(got, np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))


def offset_view(x):
    """x as a view that starts 4 bytes past a 16-byte boundary, NaN before and after it"""
    flat = torch.full((x.numel() + 1 + 64,), float("nan"), dtype=torch.float32, device=x.device)
    view = flat[1:1 + x.numel()].view(x.shape)
    view.copy_(x)
    assert view.data_ptr() % 16 == 4
    return view


def state_bits_equal(a, b):
    return all(wsc.bits_equal(getattr(a, n), getattr(b, n)) for n in STATE)


# ======================================================================================================================
# banet_prior_apply_f32 on synthetic normal equations
# ======================================================================================================================
class BareLevel:
    """a level with only what banet_prior_apply_f32 reads"""

    def __init__(self, depth, basis, pairs):
        from banet_amd import _capi as capi
        self.keep = (depth, basis)
        self.c = capi.Level()
        B, N, K = basis.shape
        self.c.B, self.c.N, self.c.K, self.c.pairs, self.c.variant = B, N, K, pairs, capi.BUNDLE
        self.c.depth, self.c.basis = depth.data_ptr(), basis.data_ptr()


def synthetic(K, pairs, seed, B=3, N=13 * 19):
    rng = np.random.RandomState(seed)
    P = 6 * pairs + K
    depth = rng.uniform(1, 3, (B, N))
    basis = rng.standard_normal((B, N, K)) / np.sqrt(K)
    obs = depth + rng.standard_normal((B, N)) * 0.1
    weight = rng.uniform(0.5, 2.0, (B, N))
    weight[:, ::5] = 0.0
    M = rng.standard_normal((B, K, K))
    Lambda = np.einsum("bik,bjk->bij", M, M) / K + np.eye(K)
    Q = rng.standard_normal((B, P, P))
    return dict(depth=t32(depth), basis=t32(basis), obs=t32(obs), weight=t32(weight), Lambda=t32(Lambda), eta=t32(rng.standard_normal((B, K))),
                AtA=t32(np.einsum("bik,bjk->bij", Q, Q) + P * np.eye(P)), Atb=t32(rng.standard_normal((B, P))),
                Wc=t32(rng.standard_normal((B, K)) * 0.3), P=P)


@pytest.mark.parametrize("pairs", [1, 2])
@pytest.mark.parametrize("K", [1, 5, 32, 130, 200])
def test_prior_apply_on_synthetic_normal_equations(K, pairs):
    from banet_amd import ops
    s = synthetic(K, pairs, 10 * K + pairs)
    scale, m, P = 0.37, 6 * pairs, s["P"]
    results = []
    for offset in (False, True):                           # aligned; basis / Lambda / Wc offset by 4 bytes
        basis, Lambda, Wc = ((offset_view(s[k]) if offset else s[k]) for k in ("basis", "Lambda", "Wc"))
        lvl = BareLevel(s["depth"], basis, pairs)
        fit = ops.basis_fit(s["depth"], basis, s["obs"], weight=s["weight"], want=("normal", "rhs"))
        sc = torch.tensor(scale, dtype=torch.float32, device=DEV)
        Le, ee = sc * (fit.normal + Lambda), sc * (fit.rhs + s["eta"])           # two roundings each
        A, b = s["AtA"].clone(), s["Atb"].clone()
        ops.prior_apply(lvl, ops.Prior(Lambda, s["eta"], s["obs"], s["weight"], scale), Wc, A, b)
        torch.cuda.synchronize()
        want = s["AtA"].clone()
        want[:, m:, m:] += Le
        assert wsc.bits_equal(A, want), "K %d pairs %d offset %s: AtA" % (K, pairs, offset)    # the depth block, and nothing else
        assert wsc.bits_equal(b[:, :m], s["Atb"][:, :m])
        d = lambda x: x.double().cpu().numpy()
        dot_abs = np.einsum("bij,bj->bi", np.abs(d(Le)), np.abs(d(Wc)))
        ref = d(s["Atb"])[:, m:] + d(ee) - np.einsum("bij,bj->bi", d(Le), d(Wc))
        bound = (K + 2) * 2.0 ** -24 * (np.abs(d(s["Atb"])[:, m:]) + np.abs(d(ee)) + dot_abs)
        err = np.abs(d(b)[:, m:] - ref)
        print("prior_apply K %d pairs %d offset %s: Atb error / bound %.3f" % (K, pairs, offset, (err / bound).max()))
        assert (err <= bound).all()
        results.append((A, b))
    assert wsc.bits_equal(results[0][0], results[1][0]) and wsc.bits_equal(results[0][1], results[1][1])      # 16-byte and 4-byte loads


def test_observation_form_equals_coefficient_form_bit_for_bit():
    from banet_amd import ops
    s = synthetic(32, 1, 77)
    obs, weight = s["obs"].clone(), s["weight"].clone()
    live = torch.nonzero(weight[0] > 0).reshape(-1)
    obs[0, live[0]] = float("nan")                          # a NaN target and an inf weight under w > 0: excluded by both forms
    weight[0, live[1]] = float("inf")
    assert int((weight == 0).sum()) > 100
    lvl = BareLevel(s["depth"], s["basis"], 1)
    fit = ops.basis_fit(s["depth"], s["basis"], obs, weight=weight, want=("normal", "rhs"))
    out = []
    for prior in (ops.Prior(obs_depth=obs, obs_weight=weight, scale=0.37), ops.Prior(Lambda=fit.normal, eta=fit.rhs, scale=0.37)):
        A, b = s["AtA"].clone(), s["Atb"].clone()
        ops.prior_apply(lvl, prior, s["Wc"], A, b)
        out.append((A, b))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out[0][0]).all()) and not wsc.bits_equal(out[0][0], s["AtA"])
    assert wsc.bits_equal(out[0][0], out[1][0]) and wsc.bits_equal(out[0][1], out[1][1])


# ======================================================================================================================
# scenes, solvers and the twin
# ======================================================================================================================
def scene(key, B, H, W, K, scales, pairs, seed, channels=C, random_basis=False):
    """-> dict(intr, levels (numpy, tgt [B,pairs,H,W,C]), mlps, T0 [B,pairs,3,1], W_gt [B,K]), built once per module.  The motion
    and the start of a multi-level scene: prior_ref.SCHEDULE_MOTION (chosen so that the last update of the schedule is not a small
    one; test_prior_cpu.py checks the float32 oracle against the float64 one on the same scenes)"""
    if key not in _CACHE:
        from oracle import banet_oracle as orc, dense as odense, synth
        trans_mag, frac = pref.SCHEDULE_MOTION if len(scales) > 1 else (0.03, 0.7)
        scenes = [synth.make_window_scene(H, W, channels, K, scales, seed + b, pairs, trans_mag=trans_mag) for b in range(B)]
        intr, levels = odense.batch_scene(scenes)
        if random_basis:                                    # (the DCT basis has numerically zero columns once K exceeds what the map resolves)
            rng = np.random.RandomState(seed + 99)
            for lv in levels:
                lv["basis"] = (rng.standard_normal(lv["basis"].shape) / np.sqrt(K)).astype(np.float32)
        _CACHE[key] = dict(intr=intr, levels=levels, mlps=[orc.he_normal_mlp_weights(channels, 5 + i) for i in range(len(levels))],
                           T0=np.stack([np.asarray(s["T_gt"]) * frac for s in scenes]).reshape(B, pairs, 3, 1).astype(np.float32),
                           W_gt=np.stack([s["W_gt"] for s in scenes]), B=B, K=K, pairs=pairs)
    return _CACHE[key]


def dense_ba(sc, windows=None, batch_invariant=False):
    from banet_amd import dense as bdense
    idx = list(range(sc["B"])) if windows is None else list(windows)
    tl = [bdense.DenseLevel(lv["scale"], *(t32(lv[k][idx]) for k in ("src", "tgt", "D0", "basis"))) for lv in sc["levels"]]
    return bdense.DenseBA(t32(sc["intr"][idx]), tl, sc["mlps"], "bundle", L2, batch_invariant=batch_invariant)


def start(ba, sc, windows=None):
    idx = list(range(sc["B"])) if windows is None else list(windows)
    T0 = sc["T0"][idx]
    return ba.new_state(T=t32(T0 if sc["pairs"] > 1 else T0[:, 0]))


def prior_inputs(sc, seed, strength=1.0):
    """per level: observations of the true depth with some noise, weights with zeros; one (Lambda, eta) around W_gt"""
    rng = np.random.RandomState(seed)
    B, K = sc["B"], sc["K"]
    M = rng.standard_normal((B, K, K))
    Lambda = (strength * (np.einsum("bik,bjk->bij", M, M) / K + np.eye(K))).astype(np.float32)
    eta = np.einsum("bij,bj->bi", Lambda.astype(np.float64), sc["W_gt"] + rng.standard_normal((B, K)) * 0.01).astype(np.float32)
    obs = []
    for lv in sc["levels"]:
        N = lv["H"] * lv["W"]
        o = lv["D0"].reshape(B, N).astype(np.float64) + np.einsum("bnk,bk->bn", lv["basis"].reshape(B, N, K).astype(np.float64), sc["W_gt"])
        w = rng.uniform(0.5, 2.0, (B, N))
        w[:, ::4] = 0.0
        obs.append(((o + rng.standard_normal((B, N)) * 0.01).astype(np.float32).reshape(lv["D0"].shape), w.astype(np.float32).reshape(lv["D0"].shape)))
    return dict(Lambda=Lambda, eta=eta, obs=obs)


def dense_prior(pi, scales, windows=None, coef=True, obs=True):
    from banet_amd import dense as bdense
    sel = (lambda x: x) if windows is None else (lambda x: x[list(windows)])
    return bdense.DensePrior(coef=(t32(sel(pi["Lambda"])), t32(sel(pi["eta"]))) if coef else None,
                             depth_obs=[(t32(sel(o)), t32(sel(w))) for o, w in pi["obs"]] if obs else None, level_scale=scales)


def twin_solve(sc, iters, pi=None, scales=None):
    """the float64 twin over the schedule -> dict(R [B,pairs,3,3], T, W [B,K], delta [B,P], first = the first iteration's record)"""
    from oracle import banet_oracle as orc, dense as odense
    B, K, pairs = sc["B"], sc["K"], sc["pairs"]
    Rs = [np.tile(np.eye(3)[None], (B, 1, 1)) for _ in range(pairs)]
    Ts = [f64(sc["T0"][:, i]) for i in range(pairs)]
    Wv = np.zeros((B, K, 1))
    first = dbg = None
    for li, (lv, n_it) in enumerate(zip(sc["levels"], iters)):
        lv64 = {k: (f64(v) if isinstance(v, np.ndarray) else v) for k, v in lv.items()}
        one = dict(lv64, tgt=lv64["tgt"][:, 0])
        a = odense.level_inputs(f64(sc["intr"]), one, True, np.float64)
        conv2s = [orc.target_map(lv64["tgt"][:, i]) for i in range(pairs)]
        term = None
        if pi is not None:
            o, w = pi["obs"][li]
            G, g = pref.fit_sums(a["D"][:, :, 0], a["Bs"], f64(o).reshape(B, -1), f64(w).reshape(B, -1))
            term = pref.terms(float(np.float32(scales[li])), f64(pi["Lambda"]), f64(pi["eta"]), G, g)
        for _ in range(n_it):
            Rs, Ts, Wv, dbg = pref.window_iteration(a, conv2s, Rs, Ts, Wv, sc["mlps"][li], L2, term)
            first = first or dbg
    return dict(R=np.stack(Rs, 1), T=np.stack(Ts, 1), W=Wv[:, :, 0], delta=dbg["solution"], first=first)


def check_against_twin(name, st, want, sc):
    B, pairs = sc["B"], sc["pairs"]
    n = lambda x: x.detach().cpu().numpy().astype(np.float64)
    errs = dict(delta=relerr(n(st.delta), want["delta"]), R=relerr(n(st.R).reshape(B, pairs, 3, 3), want["R"]),
                T=relerr(n(st.T).reshape(B, pairs, 3, 1), want["T"]), Wc=relerr(n(st.Wc).reshape(B, -1), want["W"]))
    print("%s: " % name + "  ".join("%s %.2e" % kv for kv in errs.items()))
    return errs


PARITY = {  # name: (B, H, W, K, scales, pairs, iters, channels, random basis)
    "one iteration 24x32": (3, 24, 32, 16, [1], 1, [1], C, False),
    "one iteration 13x19 two frames": (1, 13, 19, 16, [1], 2, [1], C, False),
    "one iteration K200": (1, 24, 32, 200, [1], 1, [1], C, True),
    "one iteration C128": (1, 13, 19, 16, [1], 1, [1], 128, False),
    "schedule": (3, 24, 32, 16, [4, 2, 1], 1, [2, 2, 2], C, False),
    "schedule two frames": (3, 24, 32, 16, [4, 2, 1], 2, [2, 2, 2], C, False),
}


@pytest.mark.parametrize("name", list(PARITY))
def test_solves_with_a_prior_against_the_float64_twin(name):
    B, H, W, K, scales, pairs, iters, channels, rb = PARITY[name]
    sc = scene(name, B, H, W, K, scales, pairs, 31, channels, rb)
    ba = dense_ba(sc)
    # control: the same scene without a prior
    control = twin_solve(sc, iters)
    st, _ = ba.solve(iters, start(ba, sc))
    torch.cuda.synchronize()
    e0 = check_against_twin(name + ", control", st, control, sc)
    # the prior: as strong as the data -- its scale from the control twin's first normal matrix
    pi = prior_inputs(sc, 7)
    m = 6 * pairs
    lv0 = sc["levels"][0]
    G0, _ = pref.fit_sums(lv0["D0"].reshape(B, -1), lv0["basis"].reshape(B, -1, K), pi["obs"][0][0].reshape(B, -1), pi["obs"][0][1].reshape(B, -1))
    data = np.mean([np.diag(control["first"]["AtA"][b, m:, m:]).mean() for b in range(B)])
    own = np.mean([np.diag(G0[b] + pi["Lambda"][b]).mean() for b in range(B)])
    scales_l = [float(np.float32(data / own))] * len(iters)
    want = twin_solve(sc, iters, pi, scales_l)
    assert relerr(want["W"], control["W"]) > 1e-3, "the prior does not move the solution"
    st, _ = ba.solve(iters, start(ba, sc), prior=dense_prior(pi, scales_l))
    torch.cuda.synchronize()
    e1 = check_against_twin(name + ", prior (scale %.3g)" % scales_l[0], st, want, sc)
    assert max(e0.values()) < 1e-4, ("control", e0)
    assert max(e1.values()) < 1e-4, ("prior", e1)


def test_a_strong_prior_decides_the_coefficients():
    """Lambda = s I, eta = s W*, s = 1e6 x the largest depth-block diagonal: each damped coefficient steps by (W* - Wc) / (1 + lambda),
    the last (undamped) one by W* - Wc"""
    from banet_amd import dense as bdense, ops
    sc = scene("one iteration 24x32", *PARITY["one iteration 24x32"][:6], 31)
    B, K = sc["B"], sc["K"]
    ba = dense_ba(sc)
    st = start(ba, sc)
    AtA = ops.ba_assemble(ba.problems[0], st.R, st.T, st.Wc)[0]
    s = 1e6 * torch.diagonal(AtA[:, 6:, 6:], dim1=1, dim2=2).max(dim=1).values
    Wstar = t32(np.random.RandomState(2).standard_normal((B, K)) * 0.05)
    prior = bdense.DensePrior(coef=(s[:, None, None] * torch.eye(K, device=DEV)[None].repeat(B, 1, 1), s[:, None] * Wstar))
    ba.solve([1], st, prior=prior)
    torch.cuda.synchronize()
    lam = st.lambda_out.double().cpu().numpy()
    step = st.delta[:, 6:].double().cpu().numpy()           # Wc started at 0
    want = Wstar.double().cpu().numpy() / (1.0 + lam[:, None])
    want[:, -1] = Wstar.double().cpu().numpy()[:, -1]
    print("strong prior: lambda %s, damped %.2e, undamped %.2e" % (lam, relerr(step[:, :-1], want[:, :-1]), relerr(step[:, -1], want[:, -1])))
    assert relerr(step[:, :-1], want[:, :-1]) < 1e-3 and relerr(step[:, -1], want[:, -1]) < 1e-3
    assert wsc.bits_equal(st.Wc.reshape(B, K), st.delta[:, 6:].contiguous())


# ======================================================================================================================
# the empty prior, and bit equalities
# ======================================================================================================================
def schedule_case(batch_invariant=True, windows=None):
    sc = scene("schedule", *PARITY["schedule"][:6], 31)
    return sc, dense_ba(sc, windows, batch_invariant)


def level_calls(ba, sc, iters, priors, windows=None):
    from banet_amd import ops
    st = start(ba, sc, windows)
    for prob, mlp, its, pr in zip(ba.problems, ba.mlps, iters, priors):
        ops.lm_level(prob, mlp, ba.l2_base, its, False, st, ws=ba.ws, prior=pr)
    return st


def test_the_empty_prior_is_the_existing_entry_bit_for_bit():
    from banet_amd import _capi as capi, ops
    sc, ba = schedule_case()
    iters = [2, 2, 2]
    pi = prior_inputs(sc, 7)
    plain = level_calls(ba, sc, iters, [None] * 3)
    L = capi.lib()
    for what, make in (("no pointers", lambda l: ops.Prior()),
                       ("scale 0", lambda l: ops.Prior(t32(pi["Lambda"]), t32(pi["eta"]), t32(pi["obs"][l][0]), t32(pi["obs"][l][1]), scale=0.0))):
        priors = [make(l) for l in range(3)]
        assert state_bits_equal(level_calls(ba, sc, iters, priors), plain), what
        st = start(ba, sc)
        ops.lm_solve(ba.problems, ba.mlps, ba.l2_base, iters, False, st, priors=priors)
        assert state_bits_equal(st, plain), what
        # the call's workspace need is banet_lm_level_workspace_bytes exactly, whatever the query of a scale-0 prior says
        prob = ba.problems[2]
        nb = L.banet_lm_level_workspace_bytes(ctypes.byref(prob.c))
        assert L.banet_lm_level_prior_workspace_bytes(ctypes.byref(prob.c), None) == nb
        if what == "no pointers":
            assert L.banet_lm_level_prior_workspace_bytes(ctypes.byref(prob.c), ctypes.byref(priors[2].c)) == nb
        ws, handle = wsc.guarded_workspace(nb, DEV, "nan")
        st = start(ba, sc)
        capi.check(L.banet_lm_level_prior_f32(ctypes.byref(prob.c), ctypes.byref(ba.mlps[2].c), L2, 1, None, ctypes.byref(priors[2].c),
                                              ctypes.byref(st.c), ctypes.c_void_p(ws.data_ptr()), nb, capi.stream()))
        wsc.assert_guards_intact(handle)
        ref = start(ba, sc)
        ops.lm_level(prob, ba.mlps[2], L2, 1, False, ref, ws=ba.ws)
        assert state_bits_equal(st, ref), what
        # banet_prior_apply_f32 launches nothing
        s = synthetic(32, 1, 5)
        A, b = s["AtA"].clone(), s["Atb"].clone()
        lvl = BareLevel(s["depth"], s["basis"], 1)
        for pr in (None, ops.Prior(), ops.Prior(s["Lambda"], s["eta"], s["obs"], s["weight"], scale=0.0)):
            ops.prior_apply(lvl, pr, s["Wc"], A, b)
        torch.cuda.synchronize()
        assert wsc.bits_equal(A, s["AtA"]) and wsc.bits_equal(b, s["Atb"])
    st = start(ba, sc)
    ops.lm_solve(ba.problems, ba.mlps, ba.l2_base, iters, False, st)
    assert state_bits_equal(st, plain)


def test_a_zero_prior_with_scale_one_changes_nothing():
    sc, ba = schedule_case()
    from banet_amd import dense as bdense
    B, K = sc["B"], sc["K"]
    plain, _ = ba.solve([2, 2, 2], start(ba, sc))
    zero = bdense.DensePrior(coef=(torch.zeros(B, K, K, device=DEV), torch.zeros(B, K, device=DEV)))
    st, _ = ba.solve([2, 2, 2], start(ba, sc), prior=zero)
    torch.cuda.synchronize()
    for n in STATE:
        assert torch.equal(getattr(st, n), getattr(plain, n)), n


def some_level_priors(pi, scales, windows=None):
    """level 0 none, level 1 coefficients, level 2 observations and coefficients"""
    from banet_amd import ops
    sel = (lambda x: t32(x)) if windows is None else (lambda x: t32(x[list(windows)]))
    return [None, ops.Prior(sel(pi["Lambda"]), sel(pi["eta"]), scale=scales[1]),
            ops.Prior(sel(pi["Lambda"]), sel(pi["eta"]), sel(pi["obs"][2][0]).reshape(-1, 24 * 32), sel(pi["obs"][2][1]).reshape(-1, 24 * 32),
                      scale=scales[2])]


def test_schedule_entry_equals_the_level_calls_and_is_reproducible():
    from banet_amd import _capi as capi, ops
    sc, ba = schedule_case(batch_invariant=True)
    iters, scales = [2, 2, 2], [1.0, 40.0, 25.0]
    pi = prior_inputs(sc, 7, strength=30.0)
    priors = some_level_priors(pi, scales)
    per_level = level_calls(ba, sc, iters, priors)
    plain = level_calls(ba, sc, iters, [None] * 3)
    assert not wsc.bits_equal(per_level.Wc, plain.Wc)
    runs = []
    for _ in range(2):
        st = start(ba, sc)
        trace = ops.SolveTrace(3, st)
        ops.lm_solve(ba.problems, ba.mlps, ba.l2_base, iters, False, st, priors=priors, trace=trace)
        runs.append((st, trace))
    torch.cuda.synchronize()
    assert state_bits_equal(runs[0][0], per_level) and state_bits_equal(runs[1][0], per_level)
    assert wsc.bits_equal(runs[0][1].Wc, runs[1][1].Wc) and wsc.bits_equal(runs[0][1].Wc[2], per_level.Wc)
    # a window alone and in the batch of 3, BANET_POLICY_BATCH_INVARIANT
    for b in (1,):
        ba1 = dense_ba(sc, [b], batch_invariant=True)
        st1 = start(ba1, sc, [b])
        ops.lm_solve(ba1.problems, ba1.mlps, ba1.l2_base, iters, False, st1, priors=some_level_priors(pi, scales, [b]))
        for n in STATE:
            assert wsc.bits_equal(getattr(st1, n)[0], getattr(per_level, n)[b]), (n, b)
    # a bad prior on the LAST level: nothing is enqueued, the state keeps its bits
    bad = ops.Prior(eta=t32(pi["eta"]), scale=1.0)          # eta without Lambda
    st = start(ba, sc)
    for n in STATE:
        getattr(st, n).fill_(3)
    before = [getattr(st, n).clone() for n in STATE]
    s, keep = ops._schedule(ba.problems, ba.mlps, ba.l2_base, iters, False, None, None)
    pr = (capi.Prior * 3)()
    pr[1], pr[2] = priors[1].c, bad.c
    ws = capi.workspace(64 << 20, DEV)
    s.workspace, s.workspace_bytes = ws.data_ptr(), ws.numel()
    assert capi.lib().banet_lm_solve_prior_f32(ctypes.byref(s), pr, ctypes.byref(st.c), capi.stream()) == pref.ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert all(wsc.bits_equal(getattr(st, n), x) for n, x in zip(STATE, before))
    with pytest.raises(capi.BanetError):
        ops.lm_solve(ba.problems, ba.mlps, ba.l2_base, iters, False, st, priors=[None, priors[1], bad])


def test_dense_ba_solve_with_a_prior_one_call_and_per_level():
    sc, ba = schedule_case(batch_invariant=False)
    pi = prior_inputs(sc, 7, strength=30.0)
    prior = dense_prior(pi, [1.0, 4.0, 16.0])
    snaps = []
    one, counts = ba.solve([2, 2, 2], start(ba, sc), prior=prior, snapshots=snaps)
    ba.c_schedule = False
    per, counts2 = ba.solve([2, 2, 2], start(ba, sc), prior=prior)
    torch.cuda.synchronize()
    assert state_bits_equal(one, per) and len(snaps) == 3 and wsc.bits_equal(snaps[2]["W"], one.Wc)
    assert [int(c[0]) for c in counts] == [int(c[0]) for c in counts2] == [2, 2, 2]
    plain, _ = ba.solve([2, 2, 2], start(ba, sc))
    assert not wsc.bits_equal(plain.Wc, one.Wc)


def test_workspace_contents_are_arbitrary_and_its_bounds_hold():
    from banet_amd import ops
    sc = scene("schedule", *PARITY["schedule"][:6], 31)
    other = scene("one iteration 13x19 two frames", *PARITY["one iteration 13x19 two frames"][:6], 31)
    pi = prior_inputs(sc, 7, strength=30.0)
    s = synthetic(130, 2, 9)
    arena = wsc.Arena(96 << 20, DEV)

    def run():
        ba = dense_ba(sc)                                   # (owns a workspace: built inside)
        st, _ = ba.solve([2, 2, 2], start(ba, sc), prior=dense_prior(pi, [1.0, 4.0, 16.0]))
        A, b = s["AtA"].clone(), s["Atb"].clone()
        ops.prior_apply(BareLevel(s["depth"], s["basis"], 2), ops.Prior(s["Lambda"], s["eta"], s["obs"], s["weight"], 0.37), s["Wc"], A, b)
        return tuple(getattr(st, n) for n in STATE) + (A, b)

    def primer():                                           # another shape's leftovers in the same bytes
        ba = dense_ba(other)
        ba.solve([2], start(ba, other), prior=dense_prior(prior_inputs(other, 3), [2.0]))

    outs, seen = wsc.run_under_every_fill(run, arena, primer=primer)
    assert all(len(h) >= 2 for h in seen.values())
    wsc.assert_same_bits_across_fills(outs, names=list(STATE) + ["AtA", "Atb"])


# ======================================================================================================================
# marginals -> transfer -> prior -> solve
# ======================================================================================================================
def test_transfer_prior_closes_the_loop():
    from banet_amd import dense as bdense
    sc = scene("one iteration 24x32", *PARITY["one iteration 24x32"][:6], 31)
    nxt = scene("next window", 3, 24, 32, 16, [1], 1, 57)
    B, K = sc["B"], sc["K"]
    ba, ba2 = dense_ba(sc), dense_ba(nxt)
    st, _ = ba.solve([3], start(ba, sc))
    nd, nb = ba2.levels[0].depth, ba2.levels[0].basis
    var = t32(np.random.RandomState(3).uniform(0.5, 2.0, (B, 24, 32)) * 1e-4)
    want = ba.transfer_depth(0, st, nd, nb, frame=0, depth_var=var)
    got, prior = ba.transfer_prior(0, st, nd, nb, frame=0, depth_var=var)
    for n in bdense.DepthTransfer._fields:
        assert wsc.bits_equal(getattr(got, n), getattr(want, n)), n
    assert prior.level_scale == [1.0] and prior.coef[0].shape == (B, K, K) and prior.coef[1].shape == (B, K)
    ends = []
    for pr in (prior, None):
        s2 = ba2.new_state(T=t32(nxt["T0"][:, 0]), Wc=got.Wc.reshape(B, K, 1))
        ba2.solve([3], s2, prior=pr)
        ends.append((s2.Wc.reshape(B, K) - got.Wc).double().norm(dim=1).cpu().numpy())
    print("transfer_prior: |Wc - transfer.Wc| with the prior %s, without %s" % (ends[0], ends[1]))
    assert (ends[0] < ends[1]).all()
