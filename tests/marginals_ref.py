"""Inputs and references for the tests of banet_ba_marginals_f32 (csrc/marginals.hip): synthetic symmetric positive definite
normal matrices whose conditioning the test chooses, the definition in float64 and the same route in float32 LAPACK (the
yardstick).  One table shared by test_marginals_cpu.py (the conditions on the inputs, the references against np.linalg.inv) and
test_gpu_marginals.py.  No GPU, except make("assembled", ...), whose matrix comes from ops.ba_assemble.

Per window: P = 6 pairs + K, H = AtA + mu diag(diag(AtA) + 1e-5) (every diagonal entry), Sigma = sigma2 H^-1, H = L L^T,
T = L_WW^-1 (the trailing K x K block): pose_cov = Sigma[:6 pairs, :6 pairs], depth_var[n] = sigma2 |T basis[n]|^2,
logdet = 2 sum log L_ii.  Only the lower triangle of AtA is read.

The yardstick is as specified: np.linalg.cholesky on the float32 matrix, scipy's solve_triangular (strtrs) and float32 GEMM.  numpy
factorises a float32 matrix in DOUBLE and rounds the factor (its linalg computes in double whatever the input type), so the yardstick
does not carry the cond(H) 2^-24 of a float32 factorisation: 3e-7 .. 1e-6 on the kappa = 1e6 ladder, where a float32 Cholesky gives
2e-3 .. 6e-3.  The kernel factorises in float64 for that reason (csrc/marginals.hip, profiles/marginals.txt).

Families (a case = a dict of numpy arrays: AtA, basis, damping, sigma2 hold float32 VALUES):
  ladder      H0 = D Q diag(s) Q^T D: Q random orthogonal, s log-uniform in [1, kappa] with both ends present, D = exp(U(-2, 2))
              column scales; spec (P, pairs, K, kappa, damped, scaled): damping NULL or 1e-3 per window, sigma2 NULL or U(0.5, 2)
  indefinite  a ladder case whose middle window has its smallest eigenvalue flipped to -0.01 lambda_max
  assembled   AtA from ops.ba_assemble on oracle.synth pair scenes (spec (H, W, C, K)), damping 1e-3, the scene's own basis
"""
import functools

import numpy as np
import scipy.linalg

B_WINDOWS = 3
SEEDS = (0, 1)
N_POINTS = 200                     # ladder / indefinite: pixels of the random basis (not a multiple of the kernel's 32-pixel tile)
P_MAX, K_MAX = 304, 256
KAPPAS = (10.0, 1e2, 1e4, 1e6)
LADDER_SHAPES = ((6, 1, 0), (7, 1, 1), (31, 1, 25), (38, 1, 32), (39, 1, 33), (134, 1, 128), (152, 4, 128), (190, 1, 184),
                 (191, 1, 185), (262, 1, 256), (304, 8, 256))
LADDER = [(P, pairs, K, kappa, damped, scaled) for (P, pairs, K) in LADDER_SHAPES for kappa in KAPPAS
          for damped in (False, True) for scaled in (False, True)]
INDEFINITE = [(38, 1, 32, 1e2, False, True), (134, 1, 128, 1e2, True, True), (262, 1, 256, 1e4, True, False)]
ASSEMBLED = [(24, 32, 32, 32), (48, 64, 128, 128)]
FAMILIES = {"ladder": LADDER, "indefinite": INDEFINITE, "assembled": ASSEMBLED}
OUTPUTS = ("pose_cov", "depth_var", "wfactor", "logdet")


def spec_id(spec):
    if len(spec) == 4:
        return "%dx%d-C%d-K%d" % spec
    P, pairs, K, kappa, damped, scaled = spec
    return "P%d-pairs%d-K%d-kappa%g-%s-%s" % (P, pairs, K, kappa, "damped" if damped else "undamped", "sigma" if scaled else "unit")


def _r32(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def _rng(spec, seed, salt=0):
    P, pairs, K, kappa = spec[:4]
    return np.random.RandomState((seed * 7919 + salt * 104729 + 31 * P + 17 * pairs + 13 * K + int(round(np.log10(kappa))) * 101) % (2 ** 31))


def _ladder_matrix(rs, P, kappa):
    Q, _ = np.linalg.qr(rs.standard_normal((P, P)))
    s = kappa ** rs.uniform(0.0, 1.0, P)
    s[0] = 1.0
    s[-1] = kappa if P > 1 else 1.0
    D = np.exp(rs.uniform(-2.0, 2.0, P))
    H = (Q * s[None, :]) @ Q.T
    H = D[:, None] * (0.5 * (H + H.T)) * D[None, :]
    return H


@functools.lru_cache(maxsize=8)
def make(family, spec, seed, B=B_WINDOWS):
    if family == "assembled":
        return _make_assembled(spec, seed, B)
    P, pairs, K, kappa, damped, scaled = spec
    assert P == 6 * pairs + K
    rs = _rng(spec, seed)
    A = np.stack([_ladder_matrix(rs, P, kappa) for _ in range(B)])
    if family == "indefinite":
        b = B // 2
        w, V = np.linalg.eigh(A[b])
        v = V[:, 0]
        A[b] = A[b] - (w[0] + 0.01 * w[-1]) * np.outer(v, v)          # the smallest eigenvalue becomes -0.01 lambda_max
    A = _r32(A)
    A = np.tril(A) + np.tril(A, -1).transpose(0, 2, 1)                # float32 values, exactly symmetric
    rb = _rng(spec, seed, 1)
    basis = _r32(rb.standard_normal((B, N_POINTS, K)))
    damping = _r32(np.full(B, 1e-3)) if damped else None
    sigma2 = _r32(rb.uniform(0.5, 2.0, B)) if scaled else None
    case = dict(family=family, spec=spec, seed=seed, B=B, N=N_POINTS, K=K, pairs=pairs, P=P, AtA=A, basis=basis, damping=damping,
                sigma2=sigma2, expect_fail=[family == "indefinite" and b == B // 2 for b in range(B)])
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def _make_assembled(spec, seed, B):
    """GPU: the normal matrix of a dense pair scene at a pose near the truth, from ops.ba_assemble"""
    import torch
    from banet_amd import dense as bdense, ops
    from oracle import dense as odense, synth
    H, W, C, K = spec
    scenes = [synth.make_pair_scene(H, W, C, K, [1], 100 * seed + 11 + b, normalize_rays=True, w_gt=[0.01, -0.008, 0.006],
                                    t_gt=[0.06, -0.04, 0.03]) for b in range(B)]
    intr, levels = odense.batch_scene(scenes)
    lv = levels[0]
    dev = torch.device("cuda:0")
    tl = bdense.DenseLevel(lv["scale"], *(torch.from_numpy(lv[k]).to(dev) for k in ("src", "tgt", "D0", "basis")))
    prob = ops.LevelProblem("bundle", tl.src, tl.tgt, tl.depth.reshape(B, H * W), H, W, C, basis=tl.basis.reshape(B, H * W, K),
                            intr=torch.from_numpy(intr).to(dev), scale=tl.scale, dense=True, tgt_has_grad=False, normalize_rays=True)
    R = torch.eye(3, device=dev).repeat(B, 1, 1)
    T = torch.from_numpy(np.stack([np.asarray(s["T_gt"]) * 0.7 for s in scenes]).reshape(B, 3, 1).astype(np.float32)).to(dev)
    Wc = torch.zeros(B, K, 1, device=dev)
    AtA = ops.ba_assemble(prob, R, T, Wc)[0]
    torch.cuda.synchronize()
    A = AtA.cpu().numpy().astype(np.float64)
    A = np.tril(A) + np.tril(A, -1).transpose(0, 2, 1)
    return dict(family="assembled", spec=spec, seed=seed, B=B, N=H * W, K=K, pairs=1, P=6 + K, AtA=A,
                basis=lv["basis"].reshape(B, H * W, K).astype(np.float64), damping=_r32(np.full(B, 1e-3)), sigma2=None,
                expect_fail=[False] * B, problem=prob)


# ---- the definition ---------------------------------------------------------------------------------------------------------------
def damped(case, dtype=np.float64):
    """H [B,P,P] from the lower triangle of AtA, in `dtype` arithmetic"""
    A = case["AtA"].astype(dtype)
    A = np.tril(A) + np.tril(A, -1).transpose(0, 2, 1)
    if case["damping"] is None:
        return A
    mu = case["damping"].astype(dtype)
    d = np.einsum("bii->bi", A)
    H = A.copy()
    idx = np.arange(case["P"])
    H[:, idx, idx] = d + mu[:, None] * (d + dtype(1e-5))
    assert H.dtype == dtype
    return H


def sentinel(case, dtype=np.float64):
    m, K, N = 6 * case["pairs"], case["K"], case["N"]
    return dict(pose_cov=np.diag(np.full(m, np.inf)).astype(dtype), depth_var=np.full(N, np.inf, dtype), wfactor=np.zeros((K, K), dtype),
                logdet=dtype(-np.inf), status=1)


def _window(case, b, dtype):
    """one window by the Cholesky route in `dtype` (LAPACK potrf / trtrs, GEMM); raises LinAlgError where H is not positive definite"""
    m, K = 6 * case["pairs"], case["K"]
    one = dict(case, AtA=case["AtA"][b:b + 1], damping=None if case["damping"] is None else case["damping"][b:b + 1])
    H = damped(one, dtype)[0]
    s2 = dtype(1.0) if case["sigma2"] is None else dtype(case["sigma2"][b])
    L = np.linalg.cholesky(H)
    assert L.dtype == dtype
    if not np.all(np.isfinite(L)) or not np.all(np.diag(L) > 0):
        raise np.linalg.LinAlgError("not positive definite")
    E = np.eye(case["P"], m, dtype=dtype)
    X = scipy.linalg.solve_triangular(L, E, lower=True, check_finite=False)
    cov = s2 * (X.T @ X)
    if K > 0:
        Tm = scipy.linalg.solve_triangular(L[m:, m:], np.eye(K, dtype=dtype), lower=True, check_finite=False)
        Tm = np.tril(Tm)
        y = case["basis"][b].astype(dtype) @ Tm.T
        dv = s2 * np.sum(y * y, axis=1, dtype=dtype)
    else:
        Tm, dv = np.zeros((0, 0), dtype), np.zeros(case["N"], dtype)
    logdet = dtype(2.0) * np.sum(np.log(np.diag(L)), dtype=dtype)
    out = dict(pose_cov=cov, depth_var=dv, wfactor=Tm, logdet=logdet, status=0)
    for k in OUTPUTS:
        assert np.asarray(out[k]).dtype == dtype, k
    return out


def _stack(wins):
    return {k: np.stack([np.asarray(w[k]) for w in wins]) for k in wins[0]}


def marginals64(case):
    """the definition in float64; a window whose factorisation fails gets status 1 and the sentinel outputs"""
    wins = []
    for b in range(case["B"]):
        try:
            wins.append(_window(case, b, np.float64))
        except np.linalg.LinAlgError:
            wins.append(sentinel(case))
    return _stack(wins)


def marginals32_window(case, b):
    """the yardstick for one window: the same route in float32 LAPACK; raises LinAlgError where the float32 factorisation fails"""
    return _window(case, b, np.float32)


def marginals32(case):
    """the yardstick: every window expected to succeed by marginals32_window (LinAlgError propagates), the others the sentinel"""
    return _stack([sentinel(case, np.float32) if case["expect_fail"][b] else marginals32_window(case, b) for b in range(case["B"])])


# ---- errors and gates -------------------------------------------------------------------------------------------------------------
def errors(case, got, want):
    """per output, the largest error over the windows expected to succeed, each on its own scale: depth_var relative to its
    float64 value per pixel; pose_cov[i,j] relative to sqrt(Sigma_ii Sigma_jj); wfactor relative to its largest entry per window;
    logdet absolute over P"""
    e = dict.fromkeys(OUTPUTS, 0.0)
    for b in range(case["B"]):
        if case["expect_fail"][b]:
            continue
        g = {k: np.asarray(got[k][b], np.float64) for k in OUTPUTS if got.get(k) is not None}
        w = {k: np.asarray(want[k][b], np.float64) for k in OUTPUTS}
        d = np.sqrt(np.diag(w["pose_cov"]))
        e["pose_cov"] = max(e["pose_cov"], float((np.abs(g["pose_cov"] - w["pose_cov"]) / np.outer(d, d)).max()))
        e["logdet"] = max(e["logdet"], float(abs(g["logdet"] - w["logdet"])) / case["P"])
        if case["K"] > 0:
            if "depth_var" in g:
                e["depth_var"] = max(e["depth_var"], float((np.abs(g["depth_var"] - w["depth_var"]) / w["depth_var"]).max()))
            if "wfactor" in g:
                e["wfactor"] = max(e["wfactor"], float(np.abs(g["wfactor"] - w["wfactor"]).max() / np.abs(w["wfactor"]).max()))
    return e


def yardstick(case):
    """the float32 LAPACK route's own errors on the case"""
    return errors(case, marginals32(case), marginals64(case))


def gates(case, yard):
    """per output: 4 x the yardstick's error on the same case (the margin the residual backward's tests give a float32 route with
    another summation order), never below P 2^-24, the rounding bound of one length-P float32 dot product"""
    return {k: max(4.0 * yard[k], case["P"] * 2.0 ** -24) for k in OUTPUTS}


def spectrum(case):
    """float64 eigenvalues of H per window -> [B,P] ascending"""
    return np.stack([np.linalg.eigvalsh(h) for h in damped(case)])
