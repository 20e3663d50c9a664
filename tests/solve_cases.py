"""Inputs and the float64 reference for the tests of the forward solve-and-update kernel (csrc/solve.hip:
ba_solve_update_kernel<BIG> behind banet_ba_solve_update[_ws]_f32, and banet_spd_solve_f32): one table of cases shared by the
CPU module (test_solve_cases_cpu.py: the conditions on the inputs, the float32 yardstick, the support limits) and the GPU module
(test_gpu_solve_update.py).  No GPU: numpy, torch on the CPU, the oracle, and small_step_cases.make_case for the inputs.

The kernel reads only the scalar fields of the level, so a case is synthetic normal equations: AtA [B,P,P], Atb [B,P], the
channel sums of |residual| [B,C], nvalid [B], the five lambda layers and a starting state R, T, Wc -- float32 numbers held in
float64, so that the float32 kernel, the float32 yardstick and the float64 reference start from the same inputs.

A SPEC is (family, variant, C, P, pairs, rung); P may be ("lds", C, off): the largest P whose matrix still lives in LDS at that
channel count, plus off (found by a scan of banet_ba_solve_update_workspace_bytes on the host, never a literal).  Families:
  a  `ladder`     small_step_cases' conditioning ladder (bundle) at the P where the kernel changes path or tile
  b  `camera`     bundle_camera windows, K = 0, every coefficient damped: the LU up to 5 target frames, PCG with n1 = P above
  c  `legacy`     LEGACY_LM / LEGACY_FIXED, P = 6, the one-thread QR; their own lambda (legacy/ba.py:187-190, 266-275)
  d  `pivot`      P <= 31 with the coefficients on scales decades apart: the LU's row order is not the identity
  e  `clustered`  depth columns around one common direction with a spread of noise levels and next to no damping: the damped
                  block is ill conditioned with a spread-out spectrum, so PCG cannot converge in 40 products -> LDL^T fallback
  f  `planted`    right-hand sides A x* for chosen updates x*: rotation parts of norm 1e-7 (below the theta clamp), 1e-3, 1, 3.1
"""
import ctypes
import functools

import numpy as np
import torch

import small_step_cases as ssc
from oracle import banet_oracle as orc

VARIANT_ID = {"legacy_lm": 0, "legacy_fixed": 1, "bundle_camera": 2, "bundle": 3}   # banet_hip.h: BANET_LEGACY_LM .. BANET_BUNDLE
B_WINDOWS = 3
SEEDS = ssc.SEEDS
P_MAX = 304                     # the largest system of the project's shapes (8 target frames, K = 256)
PCG_MAX_PRODUCTS, PCG_TOL2 = 40, 2.5e-14      # solve.hip: kPcgMaxIt, kPcgTol2
PLANTED_NORMS = (1e-7, 1e-3, 1.0, 3.1)
E_REF32_CAP = 1e-2              # a case is gated by 4 e_ref32 only while e_ref32 stays below this


# ---- what the library accepts (host-side queries: no GPU) ----------------------------------------------------------------------
def bare_level(variant, B, N, C, K, pairs, flags=0):
    """a banet_level_t with the scalar fields the solve reads and NULL maps"""
    from banet_amd import _capi as capi
    lv = capi.Level()
    lv.B, lv.N, lv.C, lv.K, lv.pairs = int(B), int(N), int(C), int(K), int(pairs)
    lv.variant, lv.flags = VARIANT_ID[variant], int(flags)
    return lv


def solve_workspace_bytes(B, C, P, pairs=1):
    from banet_amd import _capi as capi
    lv = bare_level("bundle", B, ssc.N_POINTS, C, P - 6 * pairs, pairs)
    return int(capi.lib().banet_ba_solve_update_workspace_bytes(ctypes.byref(lv)))


@functools.lru_cache(maxsize=None)
def p_lds(C):
    """the largest P (bundle, one target frame) for which banet_ba_solve_update_workspace_bytes returns 0"""
    P = 7
    assert solve_workspace_bytes(B_WINDOWS, C, P) == 0
    while solve_workspace_bytes(B_WINDOWS, C, P + 1) == 0:
        P += 1
        assert P < 4096, "no LDS limit found"
    return P


def lds(C, off=0):
    return ("lds", C, off)


# ---- the tables ---------------------------------------------------------------------------------------------------------------
def _bundle(family, P, rungs, pairs=1, C=32):
    return [(family, "bundle", C, P, pairs, r) for r in rungs]


ALL_RUNGS = (0, 1, 2, 3, 4, 5)
LADDER_SHAPES = (
    [(P, 1, 32) for P in (7, 19, 30, 31)] +                                   # the LU side of the switch
    [(P, 1, 32) for P in (32, 33, 47, 48, 49, 63, 64, 65)] +                  # the 16-column panel edges
    [(P, 1, 32) for P in (37, 38, 39, 40)] +                                  # n1 = P - 1 = 0, 1, 2, 3 mod 4
    [(134, 1, 32), (6 * 4 + 128, 4, 32)] +                                    # K = 128
    [(lds(32), 1, 32), (lds(32, 1), 1, 32), (lds(128), 1, 128), (lds(128, 1), 1, 128)] +   # the LDS / BIG switch
    [(208, 1, 32), (262, 1, 32), (298, 7, 32), (304, 8, 32)])                 # BIG
LADDER = [s for P, pairs, C in LADDER_SHAPES for s in _bundle("ladder", P, ALL_RUNGS, pairs, C)]
CAMERA = [("camera", "bundle_camera", 32, 6 * pairs, pairs, r) for pairs in (1, 2, 3, 4, 5, 6, 7, 8) for r in (0, 1)]
LEGACY = [("legacy", v, C, 6, 1, 1) for v in ("legacy_lm", "legacy_fixed") for C in (3, 8, 128)]
# (bundle: rungs 1 and 2 -- at rung 0 the damping, lambda ~ 1e2 .. 1e3, keeps every diagonal entry the largest of its column)
PIVOT = ([s for P, pairs in ((7, 1), (19, 1), (25, 2), (31, 1), (31, 4)) for s in _bundle("pivot", P, (1, 2), pairs)] +
         [("pivot", "bundle_camera", 32, 6 * pairs, pairs, 1) for pairs in (1, 2, 3, 5)])
CLUSTERED = [("clustered", "bundle", 32, P, 1, 1) for P in (38, 70, 134, lds(32))]
PLANTED = ([("planted", "bundle_camera", 32, 6 * pairs, pairs, 1) for pairs in (1, 4, 8)] +
           [("planted", "bundle", 32, 6 * pairs + 32, pairs, 1) for pairs in (1, 4, 8)])
FAMILIES = {"ladder": LADDER, "camera": CAMERA, "legacy": LEGACY, "pivot": PIVOT, "clustered": CLUSTERED, "planted": PLANTED}
SOLVE_FAMILIES = ("ladder", "camera", "legacy", "pivot", "clustered")        # a .. e: gated against float64 on the GPU
SPD_P = (32, 33, 47, 48, 49, 63, 64, 65, 134)                                # banet_spd_solve_f32, plus the largest P it accepts


def resolve(spec):
    family, variant, C, P, pairs, rung = spec
    if isinstance(P, tuple):
        P = p_lds(P[1]) + P[2]
    return family, variant, C, P, pairs, rung


def spec_id(spec):
    family, variant, C, P, pairs, rung = spec
    p = "P%d" % P if not isinstance(P, tuple) else "Plds%d%s" % (P[1], "+%d" % P[2] if P[2] else "")
    return "%s-%s-C%d-%s-pairs%d-rung%d" % (family, variant, C, p, pairs, rung)


def all_specs(families=tuple(FAMILIES)):
    return [s for f in families for s in FAMILIES[f]]


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def _r32(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def _rng(spec, seed, salt):
    family, variant, C, P, pairs, rung = resolve(spec)
    return np.random.RandomState((seed + 31 * (salt + 17 * (P + 311 * (pairs + 13 * (rung + 7 * C))))) % (2 ** 31))


def cluster_levels(K):
    """family e: the noise level of each clustered depth column, log-spaced over a decade -- one common dl gives the damped
    block TWO eigenvalue clusters (K and dl^2 + lambda), which CG resolves in a handful of products however small dl is"""
    return np.logspace(np.log10(0.4), np.log10(0.04), K - 1)


CLUSTER_L2_BASE = 1e-5


@functools.lru_cache(maxsize=16)
def make(spec, seed, B=B_WINDOWS):
    """-> the case: a dict of numpy float64 arrays with float32 values (AtA, Atb, absres, nvalid, R [B,pairs,3,3],
    T [B,pairs,3,1], Wc [B,K,1], layers) and the scalars of the level"""
    family, variant, C, P, pairs, rung = resolve(spec)
    K = P - 6 * pairs
    base = ssc.make_case("bundle" if K > 0 else "bundle_camera", B, C, K, pairs, rung, seed)
    n = lambda t: t.numpy().copy()
    N = base["N"]
    case = dict(spec=spec, family=family, variant=variant, B=B, N=N, C=C, K=K, pairs=pairs, P=P, rung=rung, seed=seed,
                l2_base=base["l2_base"], AtA=n(base["AtA"]), Atb=n(base["Atb"]), absres=n(base["absres"]), R=n(base["R"]),
                T=n(base["T"]), Wc=n(base["Wc"]), layers=[(n(w), n(b)) for w, b in base["layers"]])
    # in-image rows per window: below N pairs, another count in every window
    case["nvalid"] = np.floor(N * pairs * (0.95 - 0.1 * np.arange(B) / B)).astype(np.float64)
    if family == "pivot":
        # the columns of J on scales 10^U(-2, 2) in shuffled order: AtA -> S AtA S, Atb -> S Atb.  One draw per stratum of the
        # exponent range and the two ends pinned (so that six coefficients span the four decades as surely as thirty); the
        # smallest scale on the first coefficient, the largest on the last, the next two of either end beside them: step 0
        # then takes its pivot from the last rows, and the last steps cannot find theirs on the diagonal
        rs = _rng(spec, seed, 1)
        S = np.empty((B, P))
        for b in range(B):
            e = -2.0 + 4.0 * (np.arange(P) + rs.uniform(0.0, 1.0, P)) / P
            e[0], e[-1] = -2.0, 2.0
            s = 10.0 ** e
            S[b] = np.concatenate([s[:1], rs.permutation(s[1:3]), rs.permutation(s[3:P - 3]), rs.permutation(s[P - 3:P - 1]), s[P - 1:]])
        S = _r32(S)
        case["AtA"] = _r32(case["AtA"] * S[:, :, None] * S[:, None, :])
        case["AtA"] = _r32(0.5 * (case["AtA"] + case["AtA"].transpose(0, 2, 1)))
        case["Atb"] = _r32(case["Atb"] * S)
        case["scales"] = S
    if family == "clustered":
        rs = _rng(spec, seed, 2)
        J = rs.standard_normal((B, N, P))
        u = rs.standard_normal((B, N, 1))
        J[:, :, 6 * pairs:P - 1] = u + cluster_levels(K)[None, None, :] * J[:, :, 6 * pairs:P - 1]
        A = _r32(np.matmul(J.transpose(0, 2, 1), J))
        case["AtA"] = _r32(0.5 * (A + A.transpose(0, 2, 1)))
        case["l2_base"] = CLUSTER_L2_BASE
    if family == "planted":
        rs = _rng(spec, seed, 3)
        x = np.zeros((B, P))
        for b in range(B):
            for p in range(pairs):
                w = rs.standard_normal(3)
                x[b, 6 * p:6 * p + 3] = w / np.linalg.norm(w) * PLANTED_NORMS[(b * pairs + p + seed) % 4]
                x[b, 6 * p + 3:6 * p + 6] = rs.standard_normal(3) * 0.1 * (1 + p)
        x[:, 6 * pairs:] = rs.standard_normal((B, K)) * 0.05
        case["planted"] = x
        A = damped64(case, lambda64(case))
        case["Atb"] = _r32(np.matmul(A, x[:, :, None])[:, :, 0])
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


# ---- the float64 reference ----------------------------------------------------------------------------------------------------
def is_legacy(case):
    return case["variant"] in ("legacy_lm", "legacy_fixed")


def lambda64(case):
    """lambda [B] in float64.  bundle / bundle_camera: bundlenet.py:165-173, 241-253 (small_step_cases.lambda_of);
    LEGACY_LM: legacy/ba.py:266-275, the channel means scaled by N / nvalid, ||avg||^(1 + y);
    LEGACY_FIXED: legacy/ba.py:187-190, ||avg||^2 and no MLP"""
    v, Nf = case["variant"], float(case["N"] * case["pairs"])
    if not is_legacy(case):
        layers = [(torch.tensor(w), torch.tensor(b)) for w, b in case["layers"]]
        return ssc.lambda_of(torch.tensor(case["absres"]), layers, case["N"], case["pairs"], case["l2_base"],
                             v == "bundle_camera").numpy()
    avg = case["absres"] / Nf
    if v == "legacy_fixed":
        return np.sqrt(np.sum(avg * avg, axis=-1)) ** 2.0
    avg = (Nf / case["nvalid"])[:, None] * avg
    y = orc.lambda_mlp(avg[:, None, :], case["layers"])[:, 0, 0]
    return np.sqrt(np.sum(avg * avg, axis=-1)) ** (1.0 + y)


def damped64(case, lam):
    return orc.damp(case["AtA"], np.asarray(lam, np.float64).reshape(-1, 1, 1), undamped_last=case["variant"] == "bundle")


def solve64(case, lam):
    """delta [B,P]: the float64 solution of the damped system at the given lambda"""
    return np.linalg.solve(damped64(case, lam), case["Atb"][:, :, None])[:, :, 0]


def update64(case, delta, R=None, T=None, Wc=None):
    """the state after the update, in float64: R' = exp(w) R, T' = V(w) t + exp(w) T (LEGACY_FIXED: t + exp(w) T),
    Wc' = Wc + delta[6 pairs:] -- bundlenet.py:185-190, 269-276; legacy/ba.py:208-213, 295-302.  Pose slot b pairs + p."""
    B, pairs, K = case["B"], case["pairs"], case["K"]
    R = (case["R"] if R is None else R).reshape(B * pairs, 3, 3).astype(np.float64)
    T = (case["T"] if T is None else T).reshape(B * pairs, 3, 1).astype(np.float64)
    Wc = (case["Wc"] if Wc is None else Wc).reshape(B, K, 1).astype(np.float64)
    sol = np.asarray(delta, np.float64)[:, :6 * pairs].reshape(B * pairs, 6, 1)
    w, t = sol[:, 0:3, 0], sol[:, 3:6]
    dr = orc.angle_axis_rotation(w, clamp_theta=not is_legacy(case))
    Tn = (t if case["variant"] == "legacy_fixed" else np.matmul(orc.vmatrix(w), t)) + np.matmul(dr, T)
    Rn = np.matmul(dr, R)
    Wn = Wc + np.asarray(delta, np.float64)[:, 6 * pairs:, None]
    return Rn.reshape(B, pairs, 3, 3), Tn.reshape(B, pairs, 3, 1), Wn


def ratio64(case):
    """banet_state_t.ratio as documented: nvalid / (N pairs) for LEGACY_FIXED (legacy/ba.py:214), (N pairs) / nvalid otherwise"""
    Nf = float(case["N"] * case["pairs"])
    return case["nvalid"] / Nf if case["variant"] == "legacy_fixed" else Nf / case["nvalid"]


# ---- errors and the float32 yardstick -----------------------------------------------------------------------------------------
def groups(case):
    """the coefficient groups of delta: pose, and for the bundle variant the damped depth coefficients and the undamped last one"""
    o, P = 6 * case["pairs"], case["P"]
    g = {"pose": slice(0, o)}
    if case["variant"] == "bundle":
        if P - 1 > o:
            g["depth"] = slice(o, P - 1)
        g["last"] = slice(P - 1, P)
    return g


def group_errors(case, got, want):
    """per group: max |got - want| over the batch on the group's own max-norm scale"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return {k: float(np.abs(got[:, sl] - want[:, sl]).max()) / max(float(np.abs(want[:, sl]).max()), 1e-300)
            for k, sl in groups(case).items()}


def lu32(A, b):
    """A^-1 b [B,n,1] by a textbook LU with partial pivoting in float32 arithmetic: right-looking elimination with row swaps
    (the first of the maxima as the pivot), then the two triangular solves -- the algorithm of tf.matrix_solve (Eigen's
    PartialPivLU) and of LAPACK's sgetf2 / sgetrs, every operation rounded to float32.
    Written out because the libraries at hand do not provide it: numpy.linalg.solve (orc.solve_lu) computes in DOUBLE whatever
    the input type and rounds the result, which measures the rounding of the matrix alone (4e-8 on x where float32 elimination
    gives 7e-4); and the float32 solve of the BLAS behind torch is, on the badly scaled systems of the pivot family, up to 500
    times more accurate than this textbook elimination (1.9e-6 against 5.4e-3 on pivot P = 19 rung 2).  That is the outlier, not
    this routine: reference LAPACK's float32 sgesv (through scipy.linalg, where it is installed) sits with lu32 -- 2.6e-3 on the
    same case, ~4e-2 on the ladder's rung 5 -- and so does the kernel, which restates the same elimination."""
    f = np.float32
    M = np.concatenate([np.asarray(A), np.asarray(b)], axis=2).astype(f)            # [B, n, n + 1]
    B, n = M.shape[0], M.shape[1]
    rows = np.arange(B)
    for k in range(n - 1):
        p = k + np.argmax(np.abs(M[:, k:, k]), axis=1)
        tmp = M[rows, p].copy()
        M[rows, p] = M[:, k]
        M[:, k] = tmp
        l = M[:, k + 1:, k] / M[:, k, k][:, None]
        M[:, k + 1:, k + 1:] -= l[:, :, None] * M[:, k, k + 1:][:, None, :]
    x = np.zeros((B, n), f)
    for k in range(n - 1, -1, -1):
        x[:, k] = (M[:, k, n] - np.sum(M[:, k, k + 1:n] * x[:, k + 1:], axis=1, dtype=f)) / M[:, k, k]
    assert M.dtype == f and x.dtype == f
    return x[:, :, None]


def qr32(A, b):
    """legacy/ba.py:292-293 in float32: Householder QR (sgeqrf), then the triangular solve of R x = Q^T b"""
    A, b = torch.tensor(np.asarray(A), dtype=torch.float32), torch.tensor(np.asarray(b), dtype=torch.float32)
    q, r = torch.linalg.qr(A, mode="complete")
    return torch.linalg.solve_triangular(r, torch.matmul(q.transpose(-1, -2), b), upper=True).numpy()


def solve32(case, lam):
    """the yardstick: ONE float32 solve of the float32 damped matrix by the reference's algorithm -- LU with partial pivoting
    (tf.matrix_solve), Householder QR for the legacy variants (tf.qr + triangular solve)"""
    lam32 = np.asarray(lam).astype(np.float32)
    A32 = orc.damp(case["AtA"].astype(np.float32), lam32.reshape(-1, 1, 1), undamped_last=case["variant"] == "bundle")
    b32 = case["Atb"].astype(np.float32)[:, :, None]
    assert A32.dtype == np.float32
    x = qr32(A32, b32) if is_legacy(case) else lu32(A32, b32)
    assert x.dtype == np.float32
    return x[:, :, 0]


def backward_error(A, x, b):
    """normwise backward error of x as a solution of A x = b, the worst of the batch: ||A x - b|| / (||A|| ||x|| + ||b||) in the
    max-norms, evaluated in float64.  What elimination keeps small (~n 2^-24 in float32) whatever the condition number, and what
    still tells a right solver from a wrong one where the forward error no longer does"""
    A, x, b = np.asarray(A, np.float64), np.asarray(x, np.float64).reshape(A.shape[0], -1), np.asarray(b, np.float64).reshape(A.shape[0], -1)
    r = np.abs(np.matmul(A, x[:, :, None])[:, :, 0] - b).max(axis=1)
    return float((r / (np.abs(A).sum(axis=2).max(axis=1) * np.abs(x).max(axis=1) + np.abs(b).max(axis=1))).max())


def forward_gated(spec):
    """False for the ladder's rung 5: its float32 yardstick lies above 1e-2 (cond ~5e5 .. 5e6), where 4 e_ref32 would accept
    anything -- those cases are held to the backward error instead (residual_gate)"""
    return not (spec[0] == "ladder" and spec[5] == 5)


def residual_gate(n, rho_ref32):
    """largest backward error accepted of a float32 solver on an n x n system: the project's margin of 4 on the float32 LU's own
    backward error, and never less than the first-order bound of elimination, n 2^-24"""
    return max(n * 2.0 ** -24, 4.0 * rho_ref32)


def max_merge(acc, e):
    for k, v in e.items():
        acc[k] = max(acc.get(k, 0.0), v)
    return acc


def yardstick(spec):
    """e_ref32 per group: the error of solve32 against solve64, both at lambda = float32(lambda64), the maximum over the seeds"""
    return _yardsticks(spec)[0]


def yardstick_backward(spec):
    """rho_ref32: the backward error (backward_error) of solve32 on the float64 damped system, the maximum over the seeds"""
    return _yardsticks(spec)[1]


@functools.lru_cache(maxsize=None)
def _yardsticks(spec):
    e, rho = {}, 0.0
    for seed in SEEDS:
        case = make(spec, seed)
        lam = lambda64(case).astype(np.float32).astype(np.float64)
        x32 = solve32(case, lam)
        max_merge(e, group_errors(case, x32, solve64(case, lam)))
        rho = max(rho, backward_error(damped64(case, lam), x32, case["Atb"]))
    return e, rho


# ---- emulations of the kernel's decisions -------------------------------------------------------------------------------------
def lu_row_order(A):
    """row order of a plain LU with partial pivoting: the first maximal entry of the column (the smallest row index among
    ties), as lu_solve_regs picks it; rows pivoted logically, order[k] = the physical row eliminated at step k"""
    A = np.array(A, np.float64)
    n = A.shape[0]
    used, order = np.zeros(n, bool), []
    for k in range(n):
        col = np.where(used, -1.0, np.abs(A[:, k]))
        p = int(np.argmax(col))                      # (argmax: the first of the maxima)
        order.append(p)
        used[p] = True
        f = np.where(used, 0.0, A[:, k] / A[p, k])
        A -= f[:, None] * A[p][None, :]
    return order


def pcg_emulation(A, b, undamped_last):
    """Jacobi-preconditioned CG as pcg_schur_solve runs it, in float64: on the damped block (all but the last coefficient of
    the bundle variant) for the right-hand side and, bundle, for the coupling column a12; the recursively updated residual,
    stop at |r|^2 <= 2.5e-14 |b|^2 on both, at most 40 products.  -> (products until both stopped, or 41; the largest
    |r|^2 / |b|^2 over the two at the end)"""
    n = A.shape[0]
    n1 = n - 1 if undamped_last else n
    M = A[:n1, :n1]
    dinv = 1.0 / np.diag(M)
    products, worst = 0, 0.0
    for rhs in ([b[:n1], A[:n1, n - 1]] if undamped_last else [b[:n1]]):
        r = rhs.copy()
        bb = float(r @ r)
        z = dinv * r
        p, rz, it, rr = z.copy(), float(r @ z), 0, bb
        while bb > 0.0 and rr > PCG_TOL2 * bb and it < PCG_MAX_PRODUCTS:
            Ap = M @ p
            al = rz / float(p @ Ap)
            r = r - al * Ap
            z = dinv * r
            rz, rz_old = float(r @ z), rz
            rr = float(r @ r)
            p = z + (rz / rz_old) * p
            it += 1
        converged = bb == 0.0 or rr <= PCG_TOL2 * bb
        products = max(products, it if converged else PCG_MAX_PRODUCTS + 1)
        worst = max(worst, rr / bb if bb > 0.0 else 0.0)
    return products, worst
