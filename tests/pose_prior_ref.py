"""The float64 twin of the pose prior (include/banet_hip.h (5f); csrc/pose_prior.hip).  Plain module, no fixtures: shared by
test_pose_prior_cpu.py and test_gpu_pose_prior.py.

The update convention is the oracle's _se3_update: delta = [w; t], R' = exp(w) R, T' = V(w) t + exp(w) T, i.e. T' = Exp(delta) o T
with Exp([phi; rho]) = (exp(phi), V(phi) rho) -- a left perturbation.  Per window, with prior poses (R0_i, T0_i) and a joint
information matrix Lambda [m, m], m = 6 pairs:

    E_i = T_i o T0_i^-1:  Re = R_i R0_i^T, te = T_i - Re T0_i        r_i = Log(E_i) = [phi; rho],  rho = V(phi)^-1 te
    Jr  = blockdiag_i  J_l(r_i)^-1,   J_l^-1 = [[J^-1, 0], [-J^-1 Q J^-1, J^-1]],   J = V(phi),   Q = Barfoot's Q(rho, phi)
    cost = scale 1/2 r^T Lambda r      AtA[0:m, 0:m] += scale Jr^T Lambda Jr      Atb[0:m] -= scale Jr^T Lambda r

Every function takes the dtype it computes in: np.float64 is the twin, np.float32 the same formulas as the kernel evaluates them
(thresholds of csrc/pose_prior.hip), which test_pose_prior_cpu.py uses to size the GPU test's gate."""
import numpy as np

from oracle import banet_oracle as orc

OK, ERR_INVALID_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED, ERR_LAUNCH = 0, -1, -2, -3, -4

THETA_LOG = 1e-3                                   # below: theta / sin(theta) by its series (0 / 0 at theta = 0)
THETA_SERIES = {np.float64: 0.1, np.float32: 0.5}  # below: the coefficients of J^-1 and Q by their series (cancellation)
ANGLES = (0.0, 1e-7, 1e-4, 1e-2, 0.5, 2.5, 3.0)    # |phi| of the issue's cases
THRESHOLD_ANGLES = tuple(t * f for t in (THETA_LOG, 0.1, 0.5) for f in (0.999, 1.001))   # both sides of every series threshold


def hat(v):
    x, y, z = v
    o = v.dtype.type(0)
    return np.array([[o, -z, y], [z, o, -x], [-y, x, o]], v.dtype)


def exp_se3(delta):
    """delta [6] = [w; t] -> (exp(w) [3,3], V(w) t [3]) by the oracle's own functions; float64"""
    d = np.asarray(delta, np.float64)
    th = np.linalg.norm(d[:3])
    if th < 1e-5:                                   # (the oracle's V divides by theta, its exp clamps theta at 1e-6)
        W = hat(d[:3])
        return np.eye(3) + W + 0.5 * W @ W, (np.eye(3) + 0.5 * W + W @ W / 6.0) @ d[3:]
    R = orc.angle_axis_rotation(d[None, :3], clamp_theta=True)[0]
    return R, orc.vmatrix(d[None, :3])[0] @ d[3:]


def compose(delta, R, T):
    """Exp(delta) o (R, T), float64"""
    dR, dt = exp_se3(delta)
    return dR @ R, dt + dR @ np.asarray(T, np.float64).reshape(3)


def coefficients(theta, dt):
    """-> c, a1, a2, a3:  J^-1 = I - 1/2 F + c F^2;  Q = 1/2 P + a1 (FP + PF + FPF) + a2 (FFP + PFF - 3 FPF) + a3 (FPFF + FFPF)"""
    t = dt(theta)
    t2 = t * t
    if t < dt(THETA_SERIES[dt]):
        c = dt(1 / 12) + t2 * (dt(1 / 720) + t2 * (dt(1 / 30240) + t2 * dt(1 / 1209600)))
        a1 = dt(1 / 6) - t2 * (dt(1 / 120) - t2 * (dt(1 / 5040) - t2 * dt(1 / 362880)))
        a2 = dt(1 / 24) - t2 * (dt(1 / 720) - t2 * (dt(1 / 40320) - t2 * dt(1 / 3628800)))
        a3 = dt(1 / 120) - t2 * (dt(1 / 2520) - t2 * (dt(1 / 120960) - t2 * dt(1 / 9979200)))
        return c, a1, a2, a3
    s, co = np.sin(t), np.cos(t)
    h = t * dt(0.5)
    c = dt(1) / t2 - np.cos(h) / (dt(2) * t * np.sin(h))          # (1 + cos) / sin = cot(theta / 2): finite at pi
    a1 = (t - s) / (t2 * t)
    a2 = (t2 + dt(2) * co - dt(2)) / (dt(2) * t2 * t2)
    a3 = (dt(2) * t - dt(3) * s + t * co) / (dt(2) * t2 * t2 * t)
    return c, a1, a2, a3


def log_se3(R, T, R0, T0, dt=np.float64):
    """-> r [6] = Log((R, T) o (R0, T0)^-1) = [phi; rho], and J^-1 = V(phi)^-1 [3,3]"""
    R, R0 = np.asarray(R, dt).reshape(3, 3), np.asarray(R0, dt).reshape(3, 3)
    T, T0 = np.asarray(T, dt).reshape(3), np.asarray(T0, dt).reshape(3)
    Re = R @ R0.T
    te = T - Re @ T0
    w = dt(0.5) * np.array([Re[2, 1] - Re[1, 2], Re[0, 2] - Re[2, 0], Re[1, 0] - Re[0, 1]], dt)
    s = np.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    c = dt(0.5) * (Re[0, 0] + Re[1, 1] + Re[2, 2] - dt(1))
    theta = np.arctan2(s, c)
    if theta < dt(THETA_LOG):
        t2 = theta * theta
        k = dt(1) + t2 * (dt(1 / 6) + t2 * dt(7 / 360))
    else:
        k = theta / np.maximum(s, dt(1e-6))         # (past the supported range, near pi: finite)
    phi = (k * w).astype(dt)
    F = hat(phi)
    cc = coefficients(theta, dt)[0]
    Jinv = np.eye(3, dtype=dt) - dt(0.5) * F + cc * (F @ F)
    rho = Jinv @ te
    return np.concatenate([phi, rho]).astype(dt), Jinv.astype(dt)


def jr_block(r, Jinv, dt=np.float64):
    """-> J_l(r)^-1 [6,6] in [phi; rho] ordering"""
    r = np.asarray(r, dt)
    phi, rho = r[:3], r[3:]
    theta = np.sqrt(phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2])
    _, a1, a2, a3 = coefficients(theta, dt)
    F, P = hat(phi), hat(rho)
    FP, PF = F @ P, P @ F
    FPF = FP @ F
    Q = dt(0.5) * P + a1 * (FP + PF + FPF) + a2 * (F @ FP + PF @ F - dt(3) * FPF) + a3 * (FPF @ F + F @ FPF)
    J = np.zeros((6, 6), dt)
    J[:3, :3] = Jinv
    J[3:, 3:] = Jinv
    J[3:, :3] = -(Jinv @ Q.astype(dt) @ Jinv)
    return J


def window_term(R, T, R0, T0, Lambda, scale, dt=np.float64):
    """one window: R, R0 [pairs,3,3], T, T0 [pairs,3], Lambda [m,m] -> dict(H = scale Jr^T Lambda Jr [m,m], v = scale Jr^T Lambda r [m],
    r [m], Jr [m,m], cost)"""
    pairs = np.asarray(R).reshape(-1, 3, 3).shape[0]
    m = 6 * pairs
    R, R0 = np.asarray(R).reshape(pairs, 3, 3), np.asarray(R0).reshape(pairs, 3, 3)
    T, T0 = np.asarray(T).reshape(pairs, 3), np.asarray(T0).reshape(pairs, 3)
    L = np.asarray(Lambda, dt).reshape(m, m)
    r, Jr = np.zeros(m, dt), np.zeros((m, m), dt)
    for i in range(pairs):
        ri, Jinv = log_se3(R[i], T[i], R0[i], T0[i], dt)
        r[6 * i:6 * i + 6] = ri
        Jr[6 * i:6 * i + 6, 6 * i:6 * i + 6] = jr_block(ri, Jinv, dt)
    sc = dt(scale)
    H = sc * (Jr.T @ (L @ Jr))
    v = sc * (Jr.T @ (L @ r))
    return dict(H=H.astype(dt), v=v.astype(dt), r=r, Jr=Jr, cost=sc * dt(0.5) * (r @ (L @ r)))


def apply(AtA, Atb, R, T, R0, T0, Lambda, scale, dt=np.float64):
    """the term on AtA [B,P,P], Atb [B,P] (or [B,P,1]); R, R0 [B,pairs,3,3]; T, T0 [B,pairs,3]; Lambda [B,m,m]; scale a number or
    one per window -> new arrays (dtype dt) and the per-window bound matrices scale |Jr|^T |Lambda| |Jr|, scale |Jr|^T |Lambda| |r|"""
    A, b = np.array(AtA, dt), np.array(Atb, dt)
    B = A.shape[0]
    sc = np.broadcast_to(np.asarray(scale, np.float64), (B,))
    bound_A, bound_b = [], []
    for w in range(B):
        t = window_term(np.asarray(R)[w], np.asarray(T)[w], np.asarray(R0)[w], np.asarray(T0)[w], np.asarray(Lambda)[w], sc[w], dt)
        m = t["H"].shape[0]
        A[w, :m, :m] += t["H"]
        b[w, :m] -= t["v"].reshape(b[w, :m].shape)
        aJ, aL = np.abs(t["Jr"]).astype(np.float64), np.abs(np.asarray(Lambda, np.float64)[w].reshape(m, m))
        bound_A.append(sc[w] * (aJ.T @ aL @ aJ))
        bound_b.append(sc[w] * (aJ.T @ aL @ np.abs(t["r"]).astype(np.float64)))
    return A, b, np.stack(bound_A), np.stack(bound_b)


def log_norm(R, T, R0, T0):
    """|Log(T o T0^-1)| per window and pair -> [B,pairs], float64"""
    R, R0 = np.asarray(R, np.float64), np.asarray(R0, np.float64)
    B, pairs = R.shape[0], R.shape[1]
    T, T0 = np.asarray(T, np.float64).reshape(B, pairs, 3), np.asarray(T0, np.float64).reshape(B, pairs, 3)
    return np.array([[np.linalg.norm(log_se3(R[b, i], T[b, i], R0[b, i], T0[b, i])[0]) for i in range(pairs)] for b in range(B)])


def random_rotation(rng, angle):
    a = rng.standard_normal(3)
    a /= np.linalg.norm(a)
    return exp_se3(np.concatenate([a * angle, np.zeros(3)]))[0]


def apply_cases(pairs, seed, B=3, angles=ANGLES + THRESHOLD_ANGLES):
    """B windows x pairs poses whose relative rotation angles cycle through `angles` (seeded) -> dict of float32 arrays R, T, R0, T0
    (the poses as float32 rotation matrices, what the kernel is given) and Lambda [B,m,m] symmetric positive definite"""
    rng = np.random.RandomState(seed)
    m = 6 * pairs
    R, T, R0, T0 = (np.zeros((B, pairs) + s) for s in ((3, 3), (3,), (3, 3), (3,)))
    for b in range(B):
        for i in range(pairs):
            ang = angles[(seed + b * pairs + i) % len(angles)]
            R0[b, i] = random_rotation(rng, rng.uniform(0, 1.0))
            R[b, i] = random_rotation(rng, ang) @ R0[b, i]
            T0[b, i] = rng.standard_normal(3) * 0.3
            T[b, i] = T0[b, i] + rng.standard_normal(3) * 0.2
    M = rng.standard_normal((B, m, m))
    Lambda = np.einsum("bik,bjk->bij", M, M) / m + np.eye(m)
    f = lambda x: np.ascontiguousarray(x.astype(np.float32))
    return dict(R=f(R), T=f(T), R0=f(R0), T0=f(T0), Lambda=f(0.5 * (Lambda + Lambda.transpose(0, 2, 1))))


# ======================================================================================================================
# one iteration of a level with the term: the oracle's iteration, the term before its damping, the oracle's solve and update
# ======================================================================================================================
def window_iteration(a, conv2s, Rs, Ts, W, mlp, l2_base, pose=None, coef=None):
    """`bundle` levels.  a: oracle.dense.level_inputs(..., np.float64); conv2s: the target maps per frame; Rs / Ts: lists per frame
    ([B,3,3], [B,3,1]); W [B,K,1]; pose: (R0 [B,pairs,3,3], T0 [B,pairs,3], Lambda [B,m,m], scale) or None; coef: (Le, ee) of
    prior_ref.terms or None -> Rs, Ts, W, dict(solution [B,P], lam [B], AtA, Atb)"""
    import prior_ref as pref
    pairs = len(conv2s)
    _, _, _, dbg = orc.bundle_window_iteration(a["conv1"], conv2s, a["fx"], a["fy"], a["ox"], a["oy"], a["p"], a["D"], a["Bs"], Rs, Ts, W,
                                               mlp, l2_base)
    AtA0, Atb, lam = dbg["AtA"], dbg["Atb"], dbg["lam"]
    if coef is not None:
        AtA0, Atb = pref.apply(AtA0, Atb, W, coef[0], coef[1], pairs)
    if pose is not None:
        R = np.stack(Rs, 1)
        T = np.stack([t[:, :, 0] for t in Ts], 1)
        AtA0, Atb, _, _ = apply(AtA0, Atb, R, T, pose[0], pose[1], pose[2], pose[3])
    sol = orc.solve_lu(orc.damp(AtA0, lam, undamped_last=True), Atb)
    Rn, Tn = [], []
    for i in range(pairs):
        r, t = orc._se3_update(sol[:, 6 * i:6 * i + 6], Rs[i], Ts[i])
        Rn.append(r)
        Tn.append(t)
    return Rn, Tn, W + sol[:, 6 * pairs:], dict(solution=sol[:, :, 0], lam=lam.reshape(-1), AtA=AtA0, Atb=Atb)


def camera_iteration(a, conv2, R, T, mlp, pose=None):
    """the pose-only `bundle_camera` level (one target frame, every coefficient damped) -> R, T, dict(solution [B,6], lam, AtA, Atb)"""
    _, _, dbg = orc.bundle_camera_iteration(a["conv1"], conv2, a["fx"], a["fy"], a["ox"], a["oy"], a["p"], a["D"], R, T, mlp)
    AtA0, Atb, lam = dbg["AtA"], dbg["Atb"], dbg["lam"]
    if pose is not None:
        AtA0, Atb, _, _ = apply(AtA0, Atb, R[:, None], T[:, None, :, 0], pose[0], pose[1], pose[2], pose[3])
    sol = orc.solve_lu(orc.damp(AtA0, lam, undamped_last=False), Atb)
    Rn, Tn = orc._se3_update(sol, R, T)
    return Rn, Tn, dict(solution=sol[:, :, 0], lam=lam.reshape(-1), AtA=AtA0, Atb=Atb)


# ======================================================================================================================
# the cases of banet_pose_prior_apply_f32 (test_gpu_pose_prior.py), and how far float32 arithmetic is from the twin on them
# ======================================================================================================================
APPLY_SHAPES = [(pairs, K) for pairs in (1, 2, 7) for K in (0, 5, 130)]
APPLY_SCALE = 0.37
# max over APPLY_SHAPES of |float32 numpy evaluation of this module's formulas - float64 twin|, entrywise, relative to
# |AtA_ij| + scale (|Jr|^T |Lambda| |Jr|)_ij (AtA) and |Atb_i| + scale (|Jr|^T |Lambda| |r|)_i (Atb): measured by
# test_pose_prior_cpu.py::test_float32_arithmetic_is_this_far_from_the_twin (AtA 4.717e-7 at pairs 7, K 0; Atb 1.599e-7 at pairs 7,
# K 130; profiles/pose_prior.txt), the larger of the two rounded up in its third digit.
# The GPU gate is 4 x this, 1.888e-6: device sincos / atan2 differ from numpy's by ulps and the kernel sums in another order.
F32_ERR = 4.72e-7
APPLY_GATE = 4 * F32_ERR


def apply_problem(pairs, K, B=3):
    """-> apply_cases(...) plus float32 AtA [B,P,P] (symmetric positive definite), Atb [B,P] and the angles of its poses"""
    seed = 100 * pairs + K
    c = apply_cases(pairs, seed, B)
    rng = np.random.RandomState(seed + 1)
    P = 6 * pairs + K
    Q = rng.standard_normal((B, P, P))
    c["AtA"] = np.ascontiguousarray((np.einsum("bik,bjk->bij", Q, Q) / P + np.eye(P)).astype(np.float32))
    c["Atb"] = np.ascontiguousarray(rng.standard_normal((B, P)).astype(np.float32))
    angles = ANGLES + THRESHOLD_ANGLES
    c["angles"] = [angles[(seed + i) % len(angles)] for i in range(B * pairs)]
    return c


def apply_errors(got_A, got_b, c, scale=APPLY_SCALE):
    """entrywise error of (got_A, got_b) against the float64 twin on the problem c, relative to the issue's bound -> (AtA, Atb)"""
    f = lambda x: np.asarray(x, np.float32).astype(np.float64)
    A, b, bA, bb = apply(f(c["AtA"]), f(c["Atb"]), f(c["R"]), f(c["T"]), f(c["R0"]), f(c["T0"]), f(c["Lambda"]), scale)
    m = bA.shape[1]
    eA = np.abs(np.asarray(got_A, np.float64)[:, :m, :m] - A[:, :m, :m]) / (np.abs(f(c["AtA"]))[:, :m, :m] + bA)
    eb = np.abs(np.asarray(got_b, np.float64)[:, :m] - b[:, :m]) / (np.abs(f(c["Atb"]))[:, :m] + bb)
    return float(eA.max()), float(eb.max())
