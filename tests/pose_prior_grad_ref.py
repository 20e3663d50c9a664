"""The float64 twin of the pose prior's backward (include/banet_hip.h (5g); csrc/pose_prior_grad.hip).  Plain module, no fixtures:
shared by test_pose_prior_grad_cpu.py and test_gpu_pose_prior_grad.py.

With G = gAtA'[0:m, 0:m] (raw) and g = gAtb'[0:m] the gradients of the post-prior matrices of one window, and r, Jr, Lambda,
s = scale the forward's quantities (pose_prior_ref.py):

    y = Jr g     X = Lambda Jr     Xt = Lambda^T Jr     u = Lambda r
    gLambda = s (Jr G Jr^T - y r^T)        gscale = <G, Jr^T Lambda Jr> - <g, Jr^T Lambda r>        gr = -s Lambda^T y
    gJr_i   = s (X G^T + Xt G)[block i] - s u_i g_i^T
    (gR_i, gT_i, gR0_i, gT0_i) = (d(r_i, Jr_i) / d(R_i, T_i, R0_i, T0_i))^T (gr_i, gJr_i)

The last line is torch autograd over `pose_chain`, a transcription of pose_prior_ref.log_se3 / jr_block: the same branches at the
same thresholds, with theta^2 and s^2 used where a sqrt at zero would give NaN tangents (below THETA_LOG theta^2 = atan(x)^2 is a
series in x^2 = s^2 / c^2; |phi|^2 = phi . phi feeds the series of Q's coefficients directly).  R and R0 are nine free entries
each.  mode="twin" is float64 with pose_prior_ref's thresholds; mode="kernel" is the same formulas in float32 as the kernel's
tangent evaluates them (the coefficients by their series over the whole range, the kernel's orders), which
test_pose_prior_grad_cpu.py uses to size the GPU test's gate."""
import math
from fractions import Fraction

import numpy as np
import torch

import pose_prior_ref as ppr

OUTPUTS = ("gR", "gT", "gR0", "gT0", "gLambda", "gscale")
OVERWRITE_STATE, OVERWRITE_PRIOR = 1, 2


def _bernoulli(n_max):
    B = [Fraction(0)] * (n_max + 1)
    B[0] = Fraction(1)
    for m in range(1, n_max + 1):
        B[m] = -sum(Fraction(math.comb(m + 1, k)) * B[k] for k in range(m)) / (m + 1)
    return B


_B = _bernoulli(36)
# c = sum_n |B_2n| / (2n)! t2^(n-1);  a1 = sum (-1)^n t2^n / (2n+3)!;  a2 = sum (-1)^n t2^n / (2n+4)!;  a3 = sum (-1)^n (n+1) t2^n / (2n+5)!
SERIES = dict(c=[float(abs(_B[2 * n]) / math.factorial(2 * n)) for n in range(1, 19)],
              a1=[(-1.0) ** n / math.factorial(2 * n + 3) for n in range(13)],
              a2=[(-1.0) ** n / math.factorial(2 * n + 4) for n in range(13)],
              a3=[(-1.0) ** n * (n + 1) / math.factorial(2 * n + 5) for n in range(13)])
KERNEL_TERMS = dict(c=18, a1=13, a2=13, a3=13)     # csrc/pose_prior_common.hpp: kPoseGradC / A1 / A2 / A3
TWIN_TERMS = 7                                     # below pose_prior_ref's float64 threshold 0.1: the next term is 1e-16 of c'


def _horner(coefs, t2):
    p = torch.full_like(t2, coefs[-1])
    for k in reversed(coefs[:-1]):
        p = p * t2 + k
    return p


def coefficients(t2, mode):
    """c, a1, a2, a3 as functions of t2 = theta^2 (a torch scalar)"""
    if mode == "kernel":
        return tuple(_horner(SERIES[n][:KERNEL_TERMS[n]], t2) for n in ("c", "a1", "a2", "a3"))
    if float(t2.detach()) < ppr.THETA_SERIES[np.float64] ** 2:
        return tuple(_horner(SERIES[n][:TWIN_TERMS], t2) for n in ("c", "a1", "a2", "a3"))
    t = torch.sqrt(t2)
    s, co = torch.sin(t), torch.cos(t)
    h = 0.5 * t
    c = 1.0 / t2 - torch.cos(h) / (2.0 * t * torch.sin(h))
    a1 = (t - s) / (t2 * t)
    a2 = (t2 + 2.0 * co - 2.0) / (2.0 * t2 * t2)
    a3 = (2.0 * t - 3.0 * s + t * co) / (2.0 * t2 * t2 * t)
    return c, a1, a2, a3


def _hat(v):
    o = torch.zeros((), dtype=v.dtype)
    return torch.stack([torch.stack([o, -v[2], v[1]]), torch.stack([v[2], o, -v[0]]), torch.stack([-v[1], v[0], o])])


def pose_chain(x, mode="twin"):
    """x [24] = (R 9, T 3, R0 9, T0 3) of one pose -> (r [6], Jr [6,6]), differentiable"""
    R, T, R0, T0 = x[0:9].reshape(3, 3), x[9:12], x[12:21].reshape(3, 3), x[21:24]
    Re = R @ R0.T
    te = T - Re @ T0
    w = 0.5 * torch.stack([Re[2, 1] - Re[1, 2], Re[0, 2] - Re[2, 0], Re[1, 0] - Re[0, 1]])
    s2 = (w * w).sum()
    c = 0.5 * (Re[0, 0] + Re[1, 1] + Re[2, 2] - 1.0)
    theta_now = math.atan2(math.sqrt(float(s2.detach())), float(c.detach()))
    if theta_now < ppr.THETA_LOG:      # k is a function of theta alone here, and theta^2 = atan(x)^2 a series in x^2 = s^2 / c^2 < 1e-6
        z = s2 / (c * c)
        th2 = z * (1.0 - z * (1.0 / 3 - z * (1.0 / 5 - z * (1.0 / 7)))) ** 2
        k = 1.0 + th2 * (1.0 / 6 + th2 * (7.0 / 360))
    else:
        s = torch.sqrt(s2)
        theta = torch.atan2(s, c)
        th2 = theta * theta
        k = theta / torch.clamp(s, min=1e-6)
    phi = k * w
    cc = coefficients(th2, mode)[0]
    F = _hat(phi)
    eye = torch.eye(3, dtype=x.dtype)
    Ji = eye - 0.5 * F + cc * (F @ F)
    rho = Ji @ te
    _, a1, a2, a3 = coefficients((phi * phi).sum(), mode)
    Pm = _hat(rho)
    FP, PF = F @ Pm, Pm @ F
    FPF = FP @ F
    Q = 0.5 * Pm + a1 * (FP + PF + FPF) + a2 * (F @ FP + PF @ F - 3.0 * FPF) + a3 * (FPF @ F + F @ FPF)
    Jr = torch.cat([torch.cat([Ji, torch.zeros(3, 3, dtype=x.dtype)], 1), torch.cat([-(Ji @ Q @ Ji), Ji], 1)], 0)
    return torch.cat([phi, rho]), Jr


def _pack(R, T, R0, T0, i, dt):
    return torch.tensor(np.concatenate([np.asarray(R)[i].reshape(9), np.asarray(T)[i].reshape(3), np.asarray(R0)[i].reshape(9),
                                        np.asarray(T0)[i].reshape(3)]).astype(np.float64), dtype=dt)


def window_grad(R, T, R0, T0, Lambda, scale, G, g, mode="twin", with_bounds=True):
    """one window: R, R0 [pairs,3,3], T, T0 [pairs,3], Lambda, G [m,m], g [m] -> dict of the six outputs (numpy float64; mode
    "kernel": computed in float32) and, with_bounds (always from the float64 chain), "bound_<name>": the sum of the absolute values
    of each entry's terms"""
    dt = torch.float64 if mode == "twin" else torch.float32
    pairs = np.asarray(R).reshape(-1, 3, 3).shape[0]
    m = 6 * pairs
    tt = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=dt)                       # noqa: E731
    L, Gt, gt, s = tt(Lambda).reshape(m, m), tt(G).reshape(m, m), tt(g).reshape(m), float(scale)
    xs = [_pack(R, T, R0, T0, i, dt).requires_grad_(True) for i in range(pairs)]
    rs, Js = zip(*[pose_chain(x, mode) for x in xs])
    r, Jr = torch.cat(rs).detach(), torch.block_diag(*Js).detach()
    if mode == "kernel":               # the kernel recomputes r and Jr with the forward's own float32 function: pose_prior_ref's
        fw = ppr.window_term(np.asarray(R, np.float32), np.asarray(T, np.float32), np.asarray(R0, np.float32), np.asarray(T0, np.float32),
                             np.asarray(Lambda, np.float32), np.float32(scale), np.float32)
        r, Jr = torch.tensor(fw["r"]), torch.tensor(fw["Jr"])
    y, X, Xt, u = Jr @ gt, L @ Jr, L.T @ Jr, L @ r
    A = Jr @ Gt
    gL = s * (A @ Jr.T - torch.outer(y, r))
    gscale = (A.double() * X.double()).sum() - (y.double() * u.double()).sum()
    gr = -s * (L.T @ y)
    gJ = s * (X @ Gt.T + Xt @ Gt) - s * torch.outer(u, gt)
    out = dict(gLambda=gL.double().numpy(), gscale=float(gscale))
    gx = []
    for i in range(pairs):
        blk = slice(6 * i, 6 * i + 6)
        f = (gr[blk] * rs[i]).sum() + (gJ[blk, blk] * Js[i]).sum()
        gx.append(torch.autograd.grad(f, xs[i])[0].double().numpy())
    gx = np.stack(gx)
    out.update(gR=gx[:, 0:9].reshape(pairs, 3, 3), gT=gx[:, 9:12], gR0=gx[:, 12:21].reshape(pairs, 3, 3), gT0=gx[:, 21:24])
    if with_bounds:
        d = torch.float64
        L, Gt, gt = (np.abs(np.asarray(a, np.float64)) for a in (np.asarray(Lambda).reshape(m, m), np.asarray(G).reshape(m, m),
                                                                     np.asarray(g).reshape(m)))
        x64 = [_pack(R, T, R0, T0, i, d) for i in range(pairs)]
        r64, J64 = zip(*[pose_chain(x) for x in x64])
        ar, aJ = np.abs(torch.cat(r64).numpy()), np.abs(torch.block_diag(*J64).numpy())
        bX = L @ aJ
        out["bound_gLambda"] = s * (aJ @ Gt @ aJ.T + np.outer(aJ @ gt, ar))
        out["bound_gscale"] = float((Gt * (aJ.T @ L @ aJ)).sum() + (gt * (aJ.T @ (L @ ar))).sum())
        bgr = s * (L.T @ (aJ @ gt))
        bgJ = s * (bX @ Gt.T + (L.T @ aJ) @ Gt + np.outer(L @ ar, gt))
        bx = []
        for i in range(pairs):
            blk = slice(6 * i, 6 * i + 6)
            jac = torch.autograd.functional.jacobian(lambda v: torch.cat([pose_chain(v)[0], pose_chain(v)[1].reshape(36)]), x64[i])
            bx.append(np.abs(jac.numpy()).T @ np.concatenate([bgr[blk], bgJ[blk, blk].reshape(36)]))
        bx = np.stack(bx)
        out.update(bound_gR=bx[:, 0:9].reshape(pairs, 3, 3), bound_gT=bx[:, 9:12], bound_gR0=bx[:, 12:21].reshape(pairs, 3, 3),
                   bound_gT0=bx[:, 21:24])
    return out


def batch_grad(c, gAtA, gAtb, scale=ppr.APPLY_SCALE, mode="twin", with_bounds=True):
    """the B windows of a problem c (pose_prior_ref.apply_problem: float32 R, T, R0, T0, Lambda) with gAtA [B,P,P], gAtb [B,P] (only
    the pose block is read) -> dict of stacked arrays as window_grad's"""
    f = lambda x: np.asarray(x, np.float32).astype(np.float64)                              # noqa: E731
    B, pairs = c["R"].shape[0], c["R"].shape[1]
    m = 6 * pairs
    per = [window_grad(f(c["R"][b]), f(c["T"][b]), f(c["R0"][b]), f(c["T0"][b]), f(c["Lambda"][b]), scale, f(gAtA[b])[:m, :m], f(gAtb[b])[:m],
                       mode, with_bounds) for b in range(B)]
    return {k: np.stack([np.asarray(p[k]) for p in per]) for k in per[0]}


def functional(R, T, R0, T0, Lambda, scale, G, g):
    """<G, H> - <g, v> of pose_prior_ref.window_term: what the six outputs are the gradient of"""
    t = ppr.window_term(R, T, R0, T0, Lambda, scale)
    return float((G * t["H"]).sum() - (g * t["v"]).sum())


# ======================================================================================================================
# the cases of banet_pose_prior_add_grad_f32 (test_gpu_pose_prior_grad.py), and how far float32 arithmetic is from the twin on them
# ======================================================================================================================
def grad_problem(pairs, K, B=3):
    """-> pose_prior_ref.apply_problem(pairs, K) plus gAtA [B,P,P] and gAtb [B,P], float32, seeded, standard normal; gAtA is NOT
    symmetric"""
    c = ppr.apply_problem(pairs, K, B)
    rng = np.random.RandomState(7000 + 100 * pairs + K)
    P = 6 * pairs + K
    c["gAtA"] = np.ascontiguousarray(rng.standard_normal((B, P, P)).astype(np.float32))
    c["gAtb"] = np.ascontiguousarray(rng.standard_normal((B, P)).astype(np.float32))
    return c


def grad_errors(got, ref, prev=None):
    """entrywise error of got[name] against ref[name], relative to ref["bound_" + name] (+ |prev[name]| in accumulate mode, where
    ref + prev is the expected value) -> {name: largest}"""
    out = {}
    for name in OUTPUTS:
        if got.get(name) is None:
            continue
        want, bound = np.asarray(ref[name], np.float64), np.asarray(ref["bound_" + name], np.float64)
        if prev is not None and prev.get(name) is not None:
            p = np.asarray(prev[name], np.float64).reshape(want.shape)
            want, bound = want + p, bound + np.abs(p)
        out[name] = float((np.abs(np.asarray(got[name], np.float64).reshape(want.shape) - want) / bound).max())
    return out


# max over pose_prior_ref.APPLY_SHAPES and the six outputs of |float32 evaluation of this module's formulas (mode="kernel") - float64
# twin|, entrywise, relative to the bounds above: measured by test_pose_prior_grad_cpu.py::
# test_float32_arithmetic_is_this_far_from_the_twin (gLambda 2.198e-6 at pairs 7, K 130; gR0 1.2e-7, gT 1.0e-7, gR 8.4e-8, gT0 7.1e-8,
# gscale 2.8e-8; profiles/pose_prior_grad.txt), rounded up in its third digit.  gLambda leads because its bound, the sum of its terms'
# absolute values, can be as small as one entry of G, while the forward's float32 phi carries the absolute rounding of Re = R R0^T
# (3e-8 whatever |phi| is: 3e-6 of phi at |phi| = 0.01) into the small entries of Jr next to entries of G of order 1 -- the forward's
# own bits, not a derivative coefficient.
# The GPU gate is 4 x this: device sincos / atan2 differ from the host's by ulps and the kernel sums in another order (forward mode
# per input entry, where torch runs the reverse pass).
F32_GRAD_ERR = 2.20e-6
GRAD_GATE = 4 * F32_GRAD_ERR
