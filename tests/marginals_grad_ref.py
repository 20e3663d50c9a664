"""Upstream gradients and references for the tests of banet_ba_marginals_grad_f32 (csrc/marginals_grad.hip), on the cases of
tests/marginals_ref.py.  No GPU.  Shared by test_marginals_grad_cpu.py and test_gpu_marginals_grad.py.

Per window, with m = 6 pairs, P = m + K, A = AtA as a symmetric matrix, H = A + mu diag(diag A + 1e-5) = L L^T, Y = L^-1,
T = Y[m:, m:], s2 = sigma2 and the upstream gradients g_cov [m,m] (NOT symmetric), g_dv [N] (both signs, some exact zeros), g_ld:

    M    = sum_n g_dv[n] b_n b_n^T                   Gbar = blockdiag(1/2 (g_cov + g_cov^T), M)
    Q    = Y Gbar Y^T                                dH   = Y^T (g_ld I - s2 Q) Y
    gAtA = dH off the diagonal, (1 + mu) dH on it    gdamping = sum_i dH_ii (A_ii + 1e-5)    gsigma2 = trace Q
    gbasis[n] = 2 s2 g_dv[n] T^T (T b_n)

Two independent references: closed_form (the lines above, numpy float64) and autograd_ref (torch CPU float64 autograd through the
DEFINITION: cholesky, solve_triangular, 1/2 (A + A^T)).  The yardstick is closed_form with float32 arrays and np.linalg.cholesky
on the float32 matrix (marginals_ref._window's route).

Errors, each on its own scale (errors()): gAtA per block (pose x pose, pose x depth, depth x depth) relative to that block's largest
reference entry per window; gbasis per pixel relative to that row's largest reference entry (rows with g_dv = 0 must be exactly
0: reported as inf otherwise); gdamping relative to sum_i |dH_ii| (A_ii + 1e-5); gsigma2 relative to sum_i |Q_ii|.
Gates (gates()): max(4 x the yardstick's error on the same case, (P + N) 2^-24) -- the forward's margin; the floor is the rounding
bound of the longest float32 dot product that feeds an entry (P terms through H^-1, N through M)."""
import functools

import numpy as np
import scipy.linalg

import marginals_ref as mr

OUTPUTS = ("gAtA", "gdamping", "gsigma2", "gbasis")
ERRORS = ("gAtA_pp", "gAtA_pd", "gAtA_dd", "gbasis", "gdamping", "gsigma2")
MUTATIONS = ("no_diag_mu", "cov_unsym", "gbasis_no2", "no_logdet", "abs_g", "zero_block")


def upstreams(case):
    """-> dict g_cov [B,m,m], g_dv [B,N], g_ld [B]: float32 VALUES in float64 arrays, drawn from the case's seed"""
    rs = mr._rng(case["spec"], case["seed"], 2)
    B, m, N = case["B"], 6 * case["pairs"], case["N"]
    g_dv = rs.standard_normal((B, N))
    g_dv[:, ::7] = 0.0                                   # rows whose gbasis must be exactly 0
    return dict(g_cov=mr._r32(rs.standard_normal((B, m, m))), g_dv=mr._r32(g_dv), g_ld=mr._r32(rs.standard_normal(B)))


def _window(case, ups, b, dtype, mutate=None):
    """the closed form for one window in `dtype`; raises LinAlgError where H is not positive definite"""
    m, K, P = 6 * case["pairs"], case["K"], case["P"]
    one = dict(case, AtA=case["AtA"][b:b + 1], damping=None if case["damping"] is None else case["damping"][b:b + 1])
    H = mr.damped(one, dtype)[0]
    mu = dtype(0.0) if case["damping"] is None else dtype(case["damping"][b])
    s2 = dtype(1.0) if case["sigma2"] is None else dtype(case["sigma2"][b])
    L = np.linalg.cholesky(H)
    if not np.all(np.isfinite(L)) or not np.all(np.diag(L) > 0):
        raise np.linalg.LinAlgError("not positive definite")
    Y = np.tril(scipy.linalg.solve_triangular(L, np.eye(P, dtype=dtype), lower=True, check_finite=False))
    g_cov, g_dv, g_ld = (None if ups[k] is None else ups[k][b].astype(dtype) for k in ("g_cov", "g_dv", "g_ld"))
    G = np.zeros((P, P), dtype)
    if g_cov is not None:
        G[:m, :m] = g_cov if mutate == "cov_unsym" else dtype(0.5) * (g_cov + g_cov.T)
    basis = case["basis"][b].astype(dtype)
    if g_dv is not None and K > 0:
        w = np.abs(g_dv) if mutate == "abs_g" else g_dv
        Mw = (basis * w[:, None]).T @ basis
        if mutate == "zero_block":
            Mw[:32, :32] = 0
        G[m:, m:] = Mw
    Q = Y @ G @ Y.T
    S = -s2 * Q
    if g_ld is not None and mutate != "no_logdet":
        S = S + g_ld * np.eye(P, dtype=dtype)
    dH = Y.T @ S @ Y
    a1 = np.diag(one["AtA"][0].astype(dtype)) + dtype(1e-5)
    gA = dH.copy()
    if mutate != "no_diag_mu":
        gA[np.arange(P), np.arange(P)] = (dtype(1.0) + mu) * np.diag(dH)
    out = dict(gAtA=gA, gdamping=np.sum(np.diag(dH) * a1, dtype=dtype), gsigma2=np.trace(Q, dtype=dtype),
               scale_damping=np.sum(np.abs(np.diag(dH)) * a1, dtype=dtype), scale_sigma2=np.sum(np.abs(np.diag(Q)), dtype=dtype), status=0)
    if K > 0:
        Tm = Y[m:, m:]
        gb = (basis @ Tm.T) @ Tm
        if g_dv is not None:
            gb = (dtype(1.0) if mutate == "gbasis_no2" else dtype(2.0)) * s2 * g_dv[:, None] * gb
        else:
            gb = np.zeros_like(gb)
        out["gbasis"] = gb
    else:
        out["gbasis"] = np.zeros((case["N"], 0), dtype)
    return out


def _zeros(case, dtype):
    P, N, K = case["P"], case["N"], case["K"]
    return dict(gAtA=np.zeros((P, P), dtype), gdamping=dtype(0), gsigma2=dtype(0), scale_damping=dtype(0), scale_sigma2=dtype(0),
                gbasis=np.zeros((N, K), dtype), status=1)


def closed_form(case, ups, dtype=np.float64, mutate=None):
    """every window by the closed form in `dtype`; a window expected to fail (or that fails in float64) gets zeros and status 1"""
    wins = []
    for b in range(case["B"]):
        if case["expect_fail"][b]:
            wins.append(_zeros(case, dtype))
            continue
        try:
            wins.append(_window(case, ups, b, dtype, mutate))
        except np.linalg.LinAlgError:
            if dtype != np.float64:
                raise
            wins.append(_zeros(case, dtype))
    return {k: np.stack([np.asarray(w[k]) for w in wins]) for k in wins[0]}


@functools.lru_cache(maxsize=4)
def _reference_cached(family, spec, seed):
    case = mr.make(family, spec, seed)
    ups = upstreams(case)
    want = closed_form(case, ups)
    yard = errors(case, ups, closed_form(case, ups, np.float32), want)
    return ups, want, yard


def reference(case):
    """-> (upstreams, the float64 closed form, the yardstick's errors); computed once per case and shared -- do not modify"""
    if case["family"] in mr.FAMILIES and "problem" not in case:
        return _reference_cached(case["family"], case["spec"], case["seed"])
    ups = upstreams(case)
    want = closed_form(case, ups)
    return ups, want, errors(case, ups, closed_form(case, ups, np.float32), want)


def autograd_ref(case, ups):
    """torch CPU float64 autograd through the definition -> dict gAtA, gdamping, gsigma2, gbasis (windows expected to succeed)"""
    import torch
    m, K, P = 6 * case["pairs"], case["K"], case["P"]
    out = {k: [] for k in OUTPUTS}
    for b in range(case["B"]):
        A = torch.tensor(case["AtA"][b], dtype=torch.float64, requires_grad=True)
        mu = torch.tensor(0.0 if case["damping"] is None else float(case["damping"][b]), dtype=torch.float64, requires_grad=True)
        s2 = torch.tensor(1.0 if case["sigma2"] is None else float(case["sigma2"][b]), dtype=torch.float64, requires_grad=True)
        basis = torch.tensor(case["basis"][b], dtype=torch.float64, requires_grad=True)
        As = 0.5 * (A + A.T)
        H = As + mu * torch.diag(torch.diagonal(As) + 1e-5)
        L = torch.linalg.cholesky(H)
        Y = torch.linalg.solve_triangular(L, torch.eye(P, dtype=torch.float64), upper=False)
        cov = s2 * (Y.T @ Y)[:m, :m]
        loss = (torch.tensor(ups["g_cov"][b]) * cov).sum() + torch.tensor(ups["g_ld"][b]) * 2.0 * torch.log(torch.diagonal(L)).sum()
        if K > 0:
            y = basis @ Y[m:, m:].T
            loss = loss + (torch.tensor(ups["g_dv"][b]) * s2 * (y * y).sum(1)).sum()
        gA, gmu, gs2, gb = torch.autograd.grad(loss, (A, mu, s2, basis), allow_unused=True)
        out["gAtA"].append(gA.numpy())
        out["gdamping"].append(gmu.numpy())
        out["gsigma2"].append(gs2.numpy())
        out["gbasis"].append(np.zeros((case["N"], K)) if gb is None else gb.numpy())
    return {k: np.stack(v) for k, v in out.items()}


def errors(case, ups, got, want):
    """per entry of ERRORS, the largest error over the windows expected to succeed (outputs missing from `got`: 0)"""
    m, K = 6 * case["pairs"], case["K"]
    e = dict.fromkeys(ERRORS, 0.0)
    blocks = (("gAtA_pp", slice(0, m), slice(0, m)), ("gAtA_pd", slice(0, m), slice(m, None)), ("gAtA_dd", slice(m, None), slice(m, None)))
    for b in range(case["B"]):
        if case["expect_fail"][b]:
            continue
        if got.get("gAtA") is not None:
            g, w = np.asarray(got["gAtA"][b], np.float64), want["gAtA"][b]
            for name, r, c in blocks:
                if w[r, c].size:
                    scale = np.abs(w[r, c]).max()
                    for gg in ((g[r, c], w[r, c]), (g[c, r], w[c, r])):      # both halves: the output is written in full
                        e[name] = max(e[name], float(np.abs(gg[0] - gg[1]).max() / scale))
        if got.get("gbasis") is not None and K > 0:
            g, w = np.asarray(got["gbasis"][b], np.float64), want["gbasis"][b]
            rows = np.zeros(case["N"], bool) if ups["g_dv"] is None else ups["g_dv"][b] != 0
            if np.any(g[~rows] != 0):
                e["gbasis"] = np.inf
            if rows.any():
                scale = np.abs(w[rows]).max(axis=1, keepdims=True)
                e["gbasis"] = max(e["gbasis"], float((np.abs(g[rows] - w[rows]) / scale).max()))
        for name in ("gdamping", "gsigma2"):
            if got.get(name) is not None:
                scale = float(want["scale_" + name[1:]][b])
                d = abs(float(got[name][b]) - float(want[name][b]))
                e[name] = max(e[name], d / scale if scale > 0 else (0.0 if d == 0 else np.inf))
    return e


def gates(case, yard):
    floor = (case["P"] + case["N"]) * 2.0 ** -24
    return {k: max(4.0 * yard[k], floor) for k in ERRORS}
