"""The float64 twin of the prior term (include/banet_hip.h (5d)) and the host-only ABI probes of its entries.  Plain module, no
fixtures: shared by test_prior_cpu.py and test_gpu_prior.py.

The twin is composed from the oracle's own pieces: banet_oracle.bundle_window_iteration in float64 for AtA0, Atb and lambda, then the
term, then the oracle's damp, solve_lu and _se3_update:

    Le = scale (G + Lambda)      ee = scale (g + eta)        (a half that is not given is left out)
    AtA[m+i, m+j] += Le[i,j]     Atb[m+i] += ee[i] - sum_j Le[i,j] W[j]            m = 6 pairs

G = sum w b b^T and g = sum w (obs - depth) b are float64 sums over the points banet_basis_fit_f32 counts (a finite w > 0 and a
finite obs).  The oracle's Wn = W + sol[6 pairs:] and sol = solve(damp(AtA), Atb) fix the signs."""
import numpy as np

from oracle import banet_oracle as orc

OK, ERR_INVALID_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED, ERR_LAUNCH = 0, -1, -2, -3, -4

# The 3-level, 2-iteration schedule scenes of test_gpu_prior.py (24 x 32, scales 4 / 2 / 1, C = K = 16, three windows, seed 31 + b):
# (trans_mag of synth.make_window_scene, the start T0 as a fraction of the true translation).  A gate relative to max |delta| of the
# LAST iteration needs a last update that is not small: with the single-level scenes' (0.03, 0.7) the sixth update is 0.01 and the
# float32 ORACLE is already 2.4e-4 from the float64 one; with these it is 0.2 and 1e-5 (test_prior_cpu.py asserts it).
SCHEDULE_MOTION = (0.10, 0.3)


def fit_sums(depth, basis, obs, weight=None):
    """depth, obs, weight [B,N], basis [B,N,K] -> G [B,K,K], g [B,K] in float64 over the contributing points"""
    d, b, t = (np.asarray(x, np.float64) for x in (depth, basis, obs))
    w = np.ones_like(d) if weight is None else np.asarray(weight, np.float64)
    ok = np.isfinite(w) & (w > 0) & np.isfinite(t)
    w = np.where(ok, w, 0.0)
    r = np.where(ok, t - d, 0.0)
    b = np.where(ok[..., None], b, 0.0)
    return np.einsum("bn,bni,bnj->bij", w, b, b), np.einsum("bn,bni->bi", w * r, b)


def terms(scale, Lambda=None, eta=None, G=None, g=None):
    """-> Le [B,K,K], ee [B,K] (float64); at least one of Lambda / G is given"""
    assert Lambda is not None or G is not None
    L = sum(np.asarray(x, np.float64) for x in (G, Lambda) if x is not None)
    parts = [np.asarray(x, np.float64) for x in (g, eta) if x is not None]
    e = sum(parts) if parts else np.zeros(L.shape[:2])
    return float(scale) * L, float(scale) * e


def apply(AtA, Atb, W, Le, ee, pairs):
    """the term added to AtA [B,P,P] and Atb [B,P,1] at the coefficients W [B,K,1] -> new arrays"""
    m = 6 * pairs
    A, b = np.array(AtA, np.float64), np.array(Atb, np.float64)
    A[:, m:, m:] += Le
    b[:, m:, 0] += ee - np.einsum("bij,bj->bi", Le, np.asarray(W, np.float64)[:, :, 0])
    return A, b


def quadratic(W, scale, Lambda=None, eta=None, depth=None, basis=None, obs=None, weight=None):
    """the term's value at W [B,K] -> [B]"""
    W = np.asarray(W, np.float64)
    v = np.zeros(W.shape[0])
    if Lambda is not None:
        v += 0.5 * np.einsum("bi,bij,bj->b", W, np.asarray(Lambda, np.float64), W)
        if eta is not None:
            v -= np.einsum("bi,bi->b", np.asarray(eta, np.float64), W)
    if obs is not None:
        d, b, t = (np.asarray(x, np.float64) for x in (depth, basis, obs))
        w = np.ones_like(d) if weight is None else np.asarray(weight, np.float64)
        ok = np.isfinite(w) & (w > 0) & np.isfinite(t)
        res = np.where(ok, t - d - np.einsum("bnk,bk->bn", np.where(ok[..., None], b, 0.0), W), 0.0)
        v += 0.5 * (np.where(ok, w, 0.0) * res * res).sum(1)
    return float(scale) * v


def window_iteration(a, conv2s, Rs, Ts, W, mlp, l2_base, term=None):
    """One iteration of the twin.  a: oracle.dense.level_inputs(..., np.float64); conv2s: the target maps [f|gx|gy] per frame;
    Rs / Ts: lists per frame; W [B,K,1]; term: (Le, ee) or None (the oracle's iteration itself, recomputed the same way).
    -> Rs, Ts, W, dict(solution [B,P], lam [B])"""
    pairs = len(conv2s)
    _, _, _, dbg = orc.bundle_window_iteration(a["conv1"], conv2s, a["fx"], a["fy"], a["ox"], a["oy"], a["p"], a["D"], a["Bs"], Rs, Ts, W,
                                               mlp, l2_base)
    AtA0, Atb, lam = dbg["AtA"], dbg["Atb"], dbg["lam"]
    if term is not None:
        AtA0, Atb = apply(AtA0, Atb, W, term[0], term[1], pairs)
    sol = orc.solve_lu(orc.damp(AtA0, lam, undamped_last=True), Atb)
    Rn, Tn = [], []
    for i in range(pairs):
        r, t = orc._se3_update(sol[:, 6 * i:6 * i + 6], Rs[i], Ts[i])
        Rn.append(r)
        Tn.append(t)
    return Rn, Tn, W + sol[:, 6 * pairs:], dict(solution=sol[:, :, 0], lam=lam.reshape(-1), AtA=AtA0, Atb=Atb)


# ======================================================================================================================
# host-only ABI probes of the new entries: exact query / one byte less / pointer off by 4 / NULL, in a child process that sees no
# device (ws_contract.abi_sweep_in_child's arrangement): the call that passes every check fails for lack of a device.
# ======================================================================================================================
ABI_SHAPES = [  # B, H, W, K, pairs, (Lambda, eta, obs, weight)
    (2, 24, 32, 16, 1, (1, 1, 0, 0)), (3, 13, 19, 5, 2, (0, 0, 1, 1)), (1, 24, 32, 200, 1, (1, 0, 1, 0)), (2, 13, 19, 130, 2, (1, 1, 1, 1)),
    (32, 60, 80, 128, 1, (1, 1, 1, 0))]


def abi_sweep():
    """-> [{name, bytes, base, exact, minus1, off4, null}] for banet_prior_apply_f32, banet_lm_level_prior_f32 and
    banet_lm_solve_prior_f32 at ABI_SHAPES"""
    import ctypes
    import ws_contract as wsc
    from banet_amd import _capi as capi
    L = capi.lib()
    host = (ctypes.c_float * 64)()
    pv = ctypes.cast(host, ctypes.c_void_p).value
    arena = (ctypes.c_char * 512)()
    base = (ctypes.addressof(arena) + 255) & ~255
    st = capi.State()
    st.R = st.T = st.Wc = st.iters = st.ratio = st.lambda_out = st.delta = pv
    mlp = capi.Mlp()
    for i in range(5):
        mlp.w[i] = mlp.b[i] = pv
    out = []
    for B, H, W, K, pairs, has in ABI_SHAPES:
        lv = wsc._abi_level(capi, pv, B, H, W, K, pairs, C=16)
        pr = capi.Prior()
        for name, on in zip(("Lambda", "eta", "obs_depth", "obs_weight"), has):
            setattr(pr, name, pv if on else None)
        pr.scale = 0.5
        tag = "B%d %dx%d K%d pairs%d has%d%d%d%d" % ((B, H, W, K, pairs) + has)
        sched = capi.Schedule()
        lvs = (capi.Level * 2)(lv, lv)
        prs = (capi.Prior * 2)(capi.Prior(), pr)                   # level 0: the empty prior
        mp = (ctypes.POINTER(capi.Mlp) * 2)(ctypes.pointer(mlp), ctypes.pointer(mlp))
        it = (ctypes.c_int32 * 2)(1, 2)
        sched.levels, sched.n_levels = ctypes.cast(lvs, ctypes.POINTER(capi.Level)), 2
        sched.mlps = ctypes.cast(mp, ctypes.POINTER(ctypes.POINTER(capi.Mlp)))
        sched.max_iters, sched.l2_base = ctypes.cast(it, ctypes.POINTER(ctypes.c_int32)), 1000.0

        def solve(ws, n):
            sched.workspace, sched.workspace_bytes = ws, n
            return L.banet_lm_solve_prior_f32(ctypes.byref(sched), prs, ctypes.byref(st), None)
        calls = (("prior_apply", L.banet_prior_workspace_bytes(ctypes.byref(lv), ctypes.byref(pr)), 0,
                  lambda ws, n: L.banet_prior_apply_f32(ctypes.byref(lv), ctypes.byref(pr), pv, pv, pv, ws, n, None)),
                 ("lm_level_prior", L.banet_lm_level_prior_workspace_bytes(ctypes.byref(lv), ctypes.byref(pr)),
                  L.banet_lm_level_workspace_bytes(ctypes.byref(lv)),
                  lambda ws, n: L.banet_lm_level_prior_f32(ctypes.byref(lv), ctypes.byref(mlp), 1000.0, 2, None, ctypes.byref(pr),
                                                           ctypes.byref(st), ws, n, None)),
                 ("lm_solve_prior", L.banet_lm_solve_prior_workspace_bytes(ctypes.byref(sched), prs),
                  L.banet_lm_solve_workspace_bytes(ctypes.byref(sched)), solve))
        for name, nb, lvl, call in calls:
            rec = dict(name=name + " " + tag, bytes=int(nb), base=int(lvl), shape=[B, H * W, K, pairs] + list(has))
            if nb:
                rec["exact"] = call(ctypes.c_void_p(base), nb)
                rec["minus1"] = call(ctypes.c_void_p(base), nb - 1)
                rec["off4"] = call(ctypes.c_void_p(base + 4), nb)
                rec["null"] = call(None, nb)
            out.append(rec)
    return out


def abi_sweep_in_child():
    import json
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="", BANET_NUM_CUS="256")
    code = ("import sys, json; sys.path[:0] = [%r, %r]; import prior_ref; print('ABI_SWEEP ' + json.dumps(prior_ref.abi_sweep()))"
            % (os.path.dirname(here), here))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, "the ABI sweep's child process ended with %s:\n%s" % (r.returncode, (r.stdout + r.stderr)[-3000:])
    line = [l for l in r.stdout.splitlines() if l.startswith("ABI_SWEEP ")][-1]
    return json.loads(line[len("ABI_SWEEP "):])
