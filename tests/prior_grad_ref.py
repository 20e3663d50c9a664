"""The float64 twin of the prior term's backward (include/banet_hip.h (5e)) and the host-only ABI probes of its entries.  Plain
module, no fixtures: shared by test_prior_grad_cpu.py and test_gpu_prior_grad.py.  Built on prior_ref.fit_sums / terms / apply.

    gLe[i,j] = gAtA'[m+i, m+j] - gAtb'[m+i] Wc[j]      gee[i] = gAtb'[m+i]      gWc[j] = - sum_i Le[i,j] gAtb'[m+i]
    gLambda = scale gLe    geta = scale gee    gscale = (sum gLe . Le + sum gee . ee) / scale
    Gh = scale 1/2 (gLe + gLe^T)    gh = scale gee    per counted point: r = obs - depth, y = Gh b, p = b . gh, q = b . y
    gweight = q + r p    gobs = w p    gdepth = - w p    gbasis = w (2 y + r gh)

Every function also returns, where a GPU test needs it, the sum of the absolute values of the terms that make up each element:
the yardstick of a fixed-order float32 chain of at most K + 4 roundings."""
import numpy as np

import prior_ref as pref

OK, ERR_INVALID_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED, ERR_LAUNCH = 0, -1, -2, -3, -4
OVERWRITE, ACCUMULATE = 1, 2
OUTPUTS = ("gLambda", "geta", "gscale", "gobs", "gweight", "gdepth", "gbasis")


def counted(obs, weight=None):
    """the points banet_basis_fit_f32 counts: a finite weight > 0 and a finite observation -> bool [B,N]"""
    t = np.asarray(obs, np.float64)
    w = np.ones_like(t) if weight is None else np.asarray(weight, np.float64)
    return np.isfinite(w) & (w > 0) & np.isfinite(t)


def add_grad(Le, Wc, gAtA, gAtb, pairs):
    """one iteration's step -> (gLe [B,K,K], gee [B,K], gWc [B,K]) and their absolute-term sums (aLe, aWc)"""
    m = 6 * max(int(pairs), 1)
    Le, W = np.asarray(Le, np.float64), np.asarray(Wc, np.float64).reshape(Le.shape[0], -1)
    gA = np.asarray(gAtA, np.float64)[:, m:, m:]
    gb = np.asarray(gAtb, np.float64).reshape(Le.shape[0], -1)[:, m:]
    gLe = gA - gb[:, :, None] * W[:, None, :]
    aLe = np.abs(gA) + np.abs(gb)[:, :, None] * np.abs(W)[:, None, :]
    gWc = -np.einsum("bij,bi->bj", Le, gb)
    aWc = np.einsum("bij,bi->bj", np.abs(Le), np.abs(gb))
    return (gLe, gb.copy(), gWc), (aLe, aWc)


def terms_grad(scale, gLe, gee, Le=None, ee=None, depth=None, basis=None, obs=None, weight=None):
    """the once-per-level step -> (dict of OUTPUTS, dict of their absolute-term sums); an output whose input is absent is None"""
    s = float(scale)
    gLe, gee = np.asarray(gLe, np.float64), np.asarray(gee, np.float64)
    out = dict.fromkeys(OUTPUTS)
    mag = dict.fromkeys(OUTPUTS)
    out["gLambda"], out["geta"] = s * gLe, s * gee
    mag["gLambda"], mag["geta"] = np.abs(out["gLambda"]), np.abs(out["geta"])
    if Le is not None:
        Le, ee = np.asarray(Le, np.float64), np.asarray(ee, np.float64)
        out["gscale"] = ((gLe * Le).sum((1, 2)) + (gee * ee).sum(1)) / s
        mag["gscale"] = (np.abs(gLe * Le).sum((1, 2)) + np.abs(gee * ee).sum(1)) / s
    if obs is not None:
        d, b, t = (np.asarray(x, np.float64) for x in (depth, basis, obs))
        ok = counted(t, weight)
        w = np.where(ok, np.ones_like(t) if weight is None else np.asarray(weight, np.float64), 0.0)
        r = np.where(ok, t - d, 0.0)
        b = np.where(ok[..., None], b, 0.0)
        Gh, gh = s * 0.5 * (gLe + gLe.transpose(0, 2, 1)), s * gee
        y = np.einsum("bij,bnj->bni", Gh, b)
        ay = np.einsum("bij,bnj->bni", np.abs(Gh), np.abs(b))
        p = np.einsum("bni,bi->bn", b, gh)
        ap = np.einsum("bni,bi->bn", np.abs(b), np.abs(gh))
        q = np.einsum("bni,bni->bn", b, y)
        aq = np.einsum("bni,bni->bn", np.abs(b), ay)
        out["gobs"], mag["gobs"] = w * p, w * ap
        out["gdepth"], mag["gdepth"] = -w * p, w * ap
        out["gweight"] = np.where(ok, q + r * p, 0.0)
        mag["gweight"] = np.where(ok, aq + np.abs(r) * ap, 0.0)
        out["gbasis"] = w[..., None] * (2.0 * y + r[..., None] * gh[:, None, :])
        mag["gbasis"] = w[..., None] * (2.0 * ay + np.abs(r)[..., None] * np.abs(gh)[:, None, :])
        if weight is None:
            out["gweight"] = mag["gweight"] = None
    return out, mag


def forward(scale, Lambda, eta, depth, basis, obs, weight, W, AtA, Atb, pairs):
    """the twin's forward of one iteration's add: -> (AtA', Atb' [B,P,1], Le, ee)"""
    G = g = None
    if obs is not None:
        G, g = pref.fit_sums(depth, basis, obs, weight)
    Le, ee = pref.terms(scale, Lambda, eta, G, g)
    B = Le.shape[0]
    A2, b2 = pref.apply(AtA, np.asarray(Atb, np.float64).reshape(B, -1, 1), np.asarray(W, np.float64).reshape(B, -1, 1), Le, ee, pairs)
    return A2, b2, Le, ee


def backward(scale, Lambda, eta, depth, basis, obs, weight, W, gA2, gb2, pairs):
    """gradients of <gA2, AtA'> + <gb2, Atb'> with respect to every input -> dict (gAtA / gAtb pass through; gWc; OUTPUTS)"""
    G = g = None
    if obs is not None:
        G, g = pref.fit_sums(depth, basis, obs, weight)
    Le, ee = pref.terms(scale, Lambda, eta, G, g)
    (gLe, gee, gWc), _ = add_grad(Le, W, gA2, gb2, pairs)
    out, _ = terms_grad(scale, gLe, gee, Le, ee, depth, basis, obs, weight)
    if Lambda is None:
        out["gLambda"] = None
    if eta is None:
        out["geta"] = None
    out.update(gWc=gWc, gAtA=np.asarray(gA2, np.float64), gAtb=np.asarray(gb2, np.float64))
    return out


# ======================================================================================================================
# host-only ABI probes of the three entries, in a child process that sees no device (prior_ref.abi_sweep_in_child's arrangement):
# the call that passes every check fails for lack of a device (ERR_LAUNCH).
# ======================================================================================================================
def abi_sweep():
    """-> [{name, bytes, exact, minus1, off4, null}] for banet_prior_terms_f32 / banet_prior_terms_grad_f32 and {name, rc...} for
    banet_prior_add_grad_f32 at prior_ref.ABI_SHAPES, then the INVALID_ARG / UNSUPPORTED cases by name"""
    import ctypes
    import ws_contract as wsc
    from banet_amd import _capi as capi
    L = capi.lib()
    host = (ctypes.c_float * 64)()
    pv = ctypes.cast(host, ctypes.c_void_p).value
    arena = (ctypes.c_char * 512)()
    base = (ctypes.addressof(arena) + 255) & ~255
    out = []

    def prior(has, scale=0.5):
        pr = capi.Prior()
        for name, on in zip(("Lambda", "eta", "obs_depth", "obs_weight"), has):
            setattr(pr, name, pv if on else None)
        pr.scale = scale
        return pr

    def gin(flags=0, reserved=0, gLe=pv, Le=pv):
        g = capi.PriorGradIn()
        g.gLe, g.gee, g.Le, g.ee, g.flags, g.reserved_ = gLe, pv, Le, Le, flags, reserved
        return g

    def gout(names):
        g = capi.PriorGradOut()
        for n in names:
            setattr(g, n, pv)
        return g

    def allowed(has):
        names = ["gscale"]
        names += ["gLambda"] if has[0] else []
        names += ["geta"] if has[1] else []
        names += ["gobs", "gdepth", "gbasis"] if has[2] else []
        names += ["gweight"] if has[3] else []
        return names

    for B, H, W, K, pairs, has in pref.ABI_SHAPES:
        lv = wsc._abi_level(capi, pv, B, H, W, K, pairs, C=16)
        pr = prior(has)
        tag = "B%d %dx%d K%d pairs%d has%d%d%d%d" % ((B, H, W, K, pairs) + has)
        gi, go = gin(), gout(allowed(has))
        calls = (("prior_terms", L.banet_prior_workspace_bytes(ctypes.byref(lv), ctypes.byref(pr)),
                  lambda ws, n: L.banet_prior_terms_f32(ctypes.byref(lv), ctypes.byref(pr), pv, pv, ws, n, None)),
                 ("prior_terms_grad", L.banet_prior_terms_grad_workspace_bytes(ctypes.byref(lv), ctypes.byref(pr)),
                  lambda ws, n: L.banet_prior_terms_grad_f32(ctypes.byref(lv), ctypes.byref(pr), ctypes.byref(gi), ctypes.byref(go), ws, n, None)))
        for name, nb, call in calls:
            rec = dict(name=name + " " + tag, bytes=int(nb), shape=[B, H * W, K, pairs] + list(has))
            if nb:
                rec["exact"] = call(ctypes.c_void_p(base), nb)
                rec["minus1"] = call(ctypes.c_void_p(base), nb - 1)
                rec["off4"] = call(ctypes.c_void_p(base + 4), nb)
                rec["null"] = call(None, nb)
            out.append(rec)
        add = lambda flags=0, Le=pv, gWc=pv, level=lv: L.banet_prior_add_grad_f32(ctypes.byref(level), Le, pv, pv, pv, pv, pv, gWc, flags, None)  # noqa: E731
        out.append(dict(name="prior_add_grad " + tag, accumulate=add(0), overwrite=add(OVERWRITE), off4=L.banet_prior_add_grad_f32(
            ctypes.byref(lv), pv, pv + 4, pv, pv + 4, pv, pv, pv, 0, None), null_Le=add(Le=None), null_gWc=add(gWc=None), bad_flag=add(4),
            accumulate_flag=add(ACCUMULATE)))

    # the refusals, on one shape
    B, H, W, K, pairs = 2, 24, 32, 16, 1
    lv = wsc._abi_level(capi, pv, B, H, W, K, pairs, C=16)
    full = prior((1, 1, 1, 1))
    nb = L.banet_prior_terms_grad_workspace_bytes(ctypes.byref(lv), ctypes.byref(full))
    ws = ctypes.c_void_p(base)

    def tg(pr, gi, go, level=lv):
        return L.banet_prior_terms_grad_f32(ctypes.byref(level), ctypes.byref(pr) if pr is not None else None,
                                            ctypes.byref(gi) if gi is not None else None, ctypes.byref(go) if go is not None else None, ws, nb, None)
    cases = {
        "baseline passes the checks": tg(full, gin(), gout(allowed((1, 1, 1, 1)))),
        "accumulate passes the checks": tg(full, gin(ACCUMULATE), gout(["gdepth", "gbasis"])),
        "gweight without obs_weight": tg(prior((1, 1, 1, 0)), gin(), gout(["gweight"])),
        "geta without eta": tg(prior((1, 0, 1, 1)), gin(), gout(["geta"])),
        "gLambda without Lambda": tg(prior((0, 0, 1, 1)), gin(), gout(["gLambda"])),
        "gobs without obs_depth": tg(prior((1, 1, 0, 0)), gin(), gout(["gobs"])),
        "gbasis without obs_depth": tg(prior((1, 1, 0, 0)), gin(), gout(["gbasis"])),
        "gdepth without obs_depth": tg(prior((1, 1, 0, 0)), gin(), gout(["gdepth"])),
        "NULL gLe": tg(full, gin(gLe=None), gout(["gLambda"])),
        "gscale without Le": tg(full, gin(Le=None), gout(["gscale"])),
        "no output": tg(full, gin(), gout([])),
        "unknown flag": tg(full, gin(4), gout(["gLambda"])),
        "overwrite flag": tg(full, gin(OVERWRITE), gout(["gLambda"])),
        "reserved_": tg(full, gin(reserved=1), gout(["gLambda"])),
        "scale 0": tg(prior((1, 1, 1, 1), 0.0), gin(), gout(["gLambda"])),
        "no pointers": tg(prior((0, 0, 0, 0)), gin(), gout(["gscale"])),
        "NULL prior": tg(None, gin(), gout(["gscale"])),
        "NULL in": tg(full, None, gout(["gscale"])),
        "NULL out": tg(full, gin(), None),
        "eta without Lambda": tg(prior((0, 1, 1, 0)), gin(), gout(["gobs"])),
        "negative scale": tg(prior((1, 1, 1, 1), -1.0), gin(), gout(["gLambda"])),
    }
    nodepth = wsc._abi_level(capi, pv, B, H, W, K, pairs, C=16)
    nodepth.depth = None
    cases["per-pixel output on a level without depth"] = tg(full, gin(), gout(["gobs"]), nodepth)
    cases["coefficient outputs on a level without depth"] = tg(full, gin(), gout(["gLambda"]), nodepth)
    unsupported = {}
    for what, kw in (("camera variant", dict(variant=capi.BUNDLE_CAMERA)), ("K 257", dict(K=257)), ("K 0", dict(K=0, variant=capi.BUNDLE))):
        k = dict(B=B, H=H, W=W, K=K, pairs=pairs, C=16)
        k.update(kw)
        bad = wsc._abi_level(capi, pv, **k)
        unsupported[what] = dict(terms_grad=tg(full, gin(), gout(["gLambda"]), bad),
                                 query=int(L.banet_prior_terms_grad_workspace_bytes(ctypes.byref(bad), ctypes.byref(full))),
                                 add_grad=L.banet_prior_add_grad_f32(ctypes.byref(bad), pv, pv, pv, pv, pv, pv, pv, 0, None),
                                 terms=L.banet_prior_terms_f32(ctypes.byref(bad), ctypes.byref(full), pv, pv, ws, 1 << 30, None))
    terms = {
        "NULL Le": L.banet_prior_terms_f32(ctypes.byref(lv), ctypes.byref(full), None, pv, ws, 1 << 30, None),
        "NULL ee": L.banet_prior_terms_f32(ctypes.byref(lv), ctypes.byref(full), pv, None, ws, 1 << 30, None),
        "NULL level": L.banet_prior_terms_f32(None, ctypes.byref(full), pv, pv, ws, 1 << 30, None),
        "empty prior": L.banet_prior_terms_f32(ctypes.byref(lv), None, pv, pv, None, 0, None),
        "scale 0": L.banet_prior_terms_f32(ctypes.byref(lv), ctypes.byref(prior((1, 1, 1, 1), 0.0)), pv, pv, None, 0, None),
        "eta without Lambda": L.banet_prior_terms_f32(ctypes.byref(lv), ctypes.byref(prior((0, 1, 0, 0))), pv, pv, ws, 1 << 30, None),
        "observations on a level without depth": L.banet_prior_terms_f32(ctypes.byref(nodepth), ctypes.byref(full), pv, pv, ws, 1 << 30, None),
    }
    out.append(dict(name="refusals", terms_grad=cases, unsupported=unsupported, terms=terms,
                    add_null_level=L.banet_prior_add_grad_f32(None, pv, pv, pv, pv, pv, pv, pv, 0, None)))
    return out


def abi_sweep_in_child():
    import json
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="", BANET_NUM_CUS="256")
    code = ("import sys, json; sys.path[:0] = [%r, %r]; import prior_grad_ref; print('ABI_SWEEP ' + json.dumps(prior_grad_ref.abi_sweep()))"
            % (os.path.dirname(here), here))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, "the ABI sweep's child process ended with %s:\n%s" % (r.returncode, (r.stdout + r.stderr)[-3000:])
    line = [l for l in r.stdout.splitlines() if l.startswith("ABI_SWEEP ")][-1]
    return json.loads(line[len("ABI_SWEEP "):])
