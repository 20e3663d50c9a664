"""Reference for banet_ba_residual_f32, from the oracle's own functions  --  TEST INFRASTRUCTURE (numpy).

Per window b, target frame f and point n: D = D0 + Bs.W, oracle.banet_oracle.warp at (R_f, T_f), then the variant's own
residual statement -- `_bundle_residuals` (bundlenet.py:154-163: tf.contrib.resampler + the in-image mask) for `bundle` /
`bundle_camera`, `_legacy_residuals` (legacy/ba.py:256-264: interpolate2d) for `legacy_lm` / `legacy_fixed` -- and from its
masked difference rows  sq = sum_c d^2,  ab = sum_c |d|.  Everything runs in `dtype`: float64 is the truth the GPU maps are
measured against, float32 the yardstick for how far a float32 evaluation may sit from it.
"""
import numpy as np

from oracle import banet_oracle as orc, dense as odense

BUNDLE_VARIANTS = ("bundle", "bundle_camera")


def dense_inputs(variant, intr, lv, dtype, normalize=None):
    """oracle.dense.level_inputs for a dense level dict (tgt [B,H,W,C] or [B,pairs,H,W,C]) -> (inputs, [conv2 per frame]);
    normalize: as the variant has it (bundlenet.py:119 normalises the rays, legacy/ba.py:33-34 does not) unless given"""
    if normalize is None:
        normalize = variant in BUNDLE_VARIANTS
    tgt = lv["tgt"] if lv["tgt"].ndim == 5 else lv["tgt"][:, None]
    one = dict(lv)
    one["tgt"] = tgt[:, 0]
    if variant != "bundle":
        one["basis"] = None
    a = odense.level_inputs(intr, one, normalize, dtype)
    return a, [orc.target_map(tgt[:, f].astype(dtype)) for f in range(tgt.shape[1])]


def sparse_inputs(sp, dtype):
    """the given rays and per-point intrinsics instead of level_inputs: sp = dict(conv1 [B,N,C], conv2 [B,pairs,H,W,3C],
    p [B,3,N], fx / fy / ox / oy [B,N], D [B,N,1], Bs [B,N,K] or None)"""
    a = {k: sp[k].astype(dtype) for k in ("conv1", "p", "fx", "fy", "ox", "oy", "D")}
    if sp.get("Bs") is not None:
        a["Bs"] = sp["Bs"].astype(dtype)
    return a, [sp["conv2"][:, f].astype(dtype) for f in range(sp["conv2"].shape[1])]


def residual_maps(variant, a, conv2s, R, T, W=None, dtype=np.float64):
    """a, conv2s: from dense_inputs / sparse_inputs in the same dtype; R [B,pairs,3,3], T [B,pairs,3,1], W [B,K,1] or None
    -> dict(sq, ab [B,pairs,N] dtype; mask [B,pairs,N] bool; px, py [B,pairs,N]; borderline [B,pairs] int: the points whose
    projection lies within e = 4e-6 max(W, H) pixels of the mask's boundary, as oracle/torch_port.py:73-76 counts them)"""
    B, N = a["conv1"].shape[:2]
    pairs = len(conv2s)
    R = np.asarray(R, dtype).reshape(B, pairs, 3, 3)
    T = np.asarray(T, dtype).reshape(B, pairs, 3, 1)
    D = a["D"]
    if "Bs" in a and W is not None:
        D = D + np.matmul(a["Bs"], np.asarray(W, dtype).reshape(B, -1, 1))
    out = dict(sq=[], ab=[], mask=[], px=[], py=[], borderline=[])
    for f in range(pairs):
        conv2 = conv2s[f]
        Hh, Ww = conv2.shape[1], conv2.shape[2]
        w = orc.warp(R[:, f], T[:, f], a["p"], D, a["fx"], a["fy"], a["ox"], a["oy"])
        res = orc._bundle_residuals if variant in BUNDLE_VARIANTS else orc._legacy_residuals
        diff, _, mask = res(a["conv1"], conv2, w)
        d = diff[..., 0]
        out["sq"].append(np.sum(d * d, axis=-1))
        out["ab"].append(np.sum(np.abs(d), axis=-1))
        out["mask"].append(mask[..., 0] > 0)
        px, py = w["px"], w["py"]
        out["px"].append(px)
        out["py"].append(py)
        e = 4e-6 * max(Ww, Hh)
        inx, iny = (px >= -e) & (px <= Ww - 1 + e), (py >= -e) & (py <= Hh - 1 + e)
        near = (((np.abs(px) < e) | (np.abs(px - (Ww - 1)) < e)) & iny) | (((np.abs(py) < e) | (np.abs(py - (Hh - 1)) < e)) & inx)
        out["borderline"].append(near.sum(1))
    return {k: np.stack(v, axis=1) for k, v in out.items()}


def dense_residual(variant, intr, lv, R, T, W=None, dtype=np.float64, normalize=None):
    a, conv2s = dense_inputs(variant, intr, lv, dtype, normalize)
    return residual_maps(variant, a, conv2s, R, T, W, dtype)


def sparse_residual(variant, sp, R, T, W=None, dtype=np.float64):
    a, conv2s = sparse_inputs(sp, dtype)
    return residual_maps(variant, a, conv2s, R, T, W, dtype)
