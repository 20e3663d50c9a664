"""Reference for banet_ba_residual_grad_f32: the forward of tests/residual_ref.py restated in torch  --  TEST INFRASTRUCTURE.

Per window b, target frame f and point n: D = D0 + Bs.W, the warp of oracle.banet_oracle.warp at (R_f, T_f), the inclusive in-image
mask, the bilinear sample of the target map with the +1 taps clamped to the image (oracle.banet_oracle._bilinear_clamped; on a
point in the mask the zero-padded resampler of the bundle variants takes the same taps with the same weights), d = F2w - F1,
sq = sum_c d^2, ab = sum_c |d|, proj = (px, py).  The mask and the floor carry no gradient, which is the definition the kernel
implements (mask and floor of the forward held fixed).  Autograd differentiates

    L = sum gsq sq + gab ab + gproj . proj        (masked points contribute nothing)

with respect to the source rows, the target maps, depth, basis, Wc, R and T.  Everything runs in `dtype`: float64 is the truth the GPU
gradients are measured against, float32 the yardstick for how far a float32 evaluation may sit from it.
"""
import numpy as np
import torch

OUTPUTS = ("dsrc", "dtgt", "ddepth", "dbasis", "dWc", "dR", "dT")


def inputs_of(a, conv2s, R, T, Wc, dtype):
    """a, conv2s: from residual_ref.dense_inputs / sparse_inputs (any float dtype) -> dict of torch tensors in `dtype`:
    conv1 [B,N,C], tgt [B,pairs,H,W,C] (the first C channels of the [f|gx|gy] maps), p [B,3,N], fx, fy, ox, oy [B,N], D [B,N],
    Bs [B,N,K] or None, R [B,pairs,3,3], T [B,pairs,3], Wc [B,K] or None"""
    B, N, C = a["conv1"].shape
    pairs = len(conv2s)

    def t(x):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float64))).to(dtype)
    out = {k: t(a[k]) for k in ("conv1", "p", "fx", "fy", "ox", "oy")}
    out["D"] = t(a["D"]).reshape(B, N)
    out["tgt"] = torch.stack([t(c2[..., :C]) for c2 in conv2s], 1)
    out["Bs"] = t(a["Bs"]) if ("Bs" in a and Wc is not None) else None
    out["Wc"] = t(Wc).reshape(B, -1) if out["Bs"] is not None else None
    out["R"] = t(R).reshape(B, pairs, 3, 3)
    out["T"] = t(T).reshape(B, pairs, 3)
    return out


def forward(t):
    """-> dict(sq, ab [B,pairs,N]; mask [B,pairs,N] bool; proj [B,pairs,N,2]; d [B,pairs,N,C]), attached to the graph of t's tensors"""
    conv1, tgt = t["conv1"], t["tgt"]
    B, N, C = conv1.shape
    pairs, H, W = tgt.shape[1], tgt.shape[2], tgt.shape[3]
    D = t["D"]
    if t["Bs"] is not None:
        D = D + torch.matmul(t["Bs"], t["Wc"].reshape(B, -1, 1))[..., 0]
    Rp = torch.matmul(t["R"], t["p"][:, None])                              # [B,pairs,3,N]
    X = Rp * D[:, None, None, :] + t["T"][..., None]
    x, y = X[:, :, 0] / X[:, :, 2], X[:, :, 1] / X[:, :, 2]
    px, py = t["fx"][:, None] * x + t["ox"][:, None], t["fy"][:, None] * y + t["oy"][:, None]
    with torch.no_grad():
        mask = (px >= 0) & (px <= W - 1) & (py >= 0) & (py <= H - 1)          # NaN -> False
    zero = torch.zeros_like(px)
    pxs, pys = torch.where(mask, px, zero), torch.where(mask, py, zero)
    with torch.no_grad():
        x0f, y0f = torch.floor(pxs), torch.floor(pys)
        x0, y0 = x0f.long(), y0f.long()
        x1, y1 = (x0 + 1).clamp(max=W - 1), (y0 + 1).clamp(max=H - 1)
    dx, dy = pxs - x0f, pys - y0f
    bi = torch.arange(B)[:, None, None]
    fi = torch.arange(pairs)[None, :, None]
    I00, I01, I10, I11 = tgt[bi, fi, y0, x0], tgt[bi, fi, y0, x1], tgt[bi, fi, y1, x0], tgt[bi, fi, y1, x1]
    w00, w01, w10, w11 = (1 - dx) * (1 - dy), dx * (1 - dy), (1 - dx) * dy, dx * dy
    F2w = ((I00 * w00[..., None] + I01 * w01[..., None]) + I10 * w10[..., None]) + I11 * w11[..., None]
    d = torch.where(mask[..., None], F2w - conv1[:, None], torch.zeros_like(F2w))
    return dict(sq=(d * d).sum(-1), ab=d.abs().sum(-1), mask=mask, proj=torch.stack([pxs, pys], -1), d=d)


def loss(t, gsq=None, gab=None, gproj=None):
    """L and the forward maps; the upstream gradients are numpy / torch arrays [B,pairs,N] / [B,pairs,N,2] or None"""
    f = forward(t)
    dt = t["conv1"].dtype
    L = torch.zeros((), dtype=dt)
    for g, v in ((gsq, f["sq"]), (gab, f["ab"]), (gproj, f["proj"])):
        if g is not None:
            L = L + (torch.as_tensor(g).to(dt) * v).sum()
    return L, f


def gradients(a, conv2s, R, T, Wc, gsq=None, gab=None, gproj=None, dtype=torch.float64):
    """-> dict by output name (numpy float64; dbasis / dWc None without a basis): dsrc [B,N,C], dtgt [B,pairs,H,W,C], ddepth [B,N],
    dbasis [B,N,K], dWc [B,K], dR [B,pairs,9], dT [B,pairs,3]"""
    t = inputs_of(a, conv2s, R, T, Wc, dtype)
    names = dict(dsrc="conv1", dtgt="tgt", ddepth="D", dbasis="Bs", dWc="Wc", dR="R", dT="T")
    wrt = {o: t[k].requires_grad_(True) for o, k in names.items() if t[k] is not None}
    L, _ = loss(t, gsq, gab, gproj)
    grads = torch.autograd.grad(L, list(wrt.values()), allow_unused=True)
    out = {o: None for o in OUTPUTS}
    B = t["conv1"].shape[0]
    for (o, v), g in zip(wrt.items(), grads):
        g = torch.zeros_like(v) if g is None else g
        out[o] = g.detach().numpy().astype(np.float64)
    out["dR"] = out["dR"].reshape(B, -1, 9)
    return out


def borderline(a, conv2s, R, T, Wc, with_gab=True):
    """[B,pairs,N] bool: the points where the derivative is discontinuous within float32's reach of the float64 state -- a
    coordinate of the float64 projection within 4e-6 max(W, H) of an integer, or (where gab != 0) a channel with
    |d| < 1e-5 max |d|, the maximum over the whole level (the scale of the features: what float32's error in d goes with).
    Also returns the float64 in-image mask."""
    with torch.no_grad():
        f = forward(inputs_of(a, conv2s, R, T, Wc, torch.float64))
    H, W = conv2s[0].shape[1], conv2s[0].shape[2]
    e = 4e-6 * max(W, H)
    proj = f["proj"].numpy()
    near = (np.abs(proj - np.rint(proj)) < e).any(-1)
    mask = f["mask"].numpy()
    if with_gab:
        d = np.abs(f["d"].numpy())
        near |= (d < 1e-5 * d.max()).any(-1)
    return near & mask, mask
