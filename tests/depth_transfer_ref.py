"""Inputs and numpy references for the tests of banet_depth_reproject_f32 (csrc/reproject.hip) and banet_basis_fit_f32
(csrc/basisfit.hip).  Shared by test_depth_transfer_cpu.py and test_gpu_depth_transfer.py.  No GPU.

Reprojection: oracle.dense.level_inputs (rays, level intrinsics, depth, basis in the reference's layout) and
oracle.banet_oracle.warp, then the rounding and z-buffer rule of include/banet_hip.h (3e): a valid point lands on texel
(floor(px + 0.5), floor(py + 0.5)); the smallest (d', n) wins.  A float64 version (the reference) and a float32 version (the
yardstick: numpy's float32 statements of the same formulas).  A texel is AMBIGUOUS -- a float32 evaluation may legitimately decide
it differently -- when
  * a point that can reach the texel or one of its 8 neighbours has px + 0.5 or py + 0.5 within e = 4e-6 max(W, H) of an integer,
    or lies within e of the image border (the band of tests/residual_ref.py), or
  * the texel's two nearest landed depths differ by less than 1e-5 relative.

Fit: the float64 definition, and a float32 yardstick (float32 Gram matrix and right-hand side, then a float64 solve).
"""
import numpy as np

from oracle import banet_oracle as orc
from oracle import dense as odense
from oracle import synth

BAND = 4e-6
DEPTH_TIE = 1e-5


# ---- scenes -------------------------------------------------------------------------------------------------------------------------
def pair_case(H, W, K, seed, normalize, w_gt=None, t_gt=None, B=1, scale=1, C=4):
    """B windows of oracle.synth.make_pair_scene (seeds seed, seed + 100, ...) at one level -> dict(intr [B,4], lv, R [B,1,3,3],
    T [B,1,3], W_gt [B,K], normalize); lv = dict(scale, H, W, D0 [B,H,W], basis [B,H,W,K]) at the level's resolution"""
    scenes = [synth.make_pair_scene(H, W, C, K, [scale], seed + 100 * b, normalize, w_gt=w_gt, t_gt=t_gt) for b in range(B)]
    intr, levels = odense.batch_scene(scenes)
    lv = levels[0]
    return dict(intr=intr, lv=dict(scale=lv["scale"], H=lv["H"], W=lv["W"], D0=lv["D0"], basis=lv["basis"]),
                R=np.stack([s["R_gt"] for s in scenes])[:, None], T=np.stack([s["T_gt"] for s in scenes])[:, None],
                W_gt=np.stack([s["W_gt"] for s in scenes]), normalize=bool(normalize), K=K, B=B, F=1)


def window_case(H, W, K, seed, pairs, B=1, C=4):
    scenes = [synth.make_window_scene(H, W, C, K, [1], seed + 100 * b, pairs) for b in range(B)]
    l0 = [s["levels"][0] for s in scenes]
    lv = dict(scale=1, H=H, W=W, D0=np.stack([l["D0"] for l in l0]), basis=np.stack([l["basis"] for l in l0]))
    return dict(intr=np.stack([s["intr"] for s in scenes]), lv=lv, R=np.stack([s["R_gt"] for s in scenes]),
                T=np.stack([s["T_gt"] for s in scenes]), W_gt=np.stack([s["W_gt"] for s in scenes]), normalize=True, K=K, B=B, F=pairs)


# the generic poses of the GPU module: (H, W, w_gt, t_gt, seed)
GENERIC = ((24, 32, (0.02, -0.03, 0.01), (0.05, -0.02, 0.04), 1), (24, 32, (0.0, 0.05, 0.0), (-0.2, 0.0, 0.1), 2),
           (30, 40, (0.01, 0.01, 0.08), (0.0, 0.1, -0.3), 3))


def generic_case(case, normalize, K=8, B=2):
    H, W, w, t, seed = case
    return pair_case(H, W, K, seed, normalize, w_gt=w, t_gt=t, B=B)


# the fit shapes of the GPU module
FIT_SHAPES = ((768, 5), (768, 32), (768, 128), (775, 130), (1536, 256), (33, 1), (31, 32))


def fit_damping(N, K):
    """mu of a shape case: 1e-3; N < K has no unique undamped answer, H = G + diag(G) (mu = 1) bounds its condition by ~2 K"""
    return 1.0 if N < K else 1e-3


# ---- (A) reprojection ---------------------------------------------------------------------------------------------------------------
def _project(intr, lv, R, T, Wc, normalize, dtype):
    """-> D [B,N], and per frame px, py, Z, dprime [B,F,N] in `dtype`"""
    B, H, W = lv["D0"].shape
    stub = np.zeros((B, H, W, 1), dtype)
    a = odense.level_inputs(intr, dict(lv, src=stub, tgt=stub), normalize, dtype)
    D = a["D"]
    if Wc is not None and "Bs" in a:
        D = D + np.matmul(a["Bs"], np.asarray(Wc, dtype).reshape(B, -1, 1))
    R, T = np.asarray(R, dtype), np.asarray(T, dtype)
    F = R.shape[1]
    out = dict(px=[], py=[], Z=[], dp=[])
    for f in range(F):
        Tf = T[:, f].reshape(B, 3, 1)
        w = orc.warp(R[:, f].reshape(B, 3, 3), Tf, a["p"], D, a["fx"], a["fy"], a["ox"], a["oy"])
        X = w["rx"] * D[:, :, 0] + Tf[:, 0]
        Y = w["ry"] * D[:, :, 0] + Tf[:, 1]
        with np.errstate(invalid="ignore", over="ignore"):
            dp = np.sqrt(X * X + Y * Y + w["Z"] * w["Z"]) if normalize else w["Z"]
        out["px"].append(w["px"])
        out["py"].append(w["py"])
        out["Z"].append(w["Z"])
        out["dp"].append(dp)
    return D[:, :, 0], {k: np.stack(v, 1) for k, v in out.items()}


def _valid(g, H, W):
    with np.errstate(invalid="ignore"):
        return (np.isfinite(g["px"]) & np.isfinite(g["py"]) & (g["px"] >= 0) & (g["px"] <= W - 1) & (g["py"] >= 0) & (g["py"] <= H - 1) &
                (g["Z"] > 0) & np.isfinite(g["dp"]) & (g["dp"] > 0))


def reproject(intr, lv, R, T, Wc, normalize, dtype=np.float64):
    """-> dict(depth [B,F,H,W] dtype, index [B,F,H,W] int32, count [B,F,H,W] points landed, ambiguous [B,F,H,W] bool, D [B,N])"""
    B, H, W = lv["D0"].shape
    N = H * W
    D, g = _project(intr, lv, R, T, Wc, normalize, dtype)
    F = g["px"].shape[1]
    ok = _valid(g, H, W)
    depth = np.zeros((B, F, N), dtype)
    index = np.full((B, F, N), -1, np.int32)
    count = np.zeros((B, F, N), np.int64)
    amb = np.zeros((B, F, H, W), bool)
    e = BAND * max(W, H)
    for b in range(B):
        for f in range(F):
            n = np.nonzero(ok[b, f])[0]
            px, py, dp = g["px"][b, f, n], g["py"][b, f, n], g["dp"][b, f, n]
            tex = (np.floor(py + 0.5).astype(np.int64) * W + np.floor(px + 0.5).astype(np.int64))
            order = np.lexsort((n, dp, tex))                       # by texel, then d', then n
            ts, ns, ds = tex[order], n[order], dp[order]
            if n.size:
                first = np.r_[True, ts[1:] != ts[:-1]]
                depth[b, f, ts[first]] = ds[first]
                index[b, f, ts[first]] = ns[first]
                np.add.at(count[b, f], ts, 1)
                second = np.r_[False, (ts[1:] == ts[:-1]) & first[:-1]]  # the runner-up of a texel directly follows its winner
                close = np.abs(ds[second] - ds[np.nonzero(second)[0] - 1]) < DEPTH_TIE * np.abs(ds[second])
                amb[b, f].reshape(-1)[ts[second][close]] = True
            # the band: every point with a finite projection, also one just outside the image
            qx, qy = g["px"][b, f], g["py"][b, f]
            with np.errstate(invalid="ignore"):
                fin = np.isfinite(qx) & np.isfinite(qy) & (qx > -1) & (qx < W) & (qy > -1) & (qy < H)
                near = lambda v: np.abs(v + 0.5 - np.round(v + 0.5)) < e
                edge = lambda v, hi: (np.abs(v) < e) | (np.abs(v - hi) < e)
                frag = fin & (near(qx) | near(qy) | edge(qx, W - 1) | edge(qy, H - 1))
            for x, y in zip(np.round(qx[frag]).astype(int), np.round(qy[frag]).astype(int)):
                amb[b, f, max(y - 1, 0):min(y + 2, H), max(x - 1, 0):min(x + 2, W)] = True
    shape = (B, F, H, W)
    return dict(depth=depth.reshape(shape), index=index.reshape(shape), count=count.reshape(shape), ambiguous=amb, D=D)


def reproject_loop(intr, lv, R, T, Wc, normalize, dtype=np.float64):
    """the same rule as a direct loop over the points (tiny cases) -> depth, index"""
    B, H, W = lv["D0"].shape
    D, g = _project(intr, lv, R, T, Wc, normalize, dtype)
    F = g["px"].shape[1]
    depth = np.zeros((B, F, H, W), dtype)
    index = np.full((B, F, H, W), -1, np.int32)
    for b in range(B):
        for f in range(F):
            for n in range(H * W):
                px, py, Z, dp = (g[k][b, f, n] for k in ("px", "py", "Z", "dp"))
                if not (np.isfinite(px) and np.isfinite(py) and 0 <= px <= W - 1 and 0 <= py <= H - 1 and Z > 0 and np.isfinite(dp) and dp > 0):
                    continue
                x, y = int(np.floor(px + 0.5)), int(np.floor(py + 0.5))
                if index[b, f, y, x] < 0 or (dp, n) < (depth[b, f, y, x], index[b, f, y, x]):
                    depth[b, f, y, x], index[b, f, y, x] = dp, n
    return depth, index


# ---- (B) basis fit ------------------------------------------------------------------------------------------------------------------
def contributing(target, weight):
    w = np.ones_like(target) if weight is None else weight
    with np.errstate(invalid="ignore"):
        return np.isfinite(w) & (w > 0) & np.isfinite(target)


def _solve(G, g, mu):
    """float64 H = G + mu diag(diag G + 1e-5), Wc = H^-1 g; status 1 (Wc = 0) where H has no Cholesky factor"""
    B, K = g.shape
    Wc, status = np.zeros((B, K)), np.zeros(B, np.int32)
    for b in range(B):
        Hm = G[b].astype(np.float64)
        Hm = Hm + mu[b] * np.diag(np.diag(Hm) + 1e-5)
        try:
            if not np.all(np.isfinite(Hm)):
                raise np.linalg.LinAlgError
            L = np.linalg.cholesky(Hm)
            Wc[b] = np.linalg.solve(L.T, np.linalg.solve(L, g[b].astype(np.float64)))
        except np.linalg.LinAlgError:
            status[b] = 1
    return Wc, status


def basis_fit(depth, basis, target, weight=None, damping=None, dtype=np.float64):
    """depth, target, weight [B,N], basis [B,N,K], damping [B] or None -> dict(Wc, normal, rhs, stats, status).  dtype float64: the
    definition; float32: the yardstick (float32 sums, float64 solve)."""
    B, N, K = basis.shape
    ok = contributing(target, weight)
    w = np.where(ok, np.ones_like(target) if weight is None else weight, 0).astype(dtype)
    r = np.where(ok, np.where(ok, target, 0).astype(dtype) - depth.astype(dtype), 0).astype(dtype)
    b = np.where(ok[:, :, None], basis, 0).astype(dtype)
    G = np.matmul((b * w[:, :, None]).transpose(0, 2, 1), b)
    g = np.matmul(b.transpose(0, 2, 1), (w * r)[:, :, None])[:, :, 0]
    stats = np.stack([w.sum(1), (w * r * r).sum(1)], 1)
    mu = np.zeros(B) if damping is None else np.asarray(damping, np.float64).reshape(B)
    Wc, status = _solve(G, g, mu)
    return dict(Wc=Wc, normal=G, rhs=g, stats=stats, status=status)


def fit_case(N, K, seed, B=3):
    """synth.dct_basis on the first N pixels of a virtual image (N >= 768; its sides stay above the basis' highest frequencies) or
    at N random positions of a 32 x 32 one (tiny N), weights uniform in [0.2, 2] with 30 % zeros, a smooth target.  N < K is rank
    deficient by construction: such a case is well posed only with damping (the GPU module uses mu = 1 there)."""
    rs = np.random.RandomState(seed)
    if N >= 768:
        Wv = 48 if N >= 1536 else 32
        n = np.arange(N, dtype=np.float64)
        u, v = n % Wv, n // Wv
        Hv = int(v.max()) + 1
    else:
        Wv = Hv = 32
        u, v = rs.uniform(0, 31, N), rs.uniform(0, 31, N)
    basis = np.repeat(synth.dct_basis(u, v, Wv, Hv, K)[None], B, 0) * rs.uniform(0.8, 1.25, (B, 1, K))
    depth = 2.5 + 0.3 * rs.standard_normal((B, N))
    target = depth + np.matmul(basis, rs.standard_normal((B, K, 1)) * 0.1)[:, :, 0] + 0.01 * rs.standard_normal((B, N))
    weight = rs.uniform(0.2, 2.0, (B, N)) * (rs.uniform(0, 1, (B, N)) >= 0.3)
    f32 = lambda x: np.ascontiguousarray(x, np.float32)
    return dict(depth=f32(depth), basis=f32(basis), target=f32(target), weight=f32(weight), B=B, N=N, K=K)
