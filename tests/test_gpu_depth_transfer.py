"""banet_depth_reproject_f32 (csrc/reproject.hip) and banet_basis_fit_f32 (csrc/basisfit.hip) on the GPU through the C ABI, and
DenseBA.transfer_depth on top of them, against the numpy references of tests/depth_transfer_ref.py.

Reprojection: `index` must equal the float64 reference's on every texel the reference does not mark ambiguous (a projection within
4e-6 max(W, H) of a rounding boundary or of the image border nearby, or two landed depths closer than 1e-5), `depth` within
max(4 x the float32 reference's error on the same case, 2^-20) relative there; at most 2 % of the texels may be ambiguous.
Fit: normal / rhs within 3e-5 of their scale, stats 1e-5, Wc within 1e-4 of max |Wc| -- the float32 yardstick
(float32 sums, float64 solve) is printed next to every error and sits at 1e-6, so a miss is a bug and not rounding.
Shapes: 24 x 32 and 30 x 40 images, N <= 1536 points, three windows."""
import ctypes

import numpy as np
import pytest
import torch

import depth_transfer_ref as dr
import ws_contract as wsc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from banet_amd import _capi
    _capi.lib()
    return torch.device("cuda:0")


def t32(x, dev):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32))).to(dev)


def same_bits(a, b):
    return wsc.bits_equal(torch.from_numpy(np.ascontiguousarray(a)), torch.from_numpy(np.ascontiguousarray(b)))


def offset_view(x, dev):
    """x as a view that starts 4 bytes past a 16-byte boundary, NaN before and after it"""
    flat = torch.full((x.numel() + 1 + 64,), float("nan"), dtype=torch.float32, device=dev)
    view = flat[1:1 + x.numel()].view(x.shape)
    view.copy_(x)
    assert view.data_ptr() % 16 == 4
    return view


# ======================================================================================================================
# reprojection
# ======================================================================================================================
def reproject_gpu(case, dev, Wc="gt", windows=None, frames=None, fill=None, offset_basis=False, ws=None):
    """the case (or some of its windows / one of its frames) through the C entry -> (depth, index) numpy [B,F,H,W]"""
    from banet_amd import _capi as capi
    L = capi.lib()
    idx = list(range(case["B"])) if windows is None else list(windows)
    lvd = case["lv"]
    B, H, W, K = len(idx), lvd["H"], lvd["W"], case["K"]
    R, T = case["R"][idx], case["T"][idx]
    if frames is not None:
        R, T = R[:, frames], T[:, frames]
    F = R.shape[1]
    keep = dict(depth=t32(lvd["D0"][idx].reshape(B, H * W), dev), intr=t32(case["intr"][idx], dev), R=t32(R.reshape(B, F, 9), dev),
                T=t32(T.reshape(B, F, 3), dev))
    keep["basis"] = t32(lvd["basis"][idx].reshape(B, H * W, K), dev) if K > 0 else None
    if offset_basis:
        keep["basis"] = offset_view(keep["basis"], dev)
    wc = case["W_gt"][idx] if isinstance(Wc, str) else Wc
    keep["Wc"] = t32(wc, dev) if (wc is not None and K > 0) else None
    lv = capi.Level()
    lv.B, lv.N, lv.K, lv.H, lv.W, lv.dense = B, H * W, K, H, W, 1
    lv.normalize_rays, lv.scale, lv.pairs = int(case["normalize"]), float(lvd["scale"]), F
    lv.depth, lv.intr = keep["depth"].data_ptr(), keep["intr"].data_ptr()
    lv.basis = keep["basis"].data_ptr() if K > 0 else None
    depth = torch.full((B, F, H, W), -7.0, dtype=torch.float32, device=dev)
    index = torch.full((B, F, H, W), -7, dtype=torch.int32, device=dev)
    out = capi.ReprojectOut()
    out.depth, out.index = depth.data_ptr(), index.data_ptr()
    nb = L.banet_depth_reproject_workspace_bytes(ctypes.byref(lv))
    assert nb == (B * F * H * W * 8 + 255) // 256 * 256
    handle = None
    if ws is None:
        if fill is None:
            ws = capi.workspace(nb, dev)
        else:
            ws, handle = wsc.guarded_workspace(nb, dev, fill)
    capi.check(L.banet_depth_reproject_f32(ctypes.byref(lv), capi.ptr(keep["R"]), capi.ptr(keep["T"]), capi.ptr(keep["Wc"]),
                                           ctypes.byref(out), ctypes.c_void_p(ws.data_ptr()), ws.numel(), capi.stream()))
    torch.cuda.synchronize()
    if handle is not None:
        wsc.assert_guards_intact(handle)
    return depth.cpu().numpy(), index.cpu().numpy()


_REF = {}


def reference(key, case, Wc="gt"):
    """the float64 reference and the float32 one of a case, computed once per module"""
    if key not in _REF:
        wc = case["W_gt"] if isinstance(Wc, str) else Wc
        args = (case["intr"], case["lv"], case["R"], case["T"], wc if case["K"] > 0 else None, case["normalize"])
        _REF[key] = (dr.reproject(*args, np.float64), dr.reproject(*args, np.float32))
    return _REF[key]


def check_against_reference(name, got, r64, r32, cap=0.02):
    depth, index = got
    clear = ~r64["ambiguous"]
    share = r64["ambiguous"].mean()
    hit = clear & (r64["index"] >= 0)
    rel = lambda d: (np.abs(d.astype(np.float64) - r64["depth"])[hit] / r64["depth"][hit]).max() if hit.any() else 0.0
    yard = rel(r32["depth"]) if np.array_equal(r32["index"][hit], r64["index"][hit]) else float("nan")
    wrong = int((index[clear] != r64["index"][clear]).sum())
    print("%s: ambiguous share %.4f, wrong winners %d of %d, depth error %.2e (float32 reference %.2e), covered %.3f"
          % (name, share, wrong, int(clear.sum()), rel(depth) if wrong == 0 else float("nan"), yard, (r64["index"] >= 0).mean()))
    assert share <= cap
    assert wrong == 0
    assert np.array_equal(depth[clear & (r64["index"] < 0)], np.zeros(int((clear & (r64["index"] < 0)).sum()), np.float32))
    assert rel(depth) <= max(4 * yard, 2.0 ** -20)
    assert np.array_equal(depth == 0, index < 0) and index.min() >= -1 and index.max() < index.shape[2] * index.shape[3]


@pytest.mark.parametrize("normalize", [1, 0])
def test_identity_pose_gives_every_interior_pixel_back(dev, normalize):
    case = dr.pair_case(24, 32, 8, 1, bool(normalize), w_gt=(0, 0, 0), t_gt=(0, 0, 0), B=2)
    depth, index = reproject_gpu(case, dev)
    r64, _ = reference(("identity", normalize), case)
    own = np.arange(24 * 32).reshape(24, 32)
    # the rim is left out: in float32 a rim pixel projects a few ulps outside the image
    assert np.array_equal(index[:, 0, 1:-1, 1:-1], np.broadcast_to(own[1:-1, 1:-1], (2, 22, 30)))
    D = r64["D"].reshape(2, 24, 32)[:, 1:-1, 1:-1]
    err = (np.abs(depth[:, 0, 1:-1, 1:-1] - D) / D).max()
    print("identity, normalize_rays %d: depth error %.2e" % (normalize, err))
    assert err <= 2.0 ** -20


@pytest.mark.parametrize("normalize", [1, 0])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_generic_poses_against_the_float64_reference(dev, which, normalize):
    case = dr.generic_case(dr.GENERIC[which], bool(normalize))
    r64, r32 = reference(("generic", which, normalize), case)
    check_against_reference("generic %d normalize_rays %d" % (which, normalize), reproject_gpu(case, dev), r64, r32)


def occlusion_case(normalize):
    case = dr.pair_case(24, 32, 0, 1, normalize, w_gt=(0, 0, 0), t_gt=(0.3, 0.0, 0.0), B=2)
    D0 = np.full((2, 24, 32), 3.0, np.float32)
    D0[0, 6:18, 10:20] = 1.5                              # a foreground step; it moves twice as far as the background
    D0[1, 4:20, 4:12] = 1.5
    case["lv"]["D0"] = D0
    return case


@pytest.mark.parametrize("normalize", [1, 0])
def test_occlusion_the_nearest_surface_wins(dev, normalize):
    case = occlusion_case(bool(normalize))
    r64, r32 = reference(("occlusion", normalize), case)
    contested = (r64["count"] >= 2) & ~r64["ambiguous"]
    print("occlusion: %d texels receive two points or more" % contested.sum())
    assert contested.sum() >= 20
    got = reproject_gpu(case, dev)
    check_against_reference("occlusion normalize_rays %d" % normalize, got, r64, r32, cap=1.0)   # (py = v exactly: the rim rows are border cases)
    assert np.array_equal(got[1][contested], r64["index"][contested])
    if not normalize:
        assert np.all(got[0][contested][r64["depth"][contested] < 2] == np.float32(1.5))


def test_nothing_lands_behind_the_camera_and_nan_depths_land_nowhere(dev):
    case = dr.generic_case(dr.GENERIC[0], True)
    behind = dict(case, T=case["T"] + np.array([0.0, 0.0, -10.0]))
    depth, index = reproject_gpu(behind, dev)
    assert np.all(index == -1) and np.all(depth == 0)
    clean = reproject_gpu(case, dev)
    holes = np.zeros((2, 24 * 32), bool)
    holes[:, 40:700:7] = True
    bad = dict(case, lv=dict(case["lv"], D0=np.where(holes.reshape(2, 24, 32), np.nan, case["lv"]["D0"]).astype(np.float32)))
    depth, index = reproject_gpu(bad, dev)
    n_of = np.where(index >= 0, index, 0)
    assert not np.any(np.take_along_axis(holes, n_of.reshape(2, -1), 1).reshape(index.shape) & (index >= 0))
    assert np.all(np.isfinite(depth))
    # a texel whose winner is not one of the holes keeps its bits
    cn = np.where(clean[1] >= 0, clean[1], 0)
    keep = ~np.take_along_axis(holes, cn.reshape(2, -1), 1).reshape(index.shape)
    assert np.array_equal(index[keep], clean[1][keep]) and same_bits(depth[keep], clean[0][keep])
    r64, r32 = reference("nan", bad)
    check_against_reference("NaN depths", (depth, index), r64, r32)


def test_three_target_frames_equal_three_single_frame_calls(dev):
    case = dr.window_case(24, 32, 8, 4, 3, B=2)
    depth, index = reproject_gpu(case, dev)
    assert depth.shape == (2, 3, 24, 32)
    for f in range(3):
        d1, i1 = reproject_gpu(case, dev, frames=[f])
        assert same_bits(d1[:, 0], depth[:, f]) and np.array_equal(i1[:, 0], index[:, f]), f
    r64, r32 = reference("window", case)
    check_against_reference("three frames", (depth, index), r64, r32)


def test_a_level_of_scale_two(dev):
    case = dr.pair_case(24, 32, 8, 1, True, w_gt=dr.GENERIC[0][2], t_gt=dr.GENERIC[0][3], B=2, scale=2)
    assert case["lv"]["D0"].shape == (2, 12, 16) and case["lv"]["scale"] == 2
    r64, r32 = reference("scale2", case)
    check_against_reference("scale 2", reproject_gpu(case, dev), r64, r32)


@pytest.mark.parametrize("K", [0, 5, 128, 130])
def test_k_and_alignment(dev, K):
    case = dr.pair_case(24, 32, K, 1, True, w_gt=dr.GENERIC[0][2], t_gt=dr.GENERIC[0][3], B=2)
    r64, r32 = reference(("K", K), case)
    got = reproject_gpu(case, dev)
    check_against_reference("K = %d" % K, got, r64, r32)
    if K > 0:
        off = reproject_gpu(case, dev, offset_basis=True, fill="nan")
        assert same_bits(off[0], got[0]) and np.array_equal(off[1], got[1])
        none = reproject_gpu(case, dev, Wc=None)           # Wc == NULL: D = depth
        zero = reproject_gpu(dict(case, K=0), dev)
        assert same_bits(none[0], zero[0]) and np.array_equal(none[1], zero[1])


def test_reprojection_is_reproducible(dev):
    case = dr.generic_case(dr.GENERIC[1], True, K=128, B=3)
    three = reproject_gpu(case, dev)
    again = reproject_gpu(case, dev)
    assert same_bits(again[0], three[0]) and np.array_equal(again[1], three[1])
    for b in range(3):
        one = reproject_gpu(case, dev, windows=[b])
        assert same_bits(one[0][0], three[0][b]) and np.array_equal(one[1][0], three[1][b]), b
    for fill in ("zero", "nan", "one"):
        g = reproject_gpu(case, dev, fill=fill)
        assert same_bits(g[0], three[0]) and np.array_equal(g[1], three[1]), fill
    # another call's leftovers: one arena, the same bytes used by a call of another shape first
    from banet_amd import _capi as capi
    stale = capi.workspace(3 * 24 * 32 * 8, dev)
    reproject_gpu(occlusion_case(True), dev, ws=stale)
    g = reproject_gpu(case, dev, ws=stale)
    assert same_bits(g[0], three[0]) and np.array_equal(g[1], three[1])


# ======================================================================================================================
# fit
# ======================================================================================================================
FIT_NAMES = ("Wc", "normal", "rhs", "stats", "status")


def fit_gpu(fc, dev, damping=None, windows=None, names=FIT_NAMES, fill=None, offset_basis=False, weight="w", ws=None):
    """the case (or some of its windows) through the C entry -> dict of numpy arrays (the outputs named in `names`)"""
    from banet_amd import _capi as capi
    L = capi.lib()
    idx = list(range(fc["B"])) if windows is None else list(windows)
    B, N, K = len(idx), fc["N"], fc["K"]
    depth, basis, target = t32(fc["depth"][idx], dev), t32(fc["basis"][idx], dev), t32(fc["target"][idx], dev)
    if offset_basis:
        basis = offset_view(basis, dev)
    w = fc["weight"] if isinstance(weight, str) else weight
    w = t32(w[idx], dev) if w is not None else None
    mu = t32(np.asarray(damping, np.float32).reshape(-1)[idx], dev) if damping is not None else None
    lv = capi.Level()
    lv.B, lv.N, lv.K = B, N, K
    lv.depth, lv.basis = depth.data_ptr(), basis.data_ptr()
    shapes = dict(Wc=(B, K), normal=(B, K, K), rhs=(B, K), stats=(B, 2), status=(B,))
    outs = {k: torch.full(shapes[k], -7, dtype=torch.int32 if k == "status" else torch.float32, device=dev) for k in names}
    c = capi.BasisFitOut()
    for k, v in outs.items():
        setattr(c, k, v.data_ptr())
    nb = L.banet_basis_fit_workspace_bytes(ctypes.byref(lv))
    assert nb > 0
    handle = None
    if ws is None:
        if fill is None:
            ws = capi.workspace(nb, dev)
        else:
            ws, handle = wsc.guarded_workspace(nb, dev, fill)
            assert ws.numel() == nb
    capi.check(L.banet_basis_fit_f32(ctypes.byref(lv), capi.ptr(target), capi.ptr(w), capi.ptr(mu), ctypes.byref(c),
                                     ctypes.c_void_p(ws.data_ptr()), ws.numel(), capi.stream()))
    torch.cuda.synchronize()
    if handle is not None:
        wsc.assert_guards_intact(handle)
    return {k: v.cpu().numpy() for k, v in outs.items()}


def fit_refs(fc, damping, weight="w"):
    w = fc["weight"] if isinstance(weight, str) else weight
    return (dr.basis_fit(fc["depth"], fc["basis"], fc["target"], w, damping, np.float64),
            dr.basis_fit(fc["depth"], fc["basis"], fc["target"], w, damping, np.float32))


def fit_errors(got, r64):
    scale = lambda x: np.maximum(np.abs(x).reshape(x.shape[0], -1).max(1), 1e-30).reshape((-1,) + (1,) * (x.ndim - 1))
    e = {k: float((np.abs(got[k].astype(np.float64) - r64[k]) / scale(r64[k])).max()) for k in ("Wc", "normal", "rhs")}
    e["stats"] = float((np.abs(got["stats"].astype(np.float64) - r64["stats"]) / np.maximum(np.abs(r64["stats"]), 1e-30)).max())
    return e


def check_fit(name, got, r64, r32):
    err, yard = fit_errors(got, r64), fit_errors(r32, r64)
    print("%s: " % name + "  ".join("%s %.2e (yardstick %.2e)" % (k, err[k], yard[k]) for k in ("Wc", "normal", "rhs", "stats")))
    assert list(got["status"]) == list(r64["status"])
    assert err["normal"] <= 3e-5 and err["rhs"] <= 3e-5 and err["stats"] <= 1e-5
    assert np.array_equal(got["normal"], got["normal"].transpose(0, 2, 1))
    assert err["Wc"] <= 1e-4
    return err, yard


@pytest.mark.parametrize("N,K", dr.FIT_SHAPES)
def test_fit_shapes(dev, N, K):
    fc = dr.fit_case(N, K, 7)
    mu = np.full(3, dr.fit_damping(N, K), np.float32)
    r64, r32 = fit_refs(fc, mu)
    check_fit("fit N %d K %d" % (N, K), fit_gpu(fc, dev, mu), r64, r32)


@pytest.mark.parametrize("N,K", [(768, 32), (775, 130)])
def test_exact_recovery(dev, N, K):
    fc = dr.fit_case(N, K, 3)
    Wstar = np.random.RandomState(5).standard_normal((3, K)) * 0.1
    fc["target"] = (fc["depth"].astype(np.float64) + np.matmul(fc["basis"].astype(np.float64), Wstar[:, :, None])[:, :, 0]).astype(np.float32)
    got = fit_gpu(fc, dev, None, weight=None)               # w = 1, mu = 0
    err = (np.abs(got["Wc"] - Wstar).max(1) / np.abs(Wstar).max(1)).max()
    print("exact recovery N %d K %d: %.2e" % (N, K, err))
    assert list(got["status"]) == [0, 0, 0] and err <= 1e-4
    r2 = ((fc["target"].astype(np.float64) - fc["depth"].astype(np.float64)) ** 2).sum(1)
    assert np.array_equal(got["stats"][:, 0], np.full(3, N, np.float32)) and np.allclose(got["stats"][:, 1], r2, rtol=1e-5)


@pytest.mark.parametrize("N,K", [(768, 32), (1536, 256)])
def test_column_scale_ladder(dev, N, K):
    fc = dr.fit_case(N, K, 9)
    s = 2.0 ** np.random.RandomState(K).randint(-8, 9, K)
    s[:2] = (2.0 ** -8, 2.0 ** 8)
    fc["basis"] = (fc["basis"] * s.astype(np.float32)).astype(np.float32)            # exact: powers of two
    mu = np.full(3, 1e-3, np.float32)
    r64, r32 = fit_refs(fc, mu)
    got = fit_gpu(fc, dev, mu)
    scaled = lambda Wc: Wc.astype(np.float64) * s
    top = np.abs(scaled(r64["Wc"])).max(1, keepdims=True)
    err = np.abs(scaled(got["Wc"]) - scaled(r64["Wc"])) / top
    yard = np.abs(scaled(r32["Wc"]) - scaled(r64["Wc"])) / top
    print("ladder N %d K %d: error %.2e, yardstick %.2e" % (N, K, err.max(), yard.max()))
    assert list(got["status"]) == [0, 0, 0]
    assert err.max() <= max(4 * yard.max(), K * 2.0 ** -24)


def test_degenerate_and_non_finite_inputs(dev):
    fc = dr.fit_case(768, 32, 13)
    full = fit_gpu(fc, dev, None)
    dead = dict(fc, weight=fc["weight"].copy())
    dead["weight"][1] = 0
    got = fit_gpu(dead, dev, None)                          # window 1: nothing contributes, mu = 0
    assert list(got["status"]) == [0, 1, 0] and np.all(got["Wc"][1] == 0) and np.all(got["normal"][1] == 0)
    for k in FIT_NAMES:
        assert same_bits(got[k][[0, 2]], full[k][[0, 2]]), k
    alone = fit_gpu(dead, dev, None, windows=[0, 2])
    for k in FIT_NAMES:
        assert same_bits(alone[k], got[k][[0, 2]]), k
    got = fit_gpu(dead, dev, np.array([0, 1e-3, 0], np.float32))      # the same window damped: H = mu 1e-5 I, g = 0
    assert list(got["status"]) == [0, 0, 0] and np.all(got["Wc"][1] == 0)
    # NaN targets under w = 0 are ignored
    masked = dict(fc, target=np.where(fc["weight"] == 0, np.nan, fc["target"]).astype(np.float32))
    got = fit_gpu(masked, dev, None)
    for k in FIT_NAMES:
        assert same_bits(got[k], full[k]), k
    # a NaN / inf target or a non-finite weight under w > 0 is excluded: the same bits as giving the point w = 0
    bad, zeroed = dict(fc, target=fc["target"].copy(), weight=fc["weight"].copy()), dict(fc, weight=fc["weight"].copy())
    pos = np.nonzero(fc["weight"][0] > 0)[0][:6]
    bad["target"][0, pos[:2]] = np.nan
    bad["target"][0, pos[2:4]] = np.inf
    bad["weight"][0, pos[4]] = np.inf
    bad["weight"][0, pos[5]] = np.nan
    zeroed["weight"][0, pos] = 0
    got, want = fit_gpu(bad, dev, None), fit_gpu(zeroed, dev, None)
    for k in FIT_NAMES:
        assert same_bits(got[k], want[k]), k
    r64, r32 = fit_refs(bad, None)
    check_fit("non-finite inputs", got, r64, r32)


@pytest.mark.parametrize("K", [199, 200])
def test_the_last_matrix_in_lds_and_the_first_in_the_workspace(dev, K):
    from banet_amd import _capi as capi
    fc = dr.fit_case(1536, K, 17)
    lv = capi.Level()
    lv.B, lv.N, lv.K = 3, 1536, K
    up = lambda n: (n + 255) // 256 * 256
    NR = (K + 31) // 32
    small = up(3 * 6 * (NR * (NR + 1) // 2 * 1024 + NR * 32 + 32) * 4) + up(3 * K * K * 4) + up(3 * K * 4)
    nb = capi.lib().banet_basis_fit_workspace_bytes(ctypes.byref(lv))
    assert (nb > small) == (K == 200) and nb >= small
    mu = np.full(3, 1e-3, np.float32)
    r64, r32 = fit_refs(fc, mu)
    check_fit("fit K %d" % K, fit_gpu(fc, dev, mu, fill="nan"), r64, r32)


@pytest.mark.parametrize("N,K", [(775, 130), (1536, 256), (768, 32)])
def test_fit_is_reproducible(dev, N, K):
    fc = dr.fit_case(N, K, 21)
    mu = np.array([1e-3, 0.0, 0.1], np.float32)
    three = fit_gpu(fc, dev, mu)
    again = fit_gpu(fc, dev, mu)
    for k in FIT_NAMES:
        assert same_bits(again[k], three[k]), k
    for b in range(3):
        one = fit_gpu(fc, dev, mu, windows=[b])
        for k in FIT_NAMES:
            assert same_bits(one[k][0], three[k][b]), (k, b)
    for names in (("Wc", "status"), ("Wc", "status", "normal"), ("Wc", "status", "rhs", "stats")):
        part = fit_gpu(fc, dev, mu, names=names)
        for k in names:
            assert same_bits(part[k], three[k]), (names, k)
    off = fit_gpu(fc, dev, mu, offset_basis=True)           # a basis that is only 4-byte aligned
    for k in FIT_NAMES:
        assert same_bits(off[k], three[k]), k
    for fill in ("zero", "nan", "one"):
        g = fit_gpu(fc, dev, mu, fill=fill)
        for k in FIT_NAMES:
            assert same_bits(g[k], three[k]), (fill, k)
    from banet_amd import _capi as capi
    other = dr.fit_case(768, 128, 2)                        # another call's leftovers in the same bytes
    stale = capi.workspace(64 << 20, dev)
    fit_gpu(other, dev, None, ws=stale)
    g = fit_gpu(fc, dev, mu, ws=stale)
    for k in FIT_NAMES:
        assert same_bits(g[k], three[k]), k


def test_ops_basis_fit_and_depth_reproject(dev):
    from banet_amd import ops
    fc = dr.fit_case(768, 32, 7)
    raw = fit_gpu(fc, dev, np.full(3, 1e-3, np.float32))
    f = ops.basis_fit(t32(fc["depth"], dev), t32(fc["basis"], dev), t32(fc["target"], dev), weight=t32(fc["weight"], dev), damping=1e-3,
                      want=ops.BASIS_FIT_OUTPUTS)
    for k in FIT_NAMES:
        assert same_bits(getattr(f, k).cpu().numpy(), raw[k]), k
    g = ops.basis_fit(t32(fc["depth"], dev), t32(fc["basis"], dev), t32(fc["target"], dev), weight=t32(fc["weight"], dev), damping=1e-3)
    assert g.normal is None and g.rhs is None and g.stats is None and same_bits(g.Wc.cpu().numpy(), raw["Wc"])
    with pytest.raises(ops.capi.BanetError):
        ops.basis_fit(t32(fc["depth"], dev), t32(fc["basis"], dev), t32(fc["target"], dev), want=("nope",))
    with pytest.raises(ops.capi.BanetError):
        ops.basis_fit(torch.from_numpy(fc["depth"]), t32(fc["basis"], dev), t32(fc["target"], dev))      # a CPU tensor


# ======================================================================================================================
# end to end
# ======================================================================================================================
def test_dense_ba_transfer_depth(dev):
    from banet_amd import dense as bdense
    from oracle import banet_oracle as orc, dense as odense, synth
    B, C, K, Kn, H, W = 2, 32, 32, 32, 24, 32
    poses = (dr.GENERIC[0], dr.GENERIC[1])
    scenes = [synth.make_pair_scene(H, W, C, K, [1], poses[b][4], normalize_rays=True, w_gt=poses[b][2], t_gt=poses[b][3]) for b in range(B)]
    intr, levels = odense.batch_scene(scenes)
    lv = levels[0]
    tl = [bdense.DenseLevel(lv["scale"], *(torch.from_numpy(lv[k]).to(dev) for k in ("src", "tgt", "D0", "basis")))]
    ba = bdense.DenseBA(torch.from_numpy(intr).to(dev), tl, [orc.he_normal_mlp_weights(C, 5)], "bundle", 1000.0)
    R = np.stack([s["R_gt"] for s in scenes])
    T = np.stack([s["T_gt"] for s in scenes])
    Wgt = np.stack([s["W_gt"] for s in scenes])
    st = ba.new_state(t32(R, dev), t32(T.reshape(B, 3, 1), dev), t32(Wgt.reshape(B, K, 1), dev))
    # the new key frame: a constant initial depth and a dct basis on the target frame's grid
    vv, uu = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    nb = np.repeat(synth.dct_basis(uu, vv, W, H, Kn)[None], B, 0).astype(np.float32)
    nd = np.full((B, H, W), 2.8, np.float32)
    var = np.random.RandomState(3).uniform(0.5, 2.0, (B, H, W)).astype(np.float32) * 1e-2
    r64 = dr.reproject(intr, dict(scale=1, H=H, W=W, D0=lv["D0"], basis=lv["basis"]), R[:, None], T[:, None], Wgt, True)
    print("end to end: ambiguous texels %d, covered %.3f" % (r64["ambiguous"].sum(), (r64["index"] >= 0).mean()))
    ref_index, ref_depth = r64["index"][:, 0], r64["depth"][:, 0]
    for depth_var in (None, var):
        tr = ba.transfer_depth(0, st, t32(nd, dev), t32(nb, dev), frame=0, depth_var=t32(depth_var, dev), damping=1e-3)
        assert tr.Wc.shape == (B, Kn) and tr.depth_map.shape == (B, H, W) and tr.index.dtype == torch.int32
        index = tr.index.cpu().numpy()
        assert np.array_equal(index, ref_index)
        assert list(tr.covered.cpu().numpy()) == list((ref_index >= 0).reshape(B, -1).sum(1))
        assert list(tr.status.cpu().numpy()) == [0] * B
        covered = ref_index >= 0
        w = covered.astype(np.float64)
        if depth_var is not None:
            gathered = np.take_along_axis(depth_var.reshape(B, -1).astype(np.float64), np.maximum(ref_index, 0).reshape(B, -1), 1)
            w = w / (gathered.reshape(B, H, W) + bdense.DenseBA.transfer_eps)
        want = dr.basis_fit(nd.reshape(B, -1), nb.reshape(B, H * W, Kn), ref_depth.reshape(B, -1), w.reshape(B, -1), np.full(B, 1e-3))
        got = tr.Wc.cpu().numpy().astype(np.float64)
        err = (np.abs(got - want["Wc"]).max(1) / np.abs(want["Wc"]).max(1)).max()
        print("end to end, depth_var %s: Wc error %.2e" % ("given" if depth_var is not None else "none", err))
        assert err <= 1e-4
        fitted = nd.astype(np.float64) + np.matmul(nb.astype(np.float64).reshape(B, H * W, Kn), got[:, :, None]).reshape(B, H, W)
        rms = lambda x: np.sqrt(np.mean((x[covered] - ref_depth[covered]) ** 2))
        print("            rms to the true target-frame depth: %.4f before, %.4f after" % (rms(nd.astype(np.float64)), rms(fitted)))
        assert rms(fitted) < rms(nd.astype(np.float64))
    with pytest.raises(bdense.ops.capi.BanetError):
        ba.transfer_depth(0, st, torch.from_numpy(nd), torch.from_numpy(nb))                 # CPU tensors
