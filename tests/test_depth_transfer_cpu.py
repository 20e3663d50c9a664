"""banet_depth_reproject_f32 / banet_basis_fit_f32 on the host (include/banet_hip.h (3e)) and the references of
tests/depth_transfer_ref.py.  No GPU: every call here is refused by the host-side checks before anything could be launched (fake
host pointers are compared with NULL and never dereferenced)."""
import ctypes
import os
import re

import numpy as np
import pytest

import depth_transfer_ref as dr

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
os.environ.setdefault("BANET_NUM_CUS", "256")
OK, ERR_INVALID_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED, ERR_LAUNCH = 0, -1, -2, -3, -4
SYMBOLS = ("banet_depth_reproject_workspace_bytes", "banet_depth_reproject_f32", "banet_basis_fit_workspace_bytes", "banet_basis_fit_f32")


@pytest.fixture(scope="module")
def capi():
    from banet_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _capi


class Host:
    """fake host pointers (checked for NULL, never dereferenced) and an aligned fake workspace address"""

    def __init__(self):
        self.host = (ctypes.c_float * 64)()
        self.p = ctypes.cast(self.host, ctypes.c_void_p).value
        self.arena = (ctypes.c_char * 512)()
        self.base = (ctypes.addressof(self.arena) + 255) & ~255


class Reproject(Host):
    def __init__(self, capi, B=2, H=24, W=32, K=8, pairs=1, dense=1):
        Host.__init__(self)
        self.L = capi.lib()
        self.lv = capi.Level()
        lv = self.lv
        lv.B, lv.N, lv.K, lv.H, lv.W, lv.dense, lv.normalize_rays, lv.scale, lv.pairs = B, H * W, K, H, W, dense, 1, 1.0, pairs
        lv.depth = lv.intr = lv.basis = self.p
        self.out = capi.ReprojectOut()
        self.out.depth = self.out.index = self.p

    def query(self):
        return self.L.banet_depth_reproject_workspace_bytes(ctypes.byref(self.lv))

    def __call__(self, lv="lv", R="p", T="p", Wc="p", out="out", ws="base", nbytes=None):
        pick = lambda v: self.p if v == "p" else v
        return self.L.banet_depth_reproject_f32(ctypes.byref(self.lv) if lv == "lv" else lv, pick(R), pick(T), pick(Wc),
                                                ctypes.byref(self.out) if out == "out" else out, self.base if ws == "base" else ws,
                                                self.query() if nbytes is None else nbytes, None)


class Fit(Host):
    def __init__(self, capi, B=3, N=200, K=32):
        Host.__init__(self)
        self.L = capi.lib()
        self.lv = capi.Level()
        self.lv.B, self.lv.N, self.lv.K = B, N, K              # a bare level: nothing else is read
        self.lv.depth = self.lv.basis = self.p
        self.out = capi.BasisFitOut()
        self.out.Wc = self.out.normal = self.out.rhs = self.out.stats = self.out.status = self.p

    def query(self):
        return self.L.banet_basis_fit_workspace_bytes(ctypes.byref(self.lv))

    def __call__(self, lv="lv", target="p", out="out", ws="base", nbytes=None):
        return self.L.banet_basis_fit_f32(ctypes.byref(self.lv) if lv == "lv" else lv, self.p if target == "p" else target, None, None,
                                          ctypes.byref(self.out) if out == "out" else out, self.base if ws == "base" else ws,
                                          self.query() if nbytes is None else nbytes, None)


# ---- linkage ----------------------------------------------------------------------------------------------------------------------
def test_the_library_exports_the_symbols_and_capi_binds_them(capi):
    L = ctypes.CDLL(capi.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(L, name), name
        assert name in capi.EXPORTS
    assert capi.lib().banet_version() == 150              # unchanged: the entries are detected by their symbols
    assert [n for n, _ in capi.ReprojectOut._fields_] == ["depth", "index"]
    assert [n for n, _ in capi.BasisFitOut._fields_] == ["Wc", "normal", "rhs", "stats", "status"]
    header = open(os.path.join(ROOT, "include", "banet_hip.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
    assert "ws_bytes" not in header[header.index("(3e)"):header.index("/* (4)")]      # the (3c) / (3d) parameter name


# ---- banet_depth_reproject_f32 ------------------------------------------------------------------------------------------------------
def test_reproject_null_and_shape_errors_are_decided_on_the_host(capi):
    c = Reproject(capi)
    assert c(lv=None) == ERR_INVALID_ARG
    assert c(R=None) == ERR_INVALID_ARG and c(T=None) == ERR_INVALID_ARG and c(out=None) == ERR_INVALID_ARG
    for field in ("depth", "index"):
        c = Reproject(capi)
        setattr(c.out, field, None)
        assert c() == ERR_INVALID_ARG, field
    for field in ("depth", "intr", "basis"):
        c = Reproject(capi)
        setattr(c.lv, field, None)
        assert c() == ERR_INVALID_ARG, field
    c = Reproject(capi)
    c.lv.basis = None                                     # Wc == NULL: D = depth, the basis is not needed
    assert c(Wc=None, ws=None) == ERR_WORKSPACE
    c = Reproject(capi, K=0)
    c.lv.basis = None
    assert c(ws=None) == ERR_WORKSPACE
    for B, H, W in ((0, 24, 32), (2, 0, 32), (2, 24, 0)):
        c = Reproject(capi, B=B, H=H, W=W)
        assert c.query() == 0 and c(nbytes=1 << 20) == ERR_INVALID_ARG
    c = Reproject(capi)
    c.lv.N = 24 * 32 - 1                                  # N != H W
    assert c.query() == 0 and c(nbytes=1 << 20) == ERR_INVALID_ARG
    c = Reproject(capi)
    c.lv.scale = 0.0
    assert c.query() == 0 and c(nbytes=1 << 20) == ERR_INVALID_ARG
    c = Reproject(capi, dense=0)                          # sparse points have no pixel grid to land on
    assert c.query() == 0 and c(nbytes=1 << 20) == ERR_UNSUPPORTED
    assert capi.lib().banet_depth_reproject_workspace_bytes(None) == 0


def test_reproject_workspace_query_and_refusals(capi):
    up = lambda n: (n + 255) // 256 * 256
    for B, H, W, K, pairs in ((2, 24, 32, 8, 1), (1, 30, 40, 0, 0), (3, 12, 16, 130, 3), (1, 1, 1, 5, 1), (2, 37, 53, 128, 7)):
        c = Reproject(capi, B, H, W, K, pairs)
        nb = c.query()
        assert nb == up(B * max(pairs, 1) * H * W * 8) and nb > 0 and nb % 256 == 0
        assert c(nbytes=nb - 1) == ERR_WORKSPACE
        assert c(ws=c.base + 4) == ERR_WORKSPACE
        assert c(ws=None) == ERR_WORKSPACE


# ---- banet_basis_fit_f32 ------------------------------------------------------------------------------------------------------------
def test_fit_null_and_shape_errors_are_decided_on_the_host(capi):
    c = Fit(capi)
    assert c(lv=None) == ERR_INVALID_ARG and c(target=None) == ERR_INVALID_ARG and c(out=None) == ERR_INVALID_ARG
    for field in ("Wc", "status"):
        c = Fit(capi)
        setattr(c.out, field, None)
        assert c() == ERR_INVALID_ARG, field
    for field in ("depth", "basis"):
        c = Fit(capi)
        setattr(c.lv, field, None)
        assert c() == ERR_INVALID_ARG, field
    c = Fit(capi)
    c.out.normal = c.out.rhs = c.out.stats = None         # the optional outputs: accepted, refused later by the workspace
    assert c(ws=None) == ERR_WORKSPACE
    for B in (0, -1):
        c = Fit(capi, B=B)
        assert c.query() == 0 and c(nbytes=1 << 20) == ERR_INVALID_ARG
    for N, K in ((200, 0), (200, 257), (0, 32), (200, -1)):
        c = Fit(capi, N=N, K=K)
        assert c.query() == 0 and c(nbytes=1 << 30) == ERR_UNSUPPORTED, (N, K)
    assert Fit(capi, K=257).query() == 0
    assert Fit(capi, K=256).query() > 0 and Fit(capi, K=1, N=1).query() > 0
    assert capi.lib().banet_basis_fit_workspace_bytes(None) == 0


def test_fit_workspace_query_and_refusals(capi):
    up = lambda n: (n + 255) // 256 * 256
    for B, N, K in ((3, 200, 32), (1, 1, 1), (3, 768, 5), (2, 775, 130), (3, 1536, 256), (2, 4801, 199), (2, 4801, 200), (32, 307200, 128)):
        c = Fit(capi, B, N, K)
        nb = c.query()
        assert nb > 0 and nb % 256 == 0
        # the layout: partial rows, G, g, and the packed triangle in doubles where it does not fit the LDS (K >= 200)
        NR = (K + 31) // 32
        rows = min((N + 255) // 256, 64)
        chunk = (-(-N // rows) + 1) // 2 * 2
        rows = -(-N // chunk)
        pstride = NR * (NR + 1) // 2 * 1024 + NR * 32 + 32
        big = up(B * (K * (K + 1) // 2) * 8) if K >= 200 else 0
        assert nb == up(B * rows * pstride * 4) + up(B * K * K * 4) + up(B * K * 4) + big, (B, N, K)
        assert c(nbytes=nb - 1) == ERR_WORKSPACE
        assert c(ws=c.base + 4) == ERR_WORKSPACE
        assert c(ws=None) == ERR_WORKSPACE
    # the number of partial rows depends on N alone: the query is linear in B
    assert Fit(capi, 4, 5000, 64).query() == 4 * Fit(capi, 1, 5000, 64).query()


def test_python_entries_refuse_cpu_tensors(capi):
    import torch
    from banet_amd import ops
    with pytest.raises(capi.BanetError):
        ops.basis_fit(torch.zeros(2, 10), torch.zeros(2, 10, 3), torch.zeros(2, 10))
    holder = type("Bare", (), {})()
    holder.c = Reproject(capi).lv
    with pytest.raises(capi.BanetError):
        ops.depth_reproject(holder, torch.eye(3).repeat(2, 1, 1), torch.zeros(2, 3, 1))


# ---- the references -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [True, False])
def test_reprojection_reference_equals_a_direct_loop(normalize):
    c = dr.pair_case(6, 8, 3, 5, normalize, w_gt=(0.02, -0.03, 0.01), t_gt=(0.3, -0.02, 0.04), B=2)
    for dtype in (np.float64, np.float32):
        r = dr.reproject(c["intr"], c["lv"], c["R"], c["T"], c["W_gt"], normalize, dtype)
        d, i = dr.reproject_loop(c["intr"], c["lv"], c["R"], c["T"], c["W_gt"], normalize, dtype)
        assert np.array_equal(i, r["index"]) and np.array_equal(d, r["depth"])
        assert r["depth"].dtype == dtype and (r["index"] >= 0).sum() == (r["count"] > 0).sum() > 10
        assert np.array_equal(r["depth"] == 0, r["index"] < 0)
    w = dr.window_case(6, 8, 3, 4, 2)
    r = dr.reproject(w["intr"], w["lv"], w["R"], w["T"], w["W_gt"], True)
    d, i = dr.reproject_loop(w["intr"], w["lv"], w["R"], w["T"], w["W_gt"], True)
    assert r["index"].shape == (1, 2, 6, 8) and np.array_equal(i, r["index"]) and np.array_equal(d, r["depth"])


def test_reprojection_reference_at_the_identity_is_the_depth_map_itself():
    for normalize in (True, False):
        c = dr.pair_case(24, 32, 8, 1, normalize, w_gt=(0, 0, 0), t_gt=(0, 0, 0), B=2)
        r = dr.reproject(c["intr"], c["lv"], c["R"], c["T"], c["W_gt"], normalize)
        own = np.arange(24 * 32).reshape(24, 32)
        inner = (slice(None), 0, slice(1, -1), slice(1, -1))
        assert np.array_equal(r["index"][inner], np.broadcast_to(own[1:-1, 1:-1], (2, 22, 30)))
        assert np.allclose(r["depth"][inner], r["D"].reshape(2, 24, 32)[:, 1:-1, 1:-1], rtol=1e-12)


def test_the_generic_pose_cases_stay_inside_the_ambiguity_cap():
    """the cases the GPU module runs: at most 2 % ambiguous texels, and the float32 reference decides every other texel like
    the float64 one, with depths to ~2e-7"""
    for case in dr.GENERIC:
        for normalize in (True, False):
            c = dr.generic_case(case, normalize)
            r64 = dr.reproject(c["intr"], c["lv"], c["R"], c["T"], c["W_gt"], normalize)
            r32 = dr.reproject(c["intr"], c["lv"], c["R"], c["T"], c["W_gt"], normalize, np.float32)
            clear = ~r64["ambiguous"]
            print(case, normalize, "ambiguous share %.4f" % r64["ambiguous"].mean())
            assert r64["ambiguous"].mean() <= 0.02
            assert np.array_equal(r32["index"][clear], r64["index"][clear])
            hit = clear & (r64["index"] >= 0)
            assert hit.mean() > 0.5
            assert (np.abs(r32["depth"][hit] - r64["depth"][hit]) / r64["depth"][hit]).max() < 1e-6


def test_fit_reference_equals_a_direct_loop_and_ignores_what_does_not_contribute():
    fc = dr.fit_case(40, 3, 11)
    fc["target"][0, 3] = np.nan                            # under w > 0: excluded
    fc["weight"][1, 5], fc["target"][1, 5] = 0.0, np.inf   # under w = 0: ignored
    fc["weight"][2, 7] = np.inf
    mu = np.array([0.0, 1e-3, 0.5])
    r = dr.basis_fit(fc["depth"], fc["basis"], fc["target"], fc["weight"], mu)
    for b in range(3):
        G, g, sw, swr = np.zeros((3, 3)), np.zeros(3), 0.0, 0.0
        for n in range(40):
            w, t = float(fc["weight"][b, n]), float(fc["target"][b, n])
            if not (w > 0 and np.isfinite(w) and np.isfinite(t)):
                continue
            bn, rn = fc["basis"][b, n].astype(np.float64), t - float(fc["depth"][b, n])
            G += w * np.outer(bn, bn)
            g += w * rn * bn
            sw, swr = sw + w, swr + w * rn * rn
        Hm = G + mu[b] * np.diag(np.diag(G) + 1e-5)
        assert np.allclose(r["normal"][b], G, rtol=1e-12) and np.allclose(r["rhs"][b], g, rtol=1e-10, atol=1e-12)
        assert np.allclose(r["stats"][b], [sw, swr], rtol=1e-12)
        assert np.allclose(r["Wc"][b], np.linalg.solve(Hm, g), rtol=1e-9) and r["status"][b] == 0
    y = dr.basis_fit(fc["depth"], fc["basis"], fc["target"], fc["weight"], mu, np.float32)
    assert y["normal"].dtype == np.float32 and np.abs(y["Wc"] - r["Wc"]).max() < 1e-5 * np.abs(r["Wc"]).max()
    # no contributing point and no damping: not positive definite
    z = dr.basis_fit(fc["depth"], fc["basis"], fc["target"], np.zeros_like(fc["weight"]), None)
    assert list(z["status"]) == [1, 1, 1] and np.all(z["Wc"] == 0)
    z = dr.basis_fit(fc["depth"], fc["basis"], fc["target"], np.zeros_like(fc["weight"]), np.full(3, 1e-3))
    assert list(z["status"]) == [0, 0, 0] and np.all(z["Wc"] == 0)


@pytest.mark.parametrize("N,K", dr.FIT_SHAPES)
def test_the_fit_cases_are_well_posed(N, K):
    """what the GPU module's 1e-4 gate on Wc presumes: the float32 yardstick itself is at 1e-6 on every shape"""
    fc = dr.fit_case(N, K, 7)
    mu = np.full(3, dr.fit_damping(N, K))
    r64 = dr.basis_fit(fc["depth"], fc["basis"], fc["target"], fc["weight"], mu)
    r32 = dr.basis_fit(fc["depth"], fc["basis"], fc["target"], fc["weight"], mu, np.float32)
    yard = (np.abs(r32["Wc"] - r64["Wc"]).max(1) / np.abs(r64["Wc"]).max(1)).max()
    print(N, K, "yardstick %.2e" % yard)
    assert list(r64["status"]) == [0, 0, 0] and yard < 5e-6
    zero = (fc["weight"] == 0).mean()
    assert 0.2 < zero < 0.4 or N < 100
