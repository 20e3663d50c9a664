"""Gradients of the per-level preparation on HIP (`-m gpu`): banet_resample_grad_f32 / banet_depth_output_grad_f32 against the
float64 oracle (oracle.banet_oracle.resampler / interpolate2d2), run-to-run and graph-replay bit identity, deterministic mode,
and BundleNet(prep_graph="hip") through CameraResize / BundleResize against the float64 oracle drivers."""
import ctypes
import time

import numpy as np
import pytest
import torch

import cases
from oracle import banet_oracle as orc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from banet_amd import _capi
    _capi.lib()


def t(x, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype))).to(DEV)


def n(x):
    return x.detach().cpu().numpy()


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def oracle_sample(data64, warp64, clamp):
    return orc.interpolate2d2(data64, warp64) if clamp else orc.resampler(data64, warp64)


def make_warp(rng, B, N, H, W, kind):
    """kind: 'mixed' (inside, outside, rim, integer coordinates), 'cluster', 'collapsed'"""
    if kind == "collapsed":
        w = np.empty((B, N, 2), np.float32)
        w[..., 0], w[..., 1] = 0.37 * W, 0.61 * H
        return w
    if kind == "cluster":
        c = rng.uniform([0, 0], [W - 1, H - 1], size=(B, 4, 2))
        w = c[:, rng.randint(0, 4, N)] + rng.standard_normal((B, N, 2)) * 0.7
        return w.astype(np.float32)
    w = rng.uniform([-2.5, -2.5], [W + 1.5, H + 1.5], size=(B, N, 2)).astype(np.float32)
    q = N // 6
    w[:, :q] = np.round(w[:, :q])                                              # integer coordinates (inside and out)
    w[:, q:2 * q, 0] = rng.choice([-1.0, -0.5, 0.0, W - 1.0, W - 0.5, float(W)], size=(B, q))   # rim
    w[:, 2 * q:3 * q, 1] = rng.choice([-1.0, -0.5, 0.0, H - 1.0, H - 0.5, float(H)], size=(B, q))
    return w


def resample_grad(data, warp, gout, clamp, ddata=None, dwarp=None, overwrite=True):
    from banet_amd import _capi
    L = _capi.lib()
    B, H, W, C = data.shape
    N = warp.shape[1]
    nb = L.banet_resample_grad_workspace_bytes(B, N, C, H, W, int(clamp))
    assert nb > 0
    ws = _capi.workspace(nb, data.device)
    ddata = torch.empty_like(data) if ddata is None else ddata
    dwarp = torch.empty((B, N, 2), device=data.device) if dwarp is None else dwarp
    _capi.check(L.banet_resample_grad_f32(_capi.ptr(data), _capi.ptr(warp), _capi.ptr(gout), _capi.ptr(ddata), _capi.ptr(dwarp),
                                          B, N, C, H, W, int(clamp), 1 if overwrite else 0, ctypes.c_void_p(ws.data_ptr()),
                                          ws.numel(), _capi.stream()))
    return ddata, dwarp


@pytest.mark.parametrize("clamp", [False, True])
@pytest.mark.parametrize("C", [1, 3, 64, 128, 200, 256])
def test_map_gradient_is_the_exact_adjoint_on_small_maps(clamp, C):
    """ddata = A^T gout with A the interpolation matrix of the float64 oracle (its outputs on one-hot images)"""
    rng = np.random.RandomState(C + 7 * clamp)
    B, H, W, N = 3, 6, 7, 90
    for kind in ("mixed", "cluster", "collapsed"):
        warp = make_warp(rng, B, N, H, W, kind)
        data = rng.standard_normal((B, H, W, C)).astype(np.float32)
        g = rng.standard_normal((B, N, C)).astype(np.float32)
        dd, _ = resample_grad(t(data), t(warp), t(g), clamp)
        torch.cuda.synchronize()
        eye = np.eye(H * W).reshape(H * W, H, W, 1)
        want = np.empty((B, H * W, C))
        for b in range(B):
            A = oracle_sample(eye, np.repeat(warp[b:b + 1].astype(np.float64), H * W, axis=0), clamp)[..., 0]   # [HW, N]
            want[b] = A @ g[b].astype(np.float64)
        assert relerr(n(dd).reshape(B, H * W, C), want) < 1e-5, (kind, relerr(n(dd).reshape(B, H * W, C), want))


@pytest.mark.parametrize("clamp", [False, True])
@pytest.mark.parametrize("shape", [(16, 4096, 128, 32, 40), (2, 4096, 256, 128, 160), (4, 2048, 3, 256, 320), (8, 1000, 200, 64, 80)])
def test_map_gradient_dot_product_identity_on_large_maps(clamp, shape):
    """<resample(data), g> = <data, ddata> over several probes, mixed / clustered / collapsed warps"""
    B, N, C, H, W = shape
    rng = np.random.RandomState(B + N + C)
    for kind in ("mixed", "cluster", "collapsed"):
        warp = make_warp(rng, B, N, H, W, kind)
        wt = t(warp)
        for probe in range(2):
            data = rng.standard_normal((B, H, W, C)).astype(np.float32)
            g = rng.standard_normal((B, N, C)).astype(np.float32)
            dd, _ = resample_grad(t(data), wt, t(g), clamp)
            lhs = float((oracle_sample(data.astype(np.float64), warp.astype(np.float64), clamp) * g).sum())
            rhs = float((data.astype(np.float64) * n(dd).astype(np.float64)).sum())
            scale = float(np.abs(g).sum()) * 4.0
            assert abs(lhs - rhs) <= 1e-5 * scale, (kind, probe, lhs, rhs)


@pytest.mark.parametrize("clamp", [False, True])
def test_warp_gradient_against_central_differences(clamp):
    rng = np.random.RandomState(5 + clamp)
    B, N, C, H, W = 3, 300, 67, 20, 24
    lo = -0.9 if not clamp else -3.0
    warp = rng.uniform([lo, lo], [W - 0.1 if not clamp else W + 2, H - 0.1 if not clamp else H + 2], size=(B, N, 2))
    frac = warp - np.floor(warp)
    warp = np.floor(warp) + np.clip(frac, 0.15, 0.85)                    # away from texel edges: the bilinear form is linear
    if not clamp:
        warp[:, : N // 10] = [W + 3.0, 2.5]                              # not sampled: dwarp = 0
    warp = warp.astype(np.float32)
    data = rng.standard_normal((B, H, W, C)).astype(np.float32)
    g = rng.standard_normal((B, N, C)).astype(np.float32)
    _, dw = resample_grad(t(data), t(warp), t(g), clamp)
    d64, g64, w64 = data.astype(np.float64), g.astype(np.float64), warp.astype(np.float64)
    h = 1e-4
    want = np.empty((B, N, 2))
    for a in range(2):
        e = np.zeros(2)
        e[a] = h
        want[..., a] = ((oracle_sample(d64, w64 + e, clamp) - oracle_sample(d64, w64 - e, clamp)) * g64).sum(-1) / (2 * h)
    assert relerr(n(dw), want) < 1e-4, relerr(n(dw), want)
    if not clamp:
        assert (n(dw)[:, : N // 10] == 0).all()


def test_depth_output_gradient_against_float64():
    from banet_amd import prep_grad
    rng = np.random.RandomState(11)
    B, H, W, K = 4, 37, 45, 128
    init = rng.standard_normal((B, H, W)).astype(np.float32)
    basis = rng.standard_normal((B, H, W, K)).astype(np.float32)
    Wc = rng.standard_normal((B, K, 1)).astype(np.float32)
    g = rng.standard_normal((B, H, W)).astype(np.float32)
    gi, gb, gw = prep_grad.depth_output_grad_forward(t(basis), t(Wc), t(g))
    assert (n(gi) == g).all()
    assert relerr(n(gb), g.astype(np.float64)[..., None] * Wc.astype(np.float64)[:, None, None, :, 0]) < 1e-6
    want = np.einsum("bhw,bhwk->bk", g.astype(np.float64), basis.astype(np.float64))[..., None]
    assert relerr(n(gw), want) < 1e-5
    # the autograd op: forward value and all three gradients
    ti, tb, tw = (t(v).requires_grad_(True) for v in (init, basis, Wc))
    out = prep_grad.depth_output(ti, tb, tw)
    assert relerr(n(out), init + np.einsum("bhwk,bk->bhw", basis.astype(np.float64), Wc[..., 0].astype(np.float64))) < 1e-5
    out.backward(t(g))
    assert (n(ti.grad) == g).all() and relerr(n(tw.grad), want) < 1e-5


def test_gradients_are_bit_identical_run_to_run_and_overwrite_equals_accumulating_into_zeros():
    from banet_amd import prep_grad
    rng = np.random.RandomState(2)
    B, N, C, H, W = 8, 4096, 128, 64, 80
    for clamp in (False, True):
        for kind in ("mixed", "cluster"):
            warp, data = t(make_warp(rng, B, N, H, W, kind)), t(rng.standard_normal((B, H, W, C)))
            g = t(rng.standard_normal((B, N, C)))
            a = resample_grad(data, warp, g, clamp)
            b = resample_grad(data, warp, g, clamp)
            z = resample_grad(data, warp, g, clamp, ddata=torch.zeros_like(data), overwrite=False)
            for x, y, w in zip(a, b, z):
                assert torch.equal(x, y) and torch.equal(x, w)
            # accumulating on top of a buffer adds exactly the written gradient's terms after the old value
            base = t(rng.standard_normal((B, H, W, C)))
            acc, _ = resample_grad(data, warp, g, clamp, ddata=base.clone(), overwrite=False)
            assert torch.allclose(acc, base + a[0], rtol=1e-5, atol=1e-5 * float(a[0].abs().max()))     # (order of the adds differs)
    basis, Wc, gd = t(rng.standard_normal((B, 5000, 128))), t(rng.standard_normal((B, 128, 1))), t(rng.standard_normal((B, 5000)))
    r1, r2 = prep_grad.depth_output_grad_forward(basis, Wc, gd), prep_grad.depth_output_grad_forward(basis, Wc, gd)
    assert all(torch.equal(x, y) for x, y in zip(r1, r2))


def test_collapsed_warp_finishes_and_reports_its_time():
    rng = np.random.RandomState(9)
    B, N, C, H, W = 8, 4096, 128, 128, 160
    warp, data = t(make_warp(rng, B, N, H, W, "collapsed")), t(rng.standard_normal((B, H, W, C)))
    g = t(rng.standard_normal((B, N, C)))
    resample_grad(data, warp, g, False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    dd, _ = resample_grad(data, warp, g, False)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    print("collapsed warp B=%d N=%d C=%d %dx%d: %.2f ms" % (B, N, C, H, W, ms))
    lhs = float((orc.resampler(n(data).astype(np.float64), n(warp).astype(np.float64)) * n(g)).sum())
    rhs = float((n(data).astype(np.float64) * n(dd)).sum())
    assert abs(lhs - rhs) <= 1e-5 * float(n(g).__abs__().sum()) * 4


def test_graph_capture_replays_bit_identically():
    from banet_amd import _capi
    L = _capi.lib()
    rng = np.random.RandomState(4)
    B, N, C, H, W, K = 4, 3000, 128, 64, 80, 128
    data, warp = t(rng.standard_normal((B, H, W, C))), t(make_warp(rng, B, N, H, W, "mixed"))
    g = t(rng.standard_normal((B, N, C)))
    basis, Wc, gd = t(rng.standard_normal((B, H * W, K))), t(rng.standard_normal((B, K, 1))), t(rng.standard_normal((B, H * W)))
    ws1 = _capi.workspace(L.banet_resample_grad_workspace_bytes(B, N, C, H, W, 0), data.device)
    ws2 = _capi.workspace(L.banet_depth_output_grad_workspace_bytes(B, H * W, K), data.device)
    outs = [torch.empty_like(data), torch.empty((B, N, 2), device=DEV), torch.empty_like(gd), torch.empty_like(basis), torch.empty_like(Wc)]

    def enqueue():
        _capi.check(L.banet_resample_grad_f32(_capi.ptr(data), _capi.ptr(warp), _capi.ptr(g), _capi.ptr(outs[0]), _capi.ptr(outs[1]),
                                              B, N, C, H, W, 0, 1, ctypes.c_void_p(ws1.data_ptr()), ws1.numel(), _capi.stream()))
        _capi.check(L.banet_depth_output_grad_f32(_capi.ptr(basis), _capi.ptr(Wc), _capi.ptr(gd), _capi.ptr(outs[2]), _capi.ptr(outs[3]),
                                                  _capi.ptr(outs[4]), B, H * W, K, 1, ctypes.c_void_p(ws2.data_ptr()), ws2.numel(),
                                                  _capi.stream()))

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        enqueue()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    eager = [o.clone() for o in outs]
    for o in outs:
        o.fill_(float("nan"))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        enqueue()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(outs, eager))


def test_ops_run_under_deterministic_algorithms():
    from banet_amd import prep_grad
    rng = np.random.RandomState(6)
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        data = t(rng.standard_normal((2, 12, 14, 8))).requires_grad_(True)
        warp = t(make_warp(rng, 2, 50, 12, 14, "mixed")).requires_grad_(True)
        basis, Wc, init = (t(rng.standard_normal(s)).requires_grad_(True) for s in ((2, 12, 14, 3), (2, 3, 1), (2, 12, 14)))
        for clamp in (False, True):
            loss = prep_grad.resampler(data, warp, clamp).square().sum() + prep_grad.target_map(data).square().sum() \
                + prep_grad.depth_output(init, basis, Wc).square().sum()
            loss.backward()
        assert all(x.grad is not None and torch.isfinite(x.grad).all() for x in (data, warp, basis, Wc, init))
    finally:
        torch.use_deterministic_algorithms(was)


def test_target_map_op_gradient_matches_torch_expression():
    from banet_amd import bundlenet, prep_grad
    rng = np.random.RandomState(8)
    img = t(rng.standard_normal((3, 9, 11, 5))).requires_grad_(True)
    g = t(rng.standard_normal((3, 9, 11, 15)))
    (a,) = torch.autograd.grad((prep_grad.target_map(img) * g).sum(), img)
    ref = torch.cat([img, bundlenet._grad_fixed_autograd(img)], dim=-1)
    (b,) = torch.autograd.grad((ref * g).sum(), img)
    assert torch.allclose(a, b, rtol=1e-5, atol=1e-6)


# ---- the level drivers ----------------------------------------------------------------------------------------------------
def _bundle_resize_grads(c, prep_graph, Rs_o, Ts_o, cT, cD, cR):
    from banet_amd import bundlenet
    lw = {k: [(t(w).requires_grad_(True), t(b).requires_grad_(True)) for w, b in v] for k, v in c["mlp"].items()}
    net = bundlenet.BundleNet(lambda_weights=lw, prep_graph=prep_graph)
    layers = [t(l).requires_grad_(True) for l in c["layers"]]
    basis = t(c["basis"]).requires_grad_(True)
    depth = t(c["depth"]).requires_grad_(True)
    Rb, Tb, Db = net.BundleResize(t(c["intr"]), layers, t(c["points"]), basis, depth, init_rotation=t(Rs_o[-1]),
                                  init_translation=t(Ts_o[-1]))
    loss = sum((a * t(w)).sum() for a, w in zip(Tb, cT)) + sum((a * t(w)).sum() for a, w in zip(Db, cD)) \
        + sum((a * t(w)).sum() for a, w in zip(Rb, cR))
    leaves = layers[2:4] + [basis, depth, lw["2"][0][0], lw["3"][4][0]]
    return Rb + Tb + Db, [n(g).astype(np.float64) for g in torch.autograd.grad(loss, leaves)]


def test_bundle_resize_hip_prep_graph_meets_the_finite_difference_gate():
    c = cases.case_resize(C=4, K=3, N=96)
    Rs_o, Ts_o = orc.camera_resize(c["intr"], c["layers"], c["points"], c["depth"], c["mlp"])
    Rb_o, Tb_o, Db_o = orc.bundle_resize(c["intr"], c["layers"], c["points"], c["basis"], c["depth"], c["mlp"],
                                         init_rotation=Rs_o[-1], init_translation=Ts_o[-1])
    rng = np.random.RandomState(3)
    cT = [rng.standard_normal(x.shape) for x in Tb_o]
    cD = [rng.standard_normal(x.shape) / x.size for x in Db_o]
    cR = [rng.standard_normal(x.shape) for x in Rb_o]
    outs, grads = _bundle_resize_grads(c, "hip", Rs_o, Ts_o, cT, cD, cR)
    for a, b in zip(outs, Rb_o + Tb_o + Db_o):
        assert relerr(n(a), b) < 1e-4
    _, grads2 = _bundle_resize_grads(c, "hip", Rs_o, Ts_o, cT, cD, cR)
    assert all(np.array_equal(a, b) for a, b in zip(grads, grads2)), "prep_graph='hip' gradients differ between two runs"
    _, grads_t = _bundle_resize_grads(c, "torch", Rs_o, Ts_o, cT, cD, cR)
    f64 = lambda x: np.asarray(x, np.float64)  # noqa: E731

    def oracle_loss(over):
        layers64 = [f64(over.get("layer%d" % i, c["layers"][i])) for i in range(4)]
        mlp = {k: [(f64(w), f64(b)) for w, b in v] for k, v in c["mlp"].items()}
        if "w2" in over:
            mlp["2"][0] = (over["w2"], mlp["2"][0][1])
        if "w3" in over:
            mlp["3"][4] = (over["w3"], mlp["3"][4][1])
        r, tt, dd = orc.bundle_resize(f64(c["intr"]), layers64, f64(c["points"]), f64(over.get("basis", c["basis"])),
                                      f64(over.get("depth", c["depth"])), mlp, init_rotation=f64(Rs_o[-1]),
                                      init_translation=f64(Ts_o[-1]), stop_gradient_depth=f64(c["depth"]))
        return float(sum((a * w).sum() for a, w in zip(tt, cT)) + sum((a * w).sum() for a, w in zip(dd, cD))
                     + sum((a * w).sum() for a, w in zip(r, cR)))

    names = ["layer2", "layer3", "basis", "depth", "w2", "w3"]
    base = {"layer2": c["layers"][2], "layer3": c["layers"][3], "basis": c["basis"], "depth": c["depth"],
            "w2": c["mlp"]["2"][0][0], "w3": c["mlp"]["3"][4][0]}
    for name, g, gt in zip(names, grads, grads_t):
        assert np.isfinite(g).all() and np.abs(g).sum() > 0
        v = rng.standard_normal(base[name].shape)
        v /= np.linalg.norm(v)
        eps = 1e-4
        fd = (oracle_loss({name: f64(base[name]) + eps * v}) - oracle_loss({name: f64(base[name]) - eps * v})) / (2 * eps)
        ad, adt = float((g * v).sum()), float((gt * v).sum())
        assert abs(ad - fd) <= 3e-2 * max(abs(fd), abs(ad)) + 1e-7, (name, ad, fd)
        assert abs(ad - adt) <= 3e-2 * max(abs(adt), abs(ad)) + 1e-7, (name, ad, adt)


def _camera_resize_grads(c, prep_graph, cR, cT):
    from banet_amd import bundlenet
    lw = {k: [(t(w).requires_grad_(True), t(b).requires_grad_(True)) for w, b in v] for k, v in c["mlp"].items()}
    net = bundlenet.BundleNet(lambda_weights=lw, prep_graph=prep_graph)
    layers = [t(l).requires_grad_(True) for l in c["layers"]]
    Rs, Ts = net.CameraResize(t(c["intr"]), layers, t(c["points"]), t(c["depth"]))
    loss = sum((a * t(w)).sum() for a, w in zip(Ts, cT)) + sum((a * t(w)).sum() for a, w in zip(Rs, cR))
    return Rs + Ts, [n(g).astype(np.float64) for g in torch.autograd.grad(loss, layers)]


def test_camera_resize_hip_prep_graph_meets_the_finite_difference_gate():
    c = cases.case_resize(C=4, K=3, N=96)
    Rs_o, Ts_o = orc.camera_resize(c["intr"], c["layers"], c["points"], c["depth"], c["mlp"])
    rng = np.random.RandomState(5)
    cT = [rng.standard_normal(x.shape) for x in Ts_o]
    cR = [rng.standard_normal(x.shape) for x in Rs_o]
    outs, grads = _camera_resize_grads(c, "hip", cR, cT)
    for a, b in zip(outs, Rs_o + Ts_o):
        assert relerr(n(a), b) < 1e-4
    _, grads2 = _camera_resize_grads(c, "hip", cR, cT)
    assert all(np.array_equal(a, b) for a, b in zip(grads, grads2)), "prep_graph='hip' gradients differ between two runs"
    _, grads_t = _camera_resize_grads(c, "torch", cR, cT)
    f64 = lambda x: np.asarray(x, np.float64)  # noqa: E731

    def oracle_loss(over):
        layers64 = [f64(over.get("layer%d" % i, c["layers"][i])) for i in range(4)]
        mlp = {k: [(f64(w), f64(b)) for w, b in v] for k, v in c["mlp"].items()}
        r, tt = orc.camera_resize(f64(c["intr"]), layers64, f64(c["points"]), f64(c["depth"]), mlp)
        return float(sum((a * w).sum() for a, w in zip(tt, cT)) + sum((a * w).sum() for a, w in zip(r, cR)))

    names = ["layer0", "layer1", "layer2", "layer3"]          # (the pyramid: what the preparation ops differentiate)
    base = {"layer%d" % i: c["layers"][i] for i in range(4)}
    for name, g, gt in zip(names, grads, grads_t):
        assert np.isfinite(g).all() and np.abs(g).sum() > 0
        v = rng.standard_normal(base[name].shape)
        v /= np.linalg.norm(v)
        eps = 1e-4
        fd = (oracle_loss({name: f64(base[name]) + eps * v}) - oracle_loss({name: f64(base[name]) - eps * v})) / (2 * eps)
        ad, adt = float((g * v).sum()), float((gt * v).sum())
        assert abs(ad - fd) <= 3e-2 * max(abs(fd), abs(ad)) + 1e-7, (name, ad, fd)
        assert abs(ad - adt) <= 3e-2 * max(abs(adt), abs(ad)) + 1e-7, (name, ad, adt)
