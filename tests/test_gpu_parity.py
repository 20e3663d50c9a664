"""Parity of the HIP path against the oracle -- runs on a real MI355X (`-m gpu`).

Every call goes through the C ABI of libbanet_hip.so (banet_amd.ops / bundlenet / legacy /
dense are ctypes wrappers).  Tolerances: floating point, 1e-4 relative on pose/depth updates
(BASELINE.json north_star), iteration counts identical.  Normal-equation entries are compared
at 3e-5 of the matrix scale (fp32 accumulation over up to 3e5 pixels).
"""
import os

import numpy as np
import pytest
import torch

import cases
import torch_ref
from oracle import banet_oracle as orc, dense as odense, synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from banet_amd import _capi
    _capi.lib()                                   # fail loudly if the HIP library is missing


def t(x, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype))).to(DEV)


def n(x):
    return x.detach().cpu().numpy()


def relerr(got, want):
    want = np.asarray(want, np.float64)
    got = np.asarray(got, np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))


def mlp_t(layers):
    return [(w, b) for w, b in layers]


# ======================================================================================
# (1) EquationConstruction / Grad : the reference's custom ops
# ======================================================================================
@pytest.mark.parametrize("B,N,C,P", [(1, 4096, 128, 6), (2, 1000, 16, 38), (1, 2048, 128, 134), (3, 77, 7, 6),
                                     (1, 333, 6, 23), (1, 40, 128, 70), (1, 300, 32, 262), (2, 77, 5, 7), (3, 33, 64, 143), (1, 250, 9, 144),
                                     (2, 130, 16, 145), (1, 1000, 8, 200), (2, 257, 128, 272), (1, 300, 128, 298), (2, 77, 6, 304)])
def test_equation_construction_matches_oracle(B, N, C, P):
    from banet_amd import ops
    rng = np.random.RandomState(B * 1000 + N + C + P)
    J = rng.standard_normal((B, N, 2, P)).astype(np.float32)
    G = rng.standard_normal((B, N, C, 2)).astype(np.float32)
    d = rng.standard_normal((B, N, C, 1)).astype(np.float32)
    AtA, Atb = ops.equation_construction(t(J), t(G), t(d))
    AtA64, Atb64 = orc.equation_construction(J.astype(np.float64), G.astype(np.float64), d.astype(np.float64))
    assert AtA.shape == (B, P, P) and Atb.shape == (B, P, 1)
    # asymmetric random J: a transposed MFMA C/D layout or swapped operands cannot pass
    assert relerr(n(AtA), AtA64) < 3e-5, relerr(n(AtA), AtA64)
    assert relerr(n(Atb), Atb64) < 3e-5, relerr(n(Atb), Atb64)
    np.testing.assert_array_equal(n(AtA), np.swapaxes(n(AtA), 1, 2))        # exactly symmetric
    # the reference's second formulation (legacy/ba.py:282-283) agrees as well
    AtA_tf, Atb_tf = orc.equation_construction_tf_twin(J.astype(np.float64), G.astype(np.float64), d.astype(np.float64))
    assert relerr(n(AtA), AtA_tf) < 3e-5 and relerr(n(Atb), Atb_tf) < 3e-5


def test_equation_construction_is_deterministic_and_handles_zeros():
    from banet_amd import ops
    rng = np.random.RandomState(5)
    J = t(rng.standard_normal((2, 500, 2, 38)))
    G = t(rng.standard_normal((2, 500, 16, 2)))
    d = t(rng.standard_normal((2, 500, 16, 1)))
    a1, b1 = ops.equation_construction(J, G, d)
    a2, b2 = ops.equation_construction(J, G, d)
    assert torch.equal(a1, a2) and torch.equal(b1, b2)
    G[:, 100:400] = 0                                                       # masked pixels: all-zero gradient rows
    a3, _ = ops.equation_construction(J, G, d)
    ref, _ = orc.equation_construction(n(J).astype(np.float64), n(G).astype(np.float64), n(d).astype(np.float64))
    assert relerr(n(a3), ref) < 3e-5
    z, zb = ops.equation_construction(J, torch.zeros_like(G), d)            # mask all zero
    assert float(z.abs().max()) == 0.0 and float(zb.abs().max()) == 0.0


@pytest.mark.parametrize("B,N,C,P", [(1, 256, 16, 6), (2, 100, 7, 38), (1, 64, 128, 134), (2, 77, 5, 7), (1, 250, 128, 70), (3, 33, 64, 143),
                                     (1, 40, 16, 150), (1, 90, 16, 262), (2, 50, 8, 200), (1, 70, 32, 165), (1, 33, 4, 272), (1, 45, 16, 298), (2, 20, 4, 304)])
def test_equation_construction_grad_matches_oracle(B, N, C, P):
    from banet_amd import ops
    rng = np.random.RandomState(N + C + P)
    J = rng.standard_normal((B, N, 2, P))
    G = rng.standard_normal((B, N, C, 2))
    d = rng.standard_normal((B, N, C, 1))
    g0 = rng.standard_normal((B, P, P))
    g0 = g0 + np.swapaxes(g0, 1, 2)                                        # symmetric (utils.cu:651 alpha=2 assumes it)
    g1 = rng.standard_normal((B, P, 1))
    gJ, gG, gd = ops.equation_construction_grad(t(J), t(G), t(d), t(g0), t(g1))
    rJ, rG, rd = orc.equation_construction_grad(J, G, d, g0, g1)
    for got, want in ((gJ, rJ), (gG, rG), (gd, rd)):
        assert got.shape == want.shape
        assert relerr(n(got), want) < 3e-5, relerr(n(got), want)
    # without a workspace the entry point runs the first-generation kernel: same results
    import ctypes
    from banet_amd import _capi as capi
    Jc, Gc, dc, g0c, g1c = (t(x).contiguous() for x in (J, G, d, g0, g1))
    oJ, oG, od = torch.empty_like(Jc), torch.empty_like(Gc), torch.empty_like(dc)
    capi.check(capi.lib().banet_equation_construction_grad_f32(capi.ptr(Jc), capi.ptr(Gc), capi.ptr(dc), capi.ptr(g0c), capi.ptr(g1c),
                                                               capi.ptr(oJ), capi.ptr(oG), capi.ptr(od), B, N, C, P, None, 0,
                                                               capi.stream()))
    for got, want in ((oJ, rJ), (oG, rG), (od, rd)):
        assert relerr(n(got), want) < 3e-5, relerr(n(got), want)
    # and the autograd pairing of bundlenet.py:79-82
    Jt, Gt, dt_ = t(J).requires_grad_(), t(G).requires_grad_(), t(d).requires_grad_()
    AtA, Atb = ops.equation_construction(Jt, Gt, dt_)
    ((AtA * t(g0)).sum() + (Atb * t(g1)).sum()).backward()
    assert relerr(n(Jt.grad), rJ) < 3e-5 and relerr(n(Gt.grad), rG) < 3e-5 and relerr(n(dt_.grad), rd) < 3e-5
    # and the dispatcher registration (torch.ops.banet.*): same kernels, same autograd pairing
    J2, G2, d2 = t(J).requires_grad_(), t(G).requires_grad_(), t(d).requires_grad_()
    AtA2, Atb2 = torch.ops.banet.equation_construction(J2, G2, d2)
    assert torch.equal(AtA2, AtA) and torch.equal(Atb2, Atb)
    ((AtA2 * t(g0)).sum() + (Atb2 * t(g1)).sum()).backward()
    assert torch.equal(J2.grad, Jt.grad) and torch.equal(G2.grad, Gt.grad) and torch.equal(d2.grad, dt_.grad)


# ======================================================================================
# (2) golden vectors produced by the reference's own Python (tests/golden)
# ======================================================================================
def _legacy_level_inputs(c):
    N = c["points"].shape[1]
    intr = c["intr"]
    fx0, fy0 = np.tile(intr[:, 0], (1, N)), np.tile(intr[:, 1], (1, N))
    ox0, oy0 = np.tile(intr[:, 2], (1, N)), np.tile(intr[:, 3], (1, N))
    p = orc.compute_coordinates(c["points"], fx0, fy0, ox0, oy0, normalize=False)
    s = np.float32(c["scale"])
    return p, fx0 / s, fy0 / s, ox0 / s, oy0 / s


def test_golden_legacy_camera_iterations(golden_dir):
    from banet_amd import legacy
    g = np.load(os.path.join(golden_dir, "golden_legacy_ci2.npz"))
    c = cases.case_legacy_ci2()
    p, fx, fy, ox, oy = _legacy_level_inputs(c)
    conv2 = orc.target_map(c["conv2_f"])
    trk = legacy.Tracker(lambda_weights=c["mlp"])
    R, T, uw, ut, ratio = trk.CameraIteration2(t(c["conv1"]), t(conv2), t(fx), t(fy), t(ox), t(oy), t(p), t(c["d"]),
                                               t(c["R"]), t(c["T"]), c["level"])
    assert relerr(n(R), g["R"]) < 1e-4 and relerr(n(T), g["T"]) < 1e-4
    assert relerr(n(uw)[0], g["uw"]) < 1e-4 and relerr(n(ut)[0], g["ut"]) < 1e-4
    assert relerr(n(ratio)[0], g["ratio"]) < 1e-6
    R1, T1, ratio1 = trk.CameraIteration(t(c["conv1"]), t(conv2), t(fx), t(fy), t(ox), t(oy), t(p), t(c["d"]),
                                         t(c["R"]), t(c["T"]))
    assert relerr(n(R1), g["R1"]) < 1e-4 and relerr(n(T1), g["T1"]) < 1e-4
    assert relerr(n(ratio1)[0], g["ratio1"]) < 1e-6


def test_golden_legacy_track_iteration_counts_identical(golden_dir):
    from banet_amd import legacy
    g = np.load(os.path.join(golden_dir, "golden_legacy_track.npz"))
    c = cases.case_legacy_track()
    trk = legacy.Tracker(lambda_weights=c["mlp"])
    layers = [t(l) for l in c["layers"]]
    legacy.early_termination = True
    R, T, ratio = trk.trackTF(t(c["intr"]), layers, t(c["points"]), t(c["d"]), t(c["R"]), t(c["T"]), c["iters"])
    its = [int(v[0]) for v in trk.level_iters_run]
    assert its == list(g["iters"]), (its, list(g["iters"]))
    assert relerr(n(R), g["R"]) < 1e-4 and relerr(n(T), g["T"]) < 1e-4, (relerr(n(R), g["R"]), relerr(n(T), g["T"]))
    assert relerr(n(ratio)[0], g["ratio"]) < 1e-5
    try:
        legacy.early_termination = False
        R, T, ratio = trk.trackTF(t(c["intr"]), layers, t(c["points"]), t(c["d"]), t(c["R"]), t(c["T"]), c["iters"])
        assert [int(v[0]) for v in trk.level_iters_run] == c["iters"]
        assert relerr(n(R), g["Rs"][-1]) < 1e-4 and relerr(n(T), g["Ts"][-1]) < 1e-4
    finally:
        legacy.early_termination = True


def test_golden_bundlenet_iterations(golden_dir):
    from banet_amd import bundlenet
    g = np.load(os.path.join(golden_dir, "golden_bundle_iter.npz"))
    c = cases.case_bundle_iter()
    net = bundlenet.BundleNet(lambda_weights=c["mlp"])
    a = [t(c[k]) for k in ("conv1", "conv2", "fx", "fy", "ox", "oy", "p", "D")]
    R, T = net.CameraIteration(*a, t(c["R"]), t(c["T"]), 1.0, c["level"])
    assert relerr(n(R), g["Rc"]) < 1e-4 and relerr(n(T), g["Tc"]) < 1e-4, (relerr(n(R), g["Rc"]), relerr(n(T), g["Tc"]))
    R, T, W = net.BundleIteration(*a, t(c["Bs"]), t(c["R"]), t(c["T"]), t(c["W"]), 1000.0, c["level"])
    assert relerr(n(R), g["R"]) < 1e-4 and relerr(n(T), g["T"]) < 1e-4
    assert relerr(n(W) - c["W"], g["W"] - c["W"]) < 1e-4, relerr(n(W) - c["W"], g["W"] - c["W"])   # the depth UPDATE


def test_bundlenet_module_functions(golden_dir):
    from banet_amd import bundlenet as bn
    g = np.load(os.path.join(golden_dir, "golden_bundle_fns.npz"))
    c = cases.case_bundle_fns()
    assert relerr(n(bn.CameraJacobianMatrix(t(c["x"]), t(c["y"]), t(c["Z"]), t(c["fx"]), t(c["fy"]))), g["Jc"]) < 1e-5
    assert relerr(n(bn.DepthJacobianMatrix(t(c["r"][0]), t(c["r"][1]), t(c["r"][2]), t(c["x"]), t(c["y"]), t(c["Z"]),
                                           t(c["fx"]), t(c["fy"]))), g["jd"]) < 1e-5
    w1, w2 = c["w1"], c["w2"]
    assert relerr(n(bn.AngleaAxisRotation(t(w2[:, 0:1]), t(w2[:, 1:2]), t(w2[:, 2:3]))), g["rot2"]) < 1e-5
    assert relerr(n(bn.VMatrix(t(w1[:, 0:1]), t(w1[:, 1:2]), t(w1[:, 2:3]))), g["V1"]) < 1e-5
    assert relerr(n(bn.rotation2quaternion(t(c["Rm"]))), g["q"]) < 1e-5
    assert relerr(n(bn.BundleNet().grad_fixed(t(c["img"]))), g["g"]) < 1e-6


def test_resize_drivers_match_oracle():
    """B=2 here, so the comparison is with the oracle's per-item V (the reference's own B=2
    output encodes its VMatrix batch-layout defect and is covered on CPU in test_oracle_golden)."""
    from banet_amd import bundlenet
    c = cases.case_resize()
    Rs_o, Ts_o = orc.camera_resize(c["intr"], c["layers"], c["points"], c["depth"], c["mlp"])
    Rb_o, Tb_o, Db_o = orc.bundle_resize(c["intr"], c["layers"], c["points"], c["basis"], c["depth"], c["mlp"],
                                         init_rotation=Rs_o[-1], init_translation=Ts_o[-1])
    net = bundlenet.BundleNet(lambda_weights=c["mlp"])
    layers = [t(l) for l in c["layers"]]
    Rs, Ts = net.CameraResize(t(c["intr"]), layers, t(c["points"]), t(c["depth"]))
    for a, b in zip(Rs + Ts, Rs_o + Ts_o):
        assert relerr(n(a), b) < 1e-4, relerr(n(a), b)
    Rb, Tb, Db = net.BundleResize(t(c["intr"]), layers, t(c["points"]), t(c["basis"]), t(c["depth"]),
                                  init_rotation=t(Rs_o[-1]), init_translation=t(Ts_o[-1]))
    for a, b in zip(Rb + Tb + Db, Rb_o + Tb_o + Db_o):
        assert relerr(n(a), b) < 1e-4, relerr(n(a), b)


# ======================================================================================
# (2b) per-level preparation kernels
# ======================================================================================
@pytest.mark.parametrize("B,H,W,C,N", [(2, 24, 32, 128, 500), (1, 17, 23, 7, 64), (3, 8, 8, 200, 33)])
def test_resample_kernels_match_oracle(B, H, W, C, N):
    from banet_amd import ops
    rng = np.random.RandomState(B + H + C)
    img = rng.standard_normal((B, H, W, C)).astype(np.float32)
    warp = np.stack([rng.uniform(-3, W + 2, (B, N)), rng.uniform(-3, H + 2, (B, N))], -1).astype(np.float32)
    warp[:, 0] = [0.0, 0.0]                      # exact corners / integer coordinates / borders of the zero-pad rule
    warp[:, 1] = [W - 1.0, H - 1.0]
    warp[:, 2] = [-1.0, 2.5]
    warp[:, 3] = [W - 0.5, H - 0.25]
    warp[:, 4] = [-0.5, -0.75]
    warp[:, 5] = [float(W), 1.0]
    got = n(ops.resample(t(img), t(warp), clamp=False))
    want = orc.resampler(img, warp)
    assert np.abs(got - want).max() < 2e-6 * max(1.0, np.abs(want).max())
    assert not got[:, 2].any() and not got[:, 5].any()          # x <= -1 / x >= W: exactly zero
    got2 = n(ops.resample(t(img), t(warp), clamp=True))
    want2 = orc.interpolate2d2(img, warp)
    assert np.abs(got2 - want2).max() < 2e-6 * max(1.0, np.abs(want2).max())
    np.testing.assert_array_equal(got2[:, 0], img[:, 0, 0])      # integer coordinates: the texel itself


@pytest.mark.parametrize("B,H,W,C", [(2, 30, 40, 128), (1, 5, 7, 3), (1, 2, 2, 16)])
def test_target_map_and_depth_output_match_oracle(B, H, W, C):
    from banet_amd import ops
    rng = np.random.RandomState(H * W + C)
    img = rng.standard_normal((B, H, W, C)).astype(np.float32)
    got = n(ops.target_map(t(img)))
    np.testing.assert_array_equal(got, orc.target_map(img))     # differences and 0.5 scaling are exact in fp32
    assert not got[:, 0, :, 2 * C:].any() and not got[:, :, 0, C:2 * C].any()   # REFLECT rim: zero gradient
    K = 24
    init = rng.uniform(1, 3, (B, H, W, 1)).astype(np.float32)
    basis = rng.standard_normal((B, H * W, K)).astype(np.float32)
    Wc = rng.standard_normal((B, K, 1)).astype(np.float32)
    got = n(ops.depth_output(t(init), t(basis), t(Wc)))
    want = init.astype(np.float64) + np.matmul(basis.astype(np.float64), Wc.astype(np.float64)).reshape(B, H, W, 1)
    assert got.shape == init.shape and np.abs(got - want).max() < 1e-5


# ======================================================================================
# (3) dense fused path vs the oracle
# ======================================================================================
def _torch_levels(levels):
    from banet_amd import dense as bdense
    return [bdense.DenseLevel(lv["scale"], t(lv["src"]), t(lv["tgt"]), t(lv["D0"]),
                              t(lv["basis"]) if lv["basis"].shape[-1] else None) for lv in levels]


def _scenes(B, H, W, C, K, scales, seed, normalize=True, big=False, noise=0.0):
    out = []
    for b in range(B):
        s = 1.0 + 0.5 * b
        w = np.array([0.010, -0.008, 0.006]) * s * (6 if big else 1)
        tr = np.array([0.06, -0.04, 0.03]) * s * (6 if big else 1)
        out.append(synth.make_pair_scene(H, W, C, K, scales, seed + b, normalize_rays=normalize, w_gt=w, t_gt=tr,
                                         noise=noise))
    return out


@pytest.mark.parametrize("H,W,C,K,big", [(120, 160, 128, 32, False),      # BASELINE configs[0] (cfg-1)
                                         (37, 53, 6, 5, False),           # ragged tiles, K%4 != 0, tiny C
                                         (40, 56, 7, 16, True),           # odd C, large motion: masks + rim pixels
                                         (32, 48, 200, 64, False),        # two channel chunks, NB=4
                                         (48, 64, 128, 128, True)])       # the full K of cfg-2
def test_dense_bundle_assembly_matches_oracle(H, W, C, K, big):
    from banet_amd import dense as bdense, ops
    scenes = _scenes(2, H, W, C, K, [1], 21, big=big)
    intr, levels = odense.batch_scene(scenes)
    lv = levels[0]
    rng = np.random.RandomState(3)
    R = np.stack([synth.rodrigues(rng.uniform(-1, 1, 3) * 0.004) for _ in range(2)]).astype(np.float32)
    T = np.stack([np.asarray(s["T_gt"]) * 0.8 for s in scenes]).reshape(2, 3, 1).astype(np.float32)
    Wc = (rng.standard_normal((2, K, 1)) * 0.01).astype(np.float32)
    mlps = [orc.he_normal_mlp_weights(C, 9)]
    ba = bdense.DenseBA(t(intr), _torch_levels(levels), mlps, "bundle", 1000.0)
    AtA, Atb, absres, nvalid = ops.ba_assemble(ba.problems[0], t(R), t(T), t(Wc))
    a = odense.level_inputs(intr, lv, True, np.float64)
    R2, T2, W2, dbg = orc.bundle_iteration(a["conv1"], a["conv2"], a["fx"], a["fy"], a["ox"], a["oy"], a["p"], a["D"],
                                           a["Bs"], R.astype(np.float64), T.astype(np.float64), Wc.astype(np.float64),
                                           mlps[0], 1000.0)
    nv = dbg["mask"].sum(axis=(1, 2))
    assert np.abs(n(nvalid) - nv).max() <= (1 if big else 0), (n(nvalid), nv)   # fp32 vs fp64 rim decisions
    if big:
        assert (nv < H * W).all() and (nv > 0).all()
    assert relerr(n(absres) / (H * W), dbg["avg"][:, 0]) < 1e-5
    assert relerr(n(AtA), dbg["AtA"]) < 3e-5, relerr(n(AtA), dbg["AtA"])
    assert relerr(n(Atb)[..., None], dbg["Atb"]) < 3e-5, relerr(n(Atb)[..., None], dbg["Atb"])
    np.testing.assert_array_equal(n(AtA), np.swapaxes(n(AtA), 1, 2))
    # one full iteration: lambda, damping, LU solve, SE(3)/W update
    st = ba.new_state(t(R), t(T), t(Wc))
    ops.ba_solve_update(ba.problems[0], ba.mlps[0], 1000.0, AtA, Atb, absres, nvalid, st)
    assert relerr(n(st.lambda_out), dbg["lam"].reshape(-1)) < 1e-4
    sol = dbg["solution"][:, :, 0]
    assert relerr(n(st.delta)[:, :6], sol[:, :6]) < 1e-4, relerr(n(st.delta)[:, :6], sol[:, :6])
    assert relerr(n(st.delta)[:, 6:], sol[:, 6:]) < 1e-4, relerr(n(st.delta)[:, 6:], sol[:, 6:])
    assert relerr(n(st.R), R2) < 1e-5 and relerr(n(st.T), T2) < 1e-4 and relerr(n(st.Wc), W2) < 1e-4


def test_dense_cfg1_three_iterations_match_oracle_stepwise():
    """BASELINE configs[0]: 2-frame 160x120 single scale, K=32, 3 LM iterations, batch 1.
    Each HIP iteration is compared with the fp32 oracle started from the same state."""
    from banet_amd import dense as bdense, ops
    H, W, C, K = 120, 160, 128, 32
    scenes = _scenes(1, H, W, C, K, [1], 5, noise=0.01)
    intr, levels = odense.batch_scene(scenes)
    mlps = [orc.he_normal_mlp_weights(C, 2)]
    ba = bdense.DenseBA(t(intr), _torch_levels(levels), mlps, "bundle", 1000.0)
    T0 = (np.asarray(scenes[0]["T_gt"]) * 0.7).reshape(1, 3, 1).astype(np.float32)
    st = ba.new_state(T=t(T0))
    a = odense.level_inputs(intr, levels[0], True, np.float32)
    for it in range(3):
        R, T, Wc = n(st.R).copy(), n(st.T).copy(), n(st.Wc).copy()
        R2, T2, W2, dbg = orc.bundle_iteration(a["conv1"], a["conv2"], a["fx"], a["fy"], a["ox"], a["oy"], a["p"],
                                               a["D"], a["Bs"], R, T, Wc, mlps[0], 1000.0)
        ops.lm_level(ba.problems[0], ba.mlps[0], 1000.0, 1, False, st, ws=ba.ws)
        sol = dbg["solution"][:, :, 0]
        e_pose, e_w = relerr(n(st.delta)[:, :6], sol[:, :6]), relerr(n(st.delta)[:, 6:], sol[:, 6:])
        assert e_pose < 1e-4 and e_w < 1e-4, (it, e_pose, e_w)
        assert relerr(n(st.T), T2) < 1e-4 and relerr(n(st.Wc), W2) < 1e-4
        assert int(st.iters[0]) == 1


def test_dense_multilevel_bundle_solve_matches_oracle():
    from banet_amd import dense as bdense
    B, H, W, C, K = 2, 48, 64, 16, 8
    scenes = _scenes(B, H, W, C, K, [4, 2, 1], 31)
    intr, levels = odense.batch_scene(scenes)
    mlps = [orc.he_normal_mlp_weights(C, 5 + i) for i in range(3)]
    T0 = np.stack([np.asarray(s["T_gt"]) * 0.7 for s in scenes]).reshape(B, 3, 1).astype(np.float32)
    iters = [3, 3, 2]
    R = np.tile(np.eye(3, dtype=np.float32)[None], (B, 1, 1))
    T, Wc = T0.copy(), np.zeros((B, K, 1), np.float32)
    for li, lv in enumerate(levels):
        a = odense.level_inputs(intr, lv, True)
        for _ in range(iters[li]):
            R, T, Wc, _ = orc.bundle_iteration(a["conv1"], a["conv2"], a["fx"], a["fy"], a["ox"], a["oy"], a["p"],
                                               a["D"], a["Bs"], R, T, Wc, mlps[li], 1000.0)
    ba = bdense.DenseBA(t(intr), _torch_levels(levels), mlps, "bundle", 1000.0)
    st, counts = ba.solve(iters, ba.new_state(T=t(T0)))
    assert [int(c[0]) for c in counts] == iters
    assert relerr(n(st.R), R) < 1e-4 and relerr(n(st.T), T) < 1e-4 and relerr(n(st.Wc), Wc) < 2e-4, \
        (relerr(n(st.R), R), relerr(n(st.T), T), relerr(n(st.Wc), Wc))
    # and the BA went the right way
    for b in range(B):
        assert np.abs(n(st.T)[b, :, 0] - scenes[b]["T_gt"]).max() < np.abs(T0[b, :, 0] - scenes[b]["T_gt"]).max()


def test_dense_pose_only_variant_matches_oracle():
    from banet_amd import dense as bdense
    B, H, W, C = 2, 40, 56, 12
    scenes = _scenes(B, H, W, C, 0, [2, 1], 41)
    intr, levels = odense.batch_scene(scenes)
    mlps = [orc.he_normal_mlp_weights(C, 5 + i) for i in range(2)]
    R, T, _, _ = odense.solve_bundle(intr, levels, mlps, [3, 3], pose_only=True)
    ba = bdense.DenseBA(t(intr), _torch_levels(levels), mlps, "bundle_camera")
    st, _ = ba.solve([3, 3])
    assert relerr(n(st.R), R) < 1e-4 and relerr(n(st.T), T) < 1e-4, (relerr(n(st.R), R), relerr(n(st.T), T))


# ======================================================================================
# (3b) multi-frame windows (SURVEY.md 8(d) definition; BASELINE configs[2..3] are 5-frame windows)
# ======================================================================================
def _window_scenes(B, H, W, C, K, scales, seed, pairs):
    return [synth.make_window_scene(H, W, C, K, scales, seed + b, pairs, rot_mag=0.012 * (1 + 0.3 * b),
                                    trans_mag=0.04 * (1 + 0.3 * b)) for b in range(B)]


@pytest.mark.parametrize("H,W,C,K,pairs", [(40, 56, 128, 128, 4),    # cfg-3/4 shape class: 5 frames, C = K = 128 (direct SYRK, 2 record block rows)
                                           (40, 56, 128, 64, 2),     # 3 frames, K = 64 (direct SYRK, 1 block row)
                                           (37, 53, 12, 16, 3),      # generic gather + LDS-tiled SYRK passes
                                           (40, 56, 128, 32, 5)])    # 6 frames: more pairs than the direct kernel takes
def test_window_assembly_and_iteration_match_oracle(H, W, C, K, pairs):
    from banet_amd import dense as bdense, ops
    B = 2
    scenes = _window_scenes(B, H, W, C, K, [1], 77, pairs)
    intr, levels = odense.batch_window_scene(scenes)
    lv = levels[0]
    rng = np.random.RandomState(4)
    R = np.stack([[synth.rodrigues(rng.uniform(-1, 1, 3) * 0.004) for _ in range(pairs)] for _ in range(B)]).astype(np.float32)
    T = (np.stack([s["T_gt"] for s in scenes]) * 0.8).reshape(B, pairs, 3, 1).astype(np.float32)
    Wc = (rng.standard_normal((B, K, 1)) * 0.01).astype(np.float32)
    mlps = [orc.he_normal_mlp_weights(C, 9)]
    ba = bdense.DenseBA(t(intr), _torch_levels(levels), mlps, "bundle", 1000.0)
    assert ba.pairs == pairs and ba.problems[0].P == 6 * pairs + K
    AtA, Atb, absres, nvalid = ops.ba_assemble(ba.problems[0], t(R), t(T), t(Wc))
    one = dict(lv)
    one["tgt"] = lv["tgt"][:, 0]
    a = odense.level_inputs(intr, one, True, np.float64)
    conv2s = [orc.target_map(lv["tgt"][:, i].astype(np.float64)) for i in range(pairs)]
    Rn, Tn, Wn, dbg = orc.bundle_window_iteration(a["conv1"], conv2s, a["fx"], a["fy"], a["ox"], a["oy"], a["p"], a["D"],
                                                  a["Bs"], [R[:, i].astype(np.float64) for i in range(pairs)],
                                                  [T[:, i].astype(np.float64) for i in range(pairs)],
                                                  Wc.astype(np.float64), mlps[0], 1000.0)
    nv = sum(m.sum(axis=(1, 2)) for m in dbg["mask"])
    assert np.abs(n(nvalid) - nv).max() <= 1, (n(nvalid), nv)
    assert relerr(n(absres) / (H * W * pairs), dbg["avg"][:, 0]) < 1e-5
    got = n(AtA)
    assert relerr(got, dbg["AtA"]) < 3e-5, relerr(got, dbg["AtA"])
    assert relerr(n(Atb)[..., None], dbg["Atb"]) < 3e-5
    np.testing.assert_array_equal(got, np.swapaxes(got, 1, 2))
    for i in range(pairs):                              # block arrowhead: poses of different frames do not couple
        for j in range(pairs):
            if i != j:
                assert not got[:, 6 * i:6 * i + 6, 6 * j:6 * j + 6].any()
    st = ba.new_state(t(R.reshape(B * pairs, 3, 3)), t(T.reshape(B * pairs, 3, 1)), t(Wc))
    ops.ba_solve_update(ba.problems[0], ba.mlps[0], 1000.0, AtA, Atb, absres, nvalid, st)
    sol = dbg["solution"][:, :, 0]
    assert relerr(n(st.lambda_out), dbg["lam"].reshape(-1)) < 1e-4
    assert relerr(n(st.delta)[:, :6 * pairs], sol[:, :6 * pairs]) < 1e-4
    assert relerr(n(st.delta)[:, 6 * pairs:], sol[:, 6 * pairs:]) < 1e-4
    assert relerr(n(st.R), np.stack(Rn, 1)) < 1e-5 and relerr(n(st.T), np.stack(Tn, 1)) < 1e-4 and relerr(n(st.Wc), Wn) < 1e-4


@pytest.mark.parametrize("seed", range(8))
def test_random_shape_sweep_assembly_matches_oracle(seed):
    """seeded random shapes (ragged tiles, tiny / odd channel counts, K not a multiple of 4, 1-3 target frames,
    both gather kernels, both SYRK kernels, pose-only and bundle) against the float64 oracle"""
    from banet_amd import dense as bdense, ops
    rng = np.random.RandomState(1000 + seed)
    B = int(rng.randint(1, 4))
    H, W = int(rng.randint(9, 41)), int(rng.randint(9, 61))
    C = int(rng.choice([1, 2, 3, 5, 8, 13, 20, 128, 128]))
    K = int(rng.choice([0, 1, 3, 4, 7, 16, 20, 32, 64]))
    pairs = int(rng.randint(1, 4))
    scenes = [synth.make_window_scene(H, W, C, K, [1], 500 + 10 * seed + b, pairs, rot_mag=0.02, trans_mag=0.08) for b in range(B)]
    intr, levels = odense.batch_window_scene(scenes)
    lv = levels[0]
    R = np.stack([[synth.rodrigues(rng.uniform(-1, 1, 3) * 0.006) for _ in range(pairs)] for _ in range(B)]).astype(np.float32)
    T = (np.stack([s["T_gt"] for s in scenes]) * 0.8).reshape(B, pairs, 3, 1).astype(np.float32)
    Wc = (rng.standard_normal((B, K, 1)) * 0.01).astype(np.float32)
    mlps = [orc.he_normal_mlp_weights(C, 9)]
    ba = bdense.DenseBA(t(intr), _torch_levels(levels), mlps, "bundle" if K else "bundle_camera", 1000.0)
    AtA, Atb, absres, nvalid = ops.ba_assemble(ba.problems[0], t(R), t(T), t(Wc) if K else None)
    one = dict(lv)
    one["tgt"] = lv["tgt"][:, 0]
    a = odense.level_inputs(intr, one, True, np.float64)
    R64 = [R[:, i].astype(np.float64) for i in range(pairs)]
    T64 = [T[:, i].astype(np.float64) for i in range(pairs)]
    if K:
        conv2s = [orc.target_map(lv["tgt"][:, i].astype(np.float64)) for i in range(pairs)]
        dbg = orc.bundle_window_iteration(a["conv1"], conv2s, a["fx"], a["fy"], a["ox"], a["oy"], a["p"], a["D"], a["Bs"],
                                          R64, T64, Wc.astype(np.float64), mlps[0], 1000.0)[3]
        want_A, want_b = dbg["AtA"], dbg["Atb"]
    else:                                                         # pose only: independent 6x6 systems per target frame
        P = 6 * pairs
        want_A, want_b = np.zeros((B, P, P)), np.zeros((B, P, 1))
        for i in range(pairs):
            d = orc.bundle_camera_iteration(a["conv1"], orc.target_map(lv["tgt"][:, i].astype(np.float64)), a["fx"], a["fy"],
                                            a["ox"], a["oy"], a["p"], a["D"], R64[i], T64[i], mlps[0], 1.0)[2]
            want_A[:, 6 * i:6 * i + 6, 6 * i:6 * i + 6] = d["AtA"]
            want_b[:, 6 * i:6 * i + 6] = d["Atb"]
    cfg = (B, H, W, C, K, pairs)
    assert relerr(n(AtA), want_A) < 5e-5, (cfg, relerr(n(AtA), want_A))
    assert relerr(n(Atb)[..., None], want_b) < 5e-5, (cfg, relerr(n(Atb)[..., None], want_b))
    np.testing.assert_array_equal(n(AtA), np.swapaxes(n(AtA), 1, 2))


@pytest.mark.parametrize("H,W,K,big,pairs", [(48, 64, 128, False, 1), (40, 56, 16, True, 1), (37, 53, 0, True, 2), (64, 96, 64, False, 3)])
def test_patch_gather_kernel_matches_oracle(H, W, K, big, pairs):
    """ba_gather128p_kernel (the default on large levels) forced at oracle-sized inputs: staged step pairs, pairs that
    fall back to direct loads (large motion), rim pixels, masked pixels, ragged tiles, several target frames."""
    from banet_amd import dense as bdense, ops
    B, C = 2, 128
    scenes = [synth.make_window_scene(H, W, C, K, [1], 300 + b, pairs, rot_mag=0.012 * (6 if big else 1),
                                      trans_mag=0.05 * (6 if big else 1)) for b in range(B)]
    intr, levels = odense.batch_window_scene(scenes)
    lv = levels[0]
    rng = np.random.RandomState(8)
    R = np.stack([[synth.rodrigues(rng.uniform(-1, 1, 3) * 0.004) for _ in range(pairs)] for _ in range(B)]).astype(np.float32)
    T = (np.stack([s["T_gt"] for s in scenes]) * 0.8).reshape(B, pairs, 3, 1).astype(np.float32)
    Wc = (rng.standard_normal((B, K, 1)) * 0.01).astype(np.float32)
    mlps = [orc.he_normal_mlp_weights(C, 9)]
    ba = bdense.DenseBA(t(intr), _torch_levels(levels), mlps, "bundle" if K else "bundle_camera", 1000.0)
    outs = {}
    PATCH, DIRECT, PATCH_LOOP = ops.capi.DEV_FORCE_PATCH_GATHER, ops.capi.DEV_DIRECT_GATHER, ops.capi.DEV_FORCE_PATCH_GATHER | ops.capi.DEV_PATCH_PAIR_LOOP
    for bits in (PATCH, DIRECT, PATCH_LOOP):                           # patch kernel forced / direct kernel / patch kernel with the
        ba.problems[0].c.flags = bits                         # target frames looped over inside a tile (large levels)
        outs[bits] = [n(x) for x in ops.ba_assemble(ba.problems[0], t(R), t(T), t(Wc) if K else None)]
    ba.problems[0].c.flags = 0
    for x, y in zip(outs[PATCH], outs[DIRECT]):
        assert relerr(x, y) < 2e-6, relerr(x, y)
    for x, y in zip(outs[PATCH_LOOP], outs[PATCH]):                 # same arithmetic per pair: identical bits
        np.testing.assert_array_equal(x, y)
    one = dict(lv)
    one["tgt"] = lv["tgt"][:, 0]
    a = odense.level_inputs(intr, one, True, np.float64)
    R64 = [R[:, i].astype(np.float64) for i in range(pairs)]
    T64 = [T[:, i].astype(np.float64) for i in range(pairs)]
    if K:
        conv2s = [orc.target_map(lv["tgt"][:, i].astype(np.float64)) for i in range(pairs)]
        dbg = orc.bundle_window_iteration(a["conv1"], conv2s, a["fx"], a["fy"], a["ox"], a["oy"], a["p"], a["D"], a["Bs"],
                                          R64, T64, Wc.astype(np.float64), mlps[0], 1000.0)[3]
        assert relerr(outs[PATCH][0], dbg["AtA"]) < 3e-5 and relerr(outs[PATCH][1][..., None], dbg["Atb"]) < 3e-5
        nv = sum(m.sum(axis=(1, 2)) for m in dbg["mask"])
        assert np.abs(outs[PATCH][3] - nv).max() <= 1
        if big:
            assert (nv < H * W * pairs).all()                     # some pixels really leave the image
    else:
        for i in range(pairs):
            d = orc.bundle_camera_iteration(a["conv1"], orc.target_map(lv["tgt"][:, i].astype(np.float64)), a["fx"], a["fy"],
                                            a["ox"], a["oy"], a["p"], a["D"], R64[i], T64[i], mlps[0], 1.0)[2]
            assert relerr(outs[PATCH][0][:, 6 * i:6 * i + 6, 6 * i:6 * i + 6], d["AtA"]) < 3e-5


@pytest.mark.parametrize("C,K,pairs", [(128, 256, 7), (12, 200, 2), (128, 256, 1), (128, 128, 6), (20, 256, 5)])
def test_large_basis_windows_match_oracle(C, K, pairs):
    """BASELINE configs[4] class: K = 256 coefficients, up to 8 frames (P = 6*7 + 256 = 298).  K = 256 (and K = 128 with
    more than 4 target frames) runs the job kernels of syrk_wide.hip, K = 200 the LDS-tiled SYRK with 16 block rows; the
    solve keeps its matrix in the caller's workspace when it does not fit in LDS."""
    from banet_amd import dense as bdense, ops
    B, H, W = 2, 32, 40
    scenes = _window_scenes(B, H, W, C, K, [1], 55, pairs)
    intr, levels = odense.batch_window_scene(scenes)
    lv = levels[0]
    mlps = [orc.he_normal_mlp_weights(C, 9)]
    T0 = (np.stack([s["T_gt"] for s in scenes]) * 0.8).reshape(B, pairs, 3, 1).astype(np.float32)
    ba = bdense.DenseBA(t(intr), _torch_levels(levels), mlps, "bundle", 1000.0)
    assert ba.problems[0].P == 6 * pairs + K
    R = np.tile(np.eye(3, dtype=np.float32)[None, None], (B, pairs, 1, 1))
    Wc = np.zeros((B, K, 1), np.float32)
    AtA, Atb, absres, nvalid = ops.ba_assemble(ba.problems[0], t(R), t(T0), t(Wc))
    one = dict(lv)
    one["tgt"] = lv["tgt"][:, 0]
    a = odense.level_inputs(intr, one, True, np.float64)
    conv2s = [orc.target_map(lv["tgt"][:, i].astype(np.float64)) for i in range(pairs)]
    Rn, Tn, Wn, dbg = orc.bundle_window_iteration(a["conv1"], conv2s, a["fx"], a["fy"], a["ox"], a["oy"], a["p"], a["D"], a["Bs"],
                                                  [R[:, i].astype(np.float64) for i in range(pairs)],
                                                  [T0[:, i].astype(np.float64) for i in range(pairs)], Wc.astype(np.float64),
                                                  mlps[0], 1000.0)
    assert relerr(n(AtA), dbg["AtA"]) < 3e-5 and relerr(n(Atb)[..., None], dbg["Atb"]) < 3e-5
    np.testing.assert_array_equal(n(AtA), np.swapaxes(n(AtA), 1, 2))
    st, counts = ba.solve([1], ba.new_state(T=t(T0.reshape(B * pairs, 3, 1))))       # one full LM iteration through banet_lm_level_f32
    sol = dbg["solution"][:, :, 0]
    assert int(counts[0][0]) == 1
    assert relerr(n(st.delta)[:, :6 * pairs], sol[:, :6 * pairs]) < 1e-4, relerr(n(st.delta)[:, :6 * pairs], sol[:, :6 * pairs])
    assert relerr(n(st.delta)[:, 6 * pairs:], sol[:, 6 * pairs:]) < 1e-4, relerr(n(st.delta)[:, 6 * pairs:], sol[:, 6 * pairs:])
    Rg = n(st.R).reshape(B, pairs, 3, 3)
    Tg = n(st.T).reshape(B, pairs, 3, 1)
    assert relerr(Rg, np.stack(Rn, 1)) < 1e-5 and relerr(Tg, np.stack(Tn, 1)) < 1e-4 and relerr(n(st.Wc), Wn) < 1e-4


def test_window_multilevel_solve_matches_oracle_and_converges():
    """5-frame window (4 target frames), 3 levels, fp32 oracle from the same start."""
    from banet_amd import dense as bdense
    B, H, W, C, K, pairs = 2, 48, 64, 16, 8, 4
    scenes = _window_scenes(B, H, W, C, K, [4, 2, 1], 91, pairs)
    intr, levels = odense.batch_window_scene(scenes)
    mlps = [orc.he_normal_mlp_weights(C, 5 + i) for i in range(3)]
    T0 = (np.stack([s["T_gt"] for s in scenes]) * 0.7).reshape(B, pairs, 3, 1).astype(np.float32)
    iters = [3, 3, 2]
    Rs, Ts, Wo, hist = odense.solve_bundle_window(intr, levels, mlps, iters, T0=T0)
    ba = bdense.DenseBA(t(intr), _torch_levels(levels), mlps, "bundle", 1000.0)
    st, counts = ba.solve(iters, ba.new_state(T=t(T0.reshape(B * pairs, 3, 1))))
    assert [int(c[0]) for c in counts] == iters
    eR, eT, eW = relerr(n(st.R), np.stack(Rs, 1)), relerr(n(st.T), np.stack(Ts, 1)), relerr(n(st.Wc), Wo)
    assert eR < 1e-4 and eT < 1e-4 and eW < 2e-4, (eR, eT, eW)
    for b in range(B):
        for i in range(pairs):
            assert np.abs(n(st.T)[b, i, :, 0] - scenes[b]["T_gt"][i]).max() < np.abs(T0[b, i, :, 0] - scenes[b]["T_gt"][i]).max()


def test_window_with_one_pair_is_the_two_frame_path_bit_for_bit():
    from banet_amd import dense as bdense, ops
    H, W, C, K = 40, 56, 128, 128
    scenes = _window_scenes(2, H, W, C, K, [1], 13, 1)
    intr, levels = odense.batch_window_scene(scenes)
    mlps = [orc.he_normal_mlp_weights(C, 9)]
    T = (np.stack([s["T_gt"] for s in scenes]) * 0.8).reshape(2, 3, 1).astype(np.float32)
    R = np.tile(np.eye(3, dtype=np.float32)[None], (2, 1, 1))
    Wc = np.zeros((2, K, 1), np.float32)
    outs = []
    for five_d in (True, False):
        lv = [bdense.DenseLevel(l["scale"], t(l["src"]), t(l["tgt"] if five_d else l["tgt"][:, 0]), t(l["D0"]), t(l["basis"]))
              for l in levels]
        ba = bdense.DenseBA(t(intr), lv, mlps, "bundle", 1000.0)
        outs.append([n(x) for x in ops.ba_assemble(ba.problems[0], t(R), t(T), t(Wc))])
    for x, y in zip(*outs):
        np.testing.assert_array_equal(x, y)


def test_dense_legacy_lm_iteration_counts_identical():
    """legacy/ba.py early-terminated LM, three windows with different motions (so that the
    per-window loops stop at different iterations), device-side loop control."""
    from banet_amd import dense as bdense
    B, H, W, C = 3, 48, 64, 8
    scenes = _scenes(B, H, W, C, 0, [4, 2, 1], 51, normalize=False)
    intr, levels = odense.batch_scene(scenes)
    mlps = [orc.he_normal_mlp_weights(C, 5 + i) for i in range(3)]
    iters = [3, 5, 7]
    R, T, ratio, counts = odense.solve_legacy(intr, levels, mlps, iters, early_termination=True)
    ba = bdense.DenseBA(t(intr), _torch_levels(levels), mlps, "legacy_lm")
    st, got = ba.solve(iters, early_termination=True)
    got = [[int(v) for v in c] for c in got]
    assert got == counts, (got, counts)
    assert relerr(n(st.R), R) < 1e-4 and relerr(n(st.T), T) < 1e-4, (relerr(n(st.R), R), relerr(n(st.T), T))
    assert relerr(n(st.ratio), ratio) < 1e-5
    # fixed-count legacy iteration (legacy/ba.py:148-214)
    R, T, ratio, counts = odense.solve_legacy(intr, levels, mlps, iters, early_termination=False)
    ba = bdense.DenseBA(t(intr), _torch_levels(levels), mlps, "legacy_fixed")
    st, got = ba.solve(iters, early_termination=False)
    assert [[int(v) for v in c] for c in got] == counts
    assert relerr(n(st.R), R) < 1e-4 and relerr(n(st.T), T) < 1e-4


def test_all_pixels_masked_and_zero_motion_edge_cases():
    from banet_amd import dense as bdense, ops
    B, H, W, C, K = 1, 24, 32, 8, 4
    scenes = _scenes(B, H, W, C, K, [1], 61)
    intr, levels = odense.batch_scene(scenes)
    ba = bdense.DenseBA(t(intr), _torch_levels(levels), [orc.he_normal_mlp_weights(C, 1)], "bundle", 1000.0)
    far = t(np.array([[[50.0], [0.0], [0.0]]]))                             # everything projects outside
    AtA, Atb, absres, nvalid = ops.ba_assemble(ba.problems[0], t(np.eye(3)[None]), far, t(np.zeros((1, K, 1))))
    assert float(nvalid[0]) == 0.0 and float(AtA.abs().max()) == 0.0 and float(Atb.abs().max()) == 0.0
    assert float(absres.abs().max()) == 0.0
    # identical frames + identity pose: zero residual, zero update, finite pose (the reference gives NaN here)
    lv = dict(levels[0])
    lv["src"] = lv["tgt"].copy()
    ba = bdense.DenseBA(t(intr), _torch_levels([lv]), [orc.he_normal_mlp_weights(C, 1)], "bundle_camera")
    st, _ = ba.solve([2])
    assert torch.isfinite(st.R).all() and torch.isfinite(st.T).all()
    assert relerr(n(st.R), np.eye(3)[None]) < 1e-6 and float(st.T.abs().max()) < 1e-6


# ======================================================================================
# (4) BASELINE.json full size: size-independent properties + float64 twin on the GPU
# ======================================================================================
@pytest.fixture(scope="module")
def full_size():
    from banet_amd import dense as bdense, synth as bsynth
    B, H, W, C, K = 2, 480, 640, 128, 128
    torch.manual_seed(0)
    intr, levels, gt = bsynth.make_dense_windows(B, H, W, C, K, [4, 1], 77, DEV, trans_mag=0.06)
    mlps = [orc.he_normal_mlp_weights(C, 5 + i) for i in range(2)]
    ba = bdense.DenseBA(intr, levels, mlps, "bundle", 1000.0)
    return ba, intr, levels, gt


def test_full_size_assembly_matches_float64_twin(full_size):
    from banet_amd import ops
    ba, intr, levels, gt = full_size
    B, K = 2, 128
    R = torch.eye(3, device=DEV).repeat(B, 1, 1)
    T = (gt["T"] * 0.7).reshape(B, 3, 1).to(DEV)
    Wc = torch.zeros(B, K, 1, device=DEV)
    for li, lv in enumerate(levels):
        AtA, Atb, absres, nvalid = ops.ba_assemble(ba.problems[li], R, T, Wc)
        for b in range(B):                                                  # one window at a time (memory)
            r = torch_ref.dense_assemble(intr[b:b + 1], lv.scale, lv.src[b:b + 1], lv.tgt[b:b + 1], lv.depth[b:b + 1],
                                         lv.basis[b:b + 1], R[b:b + 1], T[b:b + 1], Wc[b:b + 1], True, True)
            assert float(nvalid[b]) == float(r[3][0])
            assert relerr(n(AtA[b]), n(r[0][0])) < 3e-5, (li, b, relerr(n(AtA[b]), n(r[0][0])))
            assert relerr(n(Atb[b]), n(r[1][0])) < 3e-5, (li, b, relerr(n(Atb[b]), n(r[1][0])))
            assert relerr(n(absres[b]), n(r[2][0])) < 1e-5


def test_full_size_properties(full_size):
    from banet_amd import dense as bdense, ops
    ba, intr, levels, gt = full_size
    B, K = 2, 128
    R = torch.eye(3, device=DEV).repeat(B, 1, 1)
    T = (gt["T"] * 0.7).reshape(B, 3, 1).to(DEV)
    Wc = torch.zeros(B, K, 1, device=DEV)
    p = ba.problems[1]
    out1 = ops.ba_assemble(p, R, T, Wc)
    out2 = ops.ba_assemble(p, R, T, Wc)
    for a, b in zip(out1, out2):                                            # run-to-run determinism
        assert torch.equal(a, b)
    AtA, Atb, absres, nvalid = out1
    assert torch.equal(AtA, AtA.transpose(1, 2))                            # exact symmetry
    assert (torch.diagonal(AtA, dim1=1, dim2=2) >= 0).all()
    assert (torch.linalg.eigvalsh(AtA.double()) > -1e-6 * AtA.abs().amax()).all()   # PSD up to rounding
    assert (nvalid <= 640 * 480).all() and (nvalid > 0.9 * 640 * 480).all()
    # batch-order invariance: windows are independent problems
    lv = levels[1]
    swap = [1, 0]
    lv2 = bdense.DenseLevel(lv.scale, lv.src[swap].contiguous(), lv.tgt[swap].contiguous(),
                            lv.depth[swap].contiguous(), lv.basis[swap].contiguous())
    ba2 = bdense.DenseBA(intr[swap].contiguous(), [lv2], [orc.he_normal_mlp_weights(128, 6)], "bundle", 1000.0)
    o = ops.ba_assemble(ba2.problems[0], R[swap].contiguous(), T[swap].contiguous(), Wc[swap].contiguous())
    assert torch.equal(o[0][swap], AtA) and torch.equal(o[1][swap], Atb)
    # exact scaling: features x2  =>  AtA x4, Atb x4, |r| x2 (powers of two: bit exact)
    lv3 = bdense.DenseLevel(lv.scale, lv.src * 2, lv.tgt * 2, lv.depth, lv.basis)
    ba3 = bdense.DenseBA(intr, [lv3], [orc.he_normal_mlp_weights(128, 6)], "bundle", 1000.0)
    o3 = ops.ba_assemble(ba3.problems[0], R, T, Wc)
    assert torch.equal(o3[0], AtA * 4) and torch.equal(o3[1], Atb * 4) and torch.equal(o3[2], absres * 2)


def test_full_size_solve_reduces_residual_and_pose_error(full_size):
    from banet_amd import ops
    ba, intr, levels, gt = full_size
    B = 2
    T0 = (gt["T"] * 0.7).reshape(B, 3, 1).to(DEV)
    st = ba.new_state(T=T0)
    before = ops.ba_assemble(ba.problems[1], st.R, st.T, st.Wc)[2].sum(1)
    st, counts = ba.solve([4, 4], st)
    after = ops.ba_assemble(ba.problems[1], st.R, st.T, st.Wc)[2].sum(1)
    assert [int(c[0]) for c in counts] == [4, 4]
    assert (after < before).all(), (before, after)
    e0 = (T0[:, :, 0].cpu() - gt["T"]).abs().amax(1)
    e1 = (st.T[:, :, 0].cpu() - gt["T"]).abs().amax(1)
    assert (e1 < e0).all(), (e0, e1)
    assert torch.isfinite(st.Wc).all() and torch.isfinite(st.R).all()


# ======================================================================================
# (5) caller: the keyframe sequence driver (legacy/seq_example.py:150-208)
# ======================================================================================
def test_keyframe_sequence_driver_matches_oracle():
    from banet_amd import legacy, sequence
    from oracle import sequence as oseq
    H, W, C, N = 96, 128, 8, 512
    poses = [((0, 0, 0), (0, 0, 0))] + [((0.004 * i, -0.003 * i, 0.002 * i), (0.02 * i, -0.012 * i, 0.008 * i)) for i in range(1, 5)]
    seq = synth.make_plane_sequence(H, W, C, poses, 3)
    stamps = [0.0, 0.04, 0.08, 0.12, 0.16]                      # frame 3 is > 0.1 s after key frame 0: it becomes the key frame
    mlps = {str(l): orc.he_normal_mlp_weights(C, 40 + l) for l in (1, 2, 3)}
    iters = [5, 8, 8]
    picks = {}

    def select(i):                                            # same points for both sides (host logic, fixed seed per key frame)
        if i not in picks:
            picks[i] = sequence.valid_point_and_depth(seq["images"][i], seq["depths"][i], N, 5.0, np.random.RandomState(100 + i))
        return picks[i]

    want = oseq.run_sequence(seq["intr"], seq["frames"], stamps, select, mlps, iters)

    class FixedRng:                                           # the driver draws its points through rng.randint
        def __init__(self):
            self.key = 0

        def randint(self, lo, hi, num):
            return np.random.RandomState(100 + self.key).randint(lo, hi, num)

    legacy.early_termination = True
    rng = FixedRng()
    drv = sequence.KeyframeTracker(legacy.Tracker(lambda_weights=mlps, iters=iters), seq["intr"], iters=iters, num_points=N,
                                   thres=5.0, rng=rng, device=DEV)
    drv.start([t(l) for l in seq["frames"][0]], seq["images"][0], seq["depths"][0], stamps[0])
    got = []
    for i in range(1, 5):
        rng.key = i
        got.append(drv.track([t(l) for l in seq["frames"][i]], seq["images"][i], seq["depths"][i], stamps[i]))
    assert [g["new_keyframe"] for g in got] == [w["new_keyframe"] for w in want] == [False, False, True, False]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g["iters"] == w["iters"], (i, g["iters"], w["iters"])
        assert relerr(n(g["rotation"]), w["rotation"]) < 1e-4 and relerr(n(g["translation"]), w["translation"]) < 1e-4
        assert relerr(n(g["globalRotation"]), w["globalRotation"]) < 1e-4
        assert relerr(n(g["globalTranslation"]), w["globalTranslation"]) < 1e-4
        assert abs(g["keep_ratio"] - w["keep_ratio"]) < 1e-5
        assert np.abs(n(g["camera"]) - w["camera"]).max() < 1e-4 * max(1.0, np.abs(w["camera"]).max())
        x, y, z, qw = g["quaternion"]                                   # TUM line: quaternion of the transposed global rotation
        Rq = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * qw), 2 * (x * z + y * qw)],
                       [2 * (x * y + z * qw), 1 - 2 * (x * x + z * z), 2 * (y * z - x * qw)],
                       [2 * (x * z - y * qw), 2 * (y * z + x * qw), 1 - 2 * (x * x + y * y)]])
        assert np.abs(Rq - n(g["globalRotation"])[0].T).max() < 1e-5
        assert len(g["tum"].split()) == 8 and abs(float(g["tum"].split()[1]) - float(n(g["camera"])[0])) < 1e-12
    # the tracker recovers the motion (frame 1 vs key frame 0; legacy z-depth convention)
    R1 = synth.rodrigues(np.asarray(poses[1][0], np.float64))
    assert np.abs(n(got[0]["rotation"])[0] - R1).max() < 2e-3
    assert np.abs(n(got[0]["translation"])[0, :, 0] - np.asarray(poses[1][1])).max() < 5e-3


# ======================================================================================
# (6) the layer as a differentiable op (north_star: "differentiable BA layer"): training graph =
#     differentiable tensor ops + equation_construction with its HIP backward, as in the reference
# ======================================================================================
def _sparse_case(seed, B=2, H=24, W=32, C=6, K=5, N=300):
    rng = np.random.RandomState(seed)
    sc = [synth.make_pair_scene(H, W, C, K, [1], seed + b, normalize_rays=True) for b in range(B)]
    intr, levels = odense.batch_scene(sc)
    lv = levels[0]
    pts = np.stack([rng.uniform(2, W - 3, (B, N)), rng.uniform(2, H - 3, (B, N))], -1).astype(np.float32)
    fx = np.repeat(intr[:, 0:1], N, 1); fy = np.repeat(intr[:, 1:2], N, 1)
    ox = np.repeat(intr[:, 2:3], N, 1); oy = np.repeat(intr[:, 3:4], N, 1)
    p = orc.compute_coordinates(pts, fx, fy, ox, oy, True)
    conv1 = orc.resampler(lv["src"], pts)
    conv2 = orc.target_map(lv["tgt"])
    D = orc.resampler(lv["D0"][..., None], pts)
    Bs = orc.resampler(lv["basis"], pts)
    R = np.stack([synth.rodrigues(rng.uniform(-1, 1, 3) * 0.003) for _ in range(B)]).astype(np.float32)
    T = np.stack([np.asarray(s["T_gt"]) * 0.8 for s in sc]).reshape(B, 3, 1).astype(np.float32)
    Wc = (rng.standard_normal((B, K, 1)) * 0.01).astype(np.float32)
    return dict(conv1=conv1, conv2=conv2, fx=fx, fy=fy, ox=ox, oy=oy, p=p, D=D, Bs=Bs, R=R, T=T, W=Wc,
                mlp=orc.he_normal_mlp_weights(C, 7))


@pytest.mark.parametrize("graph", ["fused", "lean", "reference"])
def test_training_graph_matches_fused_forward_and_finite_difference_gradients(graph):
    """every differentiable input of the iteration -- features, the target map, depth, basis, R, T, W AND the ten lambda-weight tensors
    (round 6: R and the weights were not checked) -- against central differences of the float64 NUMPY oracle"""
    from banet_amd.bundlenet import BundleNet
    c = _sparse_case(17)
    names = ["conv1", "conv2", "fx", "fy", "ox", "oy", "p", "D", "Bs", "R", "T", "W"]
    lw = [(t(w).requires_grad_(True), t(b).requires_grad_(True)) for w, b in c["mlp"]]
    net = BundleNet(lambda_weights={"2": lw})
    net.training_graph = graph
    args = {k: t(c[k]) for k in names}
    with torch.no_grad():
        Rf, Tf, Wf = net.BundleIteration(*[args[k] for k in names], 1000.0, "2")           # fused HIP path
    lkeys = ("conv1", "conv2", "D", "Bs", "R", "T", "W")
    leaves = {k: args[k].clone().requires_grad_(True) for k in lkeys}
    call = [leaves.get(k, args[k]) for k in names]
    Ra, Ta, Wa = net.BundleIteration(*call, 1000.0, "2")                                  # autograd graph
    assert relerr(n(Ra), n(Rf)) < 1e-5 and relerr(n(Ta), n(Tf)) < 1e-4 and relerr(n(Wa), n(Wf)) < 1e-4
    rng = np.random.RandomState(5)
    cR, cT, cW = [rng.standard_normal(x.shape) for x in (n(Ra), n(Ta), n(Wa))]
    loss = (Ra * t(cR)).sum() + (Ta * t(cT)).sum() + (Wa * t(cW)).sum()
    flat_lw = [x for wb in lw for x in wb]
    grads = torch.autograd.grad(loss, list(leaves.values()) + flat_lw)
    gl = [n(g).astype(np.float64) for g in grads[len(leaves):]]
    grads = dict(zip(leaves.keys(), [n(g).astype(np.float64) for g in grads[:len(leaves)]]))

    def oracle_loss(over, mlp=None):                                                  # float64 oracle forward
        a = {k: (over[k] if k in over else c[k]).astype(np.float64) for k in names}
        R2, T2, W2, _ = orc.bundle_iteration(a["conv1"], a["conv2"], a["fx"], a["fy"], a["ox"], a["oy"], a["p"], a["D"],
                                             a["Bs"], a["R"], a["T"], a["W"], c["mlp"] if mlp is None else mlp, 1000.0)
        return float((R2 * cR).sum() + (T2 * cT).sum() + (W2 * cW).sum())

    for k in lkeys:
        v = rng.standard_normal(c[k].shape)
        v /= np.linalg.norm(v)
        eps = 1e-4 if k in ("conv1", "conv2", "Bs") else 1e-5
        fd = (oracle_loss({k: c[k].astype(np.float64) + eps * v}) - oracle_loss({k: c[k].astype(np.float64) - eps * v})) / (2 * eps)
        ad = float((grads[k] * v).sum())
        assert abs(ad - fd) <= 3e-2 * max(abs(fd), abs(ad)) + 1e-6, (k, ad, fd)
    # the ten lambda-weight tensors (filters and biases of the five layers), one random direction each
    base = [(np.asarray(w, np.float64), np.asarray(b, np.float64)) for w, b in c["mlp"]]
    for i in range(10):
        li, isb = divmod(i, 2)
        v = rng.standard_normal(base[li][isb].shape)
        v /= np.linalg.norm(v)
        eps = 1e-5          # (the biases start at 0 and avg is small: a 1e-3 step straddles the selu kink of many units -- 6 % off)

        def shifted(sgn):
            m = [list(wb) for wb in base]
            m[li][isb] = base[li][isb] + sgn * eps * v
            return [tuple(wb) for wb in m]
        fd = (oracle_loss({}, shifted(+1)) - oracle_loss({}, shifted(-1))) / (2 * eps)
        ad = float((gl[i].reshape(v.shape) * v).sum())
        assert abs(ad - fd) <= 3e-2 * max(abs(fd), abs(ad)) + 1e-7, ("lambda tensor %d" % i, ad, fd)


def test_lean_training_graph_equals_the_reference_style_graph():
    """the two training graphs (ops.sample_stats + block-wise normal equations vs the reference's statements with the
    EquationConstruction op) give the same outputs and the same gradients w.r.t. every input and the lambda-MLP weights;
    pose-only iteration included"""
    from banet_amd.bundlenet import BundleNet
    c = _sparse_case(23)
    names = ["conv1", "conv2", "fx", "fy", "ox", "oy", "p", "D", "Bs", "R", "T", "W"]
    rng = np.random.RandomState(11)
    res = {}
    for graph in ("lean", "reference", "fused"):
        lw = [(t(w).requires_grad_(True), t(b).requires_grad_(True)) for w, b in c["mlp"]]
        net = BundleNet(lambda_weights={"2": lw})
        net.training_graph = graph
        leaves = {k: t(c[k]).requires_grad_(True) for k in ("conv1", "conv2", "D", "Bs", "R", "T", "W")}
        call = [leaves[k] if k in leaves else t(c[k]) for k in names]
        Ra, Ta, Wa = net.BundleIteration(*call, 1000.0, "2")
        if graph == "lean":
            cR, cT, cW = [t(rng.standard_normal(x.shape)) for x in (n(Ra), n(Ta), n(Wa))]
        loss = (Ra * cR).sum() + (Ta * cT).sum() + (Wa * cW).sum()
        params = list(leaves.values()) + [x for wb in lw for x in wb]
        g = torch.autograd.grad(loss, params)
        cam = [leaves[k] if k in leaves else t(c[k]) for k in names if k not in ("Bs", "W")]
        Rc, Tc = net.CameraIteration(*cam, 1.0, "2")
        gc = torch.autograd.grad((Rc * cR).sum() + (Tc * cT).sum(), [leaves[k] for k in ("conv1", "conv2", "D", "T")])
        res[graph] = ([n(Ra), n(Ta), n(Wa), n(Rc), n(Tc)], [n(x) for x in g] + [n(x) for x in gc])
    for other in ("reference", "fused"):   # fused (round 5): the whole iteration as one autograd node on the fused kernels (dense_train._SparseIteration)
        for a, b in zip(res["lean"][0], res[other][0]):
            assert relerr(a, b) < 1e-4, (other, relerr(a, b))               # the parity tolerance on updates
        for i, (a, b) in enumerate(zip(res["lean"][1], res[other][1])):
            assert relerr(a, b) < 2e-3, (other, i, relerr(a, b))


@pytest.mark.parametrize("B,N,C,H,W", [(2, 300, 128, 24, 32), (1, 77, 5, 9, 11), (2, 64, 200, 12, 16)])
def test_sample_stats_op_matches_the_torch_statements(B, N, C, H, W):
    """ops.sample_stats (HIP forward + adjoint) against bundlenet.py:230-243 written with differentiable torch ops:
    values, and gradients w.r.t. conv1, conv2 and the sampling positions; points on the rim, outside, and on integer
    coordinates included"""
    from banet_amd import ops
    from banet_amd.bundlenet import _resampler_autograd
    rng = np.random.RandomState(N + C)
    conv1 = t(rng.standard_normal((B, N, C))).requires_grad_(True)
    conv2 = t(rng.standard_normal((B, H, W, 3 * C))).requires_grad_(True)
    pos = rng.uniform(-1.5, 1.5, (B, N, 2)) + rng.uniform(0, 1, (B, N, 2)) * np.array([W - 1, H - 1])
    pos[:, :6] = np.array([[0.0, 0.0], [W - 1.0, H - 1.0], [3.0, 2.0], [W - 1.0, 1.5], [0.25, H - 1.0], [-0.5, 3.0]])
    px, py = t(pos[..., 0]).requires_grad_(True), t(pos[..., 1]).requires_grad_(True)
    cs, ca = t(rng.standard_normal((B, N, 5))), t(rng.standard_normal((B, C)))
    stats, mask, absd = ops.sample_stats(conv1, conv2, px, py)
    g_hip = torch.autograd.grad((stats * cs).sum() + (absd * ca).sum(), [conv1, conv2, px, py])
    samp = _resampler_autograd(conv2, torch.stack([px, py], dim=-1))
    m = (~((px < 0) | (px > float(W - 1)) | (py < 0) | (py > float(H - 1)))).to(torch.float32)
    d = (conv1 - samp[..., :C]) * m[..., None]
    gx, gy = samp[..., C:2 * C] * m[..., None], samp[..., 2 * C:] * m[..., None]
    ref = torch.stack([(gx * gx).sum(-1), (gx * gy).sum(-1), (gy * gy).sum(-1), (gx * d).sum(-1), (gy * d).sum(-1)], dim=-1)
    ref_abs = d.abs().sum(dim=1)
    g_ref = torch.autograd.grad((ref * cs).sum() + (ref_abs * ca).sum(), [conv1, conv2, px, py])
    assert torch.equal(mask, m)
    assert relerr(n(stats), n(ref)) < 1e-5 and relerr(n(absd), n(ref_abs)) < 1e-5
    for a, b in zip(g_hip, g_ref):
        assert relerr(n(a), n(b)) < 1e-4, relerr(n(a), n(b))


def test_solve_is_hip_graph_capturable():
    """The data path makes no allocation / synchronisation / host round trip: a whole multi-level solve (gather, fold,
    SYRK, reduce, solve kernels and the one queue memset per level) can be captured into a HIP graph and replayed."""
    from banet_amd import dense as bdense
    B, H, W, C, K = 2, 48, 64, 128, 64
    scenes = _scenes(B, H, W, C, K, [2, 1], 71)
    intr, levels = odense.batch_scene(scenes)
    mlps = [orc.he_normal_mlp_weights(C, 5 + i) for i in range(2)]
    T0 = t(np.stack([np.asarray(s["T_gt"]) * 0.7 for s in scenes]).reshape(B, 3, 1))
    ba = bdense.DenseBA(t(intr), _torch_levels(levels), mlps, "bundle", 1000.0)
    st_e, _ = ba.solve([3, 2], ba.new_state(T=T0))                       # eager reference (also warms up the kernels)
    want = [n(st_e.R).copy(), n(st_e.T).copy(), n(st_e.Wc).copy()]
    st = ba.new_state(T=T0)
    R0, Tc0, W0 = st.R.clone(), st.T.clone(), st.Wc.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for prob, mlp, its in zip(ba.problems, ba.mlps, [3, 2]):         # warm-up on the capture stream
            from banet_amd import ops
            ops.lm_level(prob, mlp, ba.l2_base, its, False, st, ws=ba.ws)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    st.R.copy_(R0); st.T.copy_(Tc0); st.Wc.copy_(W0)
    with torch.cuda.graph(graph):
        for prob, mlp, its in zip(ba.problems, ba.mlps, [3, 2]):
            ops.lm_level(prob, mlp, ba.l2_base, its, False, st, ws=ba.ws)
    for _ in range(2):                                                    # replay twice from the same start
        st.R.copy_(R0); st.T.copy_(Tc0); st.Wc.copy_(W0)
        graph.replay()
        torch.cuda.synchronize()
        for got, w_ in zip((st.R, st.T, st.Wc), want):
            np.testing.assert_array_equal(n(got), w_)                     # bit-identical to the eager run
