"""GPU tests of the dense level preparation: banet_grid_resample_f32 / banet_grid_resample_grad_f32 (csrc/grid_prep.hip) against the
general resampler on explicit grids, dense_prep.grid_pyramid's autograd, and the dense drivers BundleNet.BundleResizeDense /
CameraResizeDense against a DenseBA built by hand from the existing pieces.

The adjoint's tolerance is derived, not tuned: a texel's sum has at most 9 terms per level (a 2 x 2 footprint at step 1/2 reaches
3 x 3 pixels of a level), at most 45 over the five levels used here, accumulated in float32 with float32 weights, so
|ddata - ref| <= 64 * 2^-24 * S elementwise, S = the float64 adjoint applied to |gout| (the sum of the terms' magnitudes).  When the
kernel accumulates into a non-zero buffer, the buffer's old value is one more term of that sum and S includes its magnitude."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B = 2
U = 64.0 * 2.0 ** -24
# data [2,5,7,C]: step 1/2 -> 10 x 14, step 1 -> 5 x 7 (the identity grid), step 2 -> 3 x 4, step 4 -> 2 x 2, step 3/4 offset -1/2 -> 6 x 9
GEOMS = [(10, 14, 0.5, 0.5, 0.0, 0.0), (5, 7, 1.0, 1.0, 0.0, 0.0), (3, 4, 2.0, 2.0, 0.0, 0.0), (2, 2, 4.0, 4.0, 0.0, 0.0),
         (6, 9, 0.75, 0.75, -0.5, -0.5)]
CHANNELS = [1, 3, 32, 128, 132, 256]


def warp_of(geom, nb=B):
    """the explicit grid [nb, Ho * Wo, 2] (x, y), numpy float32 j * sx + ox"""
    Ho, Wo, sx, sy, ox, oy = geom
    x = (np.arange(Wo, dtype=np.float32) * np.float32(sx)).astype(np.float32) + np.float32(ox)
    y = (np.arange(Ho, dtype=np.float32) * np.float32(sy)).astype(np.float32) + np.float32(oy)
    w = np.stack(np.broadcast_arrays(x[None, :], y[:, None]), axis=-1).reshape(1, Ho * Wo, 2).astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(np.repeat(w, nb, axis=0))).to(DEV)


def rand(shape, seed):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(shape).astype(np.float32)).to(DEV)


def clamp_resampler64(data, warp):
    """interpolate2d2 (weights from the unclamped floor, indices clamped) as a differentiable float64 torch expression: the CLAMP
    counterpart of bundlenet._resampler_autograd, which states the zero-padding mode"""
    nb, H, W, C = data.shape
    x, y = warp[..., 0], warp[..., 1]
    x0, y0 = torch.floor(x), torch.floor(y)
    dx, dy = (x - x0).unsqueeze(-1), (y - y0).unsqueeze(-1)
    flat = data.reshape(nb, H * W, C)

    def tap(xi, yi):
        idx = (yi.long().clamp(0, H - 1) * W + xi.long().clamp(0, W - 1)).unsqueeze(-1).expand(-1, -1, C)
        return torch.gather(flat, 1, idx)

    return tap(x0, y0) * (1 - dx) * (1 - dy) + tap(x0 + 1, y0) * dx * (1 - dy) + tap(x0, y0 + 1) * (1 - dx) * dy + tap(x0 + 1, y0 + 1) * dx * dy


def adjoint64(gouts, geoms, shape, clamp):
    """float64 autograd through the reference resampler on the explicit grids, summed over the levels"""
    from banet_amd.bundlenet import _resampler_autograd
    data = torch.zeros(shape, dtype=torch.float64, device=DEV, requires_grad=True)
    total = 0.0
    for g, geom in zip(gouts, geoms):
        w = warp_of(geom, shape[0]).double()
        out = clamp_resampler64(data, w) if clamp else _resampler_autograd(data, w)
        total = total + (out * g.double().reshape(out.shape)).sum()
    return torch.autograd.grad(total, data)[0]


@pytest.fixture(scope="module")
def mods():
    from banet_amd import dense_prep, ops, prep_grad
    return dense_prep, ops, prep_grad


# ---- forward -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clamp", [False, True])
@pytest.mark.parametrize("C", CHANNELS)
def test_forward_is_bit_identical_to_the_general_resampler(mods, C, clamp):
    dense_prep, ops, _ = mods
    data = rand((B, 5, 7, C), 10 + C)
    want = [ops.resample(data, warp_of(g), clamp=clamp).reshape(B, g[0], g[1], C) for g in GEOMS]
    got = dense_prep.grid_resample(data, GEOMS, clamp=clamp)                   # ONE call, five levels
    for g, a, b in zip(GEOMS, got, want):
        assert torch.equal(a, b), (g, float((a - b).abs().max()))
    for g, b in zip(GEOMS, want):                                              # one single-level call per level
        a, = dense_prep.grid_resample(data, [g], clamp=clamp)
        assert torch.equal(a, b), g


@pytest.mark.parametrize("clamp", [False, True])
@pytest.mark.parametrize("C", [3, 4])
def test_forward_on_a_one_texel_map(mods, C, clamp):
    dense_prep, ops, _ = mods
    data = rand((B, 1, 1, C), 3 + C)
    geoms = [(1, 1, 1.0, 1.0, 0.0, 0.0), (3, 3, 0.5, 0.5, 0.0, 0.0), (2, 2, 1.0, 1.0, -0.5, -0.75), (1, 1, 4.0, 4.0, -1.0, 0.5)]
    got = dense_prep.grid_resample(data, geoms, clamp=clamp)
    for g, a in zip(geoms, got):
        assert torch.equal(a, ops.resample(data, warp_of(g), clamp=clamp).reshape(a.shape)), g
    gouts = [rand(tuple(a.shape), 5 + i) for i, a in enumerate(got)]
    dd = dense_prep.grid_resample_grad(gouts, geoms, tuple(data.shape), clamp=clamp)
    ref = adjoint64(gouts, geoms, tuple(data.shape), clamp)
    S = adjoint64([g.abs() for g in gouts], geoms, tuple(data.shape), clamp)
    assert bool(((dd.double() - ref).abs() <= U * S).all())


# ---- adjoint -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clamp", [False, True])
@pytest.mark.parametrize("C", CHANNELS)
def test_adjoint(mods, C, clamp):
    dense_prep, ops, prep_grad = mods
    shape = (B, 5, 7, C)
    gouts = [rand((B, g[0], g[1], C), 100 + C + i) for i, g in enumerate(GEOMS)]
    ref = adjoint64(gouts, GEOMS, shape, clamp)
    S = adjoint64([g.abs() for g in gouts], GEOMS, shape, clamp)
    dd = dense_prep.grid_resample_grad(gouts, GEOMS, shape, clamp=clamp)                      # OVERWRITE
    err = (dd.double() - ref).abs()
    print("adjoint C=%d clamp=%d: max err / (2^-24 S) = %.3f" % (C, clamp, float((err / (2.0 ** -24 * S).clamp(min=1e-300)).max())))
    assert bool((err <= U * S).all())                                                          # every element, none skipped
    assert bool((S > 0).any())
    # two runs are bit-equal; OVERWRITE = accumulating into zeros
    assert torch.equal(dd, dense_prep.grid_resample_grad(gouts, GEOMS, shape, clamp=clamp))
    nan = torch.full(shape, float("nan"), device=DEV)
    assert torch.equal(dd, dense_prep.grid_resample_grad(gouts, GEOMS, shape, clamp=clamp, out=nan))      # every texel is written
    zeros = torch.zeros(shape, device=DEV)
    assert torch.equal(dd, dense_prep.grid_resample_grad(gouts, GEOMS, shape, clamp=clamp, out=zeros, accumulate=True))
    # accumulating into a non-zero buffer: the old value is one more term of the sum
    buf = rand(shape, 7 + C)
    acc = dense_prep.grid_resample_grad(gouts, GEOMS, shape, clamp=clamp, out=buf.clone(), accumulate=True)
    assert bool(((acc.double() - (buf.double() + dd.double())).abs() <= U * (S + buf.double().abs())).all())
    untouched = S == 0
    assert torch.equal(acc[untouched], buf[untouched])
    # <A x, y> = <x, A^T y>: the forward against the adjoint, float64 sums of float32 products
    x = rand(shape, 9 + C)
    outs = dense_prep.grid_resample(x, GEOMS, clamp=clamp)
    lhs = sum(float((o.double() * g.double()).sum()) for o, g in zip(outs, gouts))
    rhs = float((x.double() * dd.double()).sum())
    print("dot-product identity C=%d clamp=%d: lhs %.9g rhs %.9g" % (C, clamp, lhs, rhs))
    assert abs(lhs - rhs) <= 1e-5 * abs(lhs)
    # the sort-based adjoint of the general resampler, level by level
    per = sum(prep_grad.resampler_grad_forward(x, warp_of(g), go.reshape(B, -1, C), clamp=clamp, want_warp=False)[0].double()
              for g, go in zip(GEOMS, gouts))
    assert bool(((dd.double() - per).abs() <= U * S).all())
    # a single level equals it exactly where both add one level's terms in the same (point, tap) order
    one = dense_prep.grid_resample_grad(gouts[:1], GEOMS[:1], shape, clamp=clamp)
    S1 = adjoint64([gouts[0].abs()], GEOMS[:1], shape, clamp)
    g1 = prep_grad.resampler_grad_forward(x, warp_of(GEOMS[0]), gouts[0].reshape(B, -1, C), clamp=clamp, want_warp=False)[0]
    assert bool(((one.double() - g1.double()).abs() <= U * S1).all())


def test_everything_runs_under_deterministic_algorithms(mods):
    dense_prep, _, _ = mods
    data = rand((B, 5, 7, 4), 1).requires_grad_(True)
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        outs = dense_prep.grid_pyramid(data, GEOMS, clamp=True)
        g, = torch.autograd.grad(sum((o * o).sum() for o in outs), data)
        work = [i for i in range(len(GEOMS)) if i != 1]                       # (level 1 is the identity: autograd adds its part)
        direct = dense_prep.grid_resample_grad([2 * outs[i].detach() for i in work], [GEOMS[i] for i in work], tuple(data.shape), clamp=True)
    finally:
        torch.use_deterministic_algorithms(prev)
    assert torch.equal(g, direct + 2 * data.detach())


def test_forward_and_adjoint_in_one_captured_graph(mods):
    dense_prep, _, _ = mods
    C = 32
    data = rand((B, 5, 7, C), 41)
    gouts = [rand((B, g[0], g[1], C), 50 + i) for i, g in enumerate(GEOMS)]
    outs = [torch.empty((B, g[0], g[1], C), device=DEV) for g in GEOMS]
    dd = torch.empty_like(data)
    from banet_amd import _capi as capi
    L = capi.lib()

    def enqueue():
        capi.check(L.banet_grid_resample_f32(capi.ptr(data), B, 5, 7, C, 1, dense_prep._table(GEOMS, outs), len(GEOMS), capi.stream()))
        capi.check(L.banet_grid_resample_grad_f32(capi.ptr(dd), B, 5, 7, C, 1, dense_prep._table(GEOMS, gouts), len(GEOMS), 1, capi.stream()))

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        enqueue()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    eager = [o.clone() for o in outs + [dd]]
    for o in outs + [dd]:
        o.fill_(float("nan"))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                     # a linear chain: forward, then adjoint
        enqueue()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(outs + [dd], eager))


# ---- grid_pyramid --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clamp", [False, True])
@pytest.mark.parametrize("geoms", [GEOMS, [GEOMS[0], GEOMS[2]], [GEOMS[1]]], ids=["with-identity", "no-identity", "identity-only"])
def test_grid_pyramid_autograd_is_the_direct_adjoint(mods, geoms, clamp):
    dense_prep, _, _ = mods
    C = 8
    data = rand((B, 5, 7, C), 61).requires_grad_(True)
    outs = dense_prep.grid_pyramid(data, geoms, clamp=clamp)
    coefs = [rand(tuple(o.shape), 70 + i) for i, o in enumerate(outs)]
    got, = torch.autograd.grad(sum((o * c).sum() for o, c in zip(outs, coefs)), data)
    ident = [dense_prep.is_identity(5, 7, g) for g in geoms]
    for o, idt in zip(outs, ident):
        assert (o.data_ptr() == data.data_ptr()) == idt                       # the identity level IS the input
    work = [(c, g) for c, g, idt in zip(coefs, geoms, ident) if not idt]
    want = None
    if work:
        want = dense_prep.grid_resample_grad([c for c, _ in work], [g for _, g in work], tuple(data.shape), clamp=clamp)
    for c, idt in zip(coefs, ident):
        if idt:                                          # autograd's own accumulation adds the identity level's (one add: either order)
            want = c if want is None else want + c
    assert torch.equal(got, want)
    depth = rand((B, 5, 7), 62)                                                  # a [B,H,W] depth map: C = 1, [B,Ho,Wo] levels
    d_l = dense_prep.grid_pyramid(depth, geoms, clamp=clamp)
    for o, g in zip(d_l, geoms):
        assert tuple(o.shape) == (B, g[0], g[1])
        assert torch.equal(o, dense_prep.grid_resample(depth.unsqueeze(-1), [g], clamp=clamp)[0].squeeze(-1))


# ---- the dense drivers -------------------------------------------------------------------------------------------------------------
def scene(C, K, seed, shapes=((2, 3), (4, 6), (8, 12), (16, 24))):
    """a two-image batch as the reference's drivers take it (item 1 is item 0's other frame: _swap_halves pairs them): four feature
    levels, the finest shapes[-1], and the decoder's depth / basis at half of it"""
    from banet_amd import synth
    H, W = shapes[-1]
    intr, levels, gt = synth.make_dense_windows(1, H, W, C, K, [8, 4, 2, 1], seed, torch.device(DEV), rot_mag=0.004, trans_mag=0.01)
    layers = [torch.cat([lv.src, lv.tgt], dim=0).contiguous() for lv in levels]
    half = levels[2]
    init_depth = half.depth.repeat(2, 1, 1).contiguous()
    basis = half.basis.repeat(2, 1, 1, 1).contiguous() if K > 0 else None
    # a start away from T = 0: at the identity pose with no translation the depth Jacobian vanishes, and the reference leaves the
    # last basis coefficient undamped (bundlenet.py:266), so the first bundle step would divide by rounding noise
    T0 = torch.stack([gt["T"][0] * 0.7, -gt["T"][0] * 0.7]).reshape(2, 3, 1).to(DEV)
    return intr.repeat(2, 1).reshape(2, 4, 1).contiguous(), layers, basis, init_depth, T0


def lambda_weights(C, levels, grad=False):
    from banet_amd.bundlenet import he_normal_lambda_weights
    return {str(l): [(w.to(DEV).requires_grad_(grad), b.to(DEV).requires_grad_(grad)) for w, b in he_normal_lambda_weights(C, 500 + l)]
            for l in levels}


def hand_levels(mods, layers, levels, init_depth, basis, clamp, differentiable=False):
    """the DenseLevels of the drivers from the existing pieces: the general resampler on explicit grids"""
    dense_prep, ops, prep_grad = mods
    from banet_amd import dense
    from banet_amd.bundlenet import BundleNet
    scales = [2 ** (len(layers) - 1 - l) for l in levels]
    geoms = dense_prep.grid_levels(init_depth.shape[1], init_depth.shape[2], [tuple(layers[l].shape[1:3]) for l in levels], scales, 2)
    out = []
    for l, s, g in zip(levels, scales, geoms):
        w = warp_of(g)
        d = ops.resample(init_depth.detach().unsqueeze(-1), w, clamp=clamp).reshape(B, g[0], g[1])
        b = None
        if basis is not None:
            b = (prep_grad.resampler(basis, w, clamp) if differentiable else ops.resample(basis, w, clamp=clamp)).reshape(B, g[0], g[1], -1)
        out.append(dense.DenseLevel(s, layers[l], BundleNet._swap_halves(layers[l]), d, b))
    return out


@pytest.mark.parametrize("C", [128, 16])
def test_bundle_resize_dense_forward_is_the_hand_built_solve(mods, C):
    dense_prep, ops, _ = mods
    from banet_amd import bundlenet, dense
    K, levels = 32, (2, 3)
    intr, layers, basis, init_depth, T0 = scene(C, K, 5)
    lw = lambda_weights(C, levels)
    net = bundlenet.BundleNet(lambda_weights=lw)
    Rs, Ts, Ds = net.BundleResizeDense(intr, layers, basis, init_depth, init_translation=T0, iters=2)
    ba = dense.DenseBA(intr.reshape(B, 4), hand_levels(mods, layers, levels, init_depth, basis, True), [lw[str(l)] for l in levels], "bundle", 1000.0)
    snaps = []
    ba.solve([2, 2], state=ba.new_state(None, T0), snapshots=snaps)
    assert len(Rs) == len(Ts) == len(Ds) == 2
    for R, T, D, s in zip(Rs, Ts, Ds, snaps):
        assert torch.equal(R, s["R"]) and torch.equal(T, s["T"])
        assert torch.equal(D, ops.depth_output(init_depth, basis.reshape(B, -1, K), s["W"])) and D.shape == init_depth.shape
        assert torch.isfinite(R).all() and torch.isfinite(T).all() and torch.isfinite(D).all()
    assert not torch.equal(Rs[0], Rs[1])
    Rz, Tz, Dz = net.BundleResizeDense(intr, layers, basis, init_depth, init_translation=T0, iters=2, border="zero")
    assert torch.isfinite(Rz[-1]).all() and not torch.equal(Rz[-1], Rs[-1])


def test_zero_border_differs_from_clamp_in_the_last_row_and_column_only(mods):
    """The maps hold multiples of 1/64 below 4, so every tap sum is exact in float32 and the two modes' different sum orders cannot
    show: whatever differs is the padding."""
    dense_prep, _, _ = mods
    _, layers, basis, init_depth, _ = scene(16, 32, 5)
    q = lambda t, lo: (torch.round(t * 64.0) / 64.0).clamp(lo, 3.0)   # noqa: E731
    init_depth, basis = q(init_depth, 0.25), q(basis, -3.0)
    geoms = dense_prep.grid_levels(8, 12, [(8, 12), (16, 24)], [2, 1], 2)
    for data in (init_depth, basis):
        zero, clamp = dense_prep.grid_pyramid(data, geoms, clamp=False), dense_prep.grid_pyramid(data, geoms, clamp=True)
        assert zero[0].data_ptr() == clamp[0].data_ptr() == data.data_ptr()          # level 2 is the map itself under both
        diff = zero[1] != clamp[1]
        rim = torch.zeros_like(diff)
        rim[:, -1], rim[:, :, -1] = True, True
        assert not bool((diff & ~rim).any())
        assert bool(diff[rim].any())
    dz, dc = dense_prep.grid_pyramid(init_depth, geoms, clamp=False)[1], dense_prep.grid_pyramid(init_depth, geoms, clamp=True)[1]
    assert bool((dz != dc)[:, -1].all()) and bool((dz != dc)[:, :, -1].all())           # a positive depth: the whole rim is scaled
    assert torch.equal(dz[:, -1, :-1], 0.5 * dc[:, -1, :-1]) and torch.equal(dz[:, :-1, -1], 0.5 * dc[:, :-1, -1])


def test_bundle_resize_dense_backward_is_the_composition_of_the_existing_pieces(mods):
    dense_prep, ops, prep_grad = mods
    from banet_amd import bundlenet, dense
    C, K, levels, iters = 16, 32, (2, 3), 2
    intr, layers, basis, init_depth, T0 = scene(C, K, 9)

    def leaves():
        ly = [t.clone().requires_grad_(True) for t in layers]
        return ly, basis.clone().requires_grad_(True), init_depth.clone().requires_grad_(True), lambda_weights(C, levels, grad=True)

    def loss_of(Rs, Ts, Ds):
        tot = 0.0
        for i, (R, T, D) in enumerate(zip(Rs, Ts, Ds)):
            tot = tot + (R * torch.arange(R.numel(), device=DEV).reshape(R.shape).float().add(i).cos()).sum() + (T * (1.0 + i)).sum() + \
                (D * dcoef[i]).sum()
        return tot

    dcoef = [rand(tuple(init_depth.shape), 200 + i) for i in range(len(levels))]

    def driver():
        ly, bs, d0, lw = leaves()
        net = bundlenet.BundleNet(lambda_weights=lw)
        out = net.BundleResizeDense(intr, ly, bs, d0, init_translation=T0, iters=iters)
        wl = [x for l in levels for wb in lw[str(l)] for x in wb]
        return out, torch.autograd.grad(loss_of(*out), [ly[l] for l in levels] + wl + [bs, d0])

    def composition():
        ly, bs, d0, lw = leaves()
        dls = hand_levels(mods, ly, levels, d0, bs, True, differentiable=True)
        level_grads = {}
        for i, lv in enumerate(dls):
            lv.basis.register_hook(lambda g, i=i: level_grads.__setitem__(i, g.detach().clone()))
        ba = dense.DenseBA(intr.reshape(B, 4), dls, [[(w.detach(), b.detach()) for w, b in lw[str(l)]] for l in levels], "bundle", 1000.0)
        ba.lambda_weights = [lw[str(l)] for l in levels]
        outs = []
        ba.solve_differentiable([iters] * len(levels), T=T0, outputs=outs)
        out = ([o[0] for o in outs], [o[1] for o in outs], [prep_grad.depth_output(d0, bs, o[2]) for o in outs])
        wl = [x for l in levels for wb in lw[str(l)] for x in wb]
        return out, torch.autograd.grad(loss_of(*out), [ly[l] for l in levels] + wl + [bs, d0]), level_grads, [o[2].detach() for o in outs]

    (out_a, grads_a), (out_b, grads_b, level_grads, Ws) = driver(), composition()
    for xs, ys in zip(out_a, out_b):
        for x, y in zip(xs, ys):
            assert torch.equal(x, y)
    for x, y in zip(grads_a[:-2], grads_b[:-2]):                         # layers and lambda weights: bit-identical
        assert torch.isfinite(x).all() and torch.equal(x, y)
    assert torch.equal(grads_a[-1], grads_b[-1])                         # init_depth: the output-depth term only
    assert torch.equal(grads_a[-1], sum(dcoef))
    # basis: the two differ in the order of the pyramid adjoint's and autograd's sums only
    geoms = dense_prep.grid_levels(8, 12, [(8, 12), (16, 24)], [2, 1], 2)
    S = adjoint64([level_grads[i].abs() for i in range(len(levels))], geoms, tuple(basis.shape), True)
    for i in range(len(levels)):                                         # ... and the output depths' terms dcoef_i W_i^T
        S = S + dcoef[i].double().abs().unsqueeze(-1) * Ws[i].double().abs().reshape(B, 1, 1, K)
    err = (grads_a[-2].double() - grads_b[-2].double()).abs()
    print("basis gradient: max err / (2^-24 S) = %.3f" % float((err / (2.0 ** -24 * S).clamp(min=1e-300)).max()))
    assert bool((err <= U * S).all())
    # bit-reproducible run to run
    _, again = driver()
    assert all(torch.equal(x, y) for x, y in zip(grads_a, again))


def test_camera_resize_dense_forward_is_the_hand_built_solve(mods):
    """Four levels at scales 8, 4, 2, 1 as the reference's CameraResize.  The pyramid is 4 x 6 ... 32 x 48: the dense solver takes
    levels of at least 4 x 4 pixels (plan_gather), so a 3 x 4 coarsest level is refused by every path, hand-built or not."""
    dense_prep, ops, _ = mods
    from banet_amd import bundlenet, dense
    C, levels = 64, (0, 1, 2, 3)
    intr, layers, _, depths, _ = scene(C, 0, 13, shapes=((4, 6), (8, 12), (16, 24), (32, 48)))
    lw = lambda_weights(C, levels)
    net = bundlenet.BundleNet(lambda_weights=lw)
    Rs, Ts = net.CameraResizeDense(intr, layers, depths, iters=2)
    ba = dense.DenseBA(intr.reshape(B, 4), hand_levels(mods, layers, levels, depths, None, True), [lw[str(l)] for l in levels],
                       "bundle_camera", 1000.0)
    snaps = []
    ba.solve([2] * 4, snapshots=snaps)
    assert len(Rs) == len(Ts) == 4
    for R, T, s in zip(Rs, Ts, snaps):
        assert torch.equal(R, s["R"]) and torch.equal(T, s["T"]) and torch.isfinite(R).all() and torch.isfinite(T).all()
    assert not torch.equal(Rs[0], Rs[-1])
