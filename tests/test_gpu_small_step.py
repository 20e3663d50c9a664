"""The backward's small step on HIP (`-m gpu`): banet_small_step_adjoint_f32 (csrc/smallstep.hip -- lambda MLP forward / backward,
damping, the implicit solve, the SE(3) / W update adjoint, four launches) through dense_train.SmallStepHip, against autograd
through dense_train.solve_update_graph in FLOAT64 on the same float32-rounded inputs (small_step_cases.py), where
test_gpu_round6.py runs five well-conditioned shapes:
  * P < 32 (the factorisation inside small_post_kernel) at P = 6 .. 31, bundle, bundle windows and camera windows;
  * the switch to spd_solve_kernel (P = 32, 33), camera windows on it, the largest P the ABI accepts;
  * the MLP's code paths by channel count (C = 1, 3, 5, 63, 255, 256), batches of 1, 37 and 64 windows;
  * a conditioning ladder from cond ~ 1e2 to ~ 1e6 on both solvers.
The gate is relative to what float32 delivers on the case (test_small_step_cases_cpu.py): e_hip <= max(T, 4 e_ref32), T the
tolerance of the round-6 test (2e-4; lambda weights 5e-4), e_ref32 the error of the float32 torch graph the kernels replaced, 4
the project's margin for "as accurate as the reference's algorithm in float32".
And the two autograd nodes that run the kernels: a second backward through them, and two graphs alive on one DenseBA.

What this module measured on an MI355X is kept in profiles/small_step_ladder.txt."""
import pytest
import torch

import small_step_cases as ssc
from test_small_step_cases_cpu import group_reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL, TOL_WEIGHTS, MARGIN = 2e-4, 5e-4, 4.0


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from banet_amd import _capi
    _capi.lib()


def _run_hip(case, calls=2):
    """SmallStepHip on a case, `calls` times (the weight gradients accumulate) -> the 15 outputs of ssc.OUTPUTS as they are on
    the device (gAtA not symmetrised)"""
    from banet_amd import dense_train, ops
    dev = torch.device(DEV)
    v, B, C, K, pairs, N = case["variant"], case["B"], case["C"], case["K"], case["pairs"], case["N"]
    mlp = ops.MlpWeights([(w.float(), b.float()) for w, b in case["layers"]], dev)
    assert dense_train.SmallStepHip.supported(v, B, N, C, K, pairs, dev)
    hs = dense_train.SmallStepHip(v, B, N, C, K, pairs, mlp, case["l2_base"], dev)
    c = lambda x: x.float().to(dev)
    ins = [c(case[k]) for k in ("AtA", "Atb", "absres", "delta", "R", "T", "gR", "gT", "gW")]
    for _ in range(calls):
        got = hs(*ins)
    torch.cuda.synchronize()
    return list(got) + list(hs.glayers)


_ALL = ssc.all_groups()


@pytest.mark.parametrize("grp,rung", _ALL, ids=[ssc.group_id(g, r) for g, r in _ALL])
def test_small_step_kernels_against_the_float64_graph(grp, rung):
    """Every output of the four launches -- dL/dAtA (symmetric part), dL/dAtb, dL/d sum|d|, the direct dL/d(R, T), the ten
    lambda-weight gradients after two accumulating calls -- for five seeds of one (shape, rung): finite, and
    e_hip <= max(T, 4 e_ref32) per output, the errors on each tensor's own max-norm scale, the maximum over the seeds.
    dL/dAtb IS A^-1 dL/dsol, so it is also held against ONE float32 LU solve of the damped system on the CPU (the graph yardstick
    re-solves the forward system as well, which makes it generous)."""
    ref = group_reference(grp, rung)
    e_hip, finite = dict.fromkeys(ssc.OUTPUTS, 0.0), True
    for case, want in ref["per_seed"]:
        got = _run_hip(case)
        got[0] = ssc.sym(got[0])
        for name, gv, wv in zip(ssc.OUTPUTS, got, want):
            finite = finite and bool(torch.isfinite(gv).all())
            mult = 2.0 if name in ssc.WEIGHT_OUTPUTS else 1.0
            e_hip[name] = max(e_hip[name], ssc.rel_err(gv, mult * wv))
    e32 = ref["e_ref32"]
    ww = lambda e: max(e[k] for k in ssc.WEIGHT_OUTPUTS)
    print("\nsmall_step %-36s P %3d  e_hip/e_ref32: gAtA %.1e/%.1e gAtb %.1e/%.1e gabs %.1e/%.1e dR %.1e/%.1e dT %.1e/%.1e "
          "weights %.1e/%.1e | gAtb vs one f32 LU solve %.1e/%.1e" % (
              ssc.group_id(grp, rung), ref["per_seed"][0][0]["P"], e_hip["gAtA"], e32["gAtA"], e_hip["gAtb"], e32["gAtb"], e_hip["gabs"],
              e32["gabs"], e_hip["dR"], e32["dR"], e_hip["dT"], e32["dT"], ww(e_hip), ww(e32), e_hip["gAtb"], ref["e_solve32"]))
    assert finite
    for name in ssc.OUTPUTS:
        tol = TOL_WEIGHTS if name in ssc.WEIGHT_OUTPUTS else TOL
        assert e_hip[name] <= max(tol, MARGIN * e32[name]), (name, e_hip[name], e32[name])
    assert e_hip["gAtb"] <= max(TOL, MARGIN * ref["e_solve32"]), ("gAtb against one float32 solve", e_hip["gAtb"], ref["e_solve32"])


@pytest.mark.parametrize("K", [8, 128])
def test_small_step_kernels_are_bit_reproducible(K):
    """two runs on the same inputs, P = 14 (in-kernel factorisation) and P = 134 (LDS solve): every output, incl. the weight
    gradients accumulated over two calls, bit for bit"""
    case = ssc.make_case("bundle", 3, 32, K, 1, 1, 0)
    a, b = _run_hip(case), _run_hip(case)
    for name, x, y in zip(ssc.OUTPUTS, a, b):
        assert torch.isfinite(x).all() and torch.equal(x, y), name


# ---- the autograd nodes around the kernels ------------------------------------------------------------------------------------
def _sparse_problem(B, N, C, K, H, W, seed):
    from banet_amd import ops
    g = torch.Generator().manual_seed(seed)
    img = torch.randn(B, H, W, C, generator=g).to(DEV)
    conv2 = ops.target_map(img)
    pts = torch.stack([torch.rand(B, N, generator=g) * (W - 1.5) + 0.25, torch.rand(B, N, generator=g) * (H - 1.5) + 0.25], dim=-1).to(DEV)
    conv1 = ops.resample(img, pts) + 0.05 * torch.randn(B, N, C, generator=g).to(DEV)
    fx = torch.full((B, N), 0.8 * W, device=DEV)
    fy = fx.clone()
    ox = torch.full((B, N), W / 2.0, device=DEV)
    oy = torch.full((B, N), H / 2.0, device=DEV)
    ray = torch.stack([(pts[..., 0] - ox) / fx, (pts[..., 1] - oy) / fy, torch.ones(B, N, device=DEV)], dim=1)
    p = ray / ray.norm(dim=1, keepdim=True)
    D = (2.5 + torch.rand(B, N, 1, generator=g)).to(DEV)
    Bs = (torch.randn(B, N, K, generator=g) / K ** 0.5).to(DEV) if K else None
    R = torch.eye(3, device=DEV).repeat(B, 1, 1)
    T = (0.02 * torch.randn(B, 3, 1, generator=g)).to(DEV)
    Wc = (0.01 * torch.randn(B, K, 1, generator=g)).to(DEV) if K else None
    return conv1, conv2, D, Bs, R, T, Wc, (fx, fy, ox, oy, p)


@pytest.mark.parametrize("B,N,C,K,H,W", [(2, 1000, 70, 33, 40, 56), (2, 777, 16, 0, 20, 24)])
def test_sparse_fused_node_can_be_differentiated_twice(B, N, C, K, H, W):
    """dense_train.sparse_iteration (bundle and camera): torch.autograd.grad(..., retain_graph=True) twice on one forward -- the
    second call succeeds and every gradient equals the first bit for bit"""
    from banet_amd import dense_train, ops
    from banet_amd.bundlenet import he_normal_lambda_weights
    conv1, conv2, D, Bs, R, T, Wc, data = _sparse_problem(B, N, C, K, H, W, 1000 + N)
    layers = [(w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)) for w, b in he_normal_lambda_weights(C, 7)]
    leaves = [x.clone().requires_grad_(True) for x in (conv1, conv2, D, Bs, R, T, Wc) if x is not None]
    it = iter(leaves)
    c1, c2, Dl = next(it), next(it), next(it)
    Bl = next(it) if K else None
    Rl, Tl = next(it), next(it)
    Wl = next(it) if K else None
    variant = "bundle" if K else "bundle_camera"
    mlp = ops.MlpWeights([(w.detach(), b.detach()) for w, b in layers], torch.device(DEV))
    assert dense_train.SmallStepHip.supported(variant, B, N, C, K, 1, torch.device(DEV))
    R2, T2, W2, _ = dense_train.sparse_iteration(variant, mlp, 1000.0 if K else 1.0, c1, c2, Dl, Bl, Rl, Tl, Wl, *data, layers)
    g = torch.Generator().manual_seed(5)
    loss = (R2 * torch.randn(R2.shape, generator=g).to(DEV)).sum() + (T2 * torch.randn(T2.shape, generator=g).to(DEV)).sum()
    if K:
        loss = loss + (W2 * torch.randn(W2.shape, generator=g).to(DEV)).sum()
    wrt = leaves + [x for wb in layers for x in wb]
    first = torch.autograd.grad(loss, wrt, retain_graph=True)
    second = torch.autograd.grad(loss, wrt, retain_graph=True)
    for x, y in zip(first, second):
        assert torch.isfinite(x).all() and float(x.abs().max()) > 0.0
        assert torch.equal(x, y)


def _dense_setup(K, seed, frames=2):
    from banet_amd import dense as bdense, synth as bsynth
    from banet_amd.bundlenet import he_normal_lambda_weights
    B, H, W, C = 2, 48, 64, 16
    scales = [2, 1]
    intr, levels, gt = bsynth.make_dense_windows(B, H, W, C, K, scales, seed, torch.device(DEV), trans_mag=0.06, pairs=frames - 1)
    for lv in levels:
        for name in ("src", "tgt", "depth", "basis"):
            setattr(lv, name, getattr(lv, name).requires_grad_(True))
    weights = lambda s: [[(w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)) for w, b in he_normal_lambda_weights(C, s + i)]
                         for i in range(len(scales))]
    T0 = (gt["T"] * 0.7).reshape(B * (frames - 1), 3, 1).to(DEV)
    data = [getattr(lv, nm) for lv in levels for nm in ("src", "tgt", "depth", "basis")]
    return bdense, intr, levels, weights, T0, data


def _dense_loss(R, T, Wc):
    return (R * torch.arange(R.numel(), device=DEV).reshape(R.shape).float().cos()).sum() + T.sum() + (Wc * 0.5).sum()


def test_dense_level_node_can_be_differentiated_twice():
    """DenseBA.solve_differentiable, two levels x 2 iterations, K = 8 (the HIP small step with the in-kernel factorisation):
    two torch.autograd.grad calls on one forward give the same bits"""
    from banet_amd import dense_train
    bdense, intr, levels, weights, T0, data = _dense_setup(8, 9)
    w = weights(100)
    ba = bdense.DenseBA(intr, levels, w, "bundle", 1000.0)
    assert dense_train.SmallStepHip.supported("bundle", ba.B, ba.problems[0].N, 16, 8, 1, torch.device(DEV))
    loss = _dense_loss(*ba.solve_differentiable([2, 2], T=T0))
    wrt = data + [x for lw in w for wb in lw for x in wb]
    first = torch.autograd.grad(loss, wrt, retain_graph=True)
    second = torch.autograd.grad(loss, wrt, retain_graph=True)
    for x, y in zip(first, second):
        assert torch.isfinite(x).all() and float(x.abs().max()) > 0.0
        assert torch.equal(x, y)


def test_dense_level_node_differentiates_with_the_weights_of_its_own_forward():
    """One DenseBA, K = 8: solve_differentiable with lambda weights w1, again with w2 != w1, THEN the backward of the first
    result -- every gradient equals, bit for bit, the one of a fresh DenseBA that only ever saw w1 (the level node keeps its own
    MlpWeights; ba.mlps[li] is replaced by every call)."""
    from banet_amd import dense_train
    bdense, intr, levels, weights, T0, data = _dense_setup(8, 9)
    w1, w2 = weights(100), weights(200)
    assert not torch.equal(w1[0][0][0], w2[0][0][0])
    flat1 = [x for lw in w1 for wb in lw for x in wb]

    def grads_of_first(second_forward):
        ba = bdense.DenseBA(intr, levels, w1, "bundle", 1000.0)
        out1 = dense_train.solve_differentiable(ba, levels, w1, [2, 2], T=T0)
        if second_forward:
            out2 = dense_train.solve_differentiable(ba, levels, w2, [2, 2], T=T0)
            assert not torch.equal(out1[2], out2[2])              # (the weights matter to the solve)
        g = torch.autograd.grad(_dense_loss(*out1), data + flat1)
        torch.cuda.synchronize()
        return g

    want = grads_of_first(False)
    got = grads_of_first(True)
    for x, y in zip(got, want):
        assert torch.isfinite(x).all()
        assert torch.equal(x, y)
    assert any(float(g.abs().max()) > 0.0 for g in want[len(data):])
