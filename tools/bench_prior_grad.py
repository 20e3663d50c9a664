#!/usr/bin/env python3
"""Times the backward of the prior term (csrc/prior_grad.hip; include/banet_hip.h (5e)) on the GPU, by hand -- not part of bench.py.

The `backward` block's configuration: 640x480, 5 levels (scales 16 .. 1), C = K = 128, 32 windows, 2 iterations per level.  HIP
events, median of --reps, the variants alternating within this process:
  step / step_coef / step_obs   DenseBA.solve_differentiable + torch.autograd.grad: without a prior, with a coefficient prior
                   (Lambda, eta) on every level, with a depth observation and weights on every level (gradients of the prior's
                   tensors included); the ratios to the no-prior step of the same build
  pixel_us[l]      prior_grad_pixel_kernel alone at level l: banet_prior_terms_grad_f32 asking for gscale + gdepth + gbasis in
                   accumulate mode minus the same call asking for gscale only (the preparation launch)
  mg_basis_us[l]   marg_grad_basis_kernel at the same shape, the same way: banet_ba_marginals_grad_f32 with gAtA + gbasis minus
                   gAtA alone (one basis read and one [N,K] write; the difference also holds the factor kernel's write of T)
  bound_us[l]      3 B N K 4 bytes (basis read, gbasis read and written) at the streaming-copy rate bench.py reports
  peak memory      torch.cuda.max_memory_allocated of the observation-form step minus the no-prior step's: ASSERTED below
                   B N K 4 of the finest level -- no second basis-sized buffer exists
Prints one JSON line."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from banet_amd import dense as bdense, ops, synth  # noqa: E402
from banet_amd.bundlenet import he_normal_lambda_weights  # noqa: E402

STREAMING_COPY_BYTES_PER_S = 6.3e12      # bench.py: roofline.streaming_copy_GBps


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return ms[len(ms) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=32)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--basis", type=int, default=128)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--no-step", action="store_true", help="the kernels alone (a K other than 128 has no training-step precedent)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B, H, W, C, K, scales = a.windows, a.height, a.width, 128, a.basis, [16, 8, 4, 2, 1]
    intr, levels, gt = synth.make_dense_windows(B, H, W, C, K, scales, 7, dev, trans_mag=0.06, pairs=1)
    mlps = [[(w.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)) for w, b in he_normal_lambda_weights(C, 100 + i)]
            for i in range(len(scales))]
    for lv in levels:
        for name in ("src", "tgt", "depth", "basis"):
            setattr(lv, name, getattr(lv, name).requires_grad_(True))
    ba = bdense.DenseBA(intr, levels, mlps, "bundle", 1000.0)
    T0 = (gt["T"] * 0.7).reshape(B, 3, 1).to(dev)
    its = [a.iters] * len(scales)
    leaves = [getattr(lv, n) for lv in levels for n in ("src", "tgt", "depth", "basis")] + [x for lw in mlps for wb in lw for x in wb]
    g = torch.Generator(device=dev).manual_seed(1)
    M = torch.randn((B, K, K), generator=g, device=dev)
    Lambda = (M @ M.transpose(1, 2) / K + torch.eye(K, device=dev)).requires_grad_(True)
    eta = torch.randn((B, K), generator=g, device=dev).requires_grad_(True)
    obs = []
    for lv in levels:
        o = lv.depth.detach() + 0.05 * torch.randn(lv.depth.shape, generator=g, device=dev)
        w = 0.2 + 1.8 * torch.rand(lv.depth.shape, generator=g, device=dev)
        obs.append((o.requires_grad_(True), w.requires_grad_(True)))
    sc = [1e-3] * len(scales)
    priors = dict(step=(None, []), step_coef=(bdense.DensePrior(coef=(Lambda, eta), level_scale=sc), [Lambda, eta]),
                  step_obs=(bdense.DensePrior(depth_obs=obs, level_scale=sc), [x for ow in obs for x in ow]))

    def step(kind):
        prior, extra = priors[kind]
        R_, T_, W_ = ba.solve_differentiable(its, T=T0, prior=prior)
        return torch.autograd.grad(R_.sum() + T_.sum() + W_.sum(), leaves + extra)

    rec = dict(shape="%dx%d" % (W, H), B=B, C=C, K=K, levels=len(scales), iters=a.iters)
    if not a.no_step:
        # alternating, so that a drift of the clock lands on all three
        t = {k: [] for k in priors}
        for _ in range(3):
            for k in priors:
                t[k].append(timed(lambda: step(k), a.warmup if not t[k] else 1, a.reps))
        for k, v in t.items():
            rec[k + "_ms"] = sorted(v)[1]
            rec[k + "_ms_rounds"] = [round(x, 3) for x in v]
        rec["step_coef_over_step"] = rec["step_coef_ms"] / rec["step_ms"]
        rec["step_obs_over_step"] = rec["step_obs_ms"] / rec["step_ms"]
        # peak memory of one step on top of what is allocated before it
        peak = {}
        for k in ("step", "step_obs", "step", "step_obs"):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            out = step(k)
            torch.cuda.synchronize()
            peak[k] = torch.cuda.max_memory_allocated() - base
            del out
        finest = B * levels[-1].depth[0].numel() * K * 4
        rec["peak_step_bytes"], rec["peak_step_obs_bytes"], rec["finest_basis_bytes"] = peak["step"], peak["step_obs"], finest
        rec["peak_extra_over_basis"] = (peak["step_obs"] - peak["step"]) / finest
        assert peak["step_obs"] - peak["step"] < finest, "the observation-form step allocates a basis-sized buffer: %r" % (rec,)

    # the per-pixel kernel next to marg_grad_basis_kernel and the byte bound, level by level
    rec["pixel_us"], rec["mg_basis_us"], rec["bound_us"], rec["pixel_over_mg_basis"], rec["pixel_over_bound"] = [], [], [], [], []
    P = 6 + K
    A = torch.randn((B, P, 2 * P), generator=g, device=dev)
    AtA = A @ A.transpose(1, 2) / (2 * P) + torch.eye(P, device=dev)
    gLe, gee = torch.randn((B, K, K), generator=g, device=dev), torch.randn((B, K), generator=g, device=dev)
    Le, ee = torch.randn((B, K, K), generator=g, device=dev), torch.randn((B, K), generator=g, device=dev)
    for prob, (o, w) in zip(ba.problems, obs):
        N = prob.N
        pr = ops.Prior(obs_depth=o.detach().reshape(B, N), obs_weight=w.detach().reshape(B, N), scale=1e-3)
        gd, gb = torch.zeros((B, N), device=dev), torch.zeros((B, N, K), device=dev)
        ws = ops.capi.workspace(ops.capi.lib().banet_prior_terms_grad_workspace_bytes(prob.c, pr.c), dev)
        full = timed(lambda: ops.prior_terms_grad(prob, pr, gLe, gee, Le, ee, want=("gscale", "gdepth", "gbasis"), accumulate=True,
                                                  into=dict(gdepth=gd, gbasis=gb), ws=ws), a.warmup, a.reps)
        prep = timed(lambda: ops.prior_terms_grad(prob, pr, gLe, gee, Le, ee, want=("gscale",), ws=ws), a.warmup, a.reps)
        gdv = torch.randn((B, N), generator=g, device=dev)
        nb = ops.capi.lib().banet_ba_marginals_grad_workspace_bytes(prob.c, 1)
        mws = ops.capi.workspace(nb, dev)
        both = timed(lambda: ops.ba_marginals_grad(prob, AtA, damping=1e-3, g_depth_var=gdv, want=("gAtA", "gbasis"), ws=mws), a.warmup, a.reps)
        small = timed(lambda: ops.ba_marginals_grad(prob, AtA, damping=1e-3, g_depth_var=gdv, want=("gAtA",), ws=mws), a.warmup, a.reps)
        del gd, gb, gdv
        px, mg, bd = 1e3 * (full - prep), 1e3 * (both - small), 1e6 * 3 * B * N * K * 4 / STREAMING_COPY_BYTES_PER_S
        rec["pixel_us"].append(round(px, 1))
        rec["mg_basis_us"].append(round(mg, 1))
        rec["bound_us"].append(round(bd, 1))
        rec["pixel_over_mg_basis"].append(round(px / mg, 2) if mg > 0 else None)
        rec["pixel_over_bound"].append(round(px / bd, 2))
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
