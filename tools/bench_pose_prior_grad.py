#!/usr/bin/env python3
"""Times the backward of the pose prior (csrc/pose_prior_grad.hip; include/banet_hip.h (5g)) on the GPU, by hand -- not part of
bench.py.

The `backward` block's configuration: 640x480, 5 levels (scales 16 .. 1), C = K = 128, 32 windows, 2 iterations per level.  HIP
events, median of --reps, the variants alternating within this process:
  step / step_pose / step_both   DenseBA.solve_differentiable + torch.autograd.grad: without a prior, with a pose prior alone
                   (gradients of R0, T0 and Lambda included), with a pose and a coefficient prior (Lambda, eta); the ratios to the
                   no-prior step of the same run, and the spread of the no-prior step over the rounds
  grad_us / apply_us   ba_pose_prior_grad_kernel (all six outputs, accumulating) and ba_pose_prior_add_kernel alone at pairs 1 and
                   7, B windows, K = 128: --burst launches between two events, divided by their number (the launches are shorter
                   than an event pair resolves)
Prints one JSON line."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from banet_amd import dense as bdense, ops, synth  # noqa: E402
from banet_amd.bundlenet import he_normal_lambda_weights  # noqa: E402


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


class BareLevel:
    def __init__(self, B, K, pairs):
        self.c = ops.capi.Level()
        self.c.B, self.c.K, self.c.pairs, self.c.variant = B, K, pairs, ops.capi.BUNDLE
        self.B, self.K, self.pairs = B, K, pairs


def kernels_alone(B, K, pairs, dev, g, warmup, reps, burst):
    m, P = 6 * pairs, 6 * pairs + K
    rnd = lambda *s: torch.randn(s, generator=g, device=dev)          # noqa: E731
    w = 0.05 * rnd(B, pairs, 3)
    Wh = torch.zeros(B, pairs, 3, 3, device=dev)
    Wh[..., 0, 1], Wh[..., 0, 2], Wh[..., 1, 2] = -w[..., 2], w[..., 1], -w[..., 0]
    R = torch.linalg.matrix_exp(Wh - Wh.transpose(-1, -2)).contiguous()
    R0 = torch.eye(3, device=dev).repeat(B, pairs, 1, 1).contiguous()
    T, T0 = 0.3 * rnd(B, pairs, 3), 0.3 * rnd(B, pairs, 3)
    M = rnd(B, m, m)
    Lam = (M @ M.transpose(1, 2) / m + torch.eye(m, device=dev)).contiguous()
    pp = ops.PosePrior(R0, T0, Lam, 0.37)
    lvl = BareLevel(B, K, pairs)
    AtA, Atb, gA, gb = rnd(B, P, P), rnd(B, P), rnd(B, P, P), rnd(B, P)
    into = dict(gR=torch.zeros(B, pairs, 3, 3, device=dev), gT=torch.zeros(B, pairs, 3, device=dev),
                gR0=torch.zeros(B, pairs, 3, 3, device=dev), gT0=torch.zeros(B, pairs, 3, device=dev),
                gLambda=torch.zeros(B, m, m, device=dev), gscale=torch.zeros(B, device=dev))

    def grads():
        for _ in range(burst):
            ops.pose_prior_add_grad(lvl, pp, R, T, gA, gb, into=into, overwrite=dict(state=False, prior=False))

    def applies():
        for _ in range(burst):
            ops.pose_prior_apply(lvl, pp, R, T, AtA, Atb)
    return 1e3 * timed(grads, warmup, reps) / burst, 1e3 * timed(applies, warmup, reps) / burst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=32)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--basis", type=int, default=128)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--burst", type=int, default=50)
    ap.add_argument("--no-step", action="store_true", help="the kernels alone")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B, H, W, C, K, scales = a.windows, a.height, a.width, 128, a.basis, [16, 8, 4, 2, 1]
    g = torch.Generator(device=dev).manual_seed(1)
    rec = dict(shape="%dx%d" % (W, H), B=B, C=C, K=K, levels=len(scales), iters=a.iters)
    if not a.no_step:
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
        M = torch.randn((B, K, K), generator=g, device=dev)
        Lambda = (M @ M.transpose(1, 2) / K + torch.eye(K, device=dev)).requires_grad_(True)
        eta = torch.randn((B, K), generator=g, device=dev).requires_grad_(True)
        Mp = torch.randn((B, 6, 6), generator=g, device=dev)
        pL = (Mp @ Mp.transpose(1, 2) / 6 + torch.eye(6, device=dev)).requires_grad_(True)
        pR0 = torch.eye(3, device=dev).repeat(B, 1, 1, 1).requires_grad_(True)
        pT0 = gt["T"].reshape(B, 1, 3).to(dev).clone().requires_grad_(True)
        sc = [1e-3] * len(scales)
        priors = dict(step=(None, []), step_pose=(bdense.DensePrior(pose=(pR0, pT0, pL), level_scale=sc), [pR0, pT0, pL]),
                      step_both=(bdense.DensePrior(coef=(Lambda, eta), pose=(pR0, pT0, pL), level_scale=sc), [pR0, pT0, pL, Lambda, eta]))

        def step(kind):
            prior, extra = priors[kind]
            R_, T_, W_ = ba.solve_differentiable(its, T=T0, prior=prior, pose_prior_backward=True)
            return torch.autograd.grad(R_.sum() + T_.sum() + W_.sum(), leaves + extra)

        # alternating, so that a drift of the clock lands on all three
        t = {k: [] for k in priors}
        for _ in range(3):
            for k in priors:
                t[k].append(timed(lambda: step(k), a.warmup if not t[k] else 1, a.reps))
        for k, v in t.items():
            rec[k + "_ms"] = sorted(v)[1]
            rec[k + "_ms_rounds"] = [round(x, 3) for x in v]
        rec["step_spread"] = (max(t["step"]) - min(t["step"])) / rec["step_ms"]
        rec["step_pose_over_step"] = rec["step_pose_ms"] / rec["step_ms"]
        rec["step_both_over_step"] = rec["step_both_ms"] / rec["step_ms"]
        rec["launches_per_step"] = a.iters * len(scales)
    for pairs in (1, 7):
        gu, au = kernels_alone(B, K, pairs, dev, g, a.warmup, a.reps, a.burst)
        rec["grad_us_pairs%d" % pairs], rec["apply_us_pairs%d" % pairs] = round(gu, 2), round(au, 2)
    if not a.no_step:
        rec["grad_share_of_step_pose"] = rec["launches_per_step"] * rec["grad_us_pairs1"] * 1e-3 / rec["step_pose_ms"]
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
