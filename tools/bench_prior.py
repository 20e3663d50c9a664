#!/usr/bin/env python3
"""Times the prior term (csrc/prior.hip; include/banet_hip.h (5d)) on the GPU, by hand -- not part of bench.py.

The headline shape: 640x480, 5 levels (scales 16 .. 1), C = K = 128, 32 windows, 10 iterations per level.  HIP events, median of
--reps:
  solve            banet_lm_solve_f32
  solve_coef       banet_lm_solve_prior_f32, a coefficient prior (Lambda, eta) on every level
  solve_obs        banet_lm_solve_prior_f32, a depth observation with weights on every level
  add_per_iter     (solve_coef - solve) / 50 iterations: ba_prior_add_kernel and what it displaces (the combine launch, once per
                   level, rides along: 5 launches in 55), next to the bytes it moves: B K^2 4 read (Le) and B K^2 4 read and written
                   (the depth block of AtA)
  apply_coef       banet_prior_apply_f32, coefficient form: the combine launch + ba_prior_add_kernel, back to back
  apply_obs[l]     banet_prior_apply_f32, observation form at level l: Gram pass + fold + combine + add
  gram[l]          apply_obs[l] - apply_coef: the per-level Gram pass and its fold (profiles/depth_transfer.txt times the same kernel
                   inside banet_basis_fit_f32 at the finest level)
Prints one JSON line."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from banet_amd import dense as bdense, ops, synth  # noqa: E402
from banet_amd.bundlenet import he_normal_lambda_weights  # noqa: E402

HBM_BYTES_PER_S = 6.3e12


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
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=32)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B, H, W, C, K, scales = a.windows, a.height, a.width, 128, 128, [16, 8, 4, 2, 1]
    intr, levels, gt = synth.make_dense_windows(B, H, W, C, K, scales, 9, dev, trans_mag=0.06, pairs=1)
    mlps = [he_normal_lambda_weights(C, 100 + i) for i in range(len(scales))]
    ba = bdense.DenseBA(intr, levels, mlps, "bundle", 1000.0)
    T0 = (gt["T"] * 0.7).reshape(B, 3, 1).to(dev)
    iters = [a.iters] * len(scales)
    g = torch.Generator(device=dev).manual_seed(1)
    M = torch.randn((B, K, K), generator=g, device=dev)
    Lambda = M @ M.transpose(1, 2) / K + torch.eye(K, device=dev)
    eta = torch.randn((B, K), generator=g, device=dev)
    coef = [ops.Prior(Lambda, eta, scale=1e-3) for _ in levels]
    obs = []
    for lv in levels:
        o = lv.depth + 0.05 * torch.randn(lv.depth.shape, generator=g, device=dev)
        w = 0.2 + 1.8 * torch.rand(lv.depth.shape, generator=g, device=dev)
        obs.append(ops.Prior(obs_depth=o.reshape(B, -1), obs_weight=w.reshape(B, -1), scale=1e-3))
    nb = max(ops.lm_level_workspace_bytes(p, q) for p, q in zip(ba.problems, obs))
    ws = ops.capi.workspace(nb, dev)

    def solve(priors):
        st = ba.new_state(T=T0)
        ops.lm_solve(ba.problems, ba.mlps, ba.l2_base, iters, False, st, ws=ws, priors=priors)

    rec = dict(shape="%dx%d" % (W, H), B=B, C=C, K=K, levels=len(scales), iters=a.iters)
    # alternating, so that a drift of the clock lands on all three
    t = {k: [] for k in ("solve", "solve_coef", "solve_obs")}
    for _ in range(3):
        for k, pr in (("solve", None), ("solve_coef", coef), ("solve_obs", obs)):
            t[k].append(timed(lambda: solve(pr), a.warmup if not t[k] else 1, a.reps))
    for k, v in t.items():
        rec[k + "_ms"] = sorted(v)[1]
        rec[k + "_ms_rounds"] = v
    n_it = sum(iters)
    rec["add_per_iter_us"] = 1e3 * (rec["solve_coef_ms"] - rec["solve_ms"]) / n_it
    rec["add_bytes"] = 3 * B * K * K * 4
    rec["add_bound_us"] = 1e6 * rec["add_bytes"] / HBM_BYTES_PER_S
    rec["solve_coef_over_solve"] = rec["solve_coef_ms"] / rec["solve_ms"]
    rec["solve_obs_over_solve"] = rec["solve_obs_ms"] / rec["solve_ms"]

    P = 6 + K
    A = torch.randn((B, P, 2 * P), generator=g, device=dev)
    AtA = A @ A.transpose(1, 2) / (2 * P) + torch.eye(P, device=dev)
    Atb = torch.randn((B, P), generator=g, device=dev)
    Wc = 0.01 * torch.randn((B, K), generator=g, device=dev)
    rec["apply_coef_us"] = 1e3 * timed(lambda: ops.prior_apply(ba.problems[0], coef[0], Wc, AtA, Atb, ws=ws), a.warmup, a.reps)
    rec["apply_obs_us"], rec["gram_us"], rec["gram_bound_us"] = [], [], []
    for prob, pr in zip(ba.problems, obs):
        us = 1e3 * timed(lambda: ops.prior_apply(prob, pr, Wc, AtA, Atb, ws=ws), a.warmup, a.reps)
        rec["apply_obs_us"].append(us)
        rec["gram_us"].append(us - rec["apply_coef_us"])
        rec["gram_bound_us"].append(1e6 * B * prob.N * (K + 3) * 4 / HBM_BYTES_PER_S)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
