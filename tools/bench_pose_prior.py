#!/usr/bin/env python3
"""Times the pose prior (csrc/pose_prior.hip; include/banet_hip.h (5f)) on the GPU, by hand -- not part of bench.py.

The headline shape: 640x480, 5 levels (scales 16 .. 1), C = K = 128, 32 windows, 10 iterations per level.  HIP events, median of
--reps:
  solve            banet_lm_solve_f32
  solve_coef       banet_lm_solve_prior_f32, a coefficient prior (Lambda, eta) on every level
  solve_pose       banet_lm_solve_pose_prior_f32, a pose prior on every level (no coefficient prior)
  pose_per_iter    (solve_pose - solve) / 50 iterations: ba_pose_prior_add_kernel and what it displaces, next to
  add_per_iter     (solve_coef - solve) / 50: ba_prior_add_kernel's, as tools/bench_prior.py reports it
  apply            banet_pose_prior_apply_f32 alone (one launch, with the Python call around it), pairs 1 and 7
Prints one JSON line."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from banet_amd import dense as bdense, ops, synth  # noqa: E402
from banet_amd import _capi as capi  # noqa: E402
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
        self.c = capi.Level()
        self.c.B, self.c.K, self.c.pairs, self.c.variant = B, K, pairs, capi.BUNDLE


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
    Mp = torch.randn((B, 6, 6), generator=g, device=dev)
    Lp = Mp @ Mp.transpose(1, 2) / 6 + torch.eye(6, device=dev)
    R0 = torch.eye(3, device=dev).repeat(B, 1, 1, 1)
    Tp = (gt["T"] * 0.9).reshape(B, 1, 3).to(dev)
    pose = [ops.PosePrior(R0, Tp, Lp, scale=1e-3) for _ in levels]
    nb = max(ops.lm_level_workspace_bytes(p, q) for p, q in zip(ba.problems, coef))
    ws = capi.workspace(nb, dev)

    def solve(priors, pose_priors):
        st = ba.new_state(T=T0)
        ops.lm_solve(ba.problems, ba.mlps, ba.l2_base, iters, False, st, ws=ws, priors=priors, pose_priors=pose_priors)

    rec = dict(build_id=capi.lib().banet_build_id().decode(), shape="%dx%d" % (W, H), B=B, C=C, K=K, levels=len(scales), iters=a.iters)
    # alternating, so that a drift of the clock lands on all three
    t = {k: [] for k in ("solve", "solve_coef", "solve_pose")}
    for _ in range(3):
        for k, pr, pp in (("solve", None, None), ("solve_coef", coef, None), ("solve_pose", None, pose)):
            t[k].append(timed(lambda: solve(pr, pp), a.warmup if not t[k] else 1, a.reps))
    for k, v in t.items():
        rec[k + "_ms"] = sorted(v)[1]
        rec[k + "_ms_rounds"] = v
    n_it = sum(iters)
    rec["add_per_iter_us"] = 1e3 * (rec["solve_coef_ms"] - rec["solve_ms"]) / n_it
    rec["pose_per_iter_us"] = 1e3 * (rec["solve_pose_ms"] - rec["solve_ms"]) / n_it
    rec["solve_pose_over_solve"] = rec["solve_pose_ms"] / rec["solve_ms"]

    rec["apply_us"] = {}
    for pairs in (1, 7):
        m, P = 6 * pairs, 6 * pairs + K
        A = torch.randn((B, P, 2 * P), generator=g, device=dev)
        AtA = A @ A.transpose(1, 2) / (2 * P) + torch.eye(P, device=dev)
        Atb = torch.randn((B, P), generator=g, device=dev)
        Mq = torch.randn((B, m, m), generator=g, device=dev)
        pp = ops.PosePrior(torch.eye(3, device=dev).repeat(B, pairs, 1, 1), torch.zeros((B, pairs, 3), device=dev),
                           Mq @ Mq.transpose(1, 2) / m + torch.eye(m, device=dev), scale=1e-3)
        R = torch.eye(3, device=dev).repeat(B, pairs, 1, 1)
        R[:, :, 0, 1], R[:, :, 1, 0] = -0.01, 0.01            # (not orthonormal to 1e-4: the timing does not care)
        T = 0.05 * torch.randn((B, pairs, 3), generator=g, device=dev)
        lvl = BareLevel(B, K, pairs)
        rec["apply_us"]["pairs%d" % pairs] = 1e3 * timed(lambda: ops.pose_prior_apply(lvl, pp, R, T, AtA, Atb), a.warmup, a.reps)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
