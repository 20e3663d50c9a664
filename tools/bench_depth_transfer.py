#!/usr/bin/env python3
"""Times banet_basis_fit_f32 (csrc/basisfit.hip) and banet_depth_reproject_f32 (csrc/reproject.hip) on the GPU, by hand -- not part
of bench.py.

Two shapes: 640x480 x 32 windows with K = 128, and 1280x960 x 8 windows with K = 256.  Per shape:
  fit          the whole banet_basis_fit_f32 call: Gram pass, fold, factor / solve
  fit_tail     the same call on 2 points per window: one partial row, so the fold and the factor / solve kernel alone
  gram         fit - fit_tail: the pass over the basis (with the fold's reads of the 64 partial rows per window)
  bound        max(bytes / 6.3 TB/s, lower-block FLOPs / 157 TF): one read of the basis, depth, target and weight; 2 FLOPs per entry
               of the lower 32 x 32 blocks of G per pixel
  depth_var    marg_depthvar_kernel (banet_ba_marginals_f32 with depth_var minus the call without) on the same basis, one target
               frame: the same FLOPs on the same bytes, for comparison
  reproject    the whole banet_depth_reproject_f32 call (key init, splat, decode), one target frame, against one read of the basis
Prints one JSON line per shape."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from banet_amd import ops  # noqa: E402

HBM_BYTES_PER_S, F32_MFMA_FLOPS = 6.3e12, 157e12


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


def run(H, W, B, K, warmup, reps):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    N = H * W
    basis = torch.randn((B, N, K), generator=g, device=dev)
    depth = 2.5 + torch.rand((B, N), generator=g, device=dev)
    target = depth + 0.1 * torch.randn((B, N), generator=g, device=dev)
    weight = 0.2 + 1.8 * torch.rand((B, N), generator=g, device=dev)
    rec = dict(shape="%dx%d" % (W, H), B=B, K=K)

    f = ops.basis_fit(depth, basis, target, weight=weight, damping=1e-3, want=ops.BASIS_FIT_OUTPUTS)
    torch.cuda.synchronize()
    assert int(f.status.abs().sum()) == 0 and bool(torch.isfinite(f.Wc).all())
    ws = ops.capi.workspace(512 << 20, dev)
    rec["fit_ms"] = timed(lambda: ops.basis_fit(depth, basis, target, weight=weight, damping=1e-3, ws=ws), warmup, reps)
    small = (depth[:, :2].contiguous(), basis[:, :2].contiguous(), target[:, :2].contiguous(), weight[:, :2].contiguous())
    rec["fit_tail_ms"] = timed(lambda: ops.basis_fit(small[0], small[1], small[2], weight=small[3], damping=1e-3, ws=ws), warmup, reps)
    rec["gram_ms"] = rec["fit_ms"] - rec["fit_tail_ms"]
    nr = (K + 31) // 32
    nbytes = B * N * (K + 3) * 4
    flops = 2.0 * B * N * (nr * (nr + 1) // 2) * 1024
    rec["gram_bytes"], rec["gram_lower_block_flops"] = nbytes, flops
    rec["gram_bound_ms"] = 1e3 * max(nbytes / HBM_BYTES_PER_S, flops / F32_MFMA_FLOPS)
    rec["gram_over_bound"] = rec["gram_ms"] / rec["gram_bound_ms"]

    # marg_depthvar_kernel on the same basis
    P = 6 + K
    A = torch.randn((B, P, 2 * P), generator=g, device=dev)
    AtA = A @ A.transpose(1, 2) / (2 * P) + torch.eye(P, device=dev)
    prob = type("Bare", (), {})()
    prob.c = ops.capi.Level()
    prob.c.B, prob.c.N, prob.c.K, prob.c.pairs, prob.c.basis = B, N, K, 1, basis.data_ptr()
    factor = timed(lambda: ops.ba_marginals(prob, AtA, damping=1e-3, want=("wfactor", "logdet"), ws=ws), warmup, reps)
    total = timed(lambda: ops.ba_marginals(prob, AtA, damping=1e-3, want=("depth_var",), ws=ws), warmup, reps)
    rec["depth_var_ms"] = total - factor
    rec["depth_var_over_bound"] = rec["depth_var_ms"] / rec["gram_bound_ms"]
    rec["gram_over_depth_var"] = rec["gram_ms"] / rec["depth_var_ms"]

    # reprojection: a dense level with those maps, one target frame, a small motion
    intr = torch.tensor([[0.9 * W, 0.9 * W, 0.5 * W, 0.5 * H]] * B, device=dev)
    lv = type("Bare", (), {})()
    lv.c = ops.capi.Level()
    c = lv.c
    c.B, c.N, c.K, c.H, c.W, c.dense, c.normalize_rays, c.scale, c.pairs = B, N, K, H, W, 1, 1, 1.0, 1
    c.depth, c.basis, c.intr = depth.data_ptr(), basis.data_ptr(), intr.data_ptr()
    R = torch.eye(3, device=dev).repeat(B, 1, 1)
    T = torch.tensor([[0.05, -0.02, 0.04]] * B, device=dev).reshape(B, 3, 1)
    Wc = 0.001 * torch.randn((B, K, 1), generator=g, device=dev)
    r = ops.depth_reproject(lv, R, T, Wc, ws=ws)
    torch.cuda.synchronize()
    rec["reproject_covered"] = float((r.index >= 0).float().mean())
    rec["reproject_ms"] = timed(lambda: ops.depth_reproject(lv, R, T, Wc, ws=ws), warmup, reps)
    rec["reproject_bound_ms"] = 1e3 * B * N * K * 4 / HBM_BYTES_PER_S
    rec["reproject_over_bound"] = rec["reproject_ms"] / rec["reproject_bound_ms"]
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    run(480, 640, 32, 128, a.warmup, a.reps)
    torch.cuda.empty_cache()
    run(960, 1280, 8, 256, a.warmup, a.reps)


if __name__ == "__main__":
    main()
