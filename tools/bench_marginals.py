#!/usr/bin/env python3
"""Times banet_ba_marginals_f32 (csrc/marginals.hip) on the GPU, by hand -- not part of bench.py.

Two shapes: 640x480 x 32 windows with K = 128 (one target frame), and 1280x960 x 8 windows with K = 256, pairs = 7.  Per shape:
  factor     the call without depth_var (wfactor and logdet asked for): the factorisation kernel alone
  total      the call with depth_var: both kernels; depth_var = total - factor is the pass over the basis
  bound      max(bytes / 6.3 TB/s, triangle FLOPs / 157 TF) for the depth-variance kernel: one read of the basis + 4 bytes per pixel,
             2 FLOPs per entry of the lower 32 x 32 blocks of T per pixel
  assemble   one banet_ba_assemble_f32 at the same level (random maps; the "one more iteration" comparison)
Prints one JSON line per shape.  --skip-assemble leaves the last figure out (it needs the level's feature maps in memory)."""
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


def run(H, W, B, K, pairs, C, warmup, reps, assemble):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    N, P = H * W, 6 * pairs + K
    basis = torch.randn((B, N, K), generator=g, device=dev)
    G = torch.randn((B, P, 2 * P), generator=g, device=dev)
    AtA = G @ G.transpose(1, 2) / (2 * P) + torch.eye(P, device=dev)
    rec = dict(shape="%dx%d" % (W, H), B=B, K=K, pairs=pairs, P=P)
    if assemble:
        tgt_shape = (B, pairs, H, W, C) if pairs > 1 else (B, H, W, C)
        src = torch.randn((B, H, W, C), generator=g, device=dev)
        tgt = torch.randn(tgt_shape, generator=g, device=dev)
        depth = 2.5 + torch.rand((B, N), generator=g, device=dev)
        intr = torch.tensor([[0.9 * W, 0.9 * W, 0.5 * W, 0.5 * H]] * B, device=dev)
        prob = ops.LevelProblem("bundle", src, tgt, depth, H, W, C, basis=basis * 0.01, intr=intr, scale=1.0, dense=True,
                                tgt_has_grad=False, normalize_rays=True, pairs=pairs)
        R = torch.eye(3, device=dev).repeat(B * pairs, 1, 1).reshape(B, pairs, 3, 3)
        T = torch.zeros(B, pairs, 3, 1, device=dev)
        Wc = torch.zeros(B, K, 1, device=dev)
        rec["assemble_ms"] = timed(lambda: ops.ba_assemble(prob, R, T, Wc), warmup, reps)
        del src, tgt
    else:
        prob = type("Bare", (), {})()
        prob.c = ops.capi.Level()
        prob.c.B, prob.c.N, prob.c.K, prob.c.pairs, prob.c.basis = B, N, K, pairs, basis.data_ptr()
    ws = ops.capi.workspace(ops.ba_marginals_workspace_bytes(prob, True), dev)
    m = ops.ba_marginals(prob, AtA, damping=1e-3, sigma2=None, want=ops.MARGINALS_OUTPUTS, ws=ws)
    torch.cuda.synchronize()
    assert int(m.status.abs().sum()) == 0 and bool(torch.isfinite(m.depth_var).all())
    rec["factor_ms"] = timed(lambda: ops.ba_marginals(prob, AtA, damping=1e-3, want=("wfactor", "logdet"), ws=ws), warmup, reps)
    rec["total_ms"] = timed(lambda: ops.ba_marginals(prob, AtA, damping=1e-3, want=("depth_var",), ws=ws), warmup, reps)
    rec["depth_var_ms"] = rec["total_ms"] - rec["factor_ms"]
    nr = (K + 31) // 32
    nbytes = B * N * (K + 1) * 4
    flops = 2.0 * B * N * (nr * (nr + 1) // 2) * 1024
    rec["depth_var_bytes"], rec["depth_var_triangle_flops"] = nbytes, flops
    rec["depth_var_bound_ms"] = 1e3 * max(nbytes / HBM_BYTES_PER_S, flops / F32_MFMA_FLOPS)
    rec["depth_var_over_bound"] = rec["depth_var_ms"] / rec["depth_var_bound_ms"]
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-assemble", action="store_true")
    a = ap.parse_args()
    run(480, 640, 32, 128, 1, 128, a.warmup, a.reps, not a.skip_assemble)
    torch.cuda.empty_cache()
    run(960, 1280, 8, 256, 7, 128, a.warmup, a.reps, not a.skip_assemble)


if __name__ == "__main__":
    main()
