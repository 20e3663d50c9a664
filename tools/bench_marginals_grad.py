#!/usr/bin/env python3
"""Times banet_ba_marginals_grad_f32 (csrc/marginals_grad.hip) on the GPU, by hand -- not part of bench.py.

The two shapes of tools/bench_marginals.py: 640x480 x 32 windows with K = 128 (one target frame), and 1280x960 x 8 windows with
K = 256, pairs = 7.  HIP events, median of --reps.  The kernels are separated by what a call is asked for:
  factor      g_pose_cov + g_logdet -> gAtA: marg_grad_factor_kernel alone                    (against the forward's factor kernel)
  gram        g_depth_var -> gAtA, minus `factor`: marg_grad_gram_kernel + its fold          (against ops.basis_fit on the same
              basis: fit_gram_kernel + fold + the K x K solve)
  basis       everything -> gAtA + gbasis, minus the call without gbasis: marg_grad_basis_kernel (against marg_depthvar_kernel;
              its bound: max(2 x the matrix bound of the forward pass, bytes at the streaming-copy rate measured in this run),
              bytes = one read of the basis + one write of [N,K] + g)
  total       the whole entry, next to one banet_dense_adjoint_ex_f32 call at the same level (random maps)
Prints one JSON line per shape.  --skip-adjoint leaves the last figure out (it needs the level's feature maps in memory)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from banet_amd import dense_train, ops  # noqa: E402
from bench_marginals import F32_MFMA_FLOPS, timed  # noqa: E402


def run(H, W, B, K, pairs, C, warmup, reps, adjoint):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    N, P, m = H * W, 6 * pairs + K, 6 * pairs
    basis = torch.randn((B, N, K), generator=g, device=dev)
    G = torch.randn((B, P, 2 * P), generator=g, device=dev)
    AtA = G @ G.transpose(1, 2) / (2 * P) + torch.eye(P, device=dev)
    g_cov = torch.randn((B, m, m), generator=g, device=dev)
    g_dv = torch.randn((B, N), generator=g, device=dev)
    g_ld = torch.randn((B,), generator=g, device=dev)
    rec = dict(shape="%dx%d" % (W, H), B=B, K=K, pairs=pairs, P=P)
    prob = type("Bare", (), {})()
    prob.c = ops.capi.Level()
    prob.c.B, prob.c.N, prob.c.K, prob.c.pairs, prob.c.basis = B, N, K, pairs, basis.data_ptr()
    L = ops.capi.lib()
    import ctypes
    ws = ops.capi.workspace(L.banet_ba_marginals_grad_workspace_bytes(ctypes.byref(prob.c), 1), dev)
    rec["workspace_bytes"] = ws.numel()
    call = lambda want, **ups: ops.ba_marginals_grad(prob, AtA, damping=1e-3, sigma2=None, want=want, ws=ws, **ups)  # noqa: E731
    r = call(ops.MARGINALS_GRAD_OUTPUTS, g_pose_cov=g_cov, g_depth_var=g_dv, g_logdet=g_ld)
    torch.cuda.synchronize()
    assert int(r.status.abs().sum()) == 0 and bool(torch.isfinite(r.gbasis).all()) and bool(torch.isfinite(r.gAtA).all())
    del r
    rec["factor_ms"] = timed(lambda: call(("gAtA",), g_pose_cov=g_cov, g_logdet=g_ld), warmup, reps)
    no_gb = timed(lambda: call(("gAtA",), g_pose_cov=g_cov, g_depth_var=g_dv, g_logdet=g_ld), warmup, reps)
    rec["gram_ms"] = no_gb - rec["factor_ms"]
    rec["total_ms"] = timed(lambda: call(("gAtA", "gbasis"), g_pose_cov=g_cov, g_depth_var=g_dv, g_logdet=g_ld), warmup, reps)
    rec["basis_ms"] = rec["total_ms"] - no_gb
    # the forward's kernels and the basis fit on the same basis
    fws = ops.capi.workspace(ops.ba_marginals_workspace_bytes(prob, True), dev)
    rec["fwd_factor_ms"] = timed(lambda: ops.ba_marginals(prob, AtA, damping=1e-3, want=("wfactor", "logdet"), ws=fws), warmup, reps)
    rec["fwd_depth_var_ms"] = timed(lambda: ops.ba_marginals(prob, AtA, damping=1e-3, want=("depth_var",), ws=fws), warmup, reps) - rec["fwd_factor_ms"]
    depth, w = torch.zeros((B, N), device=dev), g_dv.abs()
    rec["basis_fit_ms"] = timed(lambda: ops.basis_fit(depth, basis, g_dv, weight=w, damping=1e-3), warmup, reps)
    # the streaming-copy rate of this run, on a buffer of the basis's size
    dst = torch.empty_like(basis)
    copy_ms = timed(lambda: dst.copy_(basis), warmup, reps)
    rate = 2.0 * basis.numel() * 4 / (copy_ms * 1e-3)
    del dst
    nr = (K + 31) // 32
    flops = 2.0 * B * N * (nr * (nr + 1) // 2) * 1024             # the forward pass's triangle; the backward pass does it twice
    nbytes = B * N * (2 * K + 1) * 4
    rec["copy_bytes_per_s"] = rate
    rec["basis_matrix_bound_ms"], rec["basis_bytes_bound_ms"] = 1e3 * 2 * flops / F32_MFMA_FLOPS, 1e3 * nbytes / rate
    rec["basis_bound_ms"] = max(rec["basis_matrix_bound_ms"], rec["basis_bytes_bound_ms"])
    rec["basis_over_bound"] = rec["basis_ms"] / rec["basis_bound_ms"]
    rec["basis_over_fwd_depth_var"] = rec["basis_ms"] / rec["fwd_depth_var_ms"]
    if adjoint:
        src = torch.randn((B, H, W, C), generator=g, device=dev)
        tgt = torch.randn((B, H, W, C), generator=g, device=dev)
        intr = torch.tensor([[0.9 * W, 0.9 * W, 0.5 * W, 0.5 * H]] * B, device=dev)
        basis.mul_(0.01)
        lp = ops.LevelProblem("bundle", src, tgt, 2.5 + torch.rand((B, N), generator=g, device=dev), H, W, C, basis=basis, intr=intr,
                              scale=1.0, dense=True, tgt_has_grad=False, normalize_rays=True, pairs=1)
        R, T, Wc = torch.eye(3, device=dev).repeat(B, 1, 1), torch.zeros(B, 3, 1, device=dev), torch.zeros(B, K, 1, device=dev)
        P1 = 6 + K
        gA, gb, gabs = (torch.randn(s, generator=g, device=dev) for s in ((B, P1, P1), (B, P1), (B, C)))
        gA = gA + gA.transpose(1, 2)
        outs = [torch.empty(s, device=dev) for s in ((B, N, C), (B, H, W, C), (B, N), (B, N, K))]
        aws = [None]

        def adj():
            aws[0] = dense_train.dense_adjoint(lp, R, T, Wc, gA, gb, gabs, *outs, aws[0], overwrite=True, fold=True)[1]
        rec["dense_adjoint_ms"] = timed(adj, warmup, reps)
        rec["total_over_dense_adjoint"] = rec["total_ms"] / rec["dense_adjoint_ms"]
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-adjoint", action="store_true")
    a = ap.parse_args()
    run(480, 640, 32, 128, 1, 128, a.warmup, a.reps, not a.skip_adjoint)
    torch.cuda.empty_cache()
    run(960, 1280, 8, 256, 7, 128, a.warmup, a.reps, not a.skip_adjoint)


if __name__ == "__main__":
    main()
