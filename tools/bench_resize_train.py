#!/usr/bin/env python3
"""One training step of BundleNet.BundleResize and one of CameraResize at the reference's training shape (256x320, levels at
scale 8/4/2/1, basis and depth at half resolution, N = 4096 points, C = K = 128): forward, then backward to `layers`, `basis`,
`init_depth` and the lambda weights, with prep_graph="torch" and "hip" alternated in one process.  Per setting: the median ms per
step (device-synchronised), the peak device memory, and whether the gradients of two runs are bit-identical.  One JSON line per
(pairs, prep_graph).
    python tools/bench_resize_train.py [--pairs 4 8] [--steps 10] [--warmup 3] [--only hip --steps 1 --warmup 1]
(--only: one setting alone, e.g. under rocprofv3 --kernel-trace --stats)."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from banet_amd import bundlenet  # noqa: E402

H, W, N, C, K = 256, 320, 4096, 128, 128


def make_inputs(images, seed):
    g = torch.Generator().manual_seed(seed)
    dev = "cuda:0"
    layers = [(torch.randn(images, H // s, W // s, C, generator=g) * 0.5).to(dev) for s in (8, 4, 2, 1)]
    basis = (torch.randn(images, H // 2, W // 2, K, generator=g) * 0.05).to(dev)
    depth = (2.0 + torch.rand(images, H // 2, W // 2, 1, generator=g)).to(dev)
    pts = torch.stack([10 + 300 * torch.rand(images, N, generator=g), 10 + 220 * torch.rand(images, N, generator=g)], -1).to(dev)
    intr = torch.tensor([0.8 * W * 39 / 40, 0.8 * W * 29 / 32, (W / 2 + 160 / 39) * 39 / 40, (H / 2 + 128 / 29) * 29 / 32])
    intr = intr.reshape(1, 4, 1).repeat(images, 1, 1).to(dev)
    lw = {str(l): [(w.to(dev), b.to(dev)) for w, b in bundlenet.he_normal_lambda_weights(C, 100 + l)] for l in range(4)}
    return dict(layers=layers, basis=basis, depth=depth, points=pts, intr=intr, lw=lw)


def step(inp, prep_graph):
    """forward of both drivers + backward; returns the gradients in a fixed order"""
    lw = {k: [(w.clone().requires_grad_(True), b.clone().requires_grad_(True)) for w, b in v] for k, v in inp["lw"].items()}
    net = bundlenet.BundleNet(lambda_weights=lw, prep_graph=prep_graph)
    layers = [x.clone().requires_grad_(True) for x in inp["layers"]]
    basis, depth = inp["basis"].clone().requires_grad_(True), inp["depth"].clone().requires_grad_(True)
    Rb, Tb, Db = net.BundleResize(inp["intr"], layers, inp["points"], basis, depth)
    Rc, Tc = net.CameraResize(inp["intr"], layers, inp["points"], depth.detach())
    loss = sum(x.abs().sum() for x in Tb + Tc) + sum((x - torch.eye(3, device=x.device)).square().sum() for x in Rb + Rc) \
        + sum(x.mean() for x in Db)
    leaves = layers + [basis, depth] + [t for v in lw.values() for pair in v for t in pair]
    return torch.autograd.grad(loss, leaves, allow_unused=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, nargs="+", default=[4, 8])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=["torch", "hip"], default=None)
    a = ap.parse_args()
    settings = [a.only] if a.only else ["torch", "hip"]
    for pairs in a.pairs:
        inp = make_inputs(2 * pairs, 7)
        times = {s: [] for s in settings}
        grads = {s: [] for s in settings}
        peak = {s: 0 for s in settings}
        for it in range(a.warmup + a.steps):
            for s in settings:                                # alternated, one process
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                t0 = time.perf_counter()
                g = step(inp, s)
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) * 1e3
                peak[s] = max(peak[s], torch.cuda.max_memory_allocated())
                if it >= a.warmup:
                    times[s].append(ms)
                if len(grads[s]) < 2 and it >= a.warmup:
                    grads[s].append([None if x is None else x.detach().clone() for x in g])
                del g
        for s in settings:
            ts = sorted(times[s])
            same = None
            if len(grads[s]) == 2:
                same = all((x is None and y is None) or (x is not None and y is not None and torch.equal(x, y))
                           for x, y in zip(*grads[s]))
            print(json.dumps({"tool": "bench_resize_train", "pairs": pairs, "images": 2 * pairs, "prep_graph": s,
                              "median_ms": round(ts[len(ts) // 2], 3) if ts else None, "min_ms": round(ts[0], 3) if ts else None,
                              "steps": len(ts), "peak_mib": round(peak[s] / 2 ** 20, 1), "grads_bit_identical": same,
                              "shape": "%dx%d, levels 8/4/2/1, N=%d, C=%d, K=%d" % (H, W, N, C, K)}), flush=True)
        del inp
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
