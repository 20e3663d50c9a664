#!/usr/bin/env python3
"""banet_ba_residual_f32 (maps + sums: two launches) next to banet_ba_assemble_f32 on the same level, in one process.

The assembly pass is the only way the library gave a cost before the residual entry existed (absres / nvalid, after the 12-tap
gradient stencil, the per-pixel records, the SYRK and the reduction).  Shapes, all C = K = 128, variant `bundle`:

    640x480 x 32 windows      40x30 x 32 windows      640x480 x 8 windows x 4 target frames

Timed with HIP events on pre-allocated outputs, alternately (residual, residual without sums, assembly) per repetition, median of
--reps after --warmup.  Achieved GB/s is taken on the algorithmic bytes 4 N (C (1 + pairs) + K + 1) per window
(DenseBA.algorithmic_bytes_per_iteration), and given as a share of the streaming-copy rate bench.py reports for the box
(roofline.streaming_copy_GBps; --streaming-gbps).

    python tools/bench_residual.py [--reps 20] [--warmup 3] [--streaming-gbps 6300]      (GPU box; prints one JSON line)
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

C = K = 128
SHAPES = [("640x480_B32", 480, 640, 32, 1), ("40x30_B32", 30, 40, 32, 1), ("640x480_B8_pairs4", 480, 640, 8, 4)]


def rodrigues(w):
    th = np.linalg.norm(w)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def make_level(H, W, B, pairs, dev, scale):
    """random maps, a smooth depth around 2.8, small poses: nearly every pixel stays in the image, as in a converging solve"""
    from banet_amd import ops
    g = torch.Generator(device=dev).manual_seed(H * 7 + B)
    src = torch.randn(B, H, W, C, device=dev, generator=g)
    tgt = torch.randn(B, pairs, H, W, C, device=dev, generator=g)
    depth = 2.8 + 0.3 * torch.rand(B, H * W, device=dev, generator=g)
    basis = torch.randn(B, H * W, K, device=dev, generator=g) * 0.1
    Wf, Hf = W * scale, H * scale
    intr = torch.tensor([[0.8 * Wf, 0.8 * Wf, Wf / 2.0, Hf / 2.0]] * B, dtype=torch.float32, device=dev)
    prob = ops.LevelProblem("bundle", src, tgt, depth, H, W, C, basis=basis, intr=intr, scale=float(scale), dense=True,
                            tgt_has_grad=False, normalize_rays=True, pairs=pairs)
    rng = np.random.RandomState(B + pairs)
    R = np.stack([rodrigues(rng.uniform(-1, 1, 3) * 0.012) for _ in range(B * pairs)]).astype(np.float32)
    T = (rng.uniform(-1, 1, (B * pairs, 3, 1)) * 0.03).astype(np.float32)
    Wc = (rng.standard_normal((B, K, 1)) * 0.08 / np.sqrt(K)).astype(np.float32)
    to = lambda a: torch.from_numpy(a).to(dev)   # noqa: E731
    return prob, to(R), to(T), to(Wc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--streaming-gbps", type=float, default=6300.0, help="roofline.streaming_copy_GBps of the box's bench.py line")
    ap.add_argument("--only", default=None, help="one shape name")
    args = ap.parse_args()
    from banet_amd import _capi as capi
    L = capi.lib()
    dev = torch.device("cuda:0")
    rec = {"tool": "bench_residual", "C": C, "K": K, "reps": args.reps, "streaming_copy_GBps": args.streaming_gbps, "shapes": {}}
    for name, H, W, B, pairs in SHAPES:
        if args.only and name != args.only:
            continue
        prob, R, T, Wc = make_level(H, W, B, pairs, dev, 640 // W)
        N, P = H * W, 6 * pairs + K
        sq = torch.empty(B, pairs, N, device=dev)
        ab = torch.empty(B, pairs, N, device=dev)
        mask = torch.empty(B, pairs, N, dtype=torch.uint8, device=dev)
        sums = torch.empty(B, pairs, 4, device=dev)
        out = capi.ResidualOut()
        out.sq, out.ab, out.mask, out.sums = sq.data_ptr(), ab.data_ptr(), mask.data_ptr(), sums.data_ptr()
        bare = capi.ResidualOut()
        bare.sq, bare.ab, bare.mask = sq.data_ptr(), ab.data_ptr(), mask.data_ptr()
        AtA, Atb = torch.empty(B, P, P, device=dev), torch.empty(B, P, device=dev)
        absres, nvalid = torch.empty(B, C, device=dev), torch.empty(B, device=dev)
        ws = capi.workspace(L.banet_ba_assemble_workspace_bytes(ctypes.byref(prob.c)), dev)
        lv = ctypes.byref(prob.c)

        def residual():
            capi.check(L.banet_ba_residual_f32(lv, capi.ptr(R), capi.ptr(T), capi.ptr(Wc), ctypes.byref(out), capi.stream()))

        def residual_maps():
            capi.check(L.banet_ba_residual_f32(lv, capi.ptr(R), capi.ptr(T), capi.ptr(Wc), ctypes.byref(bare), capi.stream()))

        def assemble():
            capi.check(L.banet_ba_assemble_f32(lv, capi.ptr(R), capi.ptr(T), capi.ptr(Wc), capi.ptr(AtA), capi.ptr(Atb), capi.ptr(absres),
                                               capi.ptr(nvalid), ctypes.c_void_p(ws.data_ptr()), ws.numel(), capi.stream()))

        fns = {"residual": residual, "residual_maps_only": residual_maps, "assemble": assemble}
        times = {k: [] for k in fns}
        for it in range(args.warmup + args.reps):
            for k, fn in fns.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if it >= args.warmup:
                    times[k].append(e0.elapsed_time(e1) * 1e3)
        by = 4 * N * (C * (1 + pairs) + K + 1) * B
        row = {"windows": B, "pairs": pairs, "N": N, "algorithmic_bytes": by, "in_image_share": round(float(mask.float().mean()), 4),
               "nvalid_agrees": bool(torch.equal(sums[..., 2].sum(1), nvalid))}
        for k, v in times.items():
            med = statistics.median(v)
            row[k + "_us"] = round(med, 1)
            row[k + "_us_min_max"] = [round(min(v), 1), round(max(v), 1)]
            row[k + "_GBps"] = round(by / med / 1e3, 1)
            row[k + "_share_of_streaming_copy"] = round(by / med / 1e3 / args.streaming_gbps, 3)
        row["residual_over_assemble"] = round(row["residual_us"] / row["assemble_us"], 3)
        rec["shapes"][name] = row
        del prob, sq, ab, mask, AtA, ws
        torch.cuda.empty_cache()
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
