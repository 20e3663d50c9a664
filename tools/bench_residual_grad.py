#!/usr/bin/env python3
"""banet_ba_residual_grad_f32 next to its forward and to the assembly adjoint on the same level, in one process.

Shapes: those of tools/bench_residual.py (its levels, its states), all C = K = 128, variant `bundle`:

    640x480 x 32 windows      40x30 x 32 windows      640x480 x 8 windows x 4 target frames

Per shape, alternately per repetition: the backward with every output (gsq, gab and gproj given), the backward without dtgt, the
forward banet_ba_residual_f32 (maps only), and -- two-frame shapes -- banet_dense_adjoint_ex_f32 producing the uniform-L1 gradient
(gAtA = gAtb = 0, gabs = 1, FOLD_TARGET | OVERWRITE | OVERWRITE_MAP) next to the backward on the same gradient (gab = 1, the rest
NULL).  HIP events on pre-allocated outputs, median of --reps after --warmup.

Algorithmic bytes of the backward per window, as DESIGN.md 4.11 states them:
    reads   4 N (C (1 + pairs) + K + 1 + 4 pairs)      source, targets, basis, depth, gsq + gab + gproj
    writes  4 N (C + K + 1)                            dsrc, dbasis, ddepth
    dtgt    + 4 N C pairs (the map) + 4 N C pairs (the e rows it materialises)
GB/s on those bytes and the share of the streaming-copy rate bench.py reports for the box (--streaming-gbps).

    python tools/bench_residual_grad.py [--reps 20] [--warmup 3] [--streaming-gbps 6300] [--only NAME]     (GPU box; one JSON line)
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_residual import C, K, SHAPES, make_level  # noqa: E402

FOLD_OVERWRITE = 4 | 1 | 2      # BANET_ADJOINT_FOLD_TARGET | _OVERWRITE | _OVERWRITE_MAP


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
    rec = {"tool": "bench_residual_grad", "C": C, "K": K, "reps": args.reps, "streaming_copy_GBps": args.streaming_gbps, "shapes": {}}
    for name, H, W, B, pairs in SHAPES:
        if args.only and name != args.only:
            continue
        prob, R, T, Wc = make_level(H, W, B, pairs, dev, 640 // W)
        N, P = H * W, 6 * pairs + K
        lv = ctypes.byref(prob.c)
        g = torch.Generator(device=dev).manual_seed(5)
        gsq = torch.rand(B, pairs, N, device=dev, generator=g) + 0.5
        gab = torch.rand(B, pairs, N, device=dev, generator=g) + 0.5
        gproj = torch.randn(B, pairs, N, 2, device=dev, generator=g)
        ones = torch.ones(B, pairs, N, device=dev)
        o = dict(dsrc=torch.empty(B, N, C, device=dev), dtgt=torch.empty(B, pairs, H, W, C, device=dev), ddepth=torch.empty(B, N, device=dev),
                 dbasis=torch.empty(B, N, K, device=dev), dWc=torch.empty(B, K, device=dev), dR=torch.empty(B, pairs, 9, device=dev),
                 dT=torch.empty(B, pairs, 3, device=dev))
        gin, gl1, full, nomap = capi.ResidualGradIn(), capi.ResidualGradIn(), capi.ResidualGradOut(), capi.ResidualGradOut()
        gin.gsq, gin.gab, gin.gproj = gsq.data_ptr(), gab.data_ptr(), gproj.data_ptr()
        gl1.gab = ones.data_ptr()
        for k, v in o.items():
            setattr(full, k, v.data_ptr())
            if k != "dtgt":
                setattr(nomap, k, v.data_ptr())
        ws = capi.workspace(L.banet_ba_residual_grad_workspace_bytes(lv, 1), dev)
        sq, ab = torch.empty(B, pairs, N, device=dev), torch.empty(B, pairs, N, device=dev)
        mask = torch.empty(B, pairs, N, dtype=torch.uint8, device=dev)
        fo = capi.ResidualOut()
        fo.sq, fo.ab, fo.mask = sq.data_ptr(), ab.data_ptr(), mask.data_ptr()
        pR, pT, pW, pws = capi.ptr(R), capi.ptr(T), capi.ptr(Wc), ctypes.c_void_p(ws.data_ptr())

        def backward(gi, out):
            return lambda: capi.check(L.banet_ba_residual_grad_f32(lv, pR, pT, pW, ctypes.byref(gi), ctypes.byref(out), 3, pws, ws.numel(),
                                                                   capi.stream()))
        fns = {"backward": backward(gin, full), "backward_no_dtgt": backward(gin, nomap),
               "forward": lambda: capi.check(L.banet_ba_residual_f32(lv, pR, pT, pW, ctypes.byref(fo), capi.stream()))}
        if pairs == 1:
            zA, zb, gabs = torch.zeros(B, P, P, device=dev), torch.zeros(B, P, device=dev), torch.ones(B, C, device=dev)
            dpose = torch.empty(B, 12 + K, device=dev)
            aws = capi.workspace(L.banet_dense_adjoint_workspace_bytes_ex(lv, FOLD_OVERWRITE), dev)
            fns["backward_uniform_l1"] = backward(gl1, full)
            fns["dense_adjoint_uniform_l1"] = lambda: capi.check(L.banet_dense_adjoint_ex_f32(
                lv, pR, pT, pW, capi.ptr(zA), capi.ptr(zb), capi.ptr(gabs), capi.ptr(o["dsrc"]), capi.ptr(o["dtgt"]), capi.ptr(o["ddepth"]),
                capi.ptr(o["dbasis"]), capi.ptr(dpose), FOLD_OVERWRITE, ctypes.c_void_p(aws.data_ptr()), aws.numel(), capi.stream()))
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
        reads = 4 * N * (C * (1 + pairs) + K + 1 + 4 * pairs) * B
        writes = 4 * N * (C + K + 1) * B
        map_bytes = 2 * 4 * N * C * pairs * B
        fwd_bytes = 4 * N * (C * (1 + pairs) + K + 1) * B
        by = {"backward": reads + writes + map_bytes, "backward_no_dtgt": reads + writes, "forward": fwd_bytes,
              "backward_uniform_l1": reads + writes + map_bytes - 3 * 4 * N * pairs * B, "dense_adjoint_uniform_l1": None}
        row = {"windows": B, "pairs": pairs, "N": N, "in_image_share": round(float(mask.float().mean()), 4),
               "algorithmic_bytes": {"reads": reads, "writes": writes, "dtgt_and_e_rows": map_bytes}}
        for k, v in times.items():
            med = statistics.median(v)
            row[k + "_us"] = round(med, 1)
            row[k + "_us_min_max"] = [round(min(v), 1), round(max(v), 1)]
            if by[k]:
                row[k + "_GBps"] = round(by[k] / med / 1e3, 1)
                row[k + "_share_of_streaming_copy"] = round(by[k] / med / 1e3 / args.streaming_gbps, 3)
        row["backward_over_forward"] = round(row["backward_us"] / row["forward_us"], 3)
        if pairs == 1:
            row["backward_over_dense_adjoint_uniform_l1"] = round(row["backward_uniform_l1_us"] / row["dense_adjoint_uniform_l1_us"], 3)
        rec["shapes"][name] = row
        del prob, o, ws, gsq, gab, gproj, ones, sq, ab, mask
        if pairs == 1:
            del zA, aws
        torch.cuda.empty_cache()
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
