#!/usr/bin/env python3
"""Dense level preparation against the general resampler, in one process.

Workload: the decoder's basis map [8,240,320,128] and the five levels of the 640 x 480 headline pyramid (40x30 .. 640x480: steps
8, 4, 2, 1, 1/2 over the half-resolution map), clamped taps.  Timed alternately, median of --reps after --warmup:

  forward  (a) banet_grid_resample_f32, all levels in one launch        against   ops.resample on pre-built explicit grids, per level
  adjoint  (b) banet_grid_resample_grad_f32, one launch over the texels  against   prep_grad.resampler_grad_forward per level + the
                                                                                   adds that sum the levels

The yardstick is the existing general path (the library's own ba_resample_kernel / banet_resample_grad_f32) in the same run.  The
identity level (step 1) is timed as the C entries run it; dense_prep.grid_pyramid returns it zero-copy instead.

    python tools/bench_dense_prep.py [--reps 20] [--warmup 3] [--streaming-gbps 6300]      (GPU box; prints one JSON line)
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

B, H, W, C = 8, 240, 320, 128
SHAPES = [(30, 40), (60, 80), (120, 160), (240, 320), (480, 640)]
SCALES = [16, 8, 4, 2, 1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--streaming-gbps", type=float, default=6300.0, help="roofline.streaming_copy_GBps of the box's bench.py line")
    args = ap.parse_args()
    from banet_amd import _capi as capi, dense_prep, ops, prep_grad
    dev = torch.device("cuda:0")
    geoms = dense_prep.grid_levels(H, W, SHAPES, SCALES, 2)
    g = torch.Generator(device="cpu").manual_seed(0)
    data = torch.randn(B, H, W, C, generator=g).to(dev)
    warps, gouts = [], []
    for Ho, Wo, sx, sy, ox, oy in geoms:
        x = (np.arange(Wo, dtype=np.float32) * np.float32(sx)).astype(np.float32) + np.float32(ox)
        y = (np.arange(Ho, dtype=np.float32) * np.float32(sy)).astype(np.float32) + np.float32(oy)
        w = np.stack(np.broadcast_arrays(x[None, :], y[:, None]), axis=-1).reshape(1, Ho * Wo, 2)
        warps.append(torch.from_numpy(np.ascontiguousarray(np.repeat(w, B, axis=0))).to(dev))
        gouts.append(torch.randn(B, Ho, Wo, C, device=dev))

    def fwd_new():
        return dense_prep.grid_resample(data, geoms, clamp=True)

    def fwd_old():
        return [ops.resample(data, w, clamp=True) for w in warps]

    def bwd_new():
        return dense_prep.grid_resample_grad(gouts, geoms, tuple(data.shape), clamp=True)

    def bwd_old():
        total = None
        for w, go in zip(warps, gouts):
            d, _ = prep_grad.resampler_grad_forward(data, w, go.reshape(B, -1, C), clamp=True, want_warp=False)
            total = d if total is None else total.add_(d)
        return total

    # the two paths agree before anything is timed
    for a, b in zip(fwd_new(), fwd_old()):
        assert torch.equal(a.reshape(b.shape), b)
    dn, do = bwd_new(), bwd_old()
    scale = float(do.abs().max())
    assert float((dn - do).abs().max()) <= 1e-5 * scale, (float((dn - do).abs().max()), scale)
    del dn, do

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        del out
        return e0.elapsed_time(e1)

    res = {}
    for name, new, old in (("forward", fwd_new, fwd_old), ("adjoint", bwd_new, bwd_old)):
        for _ in range(args.warmup):
            timed(new), timed(old)
        tn, to = [], []
        for _ in range(args.reps):                   # alternating
            tn.append(timed(new))
            to.append(timed(old))
        res[name] = dict(grid_ms=round(statistics.median(tn), 4), general_ms=round(statistics.median(to), 4),
                         grid_ms_min=round(min(tn), 4), general_ms_min=round(min(to), 4))
        res[name]["speedup"] = round(res[name]["general_ms"] / res[name]["grid_ms"], 3)
    level_bytes = 4 * B * C * sum(h * w for h, w in SHAPES)
    map_bytes = 4 * B * H * W * C
    for name in ("forward", "adjoint"):          # algorithmic bytes: every level once + the map once
        gbps = (level_bytes + map_bytes) / (res[name]["grid_ms"] * 1e-3) / 1e9
        res[name]["grid_GBps"] = round(gbps, 1)
        res[name]["fraction_of_streaming_copy"] = round(gbps / args.streaming_gbps, 3)
    print(json.dumps(dict(tool="bench_dense_prep", build_id=capi.lib().banet_build_id().decode(), workload=dict(map=[B, H, W, C], levels=SHAPES,
                          mode="clamp"), reps=args.reps, warmup=args.warmup, algorithmic_bytes=level_bytes + map_bytes,
                          streaming_copy_GBps=args.streaming_gbps, device=torch.cuda.get_device_name(0), **res)))


if __name__ == "__main__":
    main()
