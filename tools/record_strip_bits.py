#!/usr/bin/env python3
"""Record the bits of the strip gather (ba_gather128s_kernel, csrc/gather128s.hip) on small seeded scenes -> an .npz file.

tests/golden/strip_parent_bits.npz was written by this script on an MI355X from the build of commit d44889b ("Gather: launches
from plan_gather_steps, one copy of shared helpers"), the last one whose strip kernel ran its lane = pixel reductions through
__shfl_xor; tests/test_gpu_strip_bits.py compares the current build with it bit for bit.  Re-record only from a build whose strip
kernel is known to be the reference.

    python3 tools/record_strip_bits.py OUT.npz

Per case: AtA, Atb, absres, nvalid and the mask of ops.ba_assemble(..., return_mask=True), and the per-pixel records the gather
leaves in the workspace for the SYRK (found through the host-side plan, tests/native/plan_host.cpp).  The inputs are made from
numpy's Mersenne Twister and + - * / sqrt alone, so that they are the same bits on every host (no libm, no BLAS)."""
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

C = 128
STRIP, SEG8, SEG32, DIRECT_ROWS, FRAME_LOOP = "DEV_FORCE_STRIP_GATHER", "DEV_QUARTER_TILES", "DEV_STRIP_ROWS32", "DEV_STRIP_DIRECT_ROWS", "DEV_STRIP_FRAME_LOOP"
# (name, W, H, windows, K, target frames, dev flags next to the forced strip kernel, large motion + ragged depth, same bits as case)
CASES = (
    ("w21_k128", 21, 24, 1, 128, 1, (), False, None),                # the narrowest map the window fits; segment rows 16 + 8
    ("w21_k0_fp4", 21, 24, 1, 0, 4, (), False, None),                # pose only, 4 waves per segment
    ("w21_k0_loop4", 21, 24, 1, 0, 4, (FRAME_LOOP,), False, "w21_k0_fp4"),
    ("w21_k256", 21, 24, 1, 256, 1, (), True, None),                 # two basis chunks per row
    ("w24h21_k128_seg8", 24, 21, 1, 128, 1, (SEG8,), False, None),   # 8-row segments: 8 + 8 + 5 rows, strips 16 + 8
    ("w24h21_k0", 24, 21, 1, 0, 1, (), True, None),
    ("w40_k128_fp4", 40, 37, 1, 128, 4, (), True, None),             # ragged both ways: strips 16 + 16 + 8, rows 16 + 16 + 5; rim, direct rows
    ("w40_k128_loop4", 40, 37, 1, 128, 4, (FRAME_LOOP,), True, "w40_k128_fp4"),
    ("w40_k256_fp4", 40, 37, 1, 256, 4, (), False, None),
    ("w40_k256_loop4", 40, 37, 1, 256, 4, (FRAME_LOOP,), False, "w40_k256_fp4"),
    ("w40_k0_seg32", 40, 37, 1, 0, 1, (SEG32,), True, None),         # 32-row segments: 32 + 5
    ("w40_k128_seg32", 40, 37, 1, 128, 1, (SEG32,), True, None),
    ("w40_k128_seg8", 40, 37, 1, 128, 1, (SEG8,), True, None),
    ("w40_k128_direct", 40, 37, 1, 128, 1, (DIRECT_ROWS,), False, None),   # every pixel row on the window-less path
    ("w40_k128", 40, 37, 1, 128, 1, (), True, None),                 # (also the differential case against ba_gather128_kernel)
    ("w64_k128", 64, 48, 2, 128, 1, (), False, None),                # whole segments, two windows
    ("w64_k0_fp4", 64, 48, 2, 0, 4, (), True, None),
    ("w64_k0_loop4", 64, 48, 2, 0, 4, (FRAME_LOOP,), True, "w64_k0_fp4"),
    ("w64_k256_seg8", 64, 48, 2, 256, 1, (SEG8,), False, None),
)
NAMES = ("AtA", "Atb", "absres", "nvalid", "mask", "records")


def case_by_name(name):
    return next(c for c in CASES if c[0] == name)


def make_inputs(case):
    """-> dict of float32 numpy arrays: intr [B,4], src [B,H,W,C], tgt [B,pairs,H,W,C], D0 [B,H,W], basis [B,H,W,K],
    R [B,pairs,3,3], T [B,pairs,3,1], Wc [B,K,1]"""
    name, W, H, B, K, pairs, _, big, _ = case
    rng = np.random.RandomState(1000 + 7 * W + 3 * K + pairs + (50 if big else 0))
    u = lambda *shape: rng.random_sample(shape) * 2.0 - 1.0
    f32 = lambda x: np.ascontiguousarray(x, np.float32)
    vv, uu = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    D0 = np.stack([1.5 + 0.25 * uu / W + 0.15 * vv / H + 0.02 * b for b in range(B)])
    if big:     # depth steps from pixel to pixel: footprints that do not fit the rolling window
        D0 = D0 + (rng.random_sample(D0.shape) < 0.08) * 1.5
    q = np.concatenate([np.ones((B, pairs, 1)), u(B, pairs, 3) * (0.02 if big else 0.003)], axis=-1)
    q = q / np.sqrt((q * q).sum(-1, keepdims=True))
    a, b_, c, d = (q[..., i] for i in range(4))
    R = np.stack([np.stack([a * a + b_ * b_ - c * c - d * d, 2 * (b_ * c - a * d), 2 * (b_ * d + a * c)], -1),
                  np.stack([2 * (b_ * c + a * d), a * a - b_ * b_ + c * c - d * d, 2 * (c * d - a * b_)], -1),
                  np.stack([2 * (b_ * d - a * c), 2 * (c * d + a * b_), a * a - b_ * b_ - c * c + d * d], -1)], -2)
    T = u(B, pairs, 3, 1) * (0.4 if big else 0.03)
    return dict(intr=f32(np.tile([0.8 * W, 0.8 * W, W / 2.0, H / 2.0], (B, 1))), src=f32(u(B, H, W, C)), tgt=f32(u(B, pairs, H, W, C)),
                D0=f32(D0), basis=f32(u(B, H, W, K) * 0.5), R=f32(R), T=f32(T), Wc=f32(u(B, K, 1) * 0.02))


def scene_stats(case):
    """float64 restatement of the kernel's geometry -> (pixels outside the target image, pixels on its rim, 16-pixel rows whose
    footprint does not fit the 21 x 7 texel window): what a scene puts in play (counts, not bits)"""
    name, W, H, B, K, pairs, _, _, _ = case
    x = {k: v.astype(np.float64) for k, v in make_inputs(case).items()}
    vv, uu = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    out = rim = wide = 0
    for b in range(B):
        fx, fy, ox, oy = x["intr"][b]
        ray = np.stack([(uu - ox) / fx, (vv - oy) / fy, np.ones_like(uu)], -1)
        ray = ray / np.sqrt((ray * ray).sum(-1, keepdims=True))
        D = x["D0"][b] + (x["basis"][b] @ x["Wc"][b])[..., 0]
        for p in range(pairs):
            X = (ray * D[..., None]) @ x["R"][b, p].T + x["T"][b, p, :, 0]
            px, py = fx * X[..., 0] / X[..., 2] + ox, fy * X[..., 1] / X[..., 2] + oy
            m = (px >= 0) & (px <= W - 1) & (py >= 0) & (py <= H - 1)
            x0, y0 = np.floor(px).astype(int), np.floor(py).astype(int)
            fast = m & (x0 >= 1) & (x0 + 2 <= W - 1) & (y0 >= 1) & (y0 + 2 <= H - 1)
            out += int((~m).sum())
            rim += int((m & ~fast).sum())
            for r in range(H):
                for s in range(0, W, 16):
                    f = fast[r, s:s + 16]
                    if f.any():
                        xs, ys = x0[r, s:s + 16][f], y0[r, s:s + 16][f]
                        wide += int(xs.max() - xs.min() + 4 > 21 or ys.max() - ys.min() + 4 > 7)
    return out, rim, wide


_plan_lib = None


def record_region(c, dev):
    """(byte offset, bytes) of the per-pixel records in the assembly workspace of level descriptor `c`: plan.hpp's AsmPlan"""
    global _plan_lib
    import tempfile
    import test_plan_cpu as tp
    if _plan_lib is None:
        _plan_lib = tp.build_host_lib(tempfile.mkdtemp(prefix="strip_bits_plan_"))
    col = {n: i for i, n in enumerate(tp.fields(_plan_lib))}
    cus = int(os.environ.get("BANET_NUM_CUS") or torch.cuda.get_device_properties(dev).multi_processor_count)
    row = np.asarray([[c.B, c.N, c.C, c.K, c.H, c.W, c.dense, c.tgt_has_grad, c.pairs, c.policy]], np.int32)
    o = tp.run_group(_plan_lib, row, int(c.flags), cus)[0]
    assert o[col["rc"]] == 0
    return int(o[col["off_rec"]]), int(o[col["g.rec_bytes"]])


def problem(case, dev, x=None):
    from banet_amd import dense as bdense
    from banet_amd.bundlenet import he_normal_lambda_weights
    name, W, H, B, K, pairs, _, _, _ = case
    x = x or make_inputs(case)
    t = lambda v: torch.from_numpy(v).to(dev)
    tgt = t(x["tgt"] if pairs > 1 else x["tgt"][:, 0])
    ba = bdense.DenseBA(t(x["intr"]), [bdense.DenseLevel(1, t(x["src"]), tgt, t(x["D0"]), t(x["basis"]) if K else None)],
                        [he_normal_lambda_weights(C, 1)], "bundle" if K else "bundle_camera", 1000.0)
    R = t(x["R"] if pairs > 1 else x["R"][:, 0])
    T = t(x["T"] if pairs > 1 else x["T"][:, 0])
    return ba, R, T, (t(x["Wc"]) if K else None)


def subsample(name, v):
    """what the file keeps of an output: AtA rows and record pixels are strided where they are large (1 MiB per committed file)"""
    if name == "AtA":
        return np.ascontiguousarray(v[:, ::max(1, v.shape[1] // 32)])
    if name == "records":
        return np.ascontiguousarray(v[:, ::(1 if v.shape[0] * v.shape[1] <= 1600 else 3)])
    return v


def run(case, dev, flags=None):
    """-> dict NAMES -> numpy array (records: [B * pairs, N, 8], absent at K = 0), subsampled as the file keeps them"""
    from banet_amd import _capi as capi, ops
    name, W, H, B, K, pairs, extra, _, _ = case
    ba, R, T, Wc = problem(case, dev)
    p = ba.problems[0]
    p.c.flags = flags if flags is not None else sum(getattr(capi, f) for f in (STRIP,) + tuple(extra))
    if flags is None:
        assert ops.gather_selection(p) == 3
    out = dict(zip(NAMES, (v.cpu().numpy() for v in ops.ba_assemble(p, R, T, Wc, return_mask=True))))
    if K:       # the same call on a workspace of our own, to read the records the gather left for the SYRK
        L = capi.lib()
        nb = L.banet_ba_assemble_workspace_bytes(ctypes.byref(p.c))
        ws = capi.workspace(nb, dev)
        ws.zero_()
        P = p.P
        o = [torch.empty(s, device=dev) for s in ((B, P, P), (B, P), (B, C), (B,))]
        capi.check(L.banet_ba_assemble_f32(ctypes.byref(p.c), capi.ptr(R), capi.ptr(T), capi.ptr(Wc), *(capi.ptr(v) for v in o),
                                           ctypes.c_void_p(ws.data_ptr()), ws.numel(), capi.stream()))
        torch.cuda.synchronize()
        off, nbytes = record_region(p.c, dev)
        n = B * pairs * W * H * 8
        assert nbytes >= 4 * n and off + nbytes <= ws.numel()
        out["records"] = ws[off:off + 4 * n].view(torch.float32).reshape(B * pairs, W * H, 8).cpu().numpy()
    return {k: subsample(k, v) for k, v in out.items()}


def main():
    dev = torch.device("cuda:0")
    rec = {}
    for case in CASES:
        if case[8] is not None:
            continue
        for k, v in run(case, dev).items():
            rec["%s/%s" % (case[0], k)] = v
        print(case[0], "outside / rim / wide rows:", scene_stats(case))
    np.savez_compressed(sys.argv[1], **rec)
    print("recorded %d arrays, %d bytes" % (len(rec), os.path.getsize(sys.argv[1])))


if __name__ == "__main__":
    main()
