"""Inputs and float64 references for the kernel-level tests of the SPARSE-layout assembly adjoint (csrc/adjoint.hip and the
adjoint_*.hip files behind it: adj_pixel_kernel<CJ, KJ, SP = true> and the seed-GEMM / cell-scan / per-texel gather kernels around
it), one generator shared by
the CPU module (test_adjoint_cases_cpu.py: the conditions on the inputs, the float32 yardstick, the dispatch coverage) and the GPU
module (test_gpu_sparse_adjoint.py).  No GPU here: torch + the oracle only.

The statement: oracle/torch_port.sparse_assemble (bundlenet.py:122-278 up to AtA / Atb, pinned to the numpy oracle in
test_torch_ref_cpu.py).  The reference adjoint is autograd through it in float64 with the loss
    sum(G * AtA) + sum(gb * Atb) + sum(gabs * absd),        G not symmetric on purpose,
w.r.t. conv1, conv2 (the [f|gx|gy] map), D, Bs, R (nine free entries), T, Wc.  All inputs are float32 numbers on both sides.

A case: target map and source features standard normal; points uniform over [-0.1 W, 1.1 W] x [-0.1 H, 1.1 H]; intrinsics that
differ from point to point and from window to window, fx = (0.7 + 0.3 u) W, fy = (0.6 + 0.3 u') W (so fx != fy), ox = W / 2 + 2 n,
oy = H / 2 + 2 n'; rays from the points and their own intrinsics, normalised; D in [2.5, 3.5]; Bs = randn / sqrt(K);
R = rodrigues(0.004 randn), T = 0.02 randn, Wc = 0.01 randn; G, gb ~ N(0, 1), gabs ~ 0.1 N(0, 1).  The bilinear gradient and the
mask jump at integer coordinates, |d| has a kink at 0: a point whose float64 projection is within INT_MARGIN of an integer gets
ox / oy moved by 0.01 (repeated until none is left), a masked-in |d| below 1e-5 gets its source feature moved by 1e-3 -- so that a
float32 and a float64 evaluation never land on different sides.
"""
import atexit
import collections
import ctypes
import functools
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import torch

from oracle import torch_port

INT_MARGIN = 2e-3          # no projection closer than this to an integer coordinate (the image border included)
MIN_ABS_D = 1e-6           # every masked-in |d| at least this
GATE = dict(dsrc=2e-4, dmap3=2e-4, ddepth=2e-4, dbasis=2e-4, dR=5e-4, dT=5e-4, dW=5e-4)      # the dense layout's gates (test_gpu_dense_backward.py)
OUTSIDE_SHARE = (0.10, 0.60)                     # share of a window's points outside the image, default recipe
FORWARD_GATE = 5e-5                              # test_random_shape_sweep_assembly_matches_oracle's
OUTPUTS = ("dsrc", "dmap3", "ddepth", "dbasis", "dR", "dT", "dW")

Case = collections.namedtuple("Case", "name variant B N C K H W seed special")
# special: None       the recipe above
#          "inside"   N <= 3: the points are drawn inside the image (a share of outside points means nothing for 1 or 3 points, and a
#                     window must not be empty by accident)
#          "empty"    window 1 of 3 is translated out of view: every point of it outside the image
#          "cluster"  every point starts in [7.3, 8.7] x [9.3, 9.7]: all projections fall into the two cells (7, 9) and (8, 9)

# ---- sparse layout, bundle: all 12 adj_pixel_kernel<cj, kj, true> instantiations and every seed-GEMM class
#      (cj, kj) / seed:   (1,1) b<1>  (2,1) b6<3>  (3,1) b6<2>  (4,1) b6<4>  (1,2) b6<5>  (2,2) b6<8>  (3,2) b6<6>  (4,2) b6<7>
#                         (1,3) w<12> (2,3) w<12>  (1,4) w<16>  (2,4) w<16>
SPARSE_BUNDLE_CK = [(5, 3), (70, 33), (130, 20), (256, 64), (64, 72), (128, 128), (192, 90), (200, 100), (32, 136), (100, 192),
                    (7, 255), (128, 256)]
# ---- sparse layout, pose only (bundle_camera, K = 0)
SPARSE_CAMERA_C = [6, 128, 131, 255]
# ---- ragged splits of the points over the waves, at (70, 33): (N, B)
RAGGED_N = [(1, 2), (3, 2), (63, 2), (64, 2), (65, 3), (257, 2)]
# ---- the cell scan across its 1024-cell chunks, at (16, 8): (H, W) = 16 cells, exactly 1024, 1025
SCAN_MAPS = [(4, 4), (32, 32), (25, 41)]


def _cases():
    out = []
    for i, (C, K) in enumerate(SPARSE_BUNDLE_CK):
        out.append(Case("bundle-C%d-K%d" % (C, K), "bundle", 2, 500, C, K, 20, 24, 100 + i, None))
    for i, C in enumerate(SPARSE_CAMERA_C):
        out.append(Case("camera-C%d" % C, "bundle_camera", 2, 500, C, 0, 20, 24, 200 + i, None))
    for i, (N, B) in enumerate(RAGGED_N):
        out.append(Case("ragged-N%d-B%d" % (N, B), "bundle", B, N, 70, 33, 20, 24, 300 + i, "inside" if N <= 3 else None))
    for i, (H, W) in enumerate(SCAN_MAPS):
        out.append(Case("scan-%dx%d" % (H, W), "bundle", 2, 500, 16, 8, H, W, 400 + i, None))
    out.append(Case("empty-window", "bundle", 3, 500, 70, 33, 20, 24, 500, "empty"))
    out.append(Case("cluster-two-cells", "bundle", 2, 300, 16, 8, 20, 24, 501, "cluster"))
    out.append(Case("N4096-8x8", "bundle", 2, 4096, 16, 8, 8, 8, 502, None))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
# the share of outside points is not asserted for (the reason per case):
NO_OUTSIDE_SHARE = {
    "ragged-N1-B2": "one point", "ragged-N3-B2": "three points",
    "scan-4x4": "the in-image region [0, 3]^2 is 39 % of the [-0.4, 4.4]^2 the points are drawn from: 61 % expected",
    "empty-window": "window 1 is empty by construction (the other two are asserted)",
    "cluster-two-cells": "every point inside by construction",
}
# banet_ba_assemble_f32 has no kernel for these (csrc/plan.hpp, plan_gather_steps: the generic gather kernel is compiled for one
# channel / coefficient per lane up to 128 and two per lane up to 256, so an odd C or K above 128 returns BANET_ERR_UNSUPPORTED): the
# adjoint takes them, the forward test asserts the refusal and that dense_train.sparse_iteration_supported says so
FORWARD_NOT_COMPILED = {"bundle-C7-K255": "odd K > 128", "camera-C131": "odd C > 128", "camera-C255": "odd C > 128"}
# one case per per-pixel code object family of the sparse layout (3 waves per SIMD: KJ <= 2; 2 waves: KJ >= 3; pose only)
ACCUMULATION_CASES = ("bundle-C70-K33", "bundle-C32-K136", "camera-C131")
REPRODUCIBILITY_CASE = "bundle-C128-K128"


def _r32(x):
    return x.to(torch.float32).to(torch.float64)


def _frac_dist(v):
    return (v - torch.round(v)).abs()


def assemble(inp, dtype=torch.float64, leaves=None):
    """oracle/torch_port.sparse_assemble on a case's inputs (or on `leaves` in place of the seven differentiable ones)"""
    c = lambda v: None if v is None else v.to(dtype)          # noqa: E731
    lv = leaves if leaves is not None else [c(inp[k]) for k in ("conv1", "conv2", "D", "Bs", "R", "T", "Wc")]
    return torch_port.sparse_assemble(lv[0], lv[1], lv[2], lv[3], lv[4], lv[5], lv[6], inp["bundle"], c(inp["fx"]), c(inp["fy"]),
                                      c(inp["ox"]), c(inp["oy"]), c(inp["p"]))


def make_case(case):
    """-> dict of float64 tensors whose values are float32 numbers: conv1 [B,N,C], conv2 [B,H,W,3C], D [B,N,1], Bs [B,N,K] / None,
    R [B,3,3], T [B,3,1], Wc [B,K,1] / None, fx, fy, ox, oy [B,N], p [B,3,N], G [B,P,P], gb [B,P], gabs [B,C]; bundle (bool);
    nudges = passes of the integer-coordinate nudge that moved something."""
    B, N, C, K, H, W = case.B, case.N, case.C, case.K, case.H, case.W
    bundle = case.variant == "bundle"
    assert bundle == (K > 0)
    g = torch.Generator().manual_seed(case.seed)
    dd = torch.float64
    r = lambda *s: torch.rand(*s, generator=g, dtype=dd)         # noqa: E731
    rn = lambda *s: torch.randn(*s, generator=g, dtype=dd)       # noqa: E731
    conv2, conv1 = rn(B, H, W, 3 * C), rn(B, N, C)
    ux, uy = r(B, N), r(B, N)
    if case.special == "inside":
        pts = torch.stack([(0.15 + 0.6 * ux) * W, (0.15 + 0.6 * uy) * H], -1)
    elif case.special == "cluster":
        pts = torch.stack([7.3 + 1.4 * ux, 9.3 + 0.4 * uy], -1)
    else:
        pts = torch.stack([ux * (1.2 * W) - 0.1 * W, uy * (1.2 * H) - 0.1 * H], -1)
    fx, fy = (0.7 + 0.3 * r(B, N)) * W, (0.6 + 0.3 * r(B, N)) * W
    ox, oy = W / 2 + 2 * rn(B, N), H / 2 + 2 * rn(B, N)
    ray = torch.stack([(pts[..., 0] - ox) / fx, (pts[..., 1] - oy) / fy, torch.ones(B, N, dtype=dd)], 1)
    p = ray / ray.norm(dim=1, keepdim=True)
    D = 2.5 + r(B, N, 1)
    Bs = rn(B, N, K) / K ** 0.5 if bundle else None
    R = torch_port._rodrigues(0.004 * rn(B, 3))[0]
    T = 0.02 * rn(B, 3, 1)
    if case.special == "empty":
        T[1, 0, 0] = 60.0                                          # every projection of window 1 far outside the image
    Wc = 0.01 * rn(B, K, 1) if bundle else None
    P = 6 + K
    G, gb, gabs = rn(B, P, P), rn(B, P), 0.1 * rn(B, C)
    inp = dict(bundle=bundle)
    for k, v in dict(conv1=conv1, conv2=conv2, D=D, Bs=Bs, R=R, T=T, Wc=Wc, fx=fx, fy=fy, ox=ox, oy=oy, p=p, G=G, gb=gb, gabs=gabs).items():
        inp[k] = None if v is None else _r32(v)
    nudges = 0
    for _ in range(20):
        with torch.no_grad():
            a = assemble(inp)
        bad = (_frac_dist(a["px"]) < INT_MARGIN) | (_frac_dist(a["py"]) < INT_MARGIN)
        if not bool(bad.any()):
            break
        nudges += 1
        inp["ox"], inp["oy"] = _r32(inp["ox"] + 0.01 * bad.double()), _r32(inp["oy"] + 0.01 * bad.double())
    else:
        raise AssertionError("%s: projections stay near integer coordinates" % case.name)
    near = (a["d"].abs() < 1e-5) & (a["mask"] > 0).unsqueeze(-1)   # |d| kink (the mask no longer changes: conv1 does not enter it)
    if bool(near.any()):
        inp["conv1"] = _r32(inp["conv1"] + 1e-3 * near.double())
    inp["nudges"] = nudges
    return inp


def gradients(inp, dtype):
    """autograd through sparse_assemble in `dtype` -> dict of float64 tensors: the OUTPUTS (dbasis / dW only for bundle)"""
    keys = ("conv1", "conv2", "D", "Bs", "R", "T", "Wc")
    leaves = [None if inp[k] is None else inp[k].to(dtype).clone().requires_grad_(True) for k in keys]
    a = assemble(inp, dtype, leaves)
    loss = (a["AtA"] * inp["G"].to(dtype)).sum() + (a["Atb"] * inp["gb"].to(dtype)).sum() + (a["absd"] * inp["gabs"].to(dtype)).sum()
    live = [x for x in leaves if x is not None]
    grads = iter(torch.autograd.grad(loss, live))
    by = {k: (None if x is None else next(grads).double()) for k, x in zip(keys, leaves)}
    B = inp["conv1"].shape[0]
    out = dict(dsrc=by["conv1"], dmap3=by["conv2"], ddepth=by["D"].reshape(B, -1), dR=by["R"].reshape(B, 9), dT=by["T"].reshape(B, 3))
    if inp["bundle"]:
        out.update(dbasis=by["Bs"], dW=by["Wc"].reshape(B, -1))
    return out


def window_errors(got, want):
    """per window: the max-norm error on THAT window's max-norm scale (a wrong window cannot hide behind a larger one).  A window
    whose reference is identically zero must be matched exactly (else inf)."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    got = got.reshape(want.shape)
    out = []
    for b in range(want.shape[0]):
        s, e = float(want[b].abs().max()), float((got[b] - want[b]).abs().max())
        if not (e == e):
            e = float("inf")                                       # a NaN anywhere
        out.append((0.0 if e == 0.0 else float("inf")) if s == 0.0 else e / s)
    return out


def touched_texels(fwd, H, W):
    """[B,H,W] bool: the texels of the [f|gx|gy] map that a bilinear tap of an in-image point reads"""
    m = fwd["mask"] > 0
    B = m.shape[0]
    x0, y0 = torch.floor(fwd["px"]).long(), torch.floor(fwd["py"]).long()
    hit = torch.zeros(B, H, W, dtype=torch.bool)
    for b in range(B):
        for dy in (0, 1):
            for dx in (0, 1):
                yy, xx = (y0[b][m[b]] + dy).clamp(0, H - 1), (x0[b][m[b]] + dx).clamp(0, W - 1)
                hit[b, yy, xx] = True
    return hit


@functools.lru_cache(maxsize=None)
def reference(name):
    """For one case, computed once and shared (never modified by its users): inp (make_case), fwd (the float64 assembly: AtA, Atb,
    absd, mask, px, py, d), want (the float64 gradients), e_ref32 (per output, per window: the error of the SAME autograd in float32
    torch on the CPU against the float64 one), finite32."""
    case = BY_NAME[name]
    inp = make_case(case)
    with torch.no_grad():
        fwd = {k: v.detach() for k, v in assemble(inp).items()}
    want = gradients(inp, torch.float64)
    got32 = gradients(inp, torch.float32)
    e32 = {k: window_errors(got32[k], want[k]) for k in want}
    finite32 = all(bool(torch.isfinite(v).all()) for v in got32.values())
    return dict(case=case, inp=inp, fwd=fwd, want=want, e_ref32=e32, finite32=finite32)


def gate_of(name, output):
    """the gate of one output of one case.  The project's convention max(T, 4 e_ref32) would be the only admissible relaxation; no
    case needs it (test_adjoint_cases_cpu.py asserts e_ref32 <= T / 4 for every case, output and window), so this is T."""
    return GATE[output]


# ---- the dispatch of launch_dense_adjoint, asked of its plan ------------------------------------------------------------------
# csrc/adjoint_plan.hpp is compiled with g++ (tests/native/adjoint_plan_host.cpp, no ROCm): plan_adjoint itself says what a level
# launches, and the instantiation lists are its X-macro lists.  Built on first use, once per process.
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ADJOINT_OVERWRITE, ADJOINT_FOLD_TARGET = 1, 4                     # banet_hip.h: BANET_ADJOINT_OVERWRITE, BANET_ADJOINT_FOLD_TARGET
BUNDLE_CAMERA, BUNDLE = 2, 3                                      # banet_hip.h: BANET_BUNDLE_CAMERA, BANET_BUNDLE


def build_host_lib(out_dir):
    """compiled exactly as test_plan_cpu.build_host_lib compiles plan_host.cpp"""
    out = os.path.join(str(out_dir), "libadjoint_plan_host.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", out,
                           os.path.join(ROOT, "tests", "native", "adjoint_plan_host.cpp")])
    L = ctypes.CDLL(out)
    for fn in ("banet_test_adjoint_plan_fields", "banet_test_adjoint_instantiations", "banet_test_sstats_det_plan_fields"):
        getattr(L, fn).restype = ctypes.c_char_p
    L.banet_test_adjoint_plan_sweep.restype = ctypes.c_size_t
    L.banet_test_adjoint_plan_sweep.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
    return L


@functools.lru_cache(maxsize=None)
def host_lib():
    tmp = tempfile.mkdtemp(prefix="banet_adjoint_plan_")
    atexit.register(shutil.rmtree, tmp, True)
    return build_host_lib(tmp)


def plan_fields(L=None):
    head, *names = (L or host_lib()).banet_test_adjoint_plan_fields().decode().split()
    assert head == "desc_ints=12"
    return names


def plan_sweep(desc, L=None):
    """desc: int32 [n, 12] rows of B, N, C, K, H, W, dense, tgt_has_grad, pairs, variant, level flags, adjoint flags
    -> (int64 [n, fields] plans, [(seed, pixel, map, tile)] kernel names per row, None where nothing is launched)"""
    L = L or host_lib()
    desc = np.ascontiguousarray(desc, np.int32).reshape(-1, 12)
    out = np.zeros((len(desc), len(plan_fields(L))), np.int64)
    need = L.banet_test_adjoint_plan_sweep(desc.ctypes.data, len(desc), None, None, 0)
    buf = ctypes.create_string_buffer(need)
    L.banet_test_adjoint_plan_sweep(desc.ctypes.data, len(desc), out.ctypes.data, buf, need)
    lines = buf.value.decode().split("\n")[:len(desc)]
    names = [tuple(k or None for k in ln.split("|")) if ln else (None,) * 4 for ln in lines]
    return out, names


@functools.lru_cache(maxsize=None)
def _from_the_lists():
    """the module constants that are read from the code: the X-macro lists of adjoint_plan.hpp and three names of dev_flags.hpp"""
    by = collections.defaultdict(list)
    for ln in host_lib().banet_test_adjoint_instantiations().decode().split("\n"):
        if ln:
            kind, name = ln.split("=")
            by[kind].append(name)
    pair = lambda n: tuple(int(v) for v in re.match(r"adj_pixel_kernel<(\d+), (\d+)", n).groups())     # noqa: E731
    import test_plan_cpu                                             # the existing banet_test_dev_flags path
    tmp = tempfile.mkdtemp(prefix="banet_plan_")
    atexit.register(shutil.rmtree, tmp, True)
    flags = test_plan_cpu.dev_flags(test_plan_cpu.build_host_lib(tmp))
    return dict(SPARSE_POINT_INSTANTIATIONS=tuple(pair(n) for n in by["point"]), DENSE_PIXEL_INSTANTIATIONS=tuple(pair(n) for n in by["pixel"]),
                # (the <NK, true> twins of adj_basis6_kernel run for target frames 2.. of a multi-frame window only: not a seed CLASS)
                ALL_SEED_KERNELS=[n for n in by["seed"] if not n.endswith(", true>") and
                                  not (n.startswith("adj_basis_kernel<") and n != "adj_basis_kernel<1>")],
                ALL_MAP_KERNELS=by["map"], ALL_TILE_KERNELS=by["tile2"] + by["tile"], ALL_INSTANTIATIONS=dict(by),
                DEV_ADJ_FP32_MFMA=flags["kDevAdjFp32Mfma"], DEV_ADJ_PIXEL_PER_WAVE=flags["kDevAdjPixelPerWave"],
                DEV_ADJ_TEXEL_PER_WAVE=flags["kDevAdjTexelPerWave"])


def __getattr__(name):                                              # SPARSE_POINT_INSTANTIATIONS, ..., DEV_ADJ_*: built on first use
    if name.isupper() and name in _from_the_lists():
        return _from_the_lists()[name]
    raise AttributeError(name)


def level_row(layout, variant, C, K, lv_flags=0, N=0, B=1, adj_flags=0, HW=None):
    """one row of plan_sweep for a level of the `layout`: dense levels are N x 1 maps (or HW = (H, W)), sparse ones look at 8 x 8"""
    assert layout in ("dense", "sparse") and (variant == "bundle") == (K > 0)
    dense = layout == "dense"
    N = N or 64
    H, W = HW if HW else ((N, 1) if dense else (8, 8))
    return (B, H * W if dense else N, C, K, H, W, int(dense), int(not dense), 1, BUNDLE if K > 0 else BUNDLE_CAMERA, lv_flags, adj_flags)


def dispatch(layout, variant, C, K, overwrite=False, lv_flags=0, N=0):
    """-> (seed-GEMM kernel, per-pixel kernel, map kernel): the instantiations banet_dense_adjoint_ex_f32 launches for a level of the
    `layout` ("dense" / "sparse") without BANET_ADJOINT_FOLD_TARGET and without BANET_ADJOINT_REUSE_DEPTH_SEED (the <NK, true> twins of
    adj_basis6_kernel: target frames 2.. of a multi-frame window only).  None where nothing is launched; a refused level launches
    nothing.  N only enters through the 32-bit offset limits of adj_pixel2_kernel."""
    _, names = plan_sweep([level_row(layout, variant, C, K, lv_flags, N, adj_flags=ADJOINT_OVERWRITE if overwrite else 0)])
    return names[0][:3]


def tile_dispatch(C, shape=0, K=16, HW=(9, 11)):
    """-> the tile kernel of a dense level with BANET_ADJOINT_FOLD_TARGET | BANET_ADJOINT_TILE_SHAPE(shape)"""
    _, names = plan_sweep([level_row("dense", "bundle", C, K, adj_flags=ADJOINT_FOLD_TARGET | (shape & 15) << 4, HW=HW)])
    assert names[0][2] is None                                      # fold mode: no per-texel gather
    return names[0][3]
