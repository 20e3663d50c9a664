"""banet_ba_residual_f32 on the GPU: per-pixel error maps, mask, projection and sums against the float64 statement of the oracle's
own functions (tests/residual_ref.py), at the smallest shapes at which each path of the kernel can go wrong.

Bounds (none of them comes from the code under test):
  mask   -- may differ from the float64 mask on at most as many points as the reference calls borderline (within 4e-6 max(W, H)
            pixels of the image border); the scenes and seeds here have none, so the masks are equal, and on dense levels equal to
            banet_ba_assemble_mask_f32's;
  sq, ab -- per window, max |gpu - f64| / max(f64 map) over the points in both masks <= max(1e-6, 4 x the same figure of the
            reference run in float32): two float32 evaluations in different operation order may sit on opposite sides of the
            float64 value (2 x), and the kernel contracts to FMA where numpy does not (another 2 x);
  sums   -- sum sq, sum ab against the float64 sum of the GPU's own float32 maps: relative error <= (N - 1) 2^-24 (non-negative
            terms: the bound of any summation order); the count and the maximum exactly;
  proj   -- within 4e-6 max(W, H) pixels of float64 on the points in the mask.
Measured on an MI355X (the figures each case prints): DESIGN.md section 4.10.
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT) if ROOT not in sys.path else None

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import residual_ref as rr  # noqa: E402
from oracle import banet_oracle as orc, dense as odense, synth  # noqa: E402

DEV = "cuda:0"
VARIANT_NORMALIZES = {"bundle": True, "bundle_camera": True, "legacy_lm": False, "legacy_fixed": False}


def t32(x):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32))).to(DEV)


def rot(w):
    return synth.rodrigues(np.asarray(w, np.float64))


# ---------------------------------------------------------------------------------------------------------------------
# cases: numpy inputs + the float64 / float32 references, built once
# ---------------------------------------------------------------------------------------------------------------------
def _dense_case(variant, H, W, C, K, B, scale, seed, poses, pairs=1, coef=0.5):
    """poses(b, scene) -> (R [pairs,3,3], T [pairs,3]) the state the level is evaluated at (never the identity)"""
    norm = VARIANT_NORMALIZES[variant]
    Kb = K if variant == "bundle" else 0
    if pairs == 1:
        scenes = [synth.make_pair_scene(H * scale, W * scale, C, Kb, [scale], seed + b, normalize_rays=norm) for b in range(B)]
    else:
        scenes = [synth.make_window_scene(H * scale, W * scale, C, Kb, [scale], seed + b, pairs, normalize_rays=norm) for b in range(B)]
    intr, levels = odense.batch_scene(scenes)
    lv = levels[0]
    assert (lv["H"], lv["W"]) == (H, W)
    RT = [poses(b, scenes[b]) for b in range(B)]
    R = np.stack([np.asarray(r, np.float64).reshape(pairs, 3, 3) for r, _ in RT]).astype(np.float32)
    T = np.stack([np.asarray(t, np.float64).reshape(pairs, 3, 1) for _, t in RT]).astype(np.float32)
    Wc = np.stack([np.asarray(s["W_gt"]) * coef for s in scenes]).reshape(B, Kb, 1).astype(np.float32) if Kb else None
    ref = {dt: rr.dense_residual(variant, intr, lv, R, T, Wc, dtype=dt) for dt in (np.float64, np.float32)}
    return dict(kind="dense", variant=variant, intr=intr, lv=lv, R=R, T=T, Wc=Wc, ref=ref, H=H, W=W, C=C, K=Kb, B=B, pairs=pairs,
                normalize=norm)


def _sparse_case(variant, C, K, seed, B=2, N=100, H=14, W=18):
    """the reference's own layout: N sampled points with their rays and per-point level intrinsics, conv1 rows, the 3C target map"""
    rng = np.random.RandomState(seed)
    Kb = K if variant == "bundle" else 0
    norm = VARIANT_NORMALIZES[variant]
    pts = np.stack([rng.uniform(1.0, W - 2.0, (B, N)), rng.uniform(1.0, H - 2.0, (B, N))], -1).astype(np.float32)
    fx = np.full((B, N), 0.8 * W, np.float32)
    fy = np.full((B, N), 0.8 * W, np.float32)
    ox = np.full((B, N), W / 2.0, np.float32)
    oy = np.full((B, N), H / 2.0, np.float32)
    p = orc.compute_coordinates(pts, fx, fy, ox, oy, norm).astype(np.float32)
    conv1 = rng.standard_normal((B, N, C)).astype(np.float32)
    conv2 = orc.target_map(rng.standard_normal((B, H, W, C)).astype(np.float32))[:, None]      # [B,1,H,W,3C]
    D = rng.uniform(2.0, 3.5, (B, N, 1)).astype(np.float32)
    Bs = (rng.standard_normal((B, N, Kb)) * 0.3).astype(np.float32) if Kb else None
    Wc = (rng.standard_normal((B, Kb, 1)) * 0.2).astype(np.float32) if Kb else None
    R = np.stack([rot(rng.uniform(-1, 1, 3) * 0.08) for _ in range(B)]).reshape(B, 1, 3, 3).astype(np.float32)
    T = (rng.uniform(-1, 1, (B, 1, 3, 1)) * 0.25).astype(np.float32)
    sp = dict(conv1=conv1, conv2=conv2, p=p, fx=fx, fy=fy, ox=ox, oy=oy, D=D, Bs=Bs)
    ref = {dt: rr.sparse_residual(variant, sp, R, T, Wc, dtype=dt) for dt in (np.float64, np.float32)}
    return dict(kind="sparse", variant=variant, sp=sp, R=R, T=T, Wc=Wc, ref=ref, H=H, W=W, C=C, K=Kb, B=B, N=N, pairs=1)


def _scaled_pose(s, frac):
    """a state close to the scene's ground truth (small residuals: cancellation in d = F2w - F1), not the identity"""
    Rg, Tg = np.asarray(s["R_gt"], np.float64), np.asarray(s["T_gt"], np.float64)
    if Rg.ndim == 2:
        Rg, Tg = Rg[None], Tg[None]
    Rs = []
    for r in Rg:
        w = np.array([r[2, 1] - r[1, 2], r[0, 2] - r[2, 0], r[1, 0] - r[0, 1]]) * 0.5      # small angles: the rotation vector
        Rs.append(rot(w * frac))
    return np.stack(Rs), Tg * frac


def _big_pose(b, s):
    """rotation ~0.3 rad, translation ~0.4: about half the pixels leave the image"""
    w = np.array([[0.05, 0.28, -0.09], [-0.22, -0.1, 0.18], [0.12, -0.25, -0.12]])[b % 3]
    t = np.array([[0.3, -0.2, 0.15], [-0.25, 0.3, 0.1], [0.2, 0.25, -0.22]])[b % 3]
    return rot(w)[None], t[None]


def _window_pose_one_frame_outside(b, s):
    """three frames near their ground truth; frame 1 of every window posed so that no pixel lands in the image"""
    R, T = _scaled_pose(s, 0.8)
    T = T.copy()
    T[1] = [40.0, 0.0, 0.5]
    return R, T


CASES = {
    "a": lambda: _dense_case("bundle", 33, 47, 20, 5, 2, 1, 101, lambda b, s: _scaled_pose(s, 0.9)),
    "b": lambda: _dense_case("bundle", 12, 20, 128, 8, 3, 2, 202, _big_pose),
    "c": lambda: _dense_case("bundle_camera", 5, 7, 3, 0, 2, 1, 303, lambda b, s: _scaled_pose(s, 0.6)),
    "d_lm": lambda: _dense_case("legacy_lm", 33, 47, 128, 0, 2, 1, 404, lambda b, s: _scaled_pose(s, 0.7)),
    "d_fixed": lambda: _dense_case("legacy_fixed", 33, 47, 128, 0, 2, 1, 414, lambda b, s: _scaled_pose(s, 1.3)),
    "e": lambda: _dense_case("bundle", 16, 24, 128, 128, 2, 1, 505, _window_pose_one_frame_outside, pairs=3),
    "f_c256": lambda: _dense_case("bundle", 12, 20, 256, 3, 2, 1, 606, lambda b, s: _scaled_pose(s, 0.5)),
    "f_c7": lambda: _dense_case("bundle", 12, 20, 7, 3, 2, 1, 616, lambda b, s: _scaled_pose(s, 0.5)),
    "g_bundle": lambda: _sparse_case("bundle", 128, 8, 707),
    "g_legacy": lambda: _sparse_case("legacy_lm", 16, 0, 717),
}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


def problem_of(c, lo=None, hi=None):
    """ops.LevelProblem over the case's tensors (windows lo .. hi-1 only, when given) + the state tensors"""
    from banet_amd import ops
    sl = slice(lo, hi)
    B = len(range(*sl.indices(c["B"])))
    H, W, C, K = c["H"], c["W"], c["C"], c["K"]
    if c["kind"] == "dense":
        lv = c["lv"]
        basis = t32(lv["basis"][sl]).reshape(B, H * W, K) if K else None
        prob = ops.LevelProblem(c["variant"], t32(lv["src"][sl]), t32(lv["tgt"][sl]), t32(lv["D0"][sl]).reshape(B, H * W), H, W, C,
                                basis=basis, intr=t32(c["intr"][sl]), scale=float(lv["scale"]), dense=True, tgt_has_grad=False,
                                normalize_rays=c["normalize"], pairs=c["pairs"])
    else:
        sp = c["sp"]
        prob = ops.LevelProblem(c["variant"], t32(sp["conv1"][sl]), t32(sp["conv2"][sl]), t32(sp["D"][sl]).reshape(B, -1), H, W, C,
                                basis=t32(sp["Bs"][sl]) if K else None, rays=t32(sp["p"][sl]), fx=t32(sp["fx"][sl]), fy=t32(sp["fy"][sl]),
                                ox=t32(sp["ox"][sl]), oy=t32(sp["oy"][sl]), dense=False, tgt_has_grad=True, pairs=1)
    return prob, t32(c["R"][sl]), t32(c["T"][sl]), (t32(c["Wc"][sl]) if K else None)


def n64(t):
    return t.detach().cpu().numpy().astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# a .. g: against the float64 reference
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_maps_mask_projection_and_sums_against_float64(name):
    from banet_amd import ops
    c = case(name)
    r64, r32 = c["ref"][np.float64], c["ref"][np.float32]
    prob, R, T, Wc = problem_of(c)
    got = ops.ba_residual(prob, R, T, Wc, proj=True, sums=True)
    torch.cuda.synchronize()
    B, pairs, N = got.sq.shape
    assert (B, pairs, N) == r64["sq"].shape and got.mask.dtype == torch.uint8 and tuple(got.sums.shape) == (B, pairs, 4)
    assert tuple(got.proj.shape) == (B, pairs, N, 2)
    sq, ab, mask, proj, sums = n64(got.sq), n64(got.ab), got.mask.cpu().numpy(), n64(got.proj), n64(got.sums)
    # the scene must not put a projection on the image border (a precondition on the seeds, not on the kernel)
    border = int(r64["borderline"].sum())
    print("case %s: borderline points %d, in-image share %.2f" % (name, border, r64["mask"].mean()))
    assert border == 0
    assert np.array_equal(r64["mask"], r32["mask"])               # float32 and float64 oracles agree on every point
    # mask
    assert set(np.unique(mask)) <= {0, 1}
    differ = int((mask.astype(bool) != r64["mask"]).sum())
    print("case %s: mask differs from float64 on %d points" % (name, differ))
    assert differ <= border
    if c["kind"] == "dense":
        asm_mask = ops.ba_assemble(prob, R, T, Wc, return_mask=True)[4].cpu().numpy()
        assert np.array_equal(asm_mask, mask)
    # masked points: exact zeros
    assert np.all(sq[mask == 0] == 0) and np.all(ab[mask == 0] == 0)
    # sq / ab per window on the points in both masks
    both = mask.astype(bool) & r64["mask"]
    for b in range(B):
        for key, g in (("sq", sq), ("ab", ab)):
            scale = r64[key][b].max()
            assert scale > 0
            err = np.abs(g[b] - r64[key][b])[both[b]].max() / scale
            yard = np.abs(r32[key][b].astype(np.float64) - r64[key][b])[both[b] & r32["mask"][b]].max() / scale
            print("case %s window %d %s: gpu %.3e, float32 reference %.3e" % (name, b, key, err, yard))
            assert err <= max(1e-6, 4 * yard), (name, b, key, err, yard)
    # sums
    cnt = mask.reshape(B, pairs, N).sum(-1)
    assert np.array_equal(sums[..., 2], cnt.astype(np.float64))
    for i, g in ((0, sq), (1, ab)):
        want = g.sum(-1)
        rel = np.abs(sums[..., i] - want) / np.maximum(want, 1e-300)
        rel = np.where(want == 0, np.abs(sums[..., i]), rel)
        print("case %s sums[%d]: max relative error %.3e (bound %.3e)" % (name, i, rel.max(), (N - 1) * 2.0 ** -24))
        assert np.all(rel <= (N - 1) * 2.0 ** -24)
    assert np.array_equal(sums[..., 3], sq.max(-1))
    # projection
    e = 4e-6 * max(c["W"], c["H"])
    dp = np.maximum(np.abs(proj[..., 0] - r64["px"]), np.abs(proj[..., 1] - r64["py"]))[both]
    print("case %s proj: max %.3e px (bound %.3e)" % (name, dp.max(), e))
    assert dp.max() <= e


def test_a_frame_with_no_pixel_in_the_image_gives_zero_sums():
    """case e: depth + basis . Wc computed once and reused by three frames; frame 1 is empty: sums (0, 0, 0, 0), nothing NaN"""
    from banet_amd import ops
    c = case("e")
    assert not c["ref"][np.float64]["mask"][:, 1].any() and c["ref"][np.float64]["mask"][:, 0].any()
    prob, R, T, Wc = problem_of(c)
    got = ops.ba_residual(prob, R, T, Wc)
    assert bool((got.sums[:, 1] == 0).all()) and bool(torch.isfinite(got.sums).all())
    assert bool((got.sums[:, 0, 2] > 0).all()) and bool((got.sums[:, 2, 2] > 0).all())
    assert bool((got.mask[:, 1] == 0).all()) and bool((got.sq[:, 1] == 0).all())


# ---------------------------------------------------------------------------------------------------------------------
# h: exact rim
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [128, 5])
def test_exact_rim(C):
    """Every projection is an exact integer texel: u' = u + 2, v' = v + 1 (fx = fy = 32, integer ox / oy, D = 1, R = I,
    T = (2/32, 1/32, 0), rays not normalised: every float32 operation is exact).  The mask is exactly u + 2 <= W - 1 and
    v + 1 <= H - 1 -- the last in-image column and row (dx = dy = 0, the clamped neighbour has weight 0) included -- and
    sq = sum_c (tgt[v+1, u+2] - src[v, u])^2: the differences are single float32 subtractions, their squares summed in some
    order, (C + 1) 2^-24 relative at most."""
    from banet_amd import ops
    H, W, B = 8, 12, 2
    rng = np.random.RandomState(8)
    src = rng.standard_normal((B, H, W, C)).astype(np.float32)
    tgt = rng.standard_normal((B, H, W, C)).astype(np.float32)
    intr = np.tile(np.array([32.0, 32.0, 5.0, 3.0], np.float32), (B, 1))
    prob = ops.LevelProblem("legacy_fixed", t32(src), t32(tgt), torch.ones(B, H * W, device=DEV), H, W, C, intr=t32(intr), scale=1.0,
                            dense=True, tgt_has_grad=False, normalize_rays=False)
    R = torch.eye(3, device=DEV).repeat(B, 1, 1)
    T = t32(np.tile(np.array([2.0 / 32, 1.0 / 32, 0.0]).reshape(1, 3, 1), (B, 1, 1)))
    got = ops.ba_residual(prob, R, T, proj=True)
    mask = got.mask.cpu().numpy().reshape(B, H, W)
    vv, uu = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    want_mask = (uu + 2 <= W - 1) & (vv + 1 <= H - 1)
    assert np.array_equal(mask.astype(bool), np.broadcast_to(want_mask, (B, H, W)))
    assert mask[:, H - 2, W - 3].all() and not mask[:, H - 1].any() and not mask[:, :, W - 2:].any()
    d = np.zeros((B, H, W, C), np.float32)
    d[:, :H - 1, :W - 2] = tgt[:, 1:, 2:] - src[:, :H - 1, :W - 2]                 # float32 subtraction, as the kernel's
    d64 = d.astype(np.float64) * want_mask[None, :, :, None]
    for key, want in (("sq", (d64 * d64).sum(-1)), ("ab", np.abs(d64).sum(-1))):
        g = n64(getattr(got, key)).reshape(B, H, W)
        assert np.all(g[:, ~want_mask] == 0)
        rel = np.abs(g - want)[:, want_mask] / want[:, want_mask]
        print("exact rim C = %d %s: max relative error %.3e (bound %.3e)" % (C, key, rel.max(), (C + 1) * 2.0 ** -24))
        assert rel.max() <= (C + 1) * 2.0 ** -24
    proj = got.proj.cpu().numpy().reshape(B, H, W, 2)
    assert np.array_equal(proj[:, want_mask, 0], np.broadcast_to((uu + 2)[want_mask].astype(np.float32), (B, want_mask.sum())))
    assert np.array_equal(proj[:, want_mask, 1], np.broadcast_to((vv + 1)[want_mask].astype(np.float32), (B, want_mask.sum())))
    assert np.array_equal(got.sums[..., 2].cpu().numpy().reshape(B), np.full(B, want_mask.sum(), np.float32))


# ---------------------------------------------------------------------------------------------------------------------
# the contract: every element written, same bits on a second run, alone and in a batch, with and without the optional outputs
# ---------------------------------------------------------------------------------------------------------------------
def _raw_call(prob, R, T, Wc, proj=True, sums=True):
    """banet_ba_residual_f32 into outputs pre-filled with NaN words (0xFF bytes)"""
    from banet_amd import _capi as capi
    B, N, pairs = prob.B, prob.N, prob.pairs

    def filled(shape, dtype):
        t = torch.empty(shape, dtype=dtype, device=DEV)
        t.view(torch.uint8).fill_(0xFF)
        return t
    out = dict(sq=filled((B, pairs, N), torch.float32), ab=filled((B, pairs, N), torch.float32), mask=filled((B, pairs, N), torch.uint8),
               proj=filled((B, pairs, N, 2), torch.float32) if proj else None, sums=filled((B, pairs, 4), torch.float32) if sums else None)
    assert bool(torch.isnan(out["sq"]).all())
    c = capi.ResidualOut()
    for k, v in out.items():
        setattr(c, k, None if v is None else v.data_ptr())
    capi.check(capi.lib().banet_ba_residual_f32(ctypes.byref(prob.c), capi.ptr(R), capi.ptr(T), capi.ptr(Wc), ctypes.byref(c), capi.stream()))
    torch.cuda.synchronize()
    return out


def _same_bits(x, y):
    return x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))


@pytest.mark.parametrize("name", ["b", "e"])
def test_contract_written_reproducible_batch_invariant(name):
    c = case(name)
    prob, R, T, Wc = problem_of(c)
    one = _raw_call(prob, R, T, Wc)
    for k, v in one.items():
        if k == "mask":
            assert bool((v <= 1).all()), k
        else:
            assert bool(torch.isfinite(v).all()), k               # every element written (proj too: zeros outside the mask)
    two = _raw_call(prob, R, T, Wc)
    for k in one:
        assert _same_bits(one[k], two[k]), k
    # window 1 alone: the same bits, sums included
    p1, R1, T1, W1 = problem_of(c, 1, 2)
    alone = _raw_call(p1, R1, T1, W1)
    for k in one:
        assert _same_bits(alone[k], one[k][1:2]), k
    # the optional outputs change nothing else
    bare = _raw_call(prob, R, T, Wc, proj=False, sums=False)
    for k in ("sq", "ab", "mask"):
        assert _same_bits(bare[k], one[k]), k


# ---------------------------------------------------------------------------------------------------------------------
# DenseBA.residual / cost_trace
# ---------------------------------------------------------------------------------------------------------------------
def test_dense_ba_residual_and_cost_trace():
    from banet_amd import dense as bdense
    C, K, B, H, W = 128, 8, 2, 48, 64
    scenes = [synth.make_pair_scene(H, W, C, K, [4, 2, 1], 21 + b, normalize_rays=True) for b in range(B)]
    intr, levels = odense.batch_scene(scenes)
    mlps = [orc.he_normal_mlp_weights(C, 5 + i) for i in range(3)]
    tl = [bdense.DenseLevel(lv["scale"], *(t32(lv[k]) for k in ("src", "tgt", "D0", "basis"))) for lv in levels]
    ba = bdense.DenseBA(t32(intr), tl, mlps, "bundle", 1000.0)
    T0 = t32(np.stack([np.asarray(s["T_gt"]) * 0.7 for s in scenes]).reshape(B, 3, 1))
    st0, st = ba.new_state(T=T0), ba.new_state(T=T0)
    # residual(): shapes and dtypes
    r = ba.residual(2, st0, proj=True)
    assert tuple(r.sq.shape) == tuple(r.ab.shape) == tuple(r.mask.shape) == (B, 1, H, W) and tuple(r.proj.shape) == (B, 1, H, W, 2)
    assert r.sq.dtype == r.ab.dtype == r.sums.dtype == torch.float32 and r.mask.dtype == torch.bool and tuple(r.sums.shape) == (B, 1, 4)
    assert ba.residual(0, R=st0.R, T=st0.T, Wc=st0.Wc).proj is None
    assert torch.equal(r.sums[..., 2], r.mask.reshape(B, 1, -1).sum(-1).float())
    # cost_trace rows = residual() at the snapshot states, bit for bit
    snaps = []
    ba.solve([3, 3, 3], st, snapshots=snaps)
    trace = ba.cost_trace(snaps, state0=st0)
    assert tuple(trace.shape) == (3, 2, B, 1, 4) and trace.dtype == torch.float32
    states = [(st0.R, st0.T, st0.Wc)] + [(s["R"], s["T"], s["W"]) for s in snaps]
    for l in range(3):
        for k in (0, 1):
            Rk, Tk, Wk = states[l + k]
            want = ba.residual(l, R=Rk, T=Tk, Wc=Wk).sums
            assert _same_bits(trace[l, k], want), (l, k)
    torch.cuda.synchronize()
    print("cost trace, sum sq [level, before/after, window]:", trace[..., 0, 0].cpu().numpy())
    # noise-free scene: the finest level reduces the cost
    assert bool((trace[2, 1, :, 0, 0] < trace[2, 0, :, 0, 0]).all())
