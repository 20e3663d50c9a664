"""banet_ba_residual_grad_f32 on the GPU: every output against float64 autograd of the torch restatement of the forward
(tests/residual_grad_ref.py), on the forward test's own cases (tests/test_gpu_residual.py: the smallest shapes at which each path
of the kernel can go wrong), plus the contract: exact zeros, reproducibility, batch invariance, overwrite / accumulate, output
subsets, the workspace, graph capture, the existing assembly adjoint, autograd.

Bound (not from the code under test): for every output, per window, max |gpu - f64| / max |f64| <= max(1e-6, 4 x the same figure
of the reference run in float32) -- the forward test's rule: two float32 evaluations in different operation order may sit on
opposite sides of the float64 value (2 x), and the kernel contracts to FMA where torch does not (another 2 x).  Where the float64
output of a window is identically zero (dsrc with gproj alone) the GPU's must be too.

The derivative is discontinuous where a coordinate of the projection crosses an integer or a channel's d changes sign; float32 and
float64 may disagree there.  So all three upstream gradients are zeroed on the borderline points (residual_grad_ref.borderline), in
the GPU run and in both reference runs; the zeroed share is asserted to stay below 2 % of a case's in-image points, a case being a
row of the issue's table: (d) is its two legacy variants and (f) its two channel counts together (C = 256 alone has 2.6 % of its 418
in-image points with one of 256 channels that close to zero; (f) as a whole 1.5 %), (g) its two sparse levels.

Measured on an MI355X (the figures each case prints): DESIGN.md section 4.11.
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import residual_grad_ref as rg  # noqa: E402
import residual_ref as rr  # noqa: E402
import test_gpu_residual as fwd  # noqa: E402  (the forward's cases, built once and shared)
import ws_contract as wsc  # noqa: E402

DEV = fwd.DEV
OUTPUTS = rg.OUTPUTS
MODES = {"all": ("gsq", "gab", "gproj"), "gsq": ("gsq",), "gab": ("gab",), "gproj": ("gproj",)}
t32, n64 = fwd.t32, fwd.n64


def bits_equal(x, y):
    return x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


@functools.lru_cache(maxsize=None)
def setup(name):
    """the case's reference inputs in float64 and float32, its borderline points and its random upstream gradients"""
    c = fwd.case(name)
    ins = {}
    for dt in (np.float64, np.float32):
        if c["kind"] == "dense":
            ins[dt] = rr.dense_inputs(c["variant"], c["intr"], c["lv"], dt, c["normalize"])
        else:
            ins[dt] = rr.sparse_inputs(c["sp"], dt)
    a, conv2s = ins[np.float64]
    near = {}
    for with_gab in (True, False):
        near[with_gab], mask = rg.borderline(a, conv2s, c["R"], c["T"], c["Wc"], with_gab)
    B, pairs, N = mask.shape
    rng = np.random.RandomState(len(name) * 131 + ord(name[0]))
    g = dict(gsq=rng.uniform(0.5, 1.5, (B, pairs, N)).astype(np.float32), gab=rng.uniform(0.5, 1.5, (B, pairs, N)).astype(np.float32),
             gproj=rng.standard_normal((B, pairs, N, 2)).astype(np.float32))
    return dict(c=c, ins=ins, near=near, mask=mask, g=g, want=tuple(o for o in OUTPUTS if not (c["kind"] == "sparse" and o == "dtgt")))


def upstream(name, mode):
    """the mode's upstream gradients (numpy float32, None = NULL), zeroed on the borderline points; the zeroed share of the
    in-image points"""
    s = setup(name)
    near = s["near"]["gab" in MODES[mode]]
    keep = (~near).astype(np.float32)
    out = {k: None for k in ("gsq", "gab", "gproj")}
    for k in MODES[mode]:
        out[k] = s["g"][k] * (keep[..., None] if k == "gproj" else keep)
    return out, float(near.sum()) / max(int(s["mask"].sum()), 1)


@functools.lru_cache(maxsize=None)
def reference(name, mode):
    s = setup(name)
    c = s["c"]
    g, _ = upstream(name, mode)
    return {dt: rg.gradients(*s["ins"][dt], c["R"], c["T"], c["Wc"], g["gsq"], g["gab"], g["gproj"],
                             dtype=torch.float64 if dt is np.float64 else torch.float32) for dt in (np.float64, np.float32)}


def run_gpu(name, mode="all", lo=None, hi=None, want=None, **kw):
    from banet_amd import ops
    s = setup(name)
    prob, R, T, Wc = fwd.problem_of(s["c"], lo, hi)
    g, _ = upstream(name, mode)
    gt = {k: (None if v is None else t32(v[slice(lo, hi)])) for k, v in g.items()}
    return ops.ba_residual_grad(prob, R, T, Wc, gt["gsq"], gt["gab"], gt["gproj"], want=s["want"] if want is None else want, **kw), prob


def zeroed_share(letter, mode):
    """the borderline share of the in-image points of a case of the table (all its levels together)"""
    names = [n for n in sorted(fwd.CASES) if n.split("_")[0] == letter]
    near = sum(int(setup(n)["near"]["gab" in MODES[mode]].sum()) for n in names)
    return near / max(sum(int(setup(n)["mask"].sum()) for n in names), 1)


def figure(got, want, b):
    """max |got - want| / max |want| of window b (inf if the window's reference is zero and the result is not)"""
    scale = np.abs(want[b]).max()
    err = np.abs(got[b] - want[b]).max()
    return (0.0 if err == 0 else np.inf) if scale == 0 else err / scale


# ---------------------------------------------------------------------------------------------------------------------
# a .. g: every output against float64, all three inputs together and each alone
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(fwd.CASES))
def test_every_output_against_float64(name):
    """Measured on an MI355X: every comparison is within the bound, most far below the float32 reference's own figure (the kernel
    evaluates the derivative in double at the forward's float32 mask and floor).  A first build whose chain was float32 missed three of
    about 500 comparisons by 4.3 - 5.1 x the reference's figure (dR / dT of cases c and g_legacy): DESIGN.md section 4.11."""
    s = setup(name)
    B = s["c"]["B"]
    misses = []                                  # every figure is printed; the misses are asserted together at the end
    for mode in MODES:
        _, own = upstream(name, mode)
        share = zeroed_share(name.split("_")[0], mode)
        print("case %s %s: zeroed share of the in-image points %.4f (this level alone %.4f)" % (name.split("_")[0], mode, share, own))
        assert share <= 0.02
        ref = reference(name, mode)
        got, _ = run_gpu(name, mode)
        torch.cuda.synchronize()
        for o in OUTPUTS:
            t = getattr(got, o)
            if o not in s["want"] or ref[np.float64][o] is None:
                assert t is None, o
                continue
            g, r64, r32 = n64(t).reshape(ref[np.float64][o].shape), ref[np.float64][o], ref[np.float32][o]
            assert np.isfinite(g).all(), o
            for b in range(B):
                err, yard = figure(g, r64, b), figure(r32, r64, b)
                print("case %s %s window %d %s: gpu %.3e, float32 reference %.3e" % (name, mode, b, o, err, yard))
                if not err <= max(1e-6, 4 * yard):
                    misses.append((name, mode, b, o, "gpu %.3e" % err, "float32 reference %.3e" % yard, "bound %.3e" % max(1e-6, 4 * yard)))
    assert not misses, misses


def test_dtgt_is_refused_on_the_3c_map():
    from banet_amd import _capi as capi, ops
    for name in ("g_bundle", "g_legacy"):
        prob, R, T, Wc = fwd.problem_of(fwd.case(name))
        assert capi.lib().banet_ba_residual_grad_workspace_bytes(ctypes.byref(prob.c), 1) == 0
        g = torch.ones(prob.B, 1, prob.N, device=DEV)
        with pytest.raises(capi.BanetError):
            ops.ba_residual_grad(prob, R, T, Wc, gab=g, want=("dtgt",))
        # the raw code
        gin, gout = capi.ResidualGradIn(), capi.ResidualGradOut()
        gin.gab, gout.dtgt = g.data_ptr(), g.data_ptr()
        ws = capi.workspace(1 << 20, DEV)
        rc = capi.lib().banet_ba_residual_grad_f32(ctypes.byref(prob.c), capi.ptr(R), capi.ptr(T), capi.ptr(Wc), ctypes.byref(gin),
                                                   ctypes.byref(gout), 3, ctypes.c_void_p(ws.data_ptr()), ws.numel(), capi.stream())
        assert rc == -3


# ---------------------------------------------------------------------------------------------------------------------
# exact zeros
# ---------------------------------------------------------------------------------------------------------------------
def test_masked_points_and_an_empty_frame_contribute_exact_zeros():
    # case b: half the pixels outside (one frame): their dsrc rows, ddepth and dbasis rows are exactly zero although their upstream
    # gradients are not
    s = setup("b")
    got, _ = run_gpu("b", "all")
    outside = torch.from_numpy(~s["mask"][:, 0]).to(DEV)
    assert bool(outside.any()) and bool((~outside).any())
    assert bool((got.dsrc[outside] == 0).all()) and bool((got.ddepth[outside] == 0).all()) and bool((got.dbasis[outside] == 0).all())
    live = torch.from_numpy(s["mask"][:, 0] & ~s["near"][True][:, 0]).to(DEV)          # in the image and not zeroed as borderline
    assert bool((got.dsrc[live].abs().sum(-1) > 0).all())
    # case e: frame 1 sees nothing -> dR = dT = 0 for it, nothing NaN; with upstream gradients on that frame alone, everything is zero
    s = setup("e")
    assert not s["mask"][:, 1].any() and s["mask"][:, 0].any()
    got, prob = run_gpu("e", "all")
    assert bool((got.dR[:, 1] == 0).all()) and bool((got.dT[:, 1] == 0).all())
    assert bool((got.dR[:, 0] != 0).any()) and bool((got.dR[:, 2] != 0).any()) and bool((got.dtgt[:, 1] == 0).all())
    for t in got:
        assert bool(torch.isfinite(t).all())
    from banet_amd import ops
    _, R, T, Wc = fwd.problem_of(s["c"])
    only = {k: torch.zeros_like(t32(v)) for k, v in s["g"].items()}
    for k, v in s["g"].items():
        only[k][:, 1] = t32(v)[:, 1]
    alone = ops.ba_residual_grad(prob, R, T, Wc, only["gsq"], only["gab"], only["gproj"])
    for o, t in zip(OUTPUTS, alone):
        assert bool((t == 0).all()), o


# ---------------------------------------------------------------------------------------------------------------------
# reproducibility, batch invariance, overwrite / accumulate, subsets
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["b", "e"])
def test_same_bits_run_to_run_and_in_any_batch(name):
    one, _ = run_gpu(name)
    two, _ = run_gpu(name)
    for o, x, y in zip(OUTPUTS, one, two):
        assert bits_equal(x, y), o
    B = setup(name)["c"]["B"]
    w = B - 2 if B > 2 else 1                                     # a window that is neither first nor (case b) last
    alone, _ = run_gpu(name, lo=w, hi=w + 1)
    for o, x, y in zip(OUTPUTS, alone, one):
        assert bits_equal(x, y[w:w + 1]), (o, "alone")
    if B > 2:                                                     # case b: windows 1..2 as a batch of two, against the batch of three
        two_of, _ = run_gpu(name, lo=1, hi=3)
        for o, x, y in zip(OUTPUTS, two_of, one):
            assert bits_equal(x, y[1:3]), (o, "batch of two")


@pytest.mark.parametrize("name", ["a", "e"])
def test_overwrite_equals_accumulate_into_zeros_and_accumulate_adds(name):
    from banet_amd import ops
    s = setup(name)
    ow, prob = run_gpu(name)
    shapes = ops._residual_grad_shapes(prob)
    acc_names = ("dsrc", "dtgt", "ddepth", "dbasis")
    zeros = {o: torch.zeros(shapes[o], device=DEV) for o in acc_names}
    acc0, _ = run_gpu(name, overwrite=False, into=zeros)
    for o, x, y in zip(OUTPUTS, ow, acc0):
        assert bits_equal(x, y), o
    rng = np.random.RandomState(4)
    buf = {o: t32(rng.standard_normal(shapes[o])) for o in acc_names}
    acc, _ = run_gpu(name, overwrite=False, into={o: v.clone() for o, v in buf.items()})
    for o in ("dsrc", "ddepth", "dbasis"):                        # buffer + result to one rounding (the kernel may fuse the last product into the addition)
        x, y = getattr(acc, o), buf[o] + getattr(ow, o)
        assert bool(((x - y).abs() <= 2.0 ** -23 * (buf[o].abs() + getattr(ow, o).abs())).all()), o
    # dtgt: the texel's sum starts from the buffer instead of +0, so its partial sums round differently: each of the k partial sums
    # within 2^-24 of its value, which |buffer| + sum |terms| bounds.  A texel collects from at most four cells, one tap of each of a
    # cell's points: k <= 4 x the largest number of in-image points in one cell; a term is a weight <= 1 times
    # |e| <= 2 gsq |d| + gab <= 3 sqrt(max sq) + 1.5
    _, R, T, Wc = fwd.problem_of(s["c"])
    fw = ops.ba_residual(prob, R, T, Wc, proj=True, sums=False)
    inside = fw.mask.reshape(-1) > 0
    cells = fw.proj.floor().long().reshape(-1, 2)[inside]
    frame = torch.arange(fw.mask.numel(), device=DEV)[inside] // prob.N
    k = 4 * int(torch.bincount((frame * int(prob.c.H) + cells[:, 1]) * int(prob.c.W) + cells[:, 0]).max())
    emax = 3.0 * float(fw.sq.max()) ** 0.5 + 1.5
    bound = (k + 1) * 2.0 ** -24 * (float(buf["dtgt"].abs().max()) + k * emax)
    print("case %s: at most %d terms per texel, bound %.3e, measured %.3e" % (name, k, bound, float((acc.dtgt - (buf["dtgt"] + ow.dtgt)).abs().max())))
    assert float((acc.dtgt - (buf["dtgt"] + ow.dtgt)).abs().max()) <= bound
    for o in ("dWc", "dR", "dT"):                                 # written, never accumulated
        assert bits_equal(getattr(acc, o), getattr(ow, o)), o


@pytest.mark.parametrize("name", ["a", "e", "g_bundle"])
def test_any_subset_of_the_outputs_has_the_same_bits(name):
    s = setup(name)
    full, _ = run_gpu(name)
    subsets = [(o,) for o in s["want"]] + [("dR", "dT"), ("dsrc", "dWc"), tuple(o for o in s["want"] if o != "dtgt"), ("ddepth", "dbasis", "dT")]
    for sub in subsets:
        sub = tuple(o for o in sub if o in s["want"])
        part, _ = run_gpu(name, want=sub)
        for o in OUTPUTS:
            if o in sub:
                assert bits_equal(getattr(part, o), getattr(full, o)), (sub, o)
            else:
                assert getattr(part, o) is None, (sub, o)


# ---------------------------------------------------------------------------------------------------------------------
# workspace contract, graph capture
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "e", "g_bundle"])
def test_workspace_contract(name):
    """the exact queried size between guard bands, pre-filled with zeros, another call's leftovers, NaN words, 1.0 words: the same bits,
    the bands untouched"""
    from banet_amd import _capi as capi
    s = setup(name)
    prob, _, _, _ = fwd.problem_of(s["c"])
    need = capi.lib().banet_ba_residual_grad_workspace_bytes(ctypes.byref(prob.c), int("dtgt" in s["want"]))
    assert need > 0
    arena = wsc.Arena(4 * need + (8 << 20), DEV)
    outs, seen = wsc.run_under_every_fill(lambda: [t for t in run_gpu(name)[0] if t is not None], arena,
                                          primer=lambda: run_gpu("b" if name != "b" else "a"))
    for fill, handles in seen.items():
        assert [h.n for h in handles] == [need], fill          # one workspace per call, of exactly the queried size
    wsc.assert_same_bits_across_fills(outs, names=list(s["want"]))            # (these cases have a basis: every wanted output exists)


def test_graph_capture_of_one_call():
    from banet_amd import _capi as capi, ops
    s = setup("e")
    prob, R, T, Wc = fwd.problem_of(s["c"])
    g, _ = upstream("e", "all")
    gt = {k: t32(v) for k, v in g.items()}
    eager = ops.ba_residual_grad(prob, R, T, Wc, **gt)
    shapes = ops._residual_grad_shapes(prob)
    into = {o: torch.full(shapes[o], float("nan"), device=DEV) for o in OUTPUTS}
    ws = capi.workspace(capi.lib().banet_ba_residual_grad_workspace_bytes(ctypes.byref(prob.c), 1), DEV)
    ws.fill_(0xFF)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.ba_residual_grad(prob, R, T, Wc, into=into, ws=ws, **gt)
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    for o, t in zip(OUTPUTS, eager):
        assert bits_equal(into[o], t), o


# ---------------------------------------------------------------------------------------------------------------------
# against the assembly adjoint: a uniform L1 gradient through banet_dense_adjoint_ex_f32
# ---------------------------------------------------------------------------------------------------------------------
def test_uniform_l1_gradient_agrees_with_the_dense_adjoint():
    """dense two-frame bundle level, 16x24, C = K = 128, gab = 1: the same loss sum |d| as gAtA = gAtb = 0, gabs = 1 through the
    assembly adjoint (FOLD_TARGET: the target map's own gradient).  Tolerance per output and window: the sum of the two routes' bounds
    against float64, 2 max(1e-6, 4 x the float32 reference's figure).  No point is dropped: the two routes are compared on the same
    float32 state, and the float64 reference enters only through the tolerance."""
    from banet_amd import dense_train, ops
    c = fwd._dense_case("bundle", 16, 24, 128, 128, 2, 1, 808, lambda b, s: fwd._scaled_pose(s, 0.8))
    prob, R, T, Wc = fwd.problem_of(c)
    B, N, C, K, H, W = c["B"], 16 * 24, 128, 128, 16, 24
    got = ops.ba_residual_grad(prob, R, T, Wc, gab=torch.ones(B, 1, N, device=DEV))
    P = 6 + K
    bufs = dict(dsrc=torch.empty(B, N, C, device=DEV), dmap=torch.empty(B, H, W, C, device=DEV), ddepth=torch.empty(B, N, device=DEV),
                dbasis=torch.empty(B, N, K, device=DEV))
    dpose, _ = dense_train.dense_adjoint(prob, R, T, Wc, torch.zeros(B, P, P, device=DEV), torch.zeros(B, P, device=DEV),
                                         torch.ones(B, C, device=DEV), bufs["dsrc"], bufs["dmap"], bufs["ddepth"], bufs["dbasis"],
                                         overwrite=True, fold=True)
    torch.cuda.synchronize()
    other = dict(dsrc=bufs["dsrc"], dtgt=bufs["dmap"].reshape(B, 1, H, W, C), ddepth=bufs["ddepth"], dbasis=bufs["dbasis"],
                 dR=dpose[:, :9].reshape(B, 1, 9), dT=dpose[:, 9:12].reshape(B, 1, 3), dWc=dpose[:, 12:])
    gab = np.ones((B, 1, N), np.float32)
    ref = {}
    for dt in (np.float64, np.float32):
        a, conv2s = rr.dense_inputs("bundle", c["intr"], c["lv"], dt, True)
        ref[dt] = rg.gradients(a, conv2s, c["R"], c["T"], c["Wc"], None, gab, None, dtype=torch.float64 if dt is np.float64 else torch.float32)
    for o in OUTPUTS:
        x, y = n64(getattr(got, o)).reshape(ref[np.float64][o].shape), n64(other[o]).reshape(ref[np.float64][o].shape)
        for b in range(B):
            scale = np.abs(ref[np.float64][o][b]).max()
            yard = figure(ref[np.float32][o], ref[np.float64][o], b)
            diff = np.abs(x[b] - y[b]).max() / scale
            print("uniform L1, window %d %s: the two routes differ by %.3e (tolerance %.3e)" % (b, o, diff, 2 * max(1e-6, 4 * yard)))
            assert diff <= 2 * max(1e-6, 4 * yard), (o, b, diff, yard)


# ---------------------------------------------------------------------------------------------------------------------
# autograd: DenseBA.residual(differentiable=True) under reprojection_loss(reduce="min")
# ---------------------------------------------------------------------------------------------------------------------
def test_autograd_through_the_min_reprojection_loss():
    """case e as a one-level DenseBA: .grad of src, tgt, depth, basis, R, T, Wc of sum_b reprojection_loss(kind, reduce="min")
    against float64 autograd of the same loss on the torch reference, same bound.  The loss decides the upstream gradients itself;
    to zero them on the borderline points as everywhere else, the maps pass through `x.detach() + (x - x.detach()) keep` (the same
    values, the gradient times keep) on both sides -- on the GPU side by wrapping ba.residual for the backward runs; the loss VALUE is
    checked on the unwrapped call.  The per-pixel argmin over the frames must be the same in the float64 and float32 reference runs
    (a precondition on the scene: a tie would be another discontinuity)."""
    from banet_amd import dense as bdense, dense_train, ops
    from oracle import banet_oracle as orc
    s = setup("e")
    c = s["c"]
    lv, B, H, W, C, K, pairs = c["lv"], c["B"], c["H"], c["W"], c["C"], c["K"], c["pairs"]
    leaves = dict(src=t32(lv["src"]), tgt=t32(lv["tgt"]), depth=t32(lv["D0"]), basis=t32(lv["basis"]), R=t32(c["R"]), T=t32(c["T"]),
                  Wc=t32(c["Wc"]))
    for v in leaves.values():
        v.requires_grad_(True)
    ba = bdense.DenseBA(t32(c["intr"]), [bdense.DenseLevel(lv["scale"], leaves["src"], leaves["tgt"], leaves["depth"], leaves["basis"])],
                        [orc.he_normal_mlp_weights(C, 5)], "bundle", 1000.0)
    plain_residual = ba.residual

    def gate(x, keep):
        return x.detach() + (x - x.detach()) * keep

    for kind in ("ab", "sq"):
        keep_np = (~s["near"][kind == "ab"]).astype(np.float32)
        keep = t32(keep_np).reshape(B, pairs, H, W)
        plain = dense_train.reprojection_loss(ba, 0, leaves["R"], leaves["T"], leaves["Wc"], kind=kind, reduce="min")
        assert tuple(plain.shape) == (B,) and bool((plain > 0).all()) and plain.requires_grad

        def gated_residual(*args, **kw):
            r = plain_residual(*args, **kw)
            return ops.Residual(gate(r.sq, keep), gate(r.ab, keep), r.mask, r.proj, r.sums)
        ba.residual = gated_residual
        for v in leaves.values():
            v.grad = None
        loss = dense_train.reprojection_loss(ba, 0, leaves["R"], leaves["T"], leaves["Wc"], kind=kind, reduce="min")
        ba.residual = plain_residual
        assert bits_equal(loss.detach(), plain.detach())
        total = loss.sum()
        total.backward(retain_graph=True)
        first = {k: v.grad.clone() for k, v in leaves.items()}
        for v in leaves.values():
            v.grad = None
        total.backward()                                          # the retained graph again: the same bits
        for k, v in leaves.items():
            assert bits_equal(v.grad, first[k]), (kind, k)
        ref, choice = {}, {}
        for dt, tdt in ((np.float64, torch.float64), (np.float32, torch.float32)):
            t = rg.inputs_of(*s["ins"][dt], c["R"], c["T"], c["Wc"], tdt)
            names = dict(src="conv1", tgt="tgt", depth="D", basis="Bs", R="R", T="T", Wc="Wc")
            wrt = [t[n].requires_grad_(True) for n in names.values()]
            f = rg.forward(t)
            v, m = gate(f[kind], torch.from_numpy(keep_np).to(tdt)), f["mask"]
            best, arg = torch.where(m, v, torch.full_like(v, float("inf"))).min(1)
            seen = m.any(1)
            L = (torch.where(seen, best, torch.zeros_like(best)).sum(1) / seen.sum(1).clamp(min=1)).sum()
            ref[dt] = dict(zip(names, [g.detach().numpy().astype(np.float64) for g in torch.autograd.grad(L, wrt)]))
            choice[dt] = (np.where(seen.numpy(), arg.numpy(), -1), None, float(L))
        assert np.array_equal(choice[np.float64][0], choice[np.float32][0])
        print("min loss %s: gpu %.9g, float64 %.9g" % (kind, float(total), choice[np.float64][2]))
        assert abs(float(total) - choice[np.float64][2]) <= 1e-5 * choice[np.float64][2]
        for k in leaves:
            g = n64(first[k]).reshape(ref[np.float64][k].shape)
            for b in range(B):
                err, yard = figure(g, ref[np.float64][k], b), figure(ref[np.float32][k], ref[np.float64][k], b)
                print("min loss %s window %d d%s: gpu %.3e, float32 reference %.3e" % (kind, b, k, err, yard))
                assert err <= max(1e-6, 4 * yard), (kind, k, b, err, yard)
    # reduce="mean" runs and is the masked mean
    r = ba.residual(0, R=leaves["R"], T=leaves["T"], Wc=leaves["Wc"], differentiable=True)
    mean = dense_train.reprojection_loss(ba, 0, leaves["R"], leaves["T"], leaves["Wc"], kind="ab", reduce="mean")
    want = (r.ab * r.mask).sum((1, 2, 3)) / r.mask.sum((1, 2, 3))
    assert torch.allclose(mean, want, rtol=1e-6) and mean.requires_grad and r.sums is None


def test_many_frames_keep_their_pose_slots_in_the_workspace():
    """more target frames than the kernel's LDS slots hold (32): the slots live in the workspace; against float64 as above"""
    from banet_amd import ops
    from oracle import dense as odense, synth
    H, W, C, K, B, pairs = 8, 12, 7, 3, 2, 34
    scenes = [synth.make_window_scene(H, W, C, K, [1], 901 + b, pairs, normalize_rays=True) for b in range(B)]
    intr, levels = odense.batch_scene(scenes)
    lv = levels[0]
    RT = [fwd._scaled_pose(sc, 0.7) for sc in scenes]
    R = np.stack([r for r, _ in RT]).reshape(B, pairs, 3, 3).astype(np.float32)
    T = np.stack([t for _, t in RT]).reshape(B, pairs, 3, 1).astype(np.float32)
    Wc = np.stack([np.asarray(sc["W_gt"]) * 0.5 for sc in scenes]).reshape(B, K, 1).astype(np.float32)
    prob = ops.LevelProblem("bundle", t32(lv["src"]), t32(lv["tgt"]), t32(lv["D0"]).reshape(B, H * W), H, W, C,
                            basis=t32(lv["basis"]).reshape(B, H * W, K), intr=t32(intr), scale=1.0, dense=True, tgt_has_grad=False,
                            normalize_rays=True, pairs=pairs)
    a, conv2s = rr.dense_inputs("bundle", intr, lv, np.float64, True)
    near, mask = rg.borderline(a, conv2s, R, T, Wc, False)
    assert mask.any() and near.sum() <= 0.02 * mask.sum()
    gsq = (np.random.RandomState(2).uniform(0.5, 1.5, mask.shape) * ~near).astype(np.float32)
    got = ops.ba_residual_grad(prob, t32(R), t32(T), t32(Wc), gsq=t32(gsq), want=("dR", "dT", "dWc"))
    ref = {dt: rg.gradients(*rr.dense_inputs("bundle", intr, lv, dt, True), R, T, Wc, gsq, None, None,
                            dtype=torch.float64 if dt is np.float64 else torch.float32) for dt in (np.float64, np.float32)}
    for o in ("dR", "dT", "dWc"):
        g = n64(getattr(got, o)).reshape(ref[np.float64][o].shape)
        for b in range(B):
            err, yard = figure(g, ref[np.float64][o], b), figure(ref[np.float32][o], ref[np.float64][o], b)
            print("34 frames window %d %s: gpu %.3e, float32 reference %.3e" % (b, o, err, yard))
            assert err <= max(1e-6, 4 * yard), (o, b, err, yard)
