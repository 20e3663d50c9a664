"""The assembly adjoint on the reference's SPARSE layout at kernel level (`-m gpu`, through the C ABI): banet_dense_adjoint_ex_f32
on a level with dense = 0, tgt_has_grad = 1 -- adj_pixel_kernel<CJ, KJ, SP = true>, per-point rays and intrinsics, the [f|gx|gy] map
sampled with four clamped taps, dmap3 as the gradient of that 3C map -- entry by entry against autograd through the float64
statement oracle/torch_port.sparse_assemble, at the dense layout's own gates (2e-4 per-pixel outputs, 5e-4 dpose), every tensor
on each WINDOW's own max-norm scale.  Cases, references and the float32 yardstick: adjoint_cases.py (its conditions are asserted
on the CPU in test_adjoint_cases_cpu.py).  The per-point intrinsics differ from point to point, from window to window, and
fx != fy.  No gate is relaxed for any case (adjoint_cases.gate_of)."""
import functools

import pytest
import torch

import adjoint_cases as ac

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_IDS = [c.name for c in ac.CASES]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from banet_amd import _capi
    _capi.lib()


def t(x):
    return x.to(torch.float32).contiguous().to(DEV)


def _problem(name):
    """ops.LevelProblem of a case, built as dense_train._SparseIteration.forward builds it; plus (R, T, Wc) on the device"""
    from banet_amd import ops
    ref = ac.reference(name)
    case, inp = ref["case"], ref["inp"]
    prob = ops.LevelProblem(case.variant, t(inp["conv1"]), t(inp["conv2"]), t(inp["D"]), case.H, case.W, case.C,
                            basis=None if case.K == 0 else t(inp["Bs"]), rays=t(inp["p"]), fx=t(inp["fx"]), fy=t(inp["fy"]),
                            ox=t(inp["ox"]), oy=t(inp["oy"]), dense=False, tgt_has_grad=True)
    Wc = t(inp["Wc"]) if case.K else torch.zeros(case.B, 0, 1, device=DEV)
    return prob, t(inp["R"]), t(inp["T"]), Wc


def _buffers(case, fill):
    B, N, C, K, H, W = case.B, case.N, case.C, case.K, case.H, case.W
    shapes = dict(dsrc=(B, N, C), dmap3=(B, H, W, 3 * C), ddepth=(B, N), dbasis=(B, N, K))
    return {k: fill(s) for k, s in shapes.items()}


def _adjoint(name, overwrite, bufs):
    """one banet_dense_adjoint_ex_f32 call on `bufs` (in place) -> dict of float32 CPU tensors: the buffers and dpose"""
    from banet_amd import dense_train
    inp = ac.reference(name)["inp"]
    prob, R, T, Wc = _problem(name)
    dpose, _ = dense_train.dense_adjoint(prob, R, T, Wc, t(inp["G"]), t(inp["gb"]), t(inp["gabs"]), bufs["dsrc"], bufs["dmap3"],
                                         bufs["ddepth"], bufs["dbasis"], None, overwrite=overwrite)
    torch.cuda.synchronize()
    out = {k: v.cpu() for k, v in bufs.items()}
    out["dpose"] = dpose.cpu()
    return out


def _run_overwrite_uncached(name):
    case = ac.BY_NAME[name]
    return _adjoint(name, True, _buffers(case, lambda s: torch.full(s, float("nan"), device=DEV)))


@functools.lru_cache(maxsize=None)
def _run_overwrite(name):
    """overwrite mode on NaN-filled buffers, once per case (shared by the tests below, never modified)"""
    return _run_overwrite_uncached(name)


def _split(got, case):
    """the kernel's outputs under the names of adjoint_cases.OUTPUTS"""
    out = dict(dsrc=got["dsrc"], dmap3=got["dmap3"], ddepth=got["ddepth"], dR=got["dpose"][:, 0:9], dT=got["dpose"][:, 9:12])
    if case.K:
        out.update(dbasis=got["dbasis"], dW=got["dpose"][:, 12:])
    return out


@pytest.mark.parametrize("name", _IDS)
def test_sparse_adjoint_matches_the_float64_statement(name):
    ref = ac.reference(name)
    case, want = ref["case"], ref["want"]
    got = _split(_run_overwrite(name), case)
    assert set(got) == set(want)
    assert got["dR"].shape[0] == case.B and _run_overwrite(name)["dpose"].shape == (case.B, 12 + case.K)
    bad = []
    for k in ac.OUTPUTS:
        if k not in want:
            continue
        errs, gate = ac.window_errors(got[k], want[k]), ac.gate_of(name, k)
        print("GATE %-20s %-7s err %.2e gate %.0e ratio %.3f e_ref32 %.1e" % (name, k, max(errs), gate, max(errs) / gate,
                                                                            max(ref["e_ref32"][k])))
        if not max(errs) < gate:
            bad.append((k, errs))
    assert not bad, (name, bad)


@pytest.mark.parametrize("name", _IDS)
def test_masked_points_and_untouched_texels_are_exact_zeros(name):
    """overwrite mode on NaN-filled buffers: no NaN is left; the rows of dsrc / dbasis and the entries of ddepth of points outside the
    image, every texel of dmap3 that no in-image point's taps touch, and the dpose row of an empty window are exactly 0.0"""
    ref = ac.reference(name)
    case, fwd = ref["case"], ref["fwd"]
    got = _run_overwrite(name)
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), k
    outside = ~(fwd["mask"] > 0)
    assert float(got["dsrc"][outside].abs().sum()) == 0.0 and float(got["ddepth"][outside].abs().sum()) == 0.0
    assert float(got["dbasis"][outside].abs().sum()) == 0.0
    inside_rows = got["dsrc"][~outside]
    assert inside_rows.numel() == 0 or bool((inside_rows.abs().amax(-1) > 0).all())          # ... and only those
    untouched = ~ac.touched_texels(fwd, case.H, case.W)
    assert float(got["dmap3"][untouched].abs().sum()) == 0.0
    assert case.special != "cluster" or int(untouched.sum()) == case.B * (case.H * case.W - 6)
    for b in range(case.B):
        if not bool((fwd["mask"][b] > 0).any()):
            assert float(got["dpose"][b].abs().max()) == 0.0 and float(got["dmap3"][b].abs().max()) == 0.0
    if case.special == "empty":
        assert not bool((fwd["mask"][1] > 0).any())


@pytest.mark.parametrize("name", ac.ACCUMULATION_CASES)
def test_accumulating_call_adds_the_reference_to_what_the_buffers_hold(name):
    """overwrite = False on buffers pre-filled with random values (of the reference's own size, window by window): the result is
    initial + reference within the gate on the reference's scale, equals initial + the overwrite-mode result to 2e-5 of that scale,
    and the rows of points outside the image keep their bits."""
    ref = ac.reference(name)
    case, want, fwd = ref["case"], ref["want"], ref["fwd"]
    ow = _run_overwrite(name)
    g = torch.Generator().manual_seed(7)
    keys = ("dsrc", "dmap3", "ddepth") + (("dbasis",) if case.K else ())
    init = {}
    for k in keys:
        scale = want[k].reshape(case.B, -1).abs().amax(1).reshape([case.B] + [1] * (want[k].dim() - 1))
        init[k] = (torch.randn(want[k].shape, generator=g, dtype=torch.float64) * scale).float()
    init["dbasis"] = init.get("dbasis", torch.zeros(case.B, case.N, 0))
    got = _adjoint(name, False, {k: v.clone().to(DEV) for k, v in init.items()})
    assert torch.equal(got["dpose"], ow["dpose"])                 # dpose is an output of its own in both modes
    bad = []
    for k in keys:
        i64 = init[k].double()
        e_ref = ac.window_errors(got[k].double() - i64, want[k])
        e_ow = ac.window_errors(got[k].double() - i64, ow[k].double())
        print("ACCUMULATE %-18s %-7s vs reference %.2e (gate %.0e)  vs overwrite %.2e (2e-5)" % (name, k, max(e_ref), ac.GATE[k], max(e_ow)))
        if not (max(e_ref) < ac.GATE[k] and max(e_ow) <= 2e-5):
            bad.append((k, e_ref, e_ow))
    assert not bad, bad
    outside = ~(fwd["mask"] > 0)
    for k in ("dsrc", "ddepth") + (("dbasis",) if case.K else ()):
        assert torch.equal(got[k][outside], init[k][outside]), k
    untouched = ~ac.touched_texels(fwd, case.H, case.W)
    assert torch.equal(got["dmap3"][untouched], init["dmap3"][untouched])


def test_two_calls_give_equal_bits():
    a, b = _run_overwrite(ac.REPRODUCIBILITY_CASE), _run_overwrite_uncached(ac.REPRODUCIBILITY_CASE)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("name", [c.name for c in ac.CASES if c.N <= 500])
def test_forward_assembly_with_per_point_intrinsics_matches_the_float64_statement(name):
    """banet_ba_assemble_f32 on the same problems: AtA / Atb / sum |d| at the gate of test_random_shape_sweep_assembly_matches_oracle
    (5e-5 of the tensor's max), here per window; the in-image count equals the reference mask's exactly; AtA is symmetric bit for bit.
    Three cases have an odd C or K above 128, for which the forward has no kernel (the adjoint has): there the refusal is asserted."""
    from banet_amd import _capi as capi, dense_train, ops
    ref = ac.reference(name)
    case, fwd = ref["case"], ref["fwd"]
    prob, R, T, Wc = _problem(name)
    conv1, conv2, basis = prob.keep[0], prob.keep[1], prob.keep[3]
    # what the fused training node is told about the shape is what the forward does with it
    assert dense_train.sparse_iteration_supported(conv1, conv2, basis, prob.keep[2], R, T) == (name not in ac.FORWARD_NOT_COMPILED)
    if name in ac.FORWARD_NOT_COMPILED:                          # no kernel (adjoint_cases.FORWARD_NOT_COMPILED): refused, loudly
        with pytest.raises(capi.BanetError, match="not supported"):
            ops.ba_assemble(prob, R, T, Wc if case.K else None)
        return
    AtA, Atb, absres, nvalid = ops.ba_assemble(prob, R, T, Wc if case.K else None)
    torch.cuda.synchronize()
    AtA, Atb, absres, nvalid = AtA.cpu(), Atb.cpu(), absres.cpu(), nvalid.cpu()
    assert torch.equal(nvalid.double(), (fwd["mask"] > 0).sum(1).double())
    assert torch.equal(AtA, AtA.transpose(1, 2))
    bad = []
    for k, g, w in (("AtA", AtA, fwd["AtA"]), ("Atb", Atb, fwd["Atb"]), ("absres", absres, fwd["absd"])):
        errs = ac.window_errors(g, w)
        print("FORWARD %-20s %-6s err %.2e gate %.0e" % (name, k, max(errs), ac.FORWARD_GATE))
        if not max(errs) <= ac.FORWARD_GATE:
            bad.append((k, errs))
    assert not bad, (name, bad)
