"""Every assembly path entry by entry against float64 (`-m gpu`, through the C ABI): banet_ba_assemble_mask_f32 on the cases of
assembly_cases.py -- every gather kernel and forced sub-mode (generic; direct tiles, quarter tiles; patches, with the frame loop;
strip segments of 8 / 16 / 32 rows, frame-parallel and frame-loop, direct rows; 4x4 items), every SYRK (the LDS-tiled kernel at
nb = 1, 2, 4, 8, 16, ba_syrk_direct_kernel, ba_syrk_bf16x6_kernel at four target frames exact and fp16, the syrk_wide.hip jobs exact
and fp16, the opt-in three-product form) and the sparse-point layout with both item sizes, on the generic kernel and (points on a
C-channel map, which no other test runs) on ba_gather128_kernel -- at shapes ragged in every work-item size, with one and several
target frames, under a small and a large motion.

The gate: every entry of AtA within 3e-5 of sqrt(A_ii A_jj), every entry of Atb within 3e-5 of sqrt(A_ii) |r|, per block (pose x pose,
pose x depth, depth x depth, Atb pose, Atb depth), against the float64 twin evaluated on the mask the kernel decided.  The max-norm gate
of the other modules sees the pose block only (test_assembly_cases_cpu.py shows what passes it); the float32 twin itself stays
below 3e-6 under this metric, so the gate has an order of magnitude of room over plain float32 arithmetic.

What this module measured on an MI355X is kept in profiles/assembly_entrywise.txt."""
import numpy as np
import pytest
import torch

import assembly_cases as ac

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_CASES = ac.all_cases()


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from banet_amd import _capi
    _capi.lib()


_PROBLEMS = {}


def _problem(case):
    """the level of a case's scene on the device (one upload per scene), its flag word set to the case's"""
    from banet_amd import ops
    key = (ac.scene_key(case), case.layout)
    if key not in _PROBLEMS:
        sc = ac.scene_of(case)
        d = lambda v: None if v is None else v.to(DEV)             # noqa: E731
        B, N = sc["B"], sc["N"]
        if sc["layout"] == "dense":
            tgt = sc["tgt"] if sc["pairs"] > 1 else sc["tgt"][:, 0]
            prob = ops.LevelProblem("bundle", d(sc["src"]), d(tgt.contiguous()), d(sc["depth"].reshape(B, N)), sc["H"], sc["W"], sc["C"],
                                    basis=d(sc["basis"].reshape(B, N, sc["K"])), intr=d(sc["intr"]), scale=sc["scale"], dense=True,
                                    tgt_has_grad=False, normalize_rays=True, pairs=sc["pairs"])
        else:                                                        # sparse points: on the [f|gx|gy] map, or on the C-channel map
            grad = case.layout == "sparse"
            prob = ops.LevelProblem("bundle" if sc["K"] else "bundle_camera", d(sc["conv1"]), d(sc["conv2"] if grad else sc["img"]), d(sc["D"]),
                                    sc["H"], sc["W"], sc["C"], basis=d(sc["Bs"]), rays=d(sc["p"]), fx=d(sc["fx"]), fy=d(sc["fy"]), ox=d(sc["ox"]),
                                    oy=d(sc["oy"]), dense=False, tgt_has_grad=grad)
        _PROBLEMS[key] = (prob, d(sc["R"]), d(sc["T"]), d(sc["Wc"]))
    return _PROBLEMS[key]


@pytest.mark.parametrize("case", _CASES, ids=[c.name for c in _CASES])
def test_assembly_entry_by_entry(case):
    from banet_amd import ops
    prob, R, T, Wc = _problem(case)
    B, pairs, N = ac.B_WINDOWS, case.pairs, case.N
    prob.c.flags = case.flags
    try:
        # a case that this part's CU count routes elsewhere is a failure of the table, not a skip
        assert (ops.gather_selection(prob), ops.syrk_selection(prob)) == (case.gather, case.syrk), case.name
        first = [x.cpu() for x in ops.ba_assemble(prob, R, T, Wc, return_mask=True)]
        again = [x.cpu() for x in ops.ba_assemble(prob, R, T, Wc, return_mask=True)]
    finally:
        prob.c.flags = 0
    for name, x, y in zip(("AtA", "Atb", "absres", "nvalid", "mask"), first, again):
        assert torch.equal(x, y), (case.name, name, "two calls differ")
    AtA, Atb, absres, nvalid, mask = (x.numpy() for x in first)
    assert np.array_equal(AtA, np.swapaxes(AtA, 1, 2)), (case.name, "AtA is not symmetric bit for bit")
    assert mask.shape == (B, pairs, N) and mask.max() <= 1          # every pixel written (the buffer starts at 255)
    assert np.array_equal(nvalid.astype(np.float64), mask.reshape(B, -1).sum(1).astype(np.float64)), (case.name, nvalid)
    # the twin's own mask: no projection is borderline on the CPU, so the kernels' float32 geometry must decide as float64 does
    # (dense: the twin is evaluated on the kernel's mask and still reports its own; the sparse statement has its own mask only)
    tw = ac.twin(case) if case.layout != "dense" else ac.twin(case, mask)
    differ = (ac.own_mask(tw) != mask).reshape(B, pairs, N).sum(-1)
    if case.layout != "dense":
        assert differ.max() == 0, (case.name, "mask bits differ from the float64 statement's", differ)
    else:
        assert differ.max() <= 1, (case.name, "mask bits differ from the float64 twin's", differ)     # (as tests/test_gpu_round4.py:82)
    worst = dict.fromkeys(ac.BLOCKS, 0.0)
    bad = []
    e_abs = 0.0
    for b in range(B):
        t = tw[b]
        err, arg = ac.entry_errors(AtA[b], Atb[b], absres[b], t.A, t.b, pairs)
        for k in ac.BLOCKS:
            worst[k] = max(worst[k], err[k])
            if not err[k] < case.gate:
                bad.append((b, k, err[k], arg[k]))
        e_abs = max(e_abs, float(np.abs(absres[b].astype(np.float64) - t.absres).max() / max(np.abs(t.absres).max(), 1e-30)))
    print("\nassembly_entrywise %-62s sel (%d, %5d)  %s  absres %.1e  mask differs %d" % (
        case.name, case.gather, case.syrk, ac.fmt(worst), e_abs, int(differ.sum())))
    assert not bad, (case.name, "gate %.0e" % case.gate, bad)
    assert e_abs < ac.ABSRES_GATE, (case.name, e_abs)
