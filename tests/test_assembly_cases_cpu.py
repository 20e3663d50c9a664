"""The inputs of the entry-by-entry assembly gate (assembly_cases.py) are what they claim to be, and the metric sees what the
max-norm gate of the other modules cannot -- all on the CPU:
  * every scene's float64 twin is finite with a positive diagonal, no window or frame is empty, the large motion leaves at least 5 % of
    every window's and frame's pixels outside the image, and no projection is borderline (which is what lets
    test_gpu_assembly_entrywise.py demand the twin's own mask of the kernels);
  * the float32 twin (the same statements in float32), compared with the float64 twin evaluated on ITS mask, stays below 3e-6 in
    every block: a tenth of the 3e-5 gate, so the gate needs no allowance for plain float32 arithmetic;
  * every mutation of the float64 result (a depth block, one 16 x 16 depth tile or one frame's pose x depth block off by 1e-3; a
    ragged last SYRK step or one frame of the last rows left out) exceeds 3e-5 entry-wise on every scene it applies to, while the
    max-norm error of the same mutation stays below 3e-5 -- printed side by side: the reason this gate exists;
  * the (gather, SYRK) selection every case names is what plan.hpp decides for it on 256 compute units, and the table covers every
    selection, forced sub-mode, frame count, shape and motion the GPU module is there for."""
import numpy as np
import pytest
import torch

import assembly_cases as ac

_SCENES = ac.all_scenes()
_SCENE_IDS = [c.name for c in _SCENES]


@pytest.mark.parametrize("case", _SCENES, ids=_SCENE_IDS)
def test_scene_conditions_and_the_float32_twin(case):
    tw = ac.twin(case)
    assert len(tw) == ac.B_WINDOWS
    for w, t in enumerate(tw):
        assert np.isfinite(t.A).all() and np.isfinite(t.b).all() and np.isfinite(t.absres).all(), (case.name, w)
        assert np.diag(t.A).min() > 0, (case.name, w, float(np.diag(t.A).min()))
        assert t.borderline == 0, (case.name, w, t.borderline)
        assert t.mask.shape == (case.pairs, case.N) and t.mask.sum(axis=1).min() > 0, (case.name, w)
        share = 1.0 - t.mask.mean(axis=1)
        if case.motion == "large":
            assert share.min() >= ac.MASKED_SHARE, (case.name, w, share)
    # the float32 twin on its own mask against the float64 twin on that mask
    tw32 = ac.twin(case, dtype=torch.float32)
    m32 = ac.own_mask(tw32)
    if case.layout == "sparse":
        assert np.array_equal(m32, ac.own_mask(tw))                 # (no forced mask in the sparse statement; none is needed)
        tw64 = tw
    else:
        tw64 = ac.twin(case, m32)
    worst = dict.fromkeys(ac.BLOCKS, 0.0)
    for t32, t64 in zip(tw32, tw64):
        err, arg = ac.entry_errors(t32.A, t32.b, t32.absres, t64.A, t64.b, case.pairs)
        for k in ac.BLOCKS:
            worst[k] = max(worst[k], err[k])
            assert err[k] < ac.TWIN32_GATE, (case.name, k, err[k], arg[k])
    print("\nassembly_twin32 %-44s %s  masked %.2f" % (case.name.split("-", 1)[1], ac.fmt(worst),
                                                      1.0 - float(np.mean([t.mask.mean() for t in tw]))))


@pytest.mark.parametrize("mutation", list(ac.MUTATIONS))
def test_mutations_fail_entrywise_and_pass_the_max_norm_gate(mutation):
    """per scene the mutation applies to (the worst window): the entry-wise error is above 3e-5; the max-norm error of AtA and of Atb
    is printed beside it and, on the pairings of assembly_cases.max_norm_asserted, is below 3e-5"""
    f = ac.MUTATIONS[mutation]
    rows = []
    for case in _SCENES:
        tw = ac.twin(case)
        mut = f(case, tw)
        if mut is None:
            continue
        entry, mx = 0.0, 0.0
        for (A, b), t in zip(mut, tw):
            err, _ = ac.entry_errors(A, b, t.absres, t.A, t.b, case.pairs)
            entry = max(entry, max(err.values()))
            mx = max(mx, *ac.max_norm_errors(A, b, t.A, t.b))
        scene = case.name.split("-", 1)[1]
        asserted = ac.max_norm_asserted(mutation, case)
        rows.append((scene, entry, mx, asserted))
        print("\nassembly_mutation %-38s %-32s entry-wise %.2e  max-norm %.2e%s" % (
            mutation, scene, entry, mx, "" if asserted else "  (max-norm not asserted)"))
    assert len(rows) >= 10, (mutation, len(rows))
    assert not [r for r in rows if not r[1] > ac.GATE], (mutation, [r for r in rows if not r[1] > ac.GATE])
    assert not [r for r in rows if r[3] and not r[2] < ac.GATE], (mutation, [r for r in rows if r[3] and not r[2] < ac.GATE])
    if mutation in ac.SCALING_MUTATIONS:
        assert sum(r[3] for r in rows) >= 10, mutation


def test_entry_errors_is_the_metric_of_the_f16_pipeline_module():
    """on a perturbed twin: the block maxima and their indices are those of _entry_errors of tests/test_gpu_syrk_f16_pipeline.py"""
    import test_gpu_syrk_f16_pipeline as f16
    case = next(c for c in _SCENES if c.layout == "dense" and c.pairs == 3 and c.K == 20)
    t = ac.twin(case)[0]
    rs = np.random.RandomState(3)
    A = (t.A * (1.0 + 1e-4 * rs.standard_normal(t.A.shape))).astype(np.float32)
    b = (t.b * (1.0 + 1e-4 * rs.standard_normal(t.b.shape))).astype(np.float32)
    ab = t.absres.astype(np.float32)
    err, arg = ac.entry_errors(A, b, ab, t.A, t.b, case.pairs)
    eA, eb, _ = f16._entry_errors(torch.tensor(A), torch.tensor(b), torch.tensor(ab), t.A, t.b)
    o = 6 * case.pairs
    assert err["pose_pose"] == eA[:o, :o].max() and err["depth_depth"] == eA[o:, o:].max()
    assert err["pose_depth"] == max(eA[:o, o:].max(), eA[o:, :o].max())
    assert err["atb_pose"] == eb[:o].max() and err["atb_depth"] == eb[o:].max()
    assert max(err[k] for k in ("pose_pose", "pose_depth", "depth_depth")) == eA.max() and max(err["atb_pose"], err["atb_depth"]) == eb.max()
    for k in ("pose_pose", "depth_depth"):
        assert eA[arg[k]] == err[k]
    assert eb[arg["atb_depth"]] == err["atb_depth"] and arg["atb_depth"][0] >= o


def test_the_table_names_what_plan_hpp_selects_on_256_compute_units():
    cases = ac.all_cases()
    F = ac._flags()
    for c, row in zip(cases, ac.plan_rows(cases)):
        assert row["rc"] == 0, c.name
        assert ac.selection_of_plan(row, c.K) == (c.gather, c.syrk), (c.name, ac.selection_of_plan(row, c.K))
        if c.K:
            assert (row["s.direct"], row["s.f16"]) == (c.direct, c.f16), c.name
            assert bool(row["s.f16"]) == bool(row["s.f16_standalone"])            # the single assembly pass runs the form the plan names
            assert row["s.x3"] == int(c.gate == ac.GATE_THREE_PRODUCTS)
        name = c.name.split("-")[0]
        if name == "gather_strip_rows8":
            assert row["g.strip"] == 8
        elif name == "gather_strip_rows32":
            assert row["g.strip"] == 32
        elif name.startswith("gather_strip"):
            assert row["g.strip"] == 16
        if name in ("gather_strip", "gather_strip_frameparallel", "gather_strip_directrows"):
            assert row["g.strip_fp"] == int(c.pairs > 1), c.name
        elif name.startswith("gather_strip"):
            assert row["g.strip_fp"] == 0, c.name
        if name == "gather_direct_quarter":
            assert row["g.qshift"] == 2
        if name == "gather_direct_tiles":
            assert row["g.qshift"] == 0
        if name == "gather_patch_frameloop":
            assert row["g.pairloop"] == 1
        if name == "gather_patch" and c.pairs > 1:
            assert row["g.pairloop"] == 0
        if c.layout != "dense":
            assert row["g.tile_pts"] == (64 if c.flags & F.DEV_SPARSE_ITEMS64 else 16), c.name


def test_the_table_covers_what_it_is_there_for():
    cases = ac.all_cases()
    dense = [c for c in cases if c.layout == "dense"]
    ragged = lambda c: (c.H, c.W) != (32, 48)                        # noqa: E731
    assert {(c.H, c.W) for c in dense} == set(ac.SHAPES) and {c.N for c in dense} == {483, 1961, 1536}
    # every gather flag set: every shape with either motion; one and several target frames (where the mode has both) at a ragged
    # shape under the large motion; K = 20 and K = 128
    for name, (bits, sel, frames) in ac.gather_flag_sets().items():
        mine = [c for c in dense if c.name.split("-")[0] == "gather_" + name]
        assert all(c.flags == bits and c.gather == sel for c in mine)
        if name != "strip_frameparallel":                            # (its other slots are `strip` itself)
            assert {((c.H, c.W), c.motion) for c in mine} == {(s, m) for s in ac.SHAPES for m in ac.MOTIONS}, name
            assert {c.K for c in mine} == {20, 128}, name
        hard = {c.pairs for c in mine if ragged(c) and c.motion == "large"}
        assert hard == ({3} if frames else {1, 3}), (name, hard)
    assert {c.gather for c in dense} == {0, 1, 2, 3, 4}
    # every SYRK form: all six (shape, motion) slots; every configuration with either motion
    for form, configs in ac.syrk_forms().items():
        mine = [c for c in dense if c.name.split("-")[0].startswith("syrk_" + form) and
                c.name.split("-")[0] in ("syrk_" + form, "syrk_" + form + "_nobf16x6")]
        if form != "three_products":
            assert {((c.H, c.W), c.motion) for c in mine} == {(s, m) for s in ac.SHAPES for m in ac.MOTIONS}, form
        for tag, C, K, pairs, bits, gsel in configs:
            assert {c.motion for c in mine if (c.C, c.K, c.pairs, c.flags) == (C, K, pairs, bits)} == set(ac.MOTIONS), (form, C, K, pairs)
    by = lambda d, f: {c.pairs for c in dense if (c.direct, c.f16) == (d, f) and c.K and ragged(c) and c.motion == "large"}     # noqa: E731
    for d, f in ((0, 0), (1, 0), (2, 0), (3, 0), (3, 1)):
        got = by(d, f)
        assert 1 in got and max(got) > 1, (d, f, got)
    assert by(2, 1) >= {4}                                           # (fp16 bf16x6 at 1 .. 3 frames: test_gpu_syrk_f16_pipeline.py)
    assert {c.K for c in dense if c.direct == 0 and c.K} >= {4, 5, 12, 16, 20, 33, 36, 128, 200, 256}
    sparse = [c for c in cases if c.layout == "sparse"]
    assert {(c.N, c.C, c.K) for c in sparse} == set(ac.SPARSE_NCK)
    F = ac._flags()
    for nck in ac.SPARSE_NCK:
        assert {(bool(c.flags & F.DEV_SPARSE_ITEMS64), c.motion) for c in sparse if (c.N, c.C, c.K) == nck} == \
            {(i, m) for i in (False, True) for m in ac.SPARSE_MOTIONS}
    # the sparse layout on the direct C = 128 kernel: both C = 128 shapes with a basis, both item counts of the plan, both motions
    smap = [c for c in cases if c.layout == "sparse_map"]
    assert {(c.N, c.K, bool(c.flags & F.DEV_SPARSE_ITEMS64), c.motion) for c in smap} == \
        {(N, K, i, m) for N, K in ((77, 128), (1000, 64)) for i in (False, True) for m in ac.SPARSE_MOTIONS}
    assert all(c.gather == 1 for c in smap)
    assert all(c.gate == ac.GATE for c in cases if "three_products" not in c.name)
