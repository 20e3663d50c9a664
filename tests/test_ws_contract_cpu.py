"""The workspace-contract harness (tests/ws_contract.py) must be able to fail, and the workspace queries must be tight.  No GPU.

* With CPU tensors and small torch stand-ins for a kernel: the guard check fires on a one-byte write just before and just after
  the body and not on writes inside it; a stand-in that reads a word it never wrote gives outputs that differ between the fills
  `zero`, `nan` and `one`; a well-behaved stand-in gives equal bits.
* Host-only ABI sweep over every entry point that takes (ws, ws_bytes), at several shapes each (P on both sides of 144 and of
  ~190, K = 0 / 32 / 128 / 256, 1 / 3 / 7 target frames, both policies): the exact `*_workspace_bytes` value passes the workspace
  check (the call goes on to fail only for lack of a device), one byte less / a pointer off by 4 bytes / NULL are refused with
  BANET_ERR_WORKSPACE.  So the guard bands of the GPU module sit directly behind the last byte the plan claims.
"""
import os
import sys
import types

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
os.environ.setdefault("BANET_NUM_CUS", "256")     # host-side plans tabulated for a 256-CU part, whatever GPU the host has

import ws_contract as wsc  # noqa: E402


# ---------------------------------------------------------------------------------------------------------------------
# the harness itself
# ---------------------------------------------------------------------------------------------------------------------
def test_guarded_workspace_has_the_exact_length_alignment_and_fill():
    for nbytes in (0, 1, 255, 256, 257, 4096, 10240, 1000003):
        for fill in ("zero", "nan", "one", "stale"):
            ws, h = wsc.guarded_workspace(nbytes, "cpu", fill)
            assert ws.numel() == max(nbytes, 256) and ws.dtype == torch.uint8      # what _capi.workspace returns
            assert ws.data_ptr() % 256 == 0
            assert h.lo.numel() >= 4096 and h.hi.numel() >= 4096
            assert h.lo.data_ptr() + h.lo.numel() == ws.data_ptr()                   # the bands touch the body
            assert h.hi.data_ptr() == ws.data_ptr() + ws.numel()
            wsc.assert_guards_intact(h)
            words = ws[:ws.numel() // 4 * 4].view(torch.int32)
            if fill != "stale":
                assert bool((words == wsc.FILL_WORDS[fill]).all())
                assert int(words[0]) >= 0                                           # no fill with the sign bit set
    assert wsc.GUARD_BYTE < 0x80 and wsc.GUARD_BYTES >= 4096 and wsc.GUARD_BYTES % 256 == 0
    f = torch.tensor([wsc.FILL_WORDS["nan"], wsc.FILL_WORDS["one"]], dtype=torch.int32).view(torch.float32)
    assert bool(torch.isnan(f[0])) and float(f[1]) == 1.0
    with pytest.raises(ValueError):
        wsc.guarded_workspace(256, "cpu", "minus_one")


@pytest.mark.parametrize("nbytes", [256, 1000, 7936])
def test_guard_check_fires_on_a_one_byte_overrun_and_not_inside(nbytes):
    ws, h = wsc.guarded_workspace(nbytes, "cpu", "zero")
    ws[0] = 7
    ws[-1] = 7
    ws[nbytes // 2] = 7
    wsc.assert_guards_intact(h)                                  # writes inside the body: fine
    raw = h.block                                                # band | body | band
    # one byte just after the body
    keep = int(raw[wsc.GUARD_BYTES + ws.numel()])
    raw[wsc.GUARD_BYTES + ws.numel()] = 0
    with pytest.raises(AssertionError, match=r"after the body.*offset 0 "):
        wsc.assert_guards_intact(h)
    raw[wsc.GUARD_BYTES + ws.numel()] = keep
    wsc.assert_guards_intact(h)
    # one byte just before it
    raw[wsc.GUARD_BYTES - 1] = 0
    with pytest.raises(AssertionError, match=r"before the body.*offset -1 "):
        wsc.assert_guards_intact(h)
    raw[wsc.GUARD_BYTES - 1] = wsc.GUARD_BYTE
    # the far ends of both bands, and the first changed byte is the one reported
    raw[0] = 1
    with pytest.raises(AssertionError, match=r"offset -%d " % wsc.GUARD_BYTES):
        wsc.assert_guards_intact(h)
    raw[0] = wsc.GUARD_BYTE
    raw[-1] = 1
    raw[-100] = 1
    with pytest.raises(AssertionError, match=r"offset %d .*\(2 bytes changed" % (wsc.GUARD_BYTES - 100)):
        wsc.assert_guards_intact(h)


# torch stand-ins for an entry point: x [n] float32 -> y [n]; `capi` is the module whose workspace() they call
def _good_kernel(capi, x):
    """partial sums into the workspace, then a fixed-order fold: reads only what it wrote"""
    part = capi.workspace(4 * 8, x.device).view(torch.float32)[:8]
    for g in range(8):
        part[g] = x[g::8].sum()
    return x * part.sum()


def _reads_unwritten_word(capi, x):
    """the same, but the fold runs over one row more than was written (a `rows` off by one)"""
    ws = capi.workspace(4 * 9, x.device).view(torch.float32)
    for g in range(8):
        ws[g] = x[g::8].sum()
    return x * ws[:9].sum()


def _relies_on_a_zero_counter(capi, x):
    """a queue head that is never reset: correct on zero pages, one item short (or empty) otherwise"""
    ws = capi.workspace(256, x.device)
    head = ws.view(torch.int32)[:1]
    acc = ws.view(torch.float32)[1:2]
    acc[0] = 0.0
    while int(head[0]) < x.numel():
        acc[0] += x[int(head[0])]
        head[0] += 1
    head[0] = 0                                        # "left zeroed for the next call"
    return x * acc[0]


def _writes_past_the_end(capi, x):
    ws = capi.workspace(256, x.device)
    torch.as_strided(ws, (257,), (1,))[256] = 0        # one byte past the query
    return x.clone()


def _fake_capi():
    return types.SimpleNamespace(workspace=lambda nbytes, device: torch.zeros(max(int(nbytes), 256), dtype=torch.uint8, device=device))


def _run(kernel, fills=wsc.FILLS):
    fake = _fake_capi()
    x = torch.arange(1, 65, dtype=torch.float32) / 7
    arena = wsc.Arena(1 << 16, "cpu")

    def primer():          # another "shape": leaves its own partials and a non-zero word where the counter lives
        w = fake.workspace(512, "cpu").view(torch.float32)
        w[:] = 3.25
    outs, seen = wsc.run_under_every_fill(lambda: (kernel(fake, x),), arena, primer=primer, fills=fills, module=fake)
    assert all(len(h) == 1 for h in seen.values())
    return outs


def test_a_well_behaved_stand_in_gives_equal_bits_under_every_fill():
    outs = _run(_good_kernel)
    assert list(outs) == ["zero", "stale", "nan", "one"]
    wsc.assert_same_bits_across_fills(outs, names=["y"])


def test_a_stand_in_that_reads_an_unwritten_word_differs_between_the_fills():
    outs = _run(_reads_unwritten_word)
    y = {k: v[0] for k, v in outs.items()}
    assert bool(torch.isnan(y["nan"]).all())                                  # the NaN word shows in the output
    assert bool(torch.isfinite(y["one"]).all()) and not torch.equal(y["one"], y["zero"])      # a visibly wrong sum
    assert not torch.equal(y["stale"], y["zero"])                             # 3.25 left by the previous user
    with pytest.raises(AssertionError, match="differs between workspace fills|not finite"):
        wsc.assert_same_bits_across_fills(outs, names=["y"])
    with pytest.raises(AssertionError, match="differs between workspace fills 'one' and 'zero'"):
        wsc.assert_same_bits_across_fills({k: outs[k] for k in ("zero", "one")}, names=["y"])


def test_a_stand_in_that_relies_on_a_zeroed_counter_differs_and_its_loop_ends():
    outs = _run(_relies_on_a_zero_counter)        # (the poison words are large positive int32: `head < n` is false at once)
    assert not torch.equal(outs["nan"][0], outs["zero"][0]) and not torch.equal(outs["one"][0], outs["zero"][0])
    assert not torch.equal(outs["stale"][0], outs["zero"][0])
    with pytest.raises(AssertionError):
        wsc.assert_same_bits_across_fills(outs)


def test_a_stand_in_that_writes_one_byte_past_the_query_is_caught_by_the_patched_allocator():
    fake = _fake_capi()
    x = torch.ones(4)
    with pytest.raises(AssertionError, match=r"after the body.*offset 0 "):
        with wsc.patched_workspace("zero", module=fake):
            _writes_past_the_end(fake, x)
    assert fake.workspace.__name__ == "<lambda>"                              # restored, also after a failure
    with wsc.patched_workspace("one", module=fake) as handles:
        _good_kernel(fake, x.repeat(16))
    assert len(handles) == 1 and handles[0].fill == "one"


def test_the_patch_reaches_every_python_side_workspace_of_the_package():
    """ops.py, dense.py, dense_train.py and prep_grad.py all allocate through `<_capi module>.workspace(...)`, looked up at call
    time: replacing that one attribute puts the whole stack under the contract (no `from ._capi import workspace` anywhere)."""
    import re
    pkg = os.path.join(ROOT, "banet_amd")
    calls = 0
    for name in sorted(os.listdir(pkg)):
        if not name.endswith(".py"):
            continue
        txt = open(os.path.join(pkg, name)).read()
        assert not re.search(r"from\s+\S*_capi\s+import[^\n]*\bworkspace\b", txt), name
        if name != "_capi.py":
            for m in re.finditer(r"(\S*)\bworkspace\(", txt):
                if m.group(1).endswith("def "):
                    continue
                assert m.group(1).endswith("capi."), (name, m.group(0))
                calls += 1
    assert calls >= 11
    sys.path.insert(0, ROOT) if ROOT not in sys.path else None
    from banet_amd import _capi, ops, dense, dense_train, prep_grad
    for mod in (ops, dense_train, prep_grad):
        assert mod.capi is _capi
    assert dense.ops.capi is _capi
    keep = _capi.workspace
    with wsc.patched_workspace("nan") as handles:
        assert ops.capi.workspace is not keep
        ws = dense.ops.capi.workspace(1000, "cpu")
        assert ws.numel() == 1000 and len(handles) == 1
    assert _capi.workspace is keep


# ---------------------------------------------------------------------------------------------------------------------
# host-only ABI: the queries are tight
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sweep():
    sys.path.insert(0, ROOT) if ROOT not in sys.path else None
    from banet_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return wsc.abi_sweep_in_child()


ENTRY_POINTS = ("equation_construction", "equation_construction_grad", "ba_assemble", "ba_assemble_mask", "ba_solve_update_ws",
                "lm_level", "lm_level_ex", "resample_grad", "depth_output_grad", "sample_stats_grad_det", "dense_adjoint",
                "dense_adjoint_ex", "small_step_adjoint")


def test_the_sweep_covers_every_entry_point_that_takes_a_workspace(sweep):
    """every function of the header with a `ws_bytes` parameter is in the sweep, at three shapes or more"""
    import re
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "banet_hip.h")).read(), flags=re.S)
    declared = sorted(m.group(1)[len("banet_"):-len("_f32")] for m in re.finditer(r"\b(banet_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", src)
                      if "ws_bytes" in m.group(2))
    assert declared == sorted(ENTRY_POINTS)
    count = {e: sum(1 for r in sweep if r["name"].split()[0] == e) for e in ENTRY_POINTS}
    assert all(c >= 3 for c in count.values()), count
    assert all(r["bytes"] > 0 and r["bytes"] % 256 == 0 for r in sweep), [r["name"] for r in sweep if not r["bytes"]]
    names = " ".join(r["name"] for r in sweep)
    for what in ("P143", "P144", "P145", "P200", "P304", " K0 ", " K32 ", " K128 ", " K256 ", "pairs1 ", "pairs3 ", "pairs7 ", "policy0",
                 "policy1", "K176 ", "K188 ", "flags1000000", "legacy_lm"):
        assert what in names, what


def test_the_exact_query_passes_the_workspace_check(sweep):
    """... and the call then fails for lack of a device only (BANET_ERR_LAUNCH): never BANET_ERR_WORKSPACE, never a refusal of
    the arguments or the shape"""
    bad = [(r["name"], r["exact"]) for r in sweep if r["exact"] != wsc.ERR_LAUNCH]
    assert not bad, bad


def test_one_byte_less_a_misaligned_pointer_and_null_are_workspace_errors(sweep):
    bad = [(r["name"], k, r[k]) for r in sweep if r["kind"] == "required" for k in ("minus1", "off4", "null") if r[k] != wsc.ERR_WORKSPACE]
    assert not bad, bad


def test_lm_level_query_is_the_smallest_accepted_value(sweep):
    """banet_lm_level_ex_f32 compares against carve_level(...).total: banet_lm_level_workspace_bytes is exactly that -- accepted,
    one byte less refused -- and never smaller than the assembly's own workspace, which is its first region"""
    lm = [r for r in sweep if r["name"].split()[0] in ("lm_level", "lm_level_ex")]
    assert len(lm) >= 20
    for r in lm:
        assert r["exact"] == wsc.ERR_LAUNCH and r["minus1"] == wsc.ERR_WORKSPACE, r
    by_tag = {r["name"].split(" ", 1)[1]: r["bytes"] for r in sweep if r["name"].startswith("ba_assemble ")}
    for r in lm:
        tag = r["name"].split(" ", 1)[1]
        if tag in by_tag:
            assert r["bytes"] > by_tag[tag]


def test_the_equation_construction_gradient_treats_its_workspace_as_optional(sweep):
    """banet_equation_construction_grad_f32 (documented in the header): with a workspace of at least the queried size, 256-byte
    aligned, the matrix-pipe kernels; with anything less -- too small, misaligned, NULL -- the first-generation kernel, which
    needs none.  It never answers BANET_ERR_WORKSPACE: every probe gets past the check and fails for lack of a device."""
    eg = [r for r in sweep if r["kind"] == "optional"]
    assert len(eg) >= 7 and all(r["name"].startswith("equation_construction_grad ") for r in eg)
    for r in eg:
        assert [r[k] for k in ("exact", "minus1", "off4", "null")] == [wsc.ERR_LAUNCH] * 4, r
