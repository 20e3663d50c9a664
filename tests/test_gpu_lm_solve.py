"""banet_lm_solve_f32 on the GPU (`-m gpu`; include/banet_hip.h (5c)): the whole coarse -> fine schedule in one call.

The definition is the test: state and trace must be BIT-equal to the sequence of banet_lm_level_ex_f32 calls (one per level, same
workspace, same stream) with a clone of the state after every level, and the per-level depth to banet_depth_output_f32 called after
that level.  Five schedules, the smallest shapes that reach each region of the workspace and each state layout:

  S1  dense bundle, B 3, C 128, K 32, 8x12 -> 16x24 -> 32x48, iters [2,3,2]   C = 128 gathers (queue heads), small levels in a large workspace
  S2  dense bundle, 3 target frames, B 2, C 128, K 64, 8x8 -> 16x16, [2,2]     multi-frame state layout in the trace
  S3  dense bundle, K 256 (P 262), B 2, C 128, 16x16 -> 24x32, [1,2]           the solve's matrix in the workspace (bigA)
  S4  dense bundle_camera, C 64, B 4, 12x10 -> 24x20, [2,2]                    generic gather, ragged sizes, no Wc
  S5  sparse legacy_lm, [f|gx|gy] targets, C 70, N 777, B 2, three levels,     LmCtl, per-window iteration counts, a window that
      max_iters 5, early termination, non-default params                        stops early
"""
import ctypes

import pytest
import torch

import ws_contract as wsc
from banet_amd import _capi as capi

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
STATE = ("R", "T", "Wc", "iters", "ratio", "lambda_out", "delta")
ERR_WORKSPACE, ERR_UNSUPPORTED = -2, -3


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    capi.lib()
    yield
    _CASES.clear()
    _REF.clear()
    _ARENA.clear()


# ======================================================================================================================
# the schedules
# ======================================================================================================================
class Case:
    def __init__(self, name, variant, levels, mlps, iters, l2, early, params, R0, T0, W0, pairs):
        self.name, self.variant, self.levels, self.mlps, self.iters = name, variant, levels, mlps, iters
        self.l2, self.early, self.params, self.R0, self.T0, self.W0, self.pairs = l2, early, params, R0, T0, W0, pairs
        self.B, self.K, self.P = levels[0].B, levels[0].K, levels[0].P
        self.n = len(levels)

    def state(self):
        from banet_amd import ops
        return ops.LmState(self.R0, self.T0, self.W0, P=self.P, pairs=self.pairs)

    def trace(self, depth=True, fill=None):
        """every row recorded; per-level depth outputs for the bundle variant"""
        from banet_amd import ops
        d = None
        if depth and self.variant == "bundle":
            d = [torch.empty(lv.B, lv.N, device=DEV) for lv in self.levels]
        tr = ops.SolveTrace(self.n, self.state(), depth=d)
        if fill is not None:
            for t in trace_tensors(tr):
                t.fill_(fill if t.dtype.is_floating_point else -7)
        return tr

    def workspace_bytes(self):
        from banet_amd import ops
        return ops.lm_solve_workspace_bytes(self.levels)


def trace_tensors(tr):
    return [getattr(tr, n) for n in STATE if getattr(tr, n) is not None] + (tr.depth or [])


def state_tensors(st):
    return [getattr(st, n) for n in STATE if getattr(st, n) is not None]


def lambda_weights(C, seed):
    from banet_amd.bundlenet import he_normal_lambda_weights
    return he_normal_lambda_weights(C, seed)


def _dense_case(name, variant, shapes, B, C, K, pairs, iters, seed):
    """levels of the given (H, W) sizes.  A true pyramid (every size the finest one divided by a power of two) comes from one
    synthetic scene; otherwise (S3) every level is a scene of its own with its own intrinsics -- the C entry takes any prepared
    levels that share B / K / pairs / variant."""
    from banet_amd import ops, synth
    Hf, Wf = shapes[-1]
    scales = [Hf // h for h, _ in shapes]
    pyramid = all(h * s == Hf and w * s == Wf for (h, w), s in zip(shapes, scales))
    built = []
    if pyramid:
        intr, lvs, gt = synth.make_dense_windows(B, Hf, Wf, C, K, scales, seed, torch.device(DEV), trans_mag=0.06, pairs=pairs)
        built = [(intr, lv) for lv in lvs]
    else:
        for i, (h, w) in enumerate(shapes):
            intr, lvs, g = synth.make_dense_windows(B, h, w, C, K, [1], seed + i, torch.device(DEV), trans_mag=0.06, pairs=pairs)
            # a random basis: the synthetic DCT basis has (numerically) zero columns once K exceeds what a 16-pixel-wide map resolves
            rg = torch.Generator().manual_seed(seed + 10 + i)
            lvs[0].basis = (torch.randn(B, h, w, K, generator=rg) / K ** 0.5).to(DEV)
            built.append((intr, lvs[0]))
            gt = g if i == 0 else gt
    levels = []
    for intr, lv in built:
        basis = lv.basis.reshape(B, lv.H * lv.W, -1) if variant == "bundle" else None
        levels.append(ops.LevelProblem(variant, lv.src, lv.tgt, lv.depth.reshape(B, lv.H * lv.W), lv.H, lv.W, C, basis=basis, intr=intr,
                                       scale=lv.scale, dense=True, tgt_has_grad=False, normalize_rays=True, pairs=pairs))
    mlps = [ops.MlpWeights(lambda_weights(C, 100 + i), DEV) for i in range(len(shapes))]
    shape = (B, pairs) if pairs > 1 else (B,)
    R0 = torch.eye(3, device=DEV).repeat(B * pairs, 1, 1).reshape(*shape, 3, 3)
    T0 = (gt["T"] * 0.7).reshape(*shape, 3, 1).to(DEV)
    W0 = torch.zeros(B, K, 1, device=DEV) if K else None
    return Case(name, variant, levels, mlps, iters, 1000.0 if variant == "bundle" else 1.0, False, None, R0, T0, W0, pairs)


def _sparse_legacy_case(name, B=2, C=70, N=777, H=48, W=64, seed=77):
    """legacy/ba.py:106-145 trackTF's preparation on a synthetic scene: N sampled points with their z-depth, per level the source
    features resampled at the points (clamped taps), the target's [f|gx|gy] map and the level's per-point intrinsics.  Window 0
    starts at the ground truth (its updates are below the thresholds at once), window 1 away from it."""
    from banet_amd import ops, synth
    scales = [4, 2, 1]
    intr, lvs, gt = synth.make_dense_windows(B, H, W, C, 0, scales, seed, torch.device(DEV), normalize_rays=False, trans_mag=0.06)
    g = torch.Generator().manual_seed(seed)
    pts = torch.stack([torch.rand(B, N, generator=g) * (W - 9) + 4, torch.rand(B, N, generator=g) * (H - 9) + 4], dim=-1).to(DEV)
    fx, fy, ox, oy = (intr[:, i:i + 1].repeat(1, N).contiguous() for i in range(4))
    p = torch.stack([(pts[..., 0] - ox) / fx, (pts[..., 1] - oy) / fy, torch.ones(B, N, device=DEV)], dim=1).contiguous()
    D = synth._depth0(pts[..., 0], pts[..., 1], W, H).contiguous()
    levels = []
    for s, lv in zip(scales, lvs):
        conv1 = ops.resample(lv.src, pts / s, clamp=True)
        conv2 = ops.target_map(lv.tgt)
        levels.append(ops.LevelProblem("legacy_lm", conv1, conv2, D, lv.H, lv.W, C, rays=p, fx=fx / s, fy=fy / s, ox=ox / s, oy=oy / s,
                                       dense=False, tgt_has_grad=True))
    mlps = [ops.MlpWeights(lambda_weights(C, 200 + i), DEV) for i in range(3)]
    R0 = torch.eye(3).repeat(B, 1, 1)
    R0[0] = gt["R"][0]
    T0 = (gt["T"] * 0.7).reshape(B, 3, 1).clone()
    T0[0] = gt["T"][0].reshape(3, 1)
    params = ops.lm_params(angle_change=2e-4, translation_change=2e-3, residual_ratio=1.01, qr=False)
    return Case(name, "legacy_lm", levels, mlps, [5, 5, 5], 1.0, True, params, R0.to(DEV), T0.to(DEV), None, 1)


_CASES, _REF, _ARENA = {}, {}, []
NAMES = ("S1", "S2", "S3", "S4", "S5")


def case(name):
    if name not in _CASES:
        if name == "S1":
            c = _dense_case(name, "bundle", [(8, 12), (16, 24), (32, 48)], 3, 128, 32, 1, [2, 3, 2], 301)
        elif name == "S2":
            c = _dense_case(name, "bundle", [(8, 8), (16, 16)], 2, 128, 64, 3, [2, 2], 302)
        elif name == "S3":
            c = _dense_case(name, "bundle", [(16, 16), (24, 32)], 2, 128, 256, 1, [1, 2], 303)
        elif name == "S4":
            c = _dense_case(name, "bundle_camera", [(12, 10), (24, 20)], 4, 64, 0, 1, [2, 2], 304)
        else:
            c = _sparse_legacy_case(name)
        _CASES[name] = c
    return _CASES[name]


# ======================================================================================================================
# the two ways to run a schedule, straight over ctypes
# ======================================================================================================================
def run_per_level(c, ws):
    """the definition: one banet_lm_level_ex_f32 call per level in `ws`, clones of the state after each level, the level's depth
    output through banet_depth_output_f32 -> (final state tensors, per-field rows [n_levels, ...], depth list)"""
    L = capi.lib()
    st = c.state()
    rows = {n: [] for n in STATE}
    depth = []
    for lv, mlp, its in zip(c.levels, c.mlps, c.iters):
        capi.check(L.banet_lm_level_ex_f32(ctypes.byref(lv.c), ctypes.byref(mlp.c), float(c.l2), int(its), int(c.early),
                                           ctypes.byref(c.params) if c.params is not None else None, ctypes.byref(st.c),
                                           ctypes.c_void_p(ws.data_ptr()), ws.numel(), capi.stream()))
        for n in STATE:
            t = getattr(st, n)
            if t is not None:
                rows[n].append(t.clone())
        if c.variant == "bundle":
            out = torch.empty(lv.B, lv.N, device=DEV)
            capi.check(L.banet_depth_output_f32(ctypes.c_void_p(lv.c.depth), ctypes.c_void_p(lv.c.basis), capi.ptr(st.Wc), capi.ptr(out),
                                                lv.B, lv.N, lv.K, capi.stream()))
            depth.append(out)
    torch.cuda.synchronize()
    return state_tensors(st), [torch.stack(rows[n]) for n in STATE if rows[n]] + depth


def make_schedule(c, ws_ptr, ws_bytes, trace, extra_levels=()):
    """banet_schedule_t over the case's levels (+ extra banet_level_t structs appended) -> (struct, keep-alive tuple)"""
    structs = [lv.c for lv in c.levels] + list(extra_levels)
    n = len(structs)
    lv = (capi.Level * n)(*structs)
    mp = (ctypes.POINTER(capi.Mlp) * n)()
    for i in range(n):
        mp[i] = ctypes.pointer(c.mlps[min(i, c.n - 1)].c)
    it = (ctypes.c_int32 * n)(*(list(c.iters) + [1] * len(extra_levels)))
    s = capi.Schedule()
    s.levels, s.n_levels = ctypes.cast(lv, ctypes.POINTER(capi.Level)), n
    s.mlps = ctypes.cast(mp, ctypes.POINTER(ctypes.POINTER(capi.Mlp)))
    s.max_iters = ctypes.cast(it, ctypes.POINTER(ctypes.c_int32))
    s.l2_base, s.early_termination = float(c.l2), int(c.early)
    if c.params is not None:
        s.params = ctypes.pointer(c.params)
    s.workspace, s.workspace_bytes = ws_ptr, ws_bytes
    if trace is not None:
        s.trace = ctypes.pointer(trace.c)
    return s, (lv, mp, it)


def solve(c, ws, st, trace, nbytes=None, extra_levels=()):
    """banet_lm_solve_f32 on the current stream -> return code"""
    s, keep = make_schedule(c, ws.data_ptr(), ws.numel() if nbytes is None else nbytes, trace, extra_levels)
    rc = capi.lib().banet_lm_solve_f32(ctypes.byref(s), ctypes.byref(st.c), capi.stream())
    del keep
    return rc


def reference(name):
    """the per-level sequence in a fresh zero-filled workspace, computed once per schedule and left unchanged"""
    if name not in _REF:
        c = case(name)
        nb = c.workspace_bytes()
        assert nb > 0
        state, trace = run_per_level(c, capi.workspace(nb, DEV))
        for t in state + trace:
            if t.dtype.is_floating_point:
                assert bool(torch.isfinite(t).all()), "%s: the per-level reference is not finite" % name
        _REF[name] = ([t.cpu() for t in state], [t.cpu() for t in trace])
    return _REF[name]


def assert_bits(got, want, what):
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        a = a.detach().cpu()
        assert a.shape == b.shape and a.dtype == b.dtype, (what, i, a.shape, b.shape)
        ai = a.contiguous().view(torch.int32) if a.dtype == torch.float32 else a
        bi = b.contiguous().view(torch.int32) if b.dtype == torch.float32 else b
        if not torch.equal(ai, bi):
            diff = (ai != bi).reshape(-1)
            k = int(diff.nonzero()[0])
            raise AssertionError("%s: tensor %d differs in %d of %d entries, first at flat index %d (%r vs %r)"
                                 % (what, i, int(diff.sum()), diff.numel(), k, a.reshape(-1)[k].item(), b.reshape(-1)[k].item()))


# ======================================================================================================================
# (a) bit equality with the per-level calls
# ======================================================================================================================
@pytest.mark.parametrize("name", NAMES)
def test_one_call_equals_the_per_level_calls_bit_for_bit(name):
    c = case(name)
    ref_state, ref_trace = reference(name)
    st, tr = c.state(), c.trace(fill=float("nan"))
    nb = c.workspace_bytes()
    per = [capi.lib().banet_lm_level_workspace_bytes(ctypes.byref(lv.c)) for lv in c.levels]
    assert nb == max(per)
    assert solve(c, capi.workspace(nb, DEV), st, tr) == 0
    torch.cuda.synchronize()
    assert_bits(state_tensors(st), ref_state, name + " state")
    assert_bits(trace_tensors(tr), ref_trace, name + " trace")
    # the last row of the trace is the final state; counts are what the fixed-count loop / the device-side loop control left
    assert_bits([getattr(tr, n)[-1] for n in STATE if getattr(tr, n) is not None], ref_state, name + " last row")
    counts = tr.iters.cpu()
    print("%s iteration counts per level: %s" % (name, counts.tolist()))
    if c.early:
        assert int(counts.min()) >= 0 and all(int(counts[l].max()) <= m for l, m in enumerate(c.iters))
        assert bool((counts < torch.tensor(c.iters).reshape(-1, 1)).any()), "no window of S5 stopped early: %s" % counts.tolist()
    else:
        assert counts.tolist() == [[m] * c.B for m in c.iters]
    if name == "S2":                                           # multi-frame layout: [n_levels, B, pairs, 3, 3]
        assert tuple(tr.R.shape) == (2, 2, 3, 3, 3) and tuple(tr.delta.shape) == (2, 2, 6 * 3 + 64)
    if name == "S4":
        assert tr.Wc is None and tr.depth is None


def test_python_entry_equals_the_per_level_calls():
    """ops.lm_solve (what DenseBA.solve calls) on S3, recording only the iteration counts and no depth"""
    from banet_amd import ops
    c = case("S3")
    ref_state, ref_trace = reference("S3")
    st = c.state()
    tr = ops.SolveTrace(c.n, st, fields=("iters",))
    ws = ops.lm_solve(c.levels, c.mlps, c.l2, c.iters, c.early, st, params=c.params, trace=tr)
    torch.cuda.synchronize()
    assert ws.numel() == c.workspace_bytes()
    assert_bits(state_tensors(st), ref_state, "S3 state through ops.lm_solve")
    assert tr.R is None and tr.delta is None and tr.iters.tolist() == [[1, 1], [2, 2]]
    st2 = c.state()
    ops.lm_solve(c.levels, c.mlps, c.l2, c.iters, c.early, st2, ws=ws, params=c.params)      # no trace at all
    torch.cuda.synchronize()
    assert_bits(state_tensors(st2), ref_state, "S3 state, no trace")


# ======================================================================================================================
# (b) the scratch contract: arbitrary workspace contents, guard bands, one byte too few
# ======================================================================================================================
def arena():
    """one buffer for the module, large enough for the largest schedule's workspace between its guard bands"""
    if not _ARENA:
        need = max(case(n).workspace_bytes() for n in NAMES)
        _ARENA.append(wsc.Arena(need + 4 * wsc.GUARD_BYTES + 4096, DEV))
    return _ARENA[0]


@pytest.mark.parametrize("name", ["S1", "S3", "S5"])
def test_workspace_contents_are_arbitrary_and_its_bounds_hold(name):
    c = case(name)
    ref_state, ref_trace = reference(name)
    nb = c.workspace_bytes()
    other = case("S4" if name != "S5" else "S2")              # whose leftovers the `stale` run starts on
    ar = arena()
    for fill in wsc.FILLS:
        ar.reset()
        if fill == "stale":
            ows = ar.take((other.workspace_bytes() + 2 * wsc.GUARD_BYTES + 255) // 256 * 256)
            assert solve(other, ows[:other.workspace_bytes()], other.state(), None) == 0
            torch.cuda.synchronize()
            ar.reset()
        ws, h = wsc.guarded_workspace(nb, DEV, fill, ar)
        assert ws.numel() == nb
        st, tr = c.state(), c.trace(fill=0.0)
        assert solve(c, ws, st, tr) == 0
        wsc.assert_guards_intact(h)                           # (synchronises)
        assert_bits(state_tensors(st), ref_state, "%s state, workspace fill %r" % (name, fill))
        assert_bits(trace_tensors(tr), ref_trace, "%s trace, workspace fill %r" % (name, fill))
    # one byte less than the query: refused, nothing enqueued -- state and trace keep their bits
    ar.reset()
    ws, h = wsc.guarded_workspace(nb, DEV, "nan", ar)
    st, tr = c.state(), c.trace(fill=float("nan"))
    before = [t.clone() for t in state_tensors(st) + trace_tensors(tr)] + [ws.clone()]
    assert solve(c, ws, st, tr, nbytes=nb - 1) == ERR_WORKSPACE
    wsc.assert_guards_intact(h)
    assert_bits(state_tensors(st) + trace_tensors(tr) + [ws], [t.cpu() for t in before], name + " after a refused call")


# ======================================================================================================================
# (c) all or nothing
# ======================================================================================================================
def test_a_bad_last_level_leaves_state_and_trace_untouched():
    """S1 with a fourth level of C = 300 (outside the compiled kernel set): BANET_ERR_UNSUPPORTED, and the three good levels in
    front of it have not run"""
    from banet_amd import ops
    c = case("S1")
    bad = capi.Level.from_buffer_copy(c.levels[-1].c)
    bad.C = 300
    assert capi.lib().banet_lm_level_workspace_bytes(ctypes.byref(bad)) == 0
    ws = capi.workspace(c.workspace_bytes(), DEV)
    st = c.state()
    tr = ops.SolveTrace(4, st, depth=[torch.empty(lv.B, lv.N, device=DEV) for lv in c.levels] + [torch.empty(3, 32 * 48, device=DEV)])
    for t in trace_tensors(tr):
        t.fill_(float("nan") if t.dtype.is_floating_point else -7)
    before = [t.clone() for t in state_tensors(st) + trace_tensors(tr)]
    assert solve(c, ws, st, tr, extra_levels=[bad]) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert_bits(state_tensors(st) + trace_tensors(tr), [t.cpu() for t in before], "S1 + unsupported level")
    assert_bits(state_tensors(st), [t.cpu() for t in state_tensors(c.state())], "S1 initial state")
    # ... and the same three levels without it do run
    assert solve(c, ws, st, c.trace()) == 0
    torch.cuda.synchronize()
    assert_bits(state_tensors(st), reference("S1")[0], "S1 state")


# ======================================================================================================================
# (d) graph capture
# ======================================================================================================================
def test_the_call_is_capturable_into_one_graph_and_replays_bit_exactly():
    c = case("S1")
    ref_state, ref_trace = reference("S1")
    ws = capi.workspace(c.workspace_bytes(), DEV)
    st, tr = c.state(), c.trace()
    init = [t.clone() for t in state_tensors(st)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                             # warm-up off the default stream
        assert solve(c, ws, st, tr) == 0
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert_bits(state_tensors(st), ref_state, "S1 eager state")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                             # torch's capture stream is the current stream in here
        rc = solve(c, ws, st, tr)
    assert rc == 0
    for rep in range(2):
        for t, t0 in zip(state_tensors(st), init):
            t.copy_(t0)
        for t in trace_tensors(tr):
            t.fill_(float("nan") if t.dtype.is_floating_point else -1)
        ws.fill_(0x7F)
        graph.replay()
        torch.cuda.synchronize()
        assert_bits(state_tensors(st), ref_state, "S1 state, replay %d" % rep)
        assert_bits(trace_tensors(tr), ref_trace, "S1 trace, replay %d" % rep)


# ======================================================================================================================
# (e) DenseBA.solve goes through the C schedule
# ======================================================================================================================
@pytest.mark.parametrize("name", ["S1", "S2"])
def test_dense_ba_routes_through_the_c_schedule_with_equal_bits(name, monkeypatch):
    from banet_amd import dense as bdense, ops, synth
    B, C, K, pairs, scales, iters, H, W, seed = {"S1": (3, 128, 32, 1, [4, 2, 1], [2, 3, 2], 32, 48, 301),
                                                 "S2": (2, 128, 64, 3, [2, 1], [2, 2], 16, 16, 302)}[name]
    intr, levels, gt = synth.make_dense_windows(B, H, W, C, K, scales, seed, torch.device(DEV), trans_mag=0.06, pairs=pairs)
    mlps = [lambda_weights(C, 100 + i) for i in range(len(scales))]
    T0 = (gt["T"] * 0.7).reshape(B * pairs, 3, 1).to(DEV)
    ba = bdense.DenseBA(intr, levels, mlps, "bundle", 1000.0)
    assert bdense.DenseBA.c_schedule is True and not ba.split_coarse
    calls = []
    keep = ops.lm_solve
    monkeypatch.setattr(ops, "lm_solve", lambda *a, **k: (calls.append(1), keep(*a, **k))[1])

    def run(c_schedule, events=None):
        ba.c_schedule = c_schedule
        snaps, depths = [], []
        st, counts = ba.solve(iters, ba.new_state(T=T0.clone()), snapshots=snaps, depth_outputs=depths, level_events=events)
        torch.cuda.synchronize()
        out = state_tensors(st) + list(counts)
        for s in snaps:
            assert sorted(s) == ["R", "T", "W", "delta", "lam"]
            out += [s[k] for k in ("R", "T", "W", "delta", "lam")]
        return [t.clone() for t in out], depths, snaps, st

    c_out, c_depths, c_snaps, st = run(True)
    assert len(calls) == 1
    py_out, py_depths, _, _ = run(False)
    assert len(calls) == 1                                    # the switch: the Python level loop, no banet_lm_solve_f32 call
    assert_bits(c_out, [t.cpu() for t in py_out], name + " DenseBA c_schedule True vs False")
    assert len(c_depths) == len(levels) == len(py_depths)
    for l, (d, lv) in enumerate(zip(c_depths, levels)):
        assert d.shape == lv.depth.shape
        want = ops.depth_output(lv.depth, lv.basis.reshape(B, lv.H * lv.W, K), c_snaps[l]["W"])
        assert_bits([d, py_depths[l]], [want.cpu(), want.cpu()], "%s depth output of level %d" % (name, l))
    assert_bits([c_snaps[-1]["R"], c_snaps[-1]["W"]], [st.R.cpu(), st.Wc.cpu()], "last snapshot = final state")
    # with level_events the Python loop runs (the events sit between the levels) and the bits are the same
    events = []
    ev_out, _, _, _ = run(True, events)
    assert len(calls) == 1 and len(events) == len(levels)
    assert all(e0.elapsed_time(e1) >= 0.0 for e0, e1 in events)
    assert_bits(ev_out, [t.cpu() for t in py_out], name + " DenseBA with level_events")
    # without snapshots only the counts are recorded
    ba.c_schedule = True
    st2, counts2 = ba.solve(iters, ba.new_state(T=T0.clone()))
    torch.cuda.synchronize()
    assert len(calls) == 2
    assert_bits(state_tensors(st2) + list(counts2), [t.cpu() for t in py_out[:len(state_tensors(st2)) + len(iters)]], name + " plain solve")
    with pytest.raises(capi.BanetError):
        bdense.DenseBA(intr, levels, mlps, "bundle_camera").solve(iters, depth_outputs=[])
