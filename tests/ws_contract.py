"""The workspace contract of libbanet_hip.so as a test harness (include/banet_hip.h, DESIGN.md "Workspace regions"):

  * on entry the workspace holds ARBITRARY bytes -- no call reads a workspace byte it did not write itself;
  * no call touches a byte outside [ws, ws + workspace_bytes).

Plain module: no fixtures, no conftest.  Shared by test_ws_contract_cpu.py (the harness must be able to fail: CPU tensors, torch
stand-ins for a kernel) and test_gpu_workspace_contract.py (the real entry points).

A guarded workspace is a body of exactly the queried size between two guard bands.  The body is filled before the call:

    zero    all bytes 0 (what a fresh process usually gets from the caching allocator -- the case the suite ran before)
    nan     32-bit words 0x7FC00000: a quiet NaN as a float, 2143289344 as an int32
    one     32-bit words 0x3F800000: 1.0 as a float, 1065353216 as an int32
    stale   whatever the previous user of the same arena left (a call of another shape / kernel selection)

Both poison words are positive as int32 on purpose: a queue head or a count misread as an integer ends a `t < tiles` loop instead
of indexing below an array.  There is no fill with the sign bit set, and the guard pattern has none either.
"""
import contextlib

import torch

GUARD_BYTES = 4096                 # per band (>= 4096, a multiple of 256)
GUARD_BYTE = 0x5A                  # 0x5A5A5A5A: positive as an int32, 1.5e16 as a float
FILL_WORDS = {"zero": 0x00000000, "nan": 0x7FC00000, "one": 0x3F800000}
FILLS = ("zero", "stale", "nan", "one")          # benign first: the order the GPU module runs them in


class Arena:
    """One device buffer that successive runs carve their workspaces from, always starting at its first byte: the `stale` fill
    of a run sees what the previous run (another shape, another kernel selection) left in the same bytes -- the C caller that
    recycles one arena.  reset() starts the next run; the buffer itself is allocated once and never cleared."""

    def __init__(self, nbytes, device):
        self.raw = torch.zeros(int(nbytes) + 256, dtype=torch.uint8, device=device)
        self.base = (-self.raw.data_ptr()) % 256
        self.nbytes = int(nbytes)
        self.used = 0

    def reset(self):
        self.used = 0

    def take(self, nbytes):
        assert self.used + nbytes <= self.nbytes, "arena too small: %d + %d > %d" % (self.used, nbytes, self.nbytes)
        lo = self.base + self.used
        self.used += nbytes
        return self.raw[lo:lo + nbytes]


class Handle:
    """What assert_guards_intact needs: the two bands, the body and where it came from."""

    def __init__(self, block, n, fill):
        self.block, self.n, self.fill = block, n, fill
        self.lo = block[:GUARD_BYTES]
        self.body = block[GUARD_BYTES:GUARD_BYTES + n]
        self.hi = block[GUARD_BYTES + n:]


def _fill_words(t, word):
    """fill a uint8 tensor (length a multiple of 4) with one little-endian 32-bit word"""
    pat = torch.tensor([(word >> (8 * i)) & 255 for i in range(4)], dtype=torch.uint8, device=t.device)
    t.view(-1, 4).copy_(pat.expand(t.numel() // 4, 4))


def guarded_workspace(nbytes, device, fill, arena=None):
    """-> (ws, handle).  `ws`: a 256-byte aligned uint8 view of exactly max(nbytes, 256) bytes -- the length
    banet_amd._capi.workspace returns, so ws.numel() stays the exact query -- with GUARD_BYTES of GUARD_BYTE directly before its
    first and directly after its last byte.  The body is filled according to `fill`; `stale` leaves it as it is (meaningful with
    an `arena`, whose bytes the previous run used; a fresh buffer is zero-filled)."""
    if fill not in FILL_WORDS and fill != "stale":
        raise ValueError("unknown fill %r" % (fill,))
    n = max(int(nbytes), 256)
    body = (n + 255) // 256 * 256                      # the upper band starts at the body's last byte + 1; the slot stays aligned
    total = GUARD_BYTES + n + GUARD_BYTES + (body - n)
    if arena is not None:
        block = arena.take((total + 255) // 256 * 256)[:GUARD_BYTES + n + GUARD_BYTES]
    else:
        raw = torch.zeros(total + 256, dtype=torch.uint8, device=device)
        off = (-raw.data_ptr()) % 256
        block = raw[off:off + GUARD_BYTES + n + GUARD_BYTES]
    h = Handle(block, n, fill)
    h.lo.fill_(GUARD_BYTE)
    h.hi.fill_(GUARD_BYTE)
    if fill in FILL_WORDS:
        whole = n // 4 * 4
        _fill_words(h.body[:whole], FILL_WORDS[fill])
        if whole < n:
            h.body[whole:].fill_(0)
    assert h.body.data_ptr() % 256 == 0 and h.body.numel() == n
    return h.body, h


def assert_guards_intact(handle):
    """Synchronise, compare both bands with the pattern; the message names the first byte that changed, relative to the body
    (negative: before its first byte; >= 0: that many bytes past its last one)."""
    if handle.block.is_cuda:
        torch.cuda.synchronize(handle.block.device)
    for name, band, origin in (("before", handle.lo, -GUARD_BYTES), ("after", handle.hi, 0)):
        bad = (band != GUARD_BYTE).nonzero()
        if bad.numel():
            first = int(bad[0])
            raise AssertionError("workspace of %d bytes (fill %r): guard band %s the body was written: first changed byte at "
                                 "offset %d relative to the body's %s (%d bytes changed, now 0x%02x)"
                                 % (handle.n, handle.fill, name, origin + first, "start" if origin else "end", bad.numel(),
                                    int(band[first])))


@contextlib.contextmanager
def patched_workspace(fill, arena=None, module=None):
    """Replace banet_amd._capi.workspace -- the one function every Python-side workspace of the package comes from (ops.py,
    dense.py, dense_train.py, prep_grad.py) -- with the guarded allocator for the duration of the block.  Yields the list of
    handles handed out; on a clean exit every guard band is checked.  `module`: the object whose `workspace` attribute is replaced
    (default banet_amd._capi; the CPU self-test passes a stand-in)."""
    if module is None:
        from banet_amd import _capi as module
    handles = []
    if arena is not None:
        arena.reset()

    def workspace(nbytes, device):
        ws, h = guarded_workspace(nbytes, device, fill, arena)
        handles.append(h)
        return ws

    keep = module.workspace
    module.workspace = workspace
    try:
        yield handles
    finally:
        module.workspace = keep
    for h in handles:
        assert_guards_intact(h)


def run_under_every_fill(run, arena, primer=None, fills=FILLS, module=None):
    """`run()` -> tuple of tensors, executed once per fill under the patched allocator (everything that owns a workspace must be
    built INSIDE run).  `primer()`: a call of another shape run (zero-filled) right before the `stale` run, so that the stale bytes
    are another kernel selection's leftovers.  -> {fill: [cpu clones of the outputs]}, {fill: handles}."""
    outs, seen = {}, {}
    for fill in fills:
        if fill == "stale" and primer is not None:
            with patched_workspace("zero", arena, module):
                primer()
        with patched_workspace(fill, arena, module) as handles:
            res = run()
            outs[fill] = [x.detach().cpu().clone() for x in res]
        seen[fill] = handles
    return outs, seen


def bits_equal(a, b):
    """torch.equal on the bit patterns (NaN == NaN with the same payload; -0.0 != 0.0)"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.float32:
        return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    return torch.equal(a, b)


def assert_same_bits_across_fills(outs, names=None, finite=True):
    """every output bit-equal to the `zero` run's, and finite (float outputs) unless finite=False"""
    ref_fill = next(iter(outs))
    ref = outs[ref_fill]
    for fill, res in outs.items():
        assert len(res) == len(ref)
        for i, (x, y) in enumerate(zip(res, ref)):
            name = names[i] if names else "output %d" % i
            if finite and x.dtype.is_floating_point:
                assert bool(torch.isfinite(x).all()), "%s is not finite under fill %r" % (name, fill)
            if not bits_equal(x, y):
                diff = (x.contiguous().view(-1) != y.contiguous().view(-1)) | (x.contiguous().view(-1) != x.contiguous().view(-1))
                where = int(diff.nonzero()[0]) if diff.any() else -1
                raise AssertionError("%s differs between workspace fills %r and %r: %d of %d entries, first at flat index %d "
                                     "(%r vs %r)" % (name, fill, ref_fill, int(diff.sum()), x.numel(), where,
                                                     x.reshape(-1)[where].item(), y.reshape(-1)[where].item()))


# ======================================================================================================================
# host-only ABI sweep: every entry point that takes (ws, ws_bytes), at several shapes -- exact query / one byte less / pointer
# off by 4 / NULL.  Runs in a child process that sees NO device (abi_sweep_in_child), so the call that passes the workspace
# check goes on to fail for lack of a device and nothing is ever launched on the fake pointers, also on a machine with a GPU.
# ======================================================================================================================
OK, ERR_INVALID_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED, ERR_LAUNCH = 0, -1, -2, -3, -4


def _abi_level(capi, ptr, B, H, W, K, pairs, C=128, variant=None, dense=1, policy=0, flags=0, N=None):
    lv = capi.Level()
    lv.B, lv.N, lv.C, lv.K, lv.H, lv.W = B, (H * W if N is None else N), C, K, H, W
    lv.variant = (capi.BUNDLE if K else capi.BUNDLE_CAMERA) if variant is None else variant
    lv.dense, lv.tgt_has_grad, lv.scale, lv.pairs, lv.normalize_rays = dense, 0 if dense else 1, 1.0, pairs, 1
    lv.policy, lv.flags = policy, flags
    lv.src = lv.tgt = lv.depth = lv.intr = ptr
    if K:
        lv.basis = ptr
    if not dense:
        lv.rays = lv.fx = lv.fy = lv.ox = lv.oy = ptr
    return lv


def abi_cases(capi):
    """-> list of (name, query bytes, call(ws, ws_bytes) -> rc, kind); kind: "required" (a refusal is BANET_ERR_WORKSPACE),
    "optional" (banet_equation_construction_grad_f32: falls back to the kernel without a workspace instead of refusing)."""
    import ctypes
    L = capi.lib()
    host = (ctypes.c_float * 64)()                     # a real host address for every tensor argument: checked for NULL, never
    p = ctypes.cast(host, ctypes.c_void_p)             # dereferenced (there is no device in this process)
    pv = p.value
    cases = []
    # --- EquationConstruction (+Grad): P on both sides of 144 (matrix-pipe fast path) and of the LDS-tiled kernel's block counts
    for B, N, C, P in ((1, 777, 128, 6), (2, 2337, 128, 38), (2, 1961, 70, 143), (1, 2337, 128, 144), (1, 2337, 128, 145),
                       (2, 130, 128, 200), (1, 777, 128, 304)):
        nb = L.banet_equation_construction_workspace_bytes(B, N, C, P)
        cases.append(("equation_construction B%d N%d C%d P%d" % (B, N, C, P), nb,
                      lambda ws, n, a=(B, N, C, P): L.banet_equation_construction_f32(p, p, p, p, p, *a, ws, n, None), "required"))
        nb = L.banet_equation_construction_grad_workspace_bytes(B, N, C, P)
        cases.append(("equation_construction_grad B%d N%d C%d P%d" % (B, N, C, P), nb,
                      lambda ws, n, a=(B, N, C, P): L.banet_equation_construction_grad_f32(p, p, p, p, p, p, p, p, *a, ws, n, None),
                      "optional"))
    # --- the level entry points: K = 0 / 32 / 128 / 256, pairs = 1 / 3 / 7, both policies, P on both sides of ~190 (bigA)
    levels = [(2, 41, 57, 0, 1, 0), (2, 37, 53, 0, 3, 1), (2, 41, 57, 32, 1, 0), (1, 10, 13, 32, 3, 1), (2, 41, 57, 128, 1, 0),
              (2, 37, 53, 128, 3, 1), (2, 30, 40, 128, 7, 0), (4, 120, 160, 128, 1, 0), (2, 35, 45, 256, 1, 0), (1, 37, 53, 256, 7, 1),
              (2, 41, 57, 176, 1, 0), (2, 41, 57, 188, 1, 1), (32, 60, 80, 128, 1, 0)]
    st = capi.State()
    st.R = st.T = st.Wc = st.iters = st.ratio = st.lambda_out = st.delta = pv
    mlp = capi.Mlp()
    for i in range(5):
        mlp.w[i] = mlp.b[i] = pv
    keep = []
    for B, H, W, K, pairs, policy in levels:
        for flags in (0, capi.DEV_SYRK_F16):                   # default selection; the fp16 two-piece SYRK where it applies (colmax / recmax regions)
            if flags and K not in (128, 256):
                continue
            lv = _abi_level(capi, pv, B, H, W, K, pairs, policy=policy, flags=flags)
            keep.append(lv)
            tag = "B%d %dx%d K%d pairs%d policy%d flags%x" % (B, H, W, K, pairs, policy, flags)
            ref = ctypes.byref(lv)
            wc = p if K else None
            cases.append(("ba_assemble " + tag, L.banet_ba_assemble_workspace_bytes(ref),
                          lambda ws, n, r=ref, w=wc: L.banet_ba_assemble_f32(r, p, p, w, p, p, p, p, ws, n, None), "required"))
            cases.append(("ba_assemble_mask " + tag, L.banet_ba_assemble_workspace_bytes(ref),
                          lambda ws, n, r=ref, w=wc: L.banet_ba_assemble_mask_f32(r, p, p, w, p, p, p, p, p, ws, n, None), "required"))
            for entry in ("lm_level", "lm_level_ex"):
                def call(ws, n, r=ref, e=entry):
                    if e == "lm_level":
                        return L.banet_lm_level_f32(r, ctypes.byref(mlp), 1000.0, 2, 0, ctypes.byref(st), ws, n, None)
                    return L.banet_lm_level_ex_f32(r, ctypes.byref(mlp), 1000.0, 2, 0, None, ctypes.byref(st), ws, n, None)
                cases.append((entry + " " + tag, L.banet_lm_level_workspace_bytes(ref), call, "required"))
            nb = L.banet_ba_solve_update_workspace_bytes(ref)
            if nb:                                     # (0: banet_ba_solve_update_f32 alone is enough, ws may be NULL)
                cases.append(("ba_solve_update_ws " + tag, nb,
                              lambda ws, n, r=ref: L.banet_ba_solve_update_ws_f32(r, ctypes.byref(mlp), 1000.0, p, p, p, p, ctypes.byref(st),
                                                                                  ws, n, None), "required"))
    # --- legacy early-terminated LM (LmCtl region), sparse points
    lv = _abi_level(capi, pv, 2, 48, 64, 0, 1, C=70, variant=capi.LEGACY_LM, dense=0, N=777)
    keep.append(lv)
    cases.append(("lm_level legacy_lm sparse N777 C70", L.banet_lm_level_workspace_bytes(ctypes.byref(lv)),
                  lambda ws, n, r=ctypes.byref(lv): L.banet_lm_level_f32(r, ctypes.byref(mlp), 1.0, 3, 1, ctypes.byref(st), ws, n, None),
                  "required"))
    # --- resampler / depth-output gradients
    for B, N, C, H, W, mode in ((2, 777, 70, 41, 57, 0), (1, 4096, 128, 37, 53, 1), (2, 130, 3, 10, 13, 0)):
        nb = L.banet_resample_grad_workspace_bytes(B, N, C, H, W, mode)
        cases.append(("resample_grad B%d N%d C%d %dx%d mode%d" % (B, N, C, H, W, mode), nb,
                      lambda ws, n, a=(B, N, C, H, W, mode): L.banet_resample_grad_f32(p, p, p, p, p, *a, 1, ws, n, None), "required"))
    for B, N, K in ((2, 2337, 128), (1, 777, 32), (3, 130, 256)):
        nb = L.banet_depth_output_grad_workspace_bytes(B, N, K)
        cases.append(("depth_output_grad B%d N%d K%d" % (B, N, K), nb,
                      lambda ws, n, a=(B, N, K): L.banet_depth_output_grad_f32(p, p, p, p, p, p, *a, 0, ws, n, None), "required"))
    # --- deterministic sample-stats gradient
    for B, N, C, H, W in ((2, 777, 128, 41, 57), (1, 4096, 70, 37, 53), (3, 130, 255, 10, 13)):
        nb = L.banet_sample_stats_grad_workspace_bytes(B, N, C, H, W)
        cases.append(("sample_stats_grad_det B%d N%d C%d %dx%d" % (B, N, C, H, W), nb,
                      lambda ws, n, a=(B, N, C, H, W): L.banet_sample_stats_grad_det_f32(p, p, p, p, *a, p, p, p, p, p, ws, n, None),
                      "required"))
    # --- dense adjoint: every flag combination that changes the layout, K <= 128 / > 128 / pose only, the sparse layout
    for B, H, W, K, dense, N in ((2, 41, 57, 128, 1, None), (2, 37, 53, 32, 1, None), (1, 35, 45, 256, 1, None), (2, 37, 53, 0, 1, None),
                                 (2, 48, 64, 128, 0, 777)):
        lv = _abi_level(capi, pv, B, H, W, K, 1, dense=dense, N=N)
        keep.append(lv)
        ref = ctypes.byref(lv)
        for flags in (0, 1, 3, 4, 5, 8) if dense else (0, 1):
            nb = L.banet_dense_adjoint_workspace_bytes_ex(ref, flags)
            wc = p if K else None
            cases.append(("dense_adjoint_ex B%d %dx%d K%d dense%d flags%d" % (B, H, W, K, dense, flags), nb,
                          lambda ws, n, r=ref, f=flags, w=wc: L.banet_dense_adjoint_ex_f32(r, p, p, w, p, p, p, p, p, p, w, p, f, ws, n, None),
                          "required"))
        cases.append(("dense_adjoint B%d %dx%d K%d dense%d" % (B, H, W, K, dense), L.banet_dense_adjoint_workspace_bytes(ref),
                      lambda ws, n, r=ref, w=(p if K else None): L.banet_dense_adjoint_f32(r, p, p, w, p, p, p, p, p, p, w, p, ws, n, None),
                      "required"))
    # --- small-step adjoint: P < 32, P >= 32, pairs > 1, camera
    for variant, B, C, K, pairs in ((capi.BUNDLE, 3, 32, 8, 1), (capi.BUNDLE, 3, 32, 33, 1), (capi.BUNDLE, 2, 128, 128, 3),
                                    (capi.BUNDLE_CAMERA, 3, 32, 0, 7), (capi.BUNDLE, 37, 255, 8, 1)):
        a = (variant, B, 4000, C, K, pairs)
        nb = L.banet_small_step_adjoint_workspace_bytes(*a)
        cases.append(("small_step_adjoint v%d B%d C%d K%d pairs%d" % (variant, B, C, K, pairs), nb,
                      lambda ws, n, a=a, w=(p if K else None): L.banet_small_step_adjoint_f32(
                          *a, 1000.0, ctypes.byref(mlp), p, p, p, p, p, p, p, p, w, p, p, p, p, p, ctypes.byref(mlp), ws, n, None), "required"))
    cases.append(keep)          # (keeps the level structs alive as long as the list)
    return cases


def abi_sweep():
    """-> [{name, bytes, kind, exact, minus1, off4, null, min_ok}]: the return codes of the four probes per case"""
    import ctypes
    from banet_amd import _capi as capi
    cases = abi_cases(capi)
    cases.pop()
    arena = (ctypes.c_char * 512)()
    base = (ctypes.addressof(arena) + 255) & ~255                  # an aligned host address: compared and offset, never dereferenced
    out = []
    for name, nb, call, kind in cases:
        rec = dict(name=name, bytes=int(nb), kind=kind)
        if nb:
            rec["exact"] = call(ctypes.c_void_p(base), nb)
            rec["minus1"] = call(ctypes.c_void_p(base), nb - 1)
            rec["off4"] = call(ctypes.c_void_p(base + 4), nb)
            rec["null"] = call(None, nb)
        out.append(rec)
    return out


def abi_sweep_in_child():
    """abi_sweep() in a child process without a visible device -> the list of records"""
    import json
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="", BANET_NUM_CUS="256")
    code = ("import sys, json; sys.path[:0] = [%r, %r]; import ws_contract; print('ABI_SWEEP ' + json.dumps(ws_contract.abi_sweep()))"
            % (os.path.dirname(here), here))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, "the ABI sweep's child process ended with %s:\n%s" % (r.returncode, (r.stdout + r.stderr)[-3000:])
    line = [l for l in r.stdout.splitlines() if l.startswith("ABI_SWEEP ")][-1]
    return json.loads(line[len("ABI_SWEEP "):])
