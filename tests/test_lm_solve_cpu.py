"""banet_lm_solve_f32 / banet_lm_solve_workspace_bytes on the host (include/banet_hip.h (5c)): struct layouts, a C99 caller,
the workspace query and the all-or-nothing validation.  No GPU: every call below is refused by the host-side checks before
anything could be launched -- except the one probe with the exact workspace size, which runs in a child process that sees no
device (as tests/ws_contract.py does) and fails there for lack of one."""
import ctypes
import json
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
os.environ.setdefault("BANET_NUM_CUS", "256")     # host-side plans tabulated for a 256-CU part, whatever GPU the host has
OK, ERR_INVALID_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED, ERR_LAUNCH = 0, -1, -2, -3, -4


@pytest.fixture(scope="module")
def capi():
    sys.path.insert(0, ROOT) if ROOT not in sys.path else None
    from banet_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _capi


# ---------------------------------------------------------------------------------------------------------------------
# a schedule of fake pointers (checked for NULL, never dereferenced: nothing here gets as far as a launch)
# ---------------------------------------------------------------------------------------------------------------------
class Sched:
    """three dense bundle levels 8x12 -> 16x24 -> 32x48 (B 3, C 128, K 32) unless told otherwise; every array kept alive here"""

    def __init__(self, capi, shapes=((8, 12), (16, 24), (32, 48)), B=3, C=128, K=32, pairs=1, variant=None, iters=None, mlps=True):
        host = (ctypes.c_float * 64)()
        self.host = host
        self.p = ctypes.cast(host, ctypes.c_void_p).value
        n = len(shapes)
        self.levels = (capi.Level * max(n, 1))()
        for lv, (H, W) in zip(self.levels, shapes):
            lv.B, lv.N, lv.C, lv.K, lv.H, lv.W = B, H * W, C, K, H, W
            lv.variant = (capi.BUNDLE if K else capi.BUNDLE_CAMERA) if variant is None else variant
            lv.dense, lv.scale, lv.pairs, lv.normalize_rays = 1, 1.0, pairs, 1
            lv.src = lv.tgt = lv.depth = lv.intr = self.p
            if K:
                lv.basis = self.p
        self.mlp = capi.Mlp()
        for i in range(5):
            self.mlp.w[i] = self.mlp.b[i] = self.p
        self.mlps = (ctypes.POINTER(capi.Mlp) * max(n, 1))()
        if mlps:
            for i in range(n):
                self.mlps[i] = ctypes.pointer(self.mlp)
        self.iters = (ctypes.c_int32 * max(n, 1))(*(iters if iters is not None else [2] * n))
        self.st = capi.State()
        self.st.R = self.st.T = self.st.Wc = self.st.iters = self.st.ratio = self.st.lambda_out = self.st.delta = self.p
        s = capi.Schedule()
        s.levels, s.n_levels = ctypes.cast(self.levels, ctypes.POINTER(capi.Level)), n
        s.mlps = ctypes.cast(self.mlps, ctypes.POINTER(ctypes.POINTER(capi.Mlp)))
        s.max_iters = ctypes.cast(self.iters, ctypes.POINTER(ctypes.c_int32))
        s.l2_base, s.early_termination = 1000.0, 0
        self.c = s
        self.L = capi.lib()
        arena = (ctypes.c_char * 512)()
        self.arena = arena
        self.base = (ctypes.addressof(arena) + 255) & ~255      # an aligned host address: compared and offset, never dereferenced

    def query(self):
        return self.L.banet_lm_solve_workspace_bytes(ctypes.byref(self.c))

    def per_level(self):
        return [self.L.banet_lm_level_workspace_bytes(ctypes.byref(self.levels[i])) for i in range(self.c.n_levels)]

    def call(self, ws="base", nbytes=None):
        self.c.workspace = self.base if ws == "base" else ws
        self.c.workspace_bytes = self.query() if nbytes is None else nbytes
        return self.L.banet_lm_solve_f32(ctypes.byref(self.c), ctypes.byref(self.st), None)

    def level_call(self, i, ws="base", nbytes=None):
        """what banet_lm_level_ex_f32 answers for level i alone, with the schedule's arguments"""
        nb = self.per_level()[i] if nbytes is None else nbytes
        return self.L.banet_lm_level_ex_f32(ctypes.byref(self.levels[i]), self.mlps[i], self.c.l2_base, self.iters[i],
                                            self.c.early_termination, self.c.params, ctypes.byref(self.st),
                                            self.base if ws == "base" else ws, nb, None)


# ---------------------------------------------------------------------------------------------------------------------
# layout and linkage
# ---------------------------------------------------------------------------------------------------------------------
def test_schedule_and_trace_layouts_match_the_header(capi, tmp_path):
    """sizeof / offsetof of every field from a compiled C program equal the ctypes mirrors"""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    tf = [n for n, _ in capi.SolveTrace._fields_]
    sf = [n for n, _ in capi.Schedule._fields_]
    assert sorted(tf) == sorted(["R", "T", "Wc", "lambda_out", "delta", "ratio", "iters", "depth"])
    assert sorted(sf) == sorted(["levels", "n_levels", "mlps", "max_iters", "l2_base", "early_termination", "params", "workspace",
                                 "workspace_bytes", "trace"])
    exprs = ["sizeof(banet_solve_trace_t)"] + ["offsetof(banet_solve_trace_t, %s)" % n for n in tf] + \
            ["sizeof(banet_schedule_t)"] + ["offsetof(banet_schedule_t, %s)" % n for n in sf]
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "banet_hip.h"\nint main(void){\n' +
                    "".join('  printf("%%zu\\n", (size_t)%s);\n' % e for e in exprs) + "  return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = [ctypes.sizeof(capi.SolveTrace)] + [getattr(capi.SolveTrace, n).offset for n in tf] + \
           [ctypes.sizeof(capi.Schedule)] + [getattr(capi.Schedule, n).offset for n in sf]
    assert got == want


def test_a_c99_program_calls_both_entry_points(capi, tmp_path):
    """a C translation unit fills a banet_schedule_t, sizes its workspace and is refused on the host (NULL state): links, runs"""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "t.c"
    src.write_text('''#include <stdio.h>
#include <string.h>
#include "banet_hip.h"
int main(void) {
  static float dummy[4];
  banet_level_t lv[2];
  banet_mlp_t mlp;
  const banet_mlp_t* mlps[2];
  int32_t iters[2] = {2, 3};
  banet_schedule_t s;
  banet_solve_trace_t tr;
  size_t one, two;
  int i;
  memset(lv, 0, sizeof lv); memset(&s, 0, sizeof s); memset(&tr, 0, sizeof tr);
  for (i = 0; i < 5; ++i) { mlp.w[i] = dummy; mlp.b[i] = dummy; }
  for (i = 0; i < 2; ++i) {
    lv[i].B = 2; lv[i].H = 16 << i; lv[i].W = 24 << i; lv[i].N = lv[i].H * lv[i].W; lv[i].C = 128; lv[i].K = 32;
    lv[i].variant = BANET_BUNDLE; lv[i].dense = 1; lv[i].scale = 1.0f; lv[i].normalize_rays = 1;
    lv[i].src = lv[i].tgt = lv[i].depth = lv[i].basis = lv[i].intr = dummy;
    mlps[i] = &mlp;
  }
  s.levels = lv; s.n_levels = 2; s.mlps = mlps; s.max_iters = iters; s.l2_base = 1000.0f; s.trace = &tr;
  two = banet_lm_solve_workspace_bytes(&s);
  one = banet_lm_level_workspace_bytes(&lv[1]);
  if (two == 0 || two != one || banet_lm_level_workspace_bytes(&lv[0]) > two) return 1;
  if (banet_lm_solve_f32(&s, 0, 0) != BANET_ERR_INVALID_ARG) return 2;     /* no state: refused before any launch */
  if (banet_lm_solve_f32(0, 0, 0) != BANET_ERR_INVALID_ARG) return 3;
  if (banet_version() != BANET_VERSION) return 4;
  printf("schedule ok %zu\\n", two);
  return 0;
}
''')
    libdir = os.path.join(ROOT, "banet_amd", "lib")
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-lbanet_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    env = dict(os.environ, BANET_NUM_CUS="256")
    assert subprocess.check_output([str(exe)], env=env).decode().startswith("schedule ok ")


def test_the_version_is_unchanged_and_the_entry_is_found_by_symbol(capi):
    L = capi.lib()
    assert L.banet_version() == 150
    assert hasattr(L, "banet_lm_solve_f32") and hasattr(L, "banet_lm_solve_workspace_bytes")
    assert "banet_lm_solve_f32" in capi.EXPORTS and "banet_lm_solve_workspace_bytes" in capi.EXPORTS


# ---------------------------------------------------------------------------------------------------------------------
# the workspace query
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(), dict(shapes=((32, 48), (16, 24), (8, 12))), dict(shapes=((16, 16), (24, 32)), K=256, B=2),
                                dict(shapes=((12, 10), (24, 20)), C=64, K=0, B=4), dict(shapes=((8, 8), (16, 16)), K=64, pairs=3, B=2),
                                dict(shapes=((30, 40),))])
def test_the_query_is_the_maximum_of_the_per_level_queries(capi, kw):
    s = Sched(capi, **kw)
    per = s.per_level()
    assert all(v > 0 for v in per) and s.query() == max(per) and s.query() % 256 == 0
    if len(per) > 1:
        assert len(set(per)) > 1                              # (the levels really differ in their needs)


def test_the_query_is_zero_for_bad_level_counts_mismatched_or_unsupported_levels(capi):
    L = capi.lib()
    assert L.banet_lm_solve_workspace_bytes(None) == 0
    assert Sched(capi, shapes=()).query() == 0                                    # n_levels 0
    assert Sched(capi, shapes=((8, 12),) * 16).query() > 0
    assert Sched(capi, shapes=((8, 12),) * 17).query() == 0                       # n_levels 17
    s = Sched(capi)
    s.c.levels = None
    assert s.query() == 0
    for field, bad in (("B", 4), ("K", 64), ("pairs", 2), ("variant", capi.BUNDLE_CAMERA), ("policy", capi.POLICY_BATCH_INVARIANT)):
        for which in (0, 2):
            s = Sched(capi)
            assert s.query() > 0
            setattr(s.levels[which], field, bad)
            if field == "variant":                                               # a valid pose-only level, still a mismatch
                s.levels[which].K = 0
            if field != "variant":
                assert s.per_level()[which] > 0, field                            # each level alone is fine
            assert s.query() == 0, (field, which)
    s = Sched(capi)                                                               # pairs 0 and 1 are the same two-frame window
    s.levels[1].pairs = 0
    assert s.query() > 0
    for which in (0, 1, 2):                                                       # one unsupported level (C = 300), any position
        s = Sched(capi)
        s.levels[which].C = 300
        assert s.per_level()[which] == 0 and s.query() == 0
    s = Sched(capi)                                                               # H, W, N, C, scale, flags may differ
    s.levels[0].C, s.levels[1].scale, s.levels[2].flags = 64, 2.0, capi.DEV_NO_QUAD_GATHER
    assert s.query() == max(s.per_level()) > 0


# ---------------------------------------------------------------------------------------------------------------------
# validation: every error carries the per-level entry's code, and comes before any launch
# ---------------------------------------------------------------------------------------------------------------------
def test_every_error_is_reported_with_the_per_level_code(capi):
    def expect(s, code, level=None):
        if level is not None:
            assert s.level_call(level, nbytes=1 << 30) == code, "the per-level entry"
        assert s.call(nbytes=1 << 30) == code

    L = capi.lib()
    st = capi.State()
    assert L.banet_lm_solve_f32(None, ctypes.byref(st), None) == ERR_INVALID_ARG
    for n in (0, 17, -1):
        s = Sched(capi)
        s.c.n_levels = n
        assert s.call(nbytes=1 << 30) == ERR_INVALID_ARG
    s = Sched(capi)
    s.c.max_iters = None
    assert s.call(nbytes=1 << 30) == ERR_INVALID_ARG
    s = Sched(capi)
    s.c.levels = None
    assert s.call(nbytes=1 << 30) == ERR_INVALID_ARG
    for which in (0, 1, 2):                      # the bad level first, in the middle, last: the same code, nothing enqueued before it
        s = Sched(capi)
        s.levels[which].src = None               # check_level
        expect(s, ERR_INVALID_ARG, which)
        s = Sched(capi)
        s.levels[which].variant = 7
        expect(s, ERR_INVALID_ARG, which)
        s = Sched(capi)
        s.levels[which].policy = 5
        expect(s, ERR_INVALID_ARG, which)
        s = Sched(capi)
        s.levels[which].basis = None
        expect(s, ERR_INVALID_ARG, which)
        s = Sched(capi)
        s.iters[which] = -1                      # max_iters < 0
        expect(s, ERR_INVALID_ARG, which)
        s = Sched(capi)
        s.mlps[which] = None                     # check_state: the bundle variants need the lambda MLP
        expect(s, ERR_INVALID_ARG, which)
        s = Sched(capi)
        s.levels[which].C = 300                  # plan_assemble
        expect(s, ERR_UNSUPPORTED, which)
        s = Sched(capi)
        s.levels[which].K = 257
        expect(s, ERR_UNSUPPORTED, which)
        s = Sched(capi)                          # each level alone is valid, but they disagree
        s.levels[which].B = 5
        assert s.call(nbytes=1 << 30) == ERR_INVALID_ARG
    s = Sched(capi)                              # the state
    s.st.delta = None
    expect(s, ERR_INVALID_ARG, 0)
    s = Sched(capi)
    s.st.Wc = None
    expect(s, ERR_INVALID_ARG, 0)
    assert s.L.banet_lm_solve_f32(ctypes.byref(s.c), None, None) == ERR_INVALID_ARG
    for field, bad in (("solver", 2), ("angle_change", -1.0), ("translation_change", float("nan")), ("residual_ratio", 0.0)):
        s = Sched(capi)                          # params
        p = capi.LmParams()
        s.L.banet_lm_params_default(ctypes.byref(p))
        setattr(p, field, bad)
        s.c.params = ctypes.pointer(p)
        expect(s, ERR_INVALID_ARG, 0)
    s = Sched(capi, mlps=False, K=0, variant=capi.LEGACY_FIXED)     # no MLP in this variant: NULL entries, or no array at all
    s.c.mlps = None
    s.levels[1].C = 300
    assert s.call(nbytes=1 << 30) == ERR_UNSUPPORTED


def test_workspace_errors(capi):
    s = Sched(capi)
    nb = s.query()
    per = s.per_level()
    assert nb == per[2] > per[1] > per[0]
    assert s.call(nbytes=nb - 1) == ERR_WORKSPACE                    # one byte less than the query
    assert s.call(nbytes=per[1]) == ERR_WORKSPACE                    # enough for the first two levels only: still nothing runs
    assert s.call(nbytes=0) == ERR_WORKSPACE
    assert s.call(ws=None, nbytes=nb) == ERR_WORKSPACE               # NULL
    assert s.call(ws=s.base + 4, nbytes=nb) == ERR_WORKSPACE         # misaligned
    assert s.call(ws=s.base + 128, nbytes=nb + 128) == ERR_WORKSPACE
    assert s.level_call(2, nbytes=nb - 1) == ERR_WORKSPACE and s.level_call(2, ws=s.base + 4) == ERR_WORKSPACE
    # an argument error of a later level wins over nothing: the first failing check in level order is reported
    s = Sched(capi)
    s.levels[2].C = 300
    assert s.call(nbytes=s.per_level()[0] - 1) == ERR_WORKSPACE      # level 0 already fails on the workspace
    assert s.call(nbytes=1 << 30) == ERR_UNSUPPORTED


def test_trace_depth_needs_the_bundle_variant(capi):
    s = Sched(capi, shapes=((12, 10), (24, 20)), C=64, K=0, B=4)
    tr = capi.SolveTrace()
    s.c.trace = ctypes.pointer(tr)
    ptrs = (capi._FP * 2)(s.p, s.p)
    tr.depth = ctypes.cast(ptrs, ctypes.POINTER(capi._FP))
    assert s.call(nbytes=1 << 30) == ERR_INVALID_ARG                 # bundle_camera, K = 0
    s = Sched(capi, shapes=((12, 10), (24, 20)), C=8, K=0, B=2, variant=capi.LEGACY_FIXED, mlps=False)
    s.c.trace = ctypes.pointer(tr)
    assert s.call(nbytes=1 << 30) == ERR_INVALID_ARG


def test_the_exact_query_passes_every_check(capi):
    """in a child process without a device: with exactly the queried bytes the call gets past the host-side checks of all levels
    and fails for lack of a device (BANET_ERR_LAUNCH); one byte less is refused -- so the query is the smallest accepted value"""
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys, json; sys.path[:0] = [%r, %r]\n"
            "from banet_amd import _capi\n"
            "import test_lm_solve_cpu as t\n"
            "out = []\n"
            "for kw in (dict(), dict(shapes=((16, 16), (24, 32)), K=256, B=2), dict(shapes=((12, 10), (24, 20)), C=64, K=0, B=4)):\n"
            "    s = t.Sched(_capi, **kw)\n"
            "    tr = _capi.SolveTrace()\n"
            "    tr.R = tr.T = tr.iters = s.p\n"
            "    s.c.trace = __import__('ctypes').pointer(tr)\n"
            "    out.append([s.query(), s.call(), s.call(nbytes=s.query() - 1)])\n"
            "print('LM_SOLVE ' + json.dumps(out))\n" % (ROOT, here))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="", BANET_NUM_CUS="256")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("LM_SOLVE ")][-1]
    for nb, exact, minus1 in json.loads(line[len("LM_SOLVE "):]):
        assert nb > 0 and exact == ERR_LAUNCH and minus1 == ERR_WORKSPACE, (nb, exact, minus1)


def test_python_mirror_refuses_inconsistent_schedules(capi):
    """ops.lm_solve checks its lists before it builds the struct (no GPU needed: CPU-side errors)"""
    from banet_amd import ops
    with pytest.raises(capi.BanetError):
        ops.lm_solve([], [], 1.0, [], False, None)
    assert ops.lm_solve_workspace_bytes([]) == 0
