"""banet_ba_residual_f32 on the host: the symbol, the struct layout, the argument checks (the assembly pass's, with its codes) and
the numpy reference the GPU tests measure against.  No GPU: a valid call gets past every check and fails for lack of a device."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
os.environ.setdefault("BANET_NUM_CUS", "256")
OK, INVALID, UNSUPPORTED, LAUNCH = 0, -1, -3, -4


@pytest.fixture(scope="module")
def capi():
    sys.path.insert(0, ROOT) if ROOT not in sys.path else None
    from banet_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _capi


def test_the_symbol_is_exported_and_bound(capi):
    L = capi.lib()
    assert hasattr(L, "banet_ba_residual_f32") and "banet_ba_residual_f32" in capi.EXPORTS
    res, args = capi.EXPORTS["banet_ba_residual_f32"]
    assert res is ctypes.c_int and len(args) == 6 and args[4] == ctypes.POINTER(capi.ResidualOut)
    assert L.banet_version() == 150                      # detected by its symbol: the version does not move
    from banet_amd import ops, dense
    assert callable(ops.ba_residual) and ops.Residual._fields == ("sq", "ab", "mask", "proj", "sums")
    assert callable(dense.DenseBA.residual) and callable(dense.DenseBA.cost_trace)


def test_residual_out_layout_matches_the_header(capi, tmp_path):
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "banet_hip.h"\n'
                    'int main(){printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(banet_residual_out_t), offsetof(banet_residual_out_t, sq), '
                    'offsetof(banet_residual_out_t, ab), offsetof(banet_residual_out_t, mask), offsetof(banet_residual_out_t, proj), '
                    'offsetof(banet_residual_out_t, sums));return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    R = capi.ResidualOut
    assert got == [ctypes.sizeof(R), R.sq.offset, R.ab.offset, R.mask.offset, R.proj.offset, R.sums.offset]


def _level(capi, variant=None, B=2, H=12, W=20, C=128, K=8, pairs=1, dense=1, N=None):
    """a level whose pointers are never dereferenced on the host (any non-null value)"""
    lv = capi.Level()
    lv.B, lv.N, lv.C, lv.K, lv.H, lv.W = B, (H * W if N is None else N), C, K, H, W
    lv.variant = capi.BUNDLE if variant is None else variant
    lv.dense, lv.scale, lv.pairs, lv.normalize_rays = dense, 1.0, pairs, 1
    lv.src = lv.tgt = lv.depth = 4096
    if K > 0:
        lv.basis = 4096
    if dense:
        lv.intr = 4096
    else:
        lv.rays = lv.fx = lv.fy = lv.ox = lv.oy = 4096
        lv.tgt_has_grad = 1
    return lv


def _out(capi, sq=4096, ab=4096, mask=4096, proj=None, sums=None):
    o = capi.ResidualOut()
    o.sq, o.ab, o.mask, o.proj, o.sums = sq, ab, mask, proj, sums
    return o


def _call(capi, lv, R=4096, T=4096, Wc=4096, out=None, no_out=False):
    o = _out(capi) if out is None else out
    return capi.lib().banet_ba_residual_f32(ctypes.byref(lv) if lv is not None else None, R, T, Wc,
                                            None if no_out else ctypes.byref(o), None)


def test_null_arguments_are_invalid(capi):
    lv = _level(capi)
    assert _call(capi, None) == INVALID
    assert _call(capi, lv, R=None) == INVALID and _call(capi, lv, T=None) == INVALID
    assert _call(capi, lv, Wc=None) == INVALID                                   # K > 0 needs the coefficients
    assert _call(capi, lv, no_out=True) == INVALID
    for name in ("sq", "ab", "mask"):
        assert _call(capi, lv, out=_out(capi, **{name: None})) == INVALID, name
    # (K = 0 needs no coefficients, proj / sums are optional: the valid calls of probe_without_a_device)


VALID = [dict(C=20, K=5, H=33, W=47), dict(C=128, K=8), dict(variant=2, C=3, K=0, H=5, W=7), dict(variant=0, C=128, K=0, H=33, W=47),
         dict(variant=1, C=128, K=0), dict(C=128, K=128, pairs=3), dict(C=256, K=3), dict(C=7, K=256), dict(C=128, K=8, dense=0, N=100),
         dict(variant=0, C=16, K=0, dense=0, N=100)]
REFUSED = {"C = 257": (dict(C=257), UNSUPPORTED), "K = 257": (dict(K=257), UNSUPPORTED),
           "pairs = 2, legacy": (dict(variant=0, K=0, pairs=2), INVALID), "bundle without a basis": (dict(K=0), INVALID),
           "bundle_camera with a basis": (dict(variant=2, K=8), INVALID), "dense with N != H W": (dict(N=100), INVALID),
           "H < 4": (dict(H=3), INVALID), "unknown policy": (dict(policy=7), INVALID),
           "odd C above 128": (dict(C=131), UNSUPPORTED), "odd K above 128": (dict(K=131), UNSUPPORTED)}


def probe_without_a_device():
    """runs in a child process that sees no device (the pointers are made up): the codes of every call that gets as far as a launch"""
    sys.path.insert(0, ROOT) if ROOT not in sys.path else None
    from banet_amd import _capi as capi
    L = capi.lib()
    out = {"valid": [], "valid_flags": [], "refused": {}}
    for kw in VALID:
        lv = _level(capi, **kw)
        out["valid"].append(_call(capi, lv, out=_out(capi, proj=4096, sums=4096)))
        lv.flags, lv.policy = capi.DEV_FORCE_STRIP_GATHER | capi.DEV_SYRK_F16, capi.POLICY_BATCH_INVARIANT      # accepted and ignored
        out["valid_flags"].append(_call(capi, lv, Wc=4096 if lv.K > 0 else None))      # K = 0: no coefficients; proj / sums optional
    for name, (kw, _) in REFUSED.items():
        kw = dict(kw)
        policy = kw.pop("policy", 0)
        lv = _level(capi, **kw)
        lv.policy = policy
        asm = L.banet_ba_assemble_f32(ctypes.byref(lv), 4096, 4096, 4096, 4096, 4096, 4096, 4096, ctypes.c_void_p(4096), 1 << 40, None)
        out["refused"][name] = [_call(capi, lv), asm]
    return out


@pytest.fixture(scope="module")
def probe(capi):
    import json
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="", BANET_NUM_CUS="256")
    code = ("import sys, json; sys.path[:0] = [%r, %r]; import test_residual_cpu as t; print('PROBE ' + json.dumps(t.probe_without_a_device()))"
            % (ROOT, here))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("PROBE ")][-1][len("PROBE "):])


def test_a_level_the_assembly_refuses_gets_the_assembly_s_code(probe):
    for name, (_, want) in REFUSED.items():
        got, asm = probe["refused"][name]
        assert got == want == asm, (name, got, asm)


def test_a_valid_level_fails_for_lack_of_a_device_only(probe):
    assert probe["valid"] == [LAUNCH] * len(VALID), probe["valid"]
    assert probe["valid_flags"] == [LAUNCH] * len(VALID), probe["valid_flags"]


def test_cpu_tensors_raise(capi):
    import torch
    from banet_amd import ops
    B, H, W, C = 1, 4, 6, 8
    with pytest.raises(capi.BanetError):
        prob = ops.LevelProblem("bundle_camera", torch.zeros(B, H, W, C), torch.zeros(B, H, W, C), torch.ones(B, H * W), H, W, C,
                                intr=torch.ones(B, 4), dense=True, tgt_has_grad=False)
        ops.ba_residual(prob, torch.eye(3)[None], torch.zeros(1, 3, 1))
    # ... also when only the state is on the CPU (a level that claims device tensors: never dereferenced)
    fake = type("P", (), {})()
    fake.c, fake.B, fake.N, fake.K, fake.device = _level(capi, variant=capi.BUNDLE_CAMERA, K=0, B=1), 1, 240, 0, "cpu"
    with pytest.raises(capi.BanetError):
        ops.ba_residual(fake, torch.eye(3)[None], torch.zeros(1, 3, 1))


def test_the_reference_agrees_with_the_oracle_s_check_update():
    """sum_n ab and sum mask of tests/residual_ref.py (float64) are the numerator and the mask count of legacy_avg_residual
    (legacy/ba.py:306-324): avg_c = N / sum(mask) x mean_n |d_nc|."""
    sys.path.insert(0, ROOT) if ROOT not in sys.path else None
    import residual_ref as rr
    from oracle import banet_oracle as orc, dense as odense, synth
    H, W, C = 20, 28, 6
    scenes = [synth.make_pair_scene(H, W, C, 0, [1], 41 + b, normalize_rays=False, dtype=np.float64) for b in range(2)]
    intr, levels = odense.batch_scene(scenes)
    R = np.stack([synth.rodrigues(np.array([0.02, -0.03, 0.05]) * (b + 1)) for b in range(2)])
    T = np.array([[0.05, -0.02, 0.04], [-0.3, 0.1, 0.02]]).reshape(2, 3, 1)
    ref = rr.dense_residual("legacy_lm", intr, levels[0], R, T, dtype=np.float64)
    a = odense.level_inputs(intr, levels[0], False, np.float64)
    avg, num_valid = orc.legacy_avg_residual(a["conv1"], a["conv2"], a["fx"], a["fy"], a["ox"], a["oy"], a["p"], a["D"], R, T)
    N = H * W
    count = N / num_valid[:, 0, 0]
    assert np.array_equal(ref["mask"].sum(-1)[:, 0], np.rint(count)) and np.all(0 < count) and np.all(count < N)
    want = avg[:, 0, :].sum(-1) * N / num_valid[:, 0, 0]
    np.testing.assert_allclose(ref["ab"].sum(-1)[:, 0], want, rtol=1e-12)
    assert ref["sq"].shape == (2, 1, N) and np.all(ref["sq"][~ref["mask"]] == 0) and np.all(ref["ab"][~ref["mask"]] == 0)
    assert ref["borderline"].shape == (2, 1)
