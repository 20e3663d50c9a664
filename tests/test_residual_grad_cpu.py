"""banet_ba_residual_grad_f32 on the host: the symbols, the struct layouts, the argument checks (decided before any launch), the
workspace arithmetic of DESIGN.md section 2.1, and the torch reference the GPU tests measure against (tests/residual_grad_ref.py):
its forward against the numpy reference of the forward op, its gradient against central differences.  No GPU: a valid call gets
past every check and fails for lack of a device."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HERE = os.path.dirname(os.path.abspath(__file__))
os.environ.setdefault("BANET_NUM_CUS", "256")
OK, INVALID, WORKSPACE, UNSUPPORTED, LAUNCH = 0, -1, -2, -3, -4
OVERWRITE, OVERWRITE_MAP = 1, 2

for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import test_residual_cpu as fwd  # noqa: E402  (the forward's host tests: its level builder, its valid and refused levels)


@pytest.fixture(scope="module")
def capi():
    from banet_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _capi


def test_the_symbols_are_exported_and_bound(capi):
    L = capi.lib()
    for name in ("banet_ba_residual_grad_f32", "banet_ba_residual_grad_workspace_bytes"):
        assert hasattr(L, name) and name in capi.EXPORTS, name
    res, args = capi.EXPORTS["banet_ba_residual_grad_f32"]
    assert res is ctypes.c_int and len(args) == 10
    assert args[4] == ctypes.POINTER(capi.ResidualGradIn) and args[5] == ctypes.POINTER(capi.ResidualGradOut)
    assert args[6] is ctypes.c_int and args[8] is ctypes.c_size_t
    res, args = capi.EXPORTS["banet_ba_residual_grad_workspace_bytes"]
    assert res is ctypes.c_size_t and args == [ctypes.POINTER(capi.Level), ctypes.c_int]
    assert L.banet_version() == 150                      # detected by its symbol: the version does not move
    from banet_amd import ops, dense, dense_train
    assert callable(ops.ba_residual_grad) and callable(ops.ba_residual_diff) and callable(dense_train.reprojection_loss)
    assert ops.ResidualGrad._fields == ("dsrc", "dtgt", "ddepth", "dbasis", "dWc", "dR", "dT")
    import inspect
    assert "differentiable" in inspect.signature(dense.DenseBA.residual).parameters


def test_struct_layouts_and_prototypes_match_the_header(capi, tmp_path):
    fin, fout = ("gsq", "gab", "gproj"), ("dsrc", "dtgt", "ddepth", "dbasis", "dWc", "dR", "dT")
    fmt = " ".join(["%zu"] * (2 + len(fin) + len(fout)))
    offs = ", ".join(["offsetof(banet_residual_grad_in_t, %s)" % f for f in fin] + ["offsetof(banet_residual_grad_out_t, %s)" % f for f in fout])
    # the two initialisers compile (-Werror) only if the header's prototypes are exactly these
    proto = tmp_path / "proto.c"
    proto.write_text('#include "banet_hip.h"\n'
                     'size_t (*q)(const banet_level_t*, int) = banet_ba_residual_grad_workspace_bytes;\n'
                     'int (*f)(const banet_level_t*, const float*, const float*, const float*, const banet_residual_grad_in_t*, '
                     'const banet_residual_grad_out_t*, int, void*, size_t, banet_stream_t) = banet_ba_residual_grad_f32;\n')
    subprocess.check_call(["gcc", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(proto), "-o", str(tmp_path / "proto.o")])
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "banet_hip.h"\n'
                    'int main(){printf("' + fmt + '\\n", sizeof(banet_residual_grad_in_t), sizeof(banet_residual_grad_out_t), ' + offs +
                    ');return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    I, O = capi.ResidualGradIn, capi.ResidualGradOut
    assert got == [ctypes.sizeof(I), ctypes.sizeof(O)] + [getattr(I, f).offset for f in fin] + [getattr(O, f).offset for f in fout]


def _gin(capi, gsq=4096, gab=4096, gproj=4096):
    g = capi.ResidualGradIn()
    g.gsq, g.gab, g.gproj = gsq, gab, gproj
    return g


def _gout(capi, **kw):
    o = capi.ResidualGradOut()
    for name in ("dsrc", "dtgt", "ddepth", "dbasis", "dWc", "dR", "dT"):
        setattr(o, name, kw.get(name, 4096))
    return o


def _query(capi, lv, want_dtgt):
    return capi.lib().banet_ba_residual_grad_workspace_bytes(ctypes.byref(lv), want_dtgt)


def _call(capi, lv, R=4096, T=4096, Wc=4096, gin=None, gout=None, no_g=False, no_out=False, flags=OVERWRITE | OVERWRITE_MAP, ws=1 << 20,
          ws_bytes=1 << 60):
    g = _gin(capi) if gin is None else gin
    o = _gout(capi, dtgt=None) if gout is None else gout
    return capi.lib().banet_ba_residual_grad_f32(ctypes.byref(lv) if lv is not None else None, R, T, Wc, None if no_g else ctypes.byref(g),
                                                 None if no_out else ctypes.byref(o), flags, ws, ws_bytes, None)


def test_null_arguments_and_bad_flags_are_invalid(capi):
    lv = fwd._level(capi)
    assert _call(capi, None) == INVALID
    assert _call(capi, lv, R=None) == INVALID and _call(capi, lv, T=None) == INVALID
    assert _call(capi, lv, Wc=None) == INVALID                                   # K > 0 needs the coefficients
    assert _call(capi, lv, no_g=True) == INVALID and _call(capi, lv, no_out=True) == INVALID
    assert _call(capi, lv, gin=_gin(capi, None, None, None)) == INVALID          # at least one upstream gradient
    for bad in (4, 8, 16, 1 << 4, 1 << 30, -1):
        assert _call(capi, lv, flags=bad) == INVALID, bad
        assert _call(capi, lv, flags=bad | OVERWRITE) == INVALID, bad


def test_workspace_is_checked_before_any_launch(capi):
    for kw, want_dtgt in ((dict(), 1), (dict(), 0), (dict(C=20, K=5, H=33, W=47), 1), (dict(C=128, K=8, dense=0, N=100), 0)):
        lv = fwd._level(capi, **kw)
        need = _query(capi, lv, want_dtgt)
        assert need > 0 and need % 256 == 0
        o = _gout(capi) if want_dtgt else _gout(capi, dtgt=None)
        assert _call(capi, lv, gout=o, ws=None) == WORKSPACE
        assert _call(capi, lv, gout=o, ws=(1 << 20) + 16) == WORKSPACE           # misaligned
        assert _call(capi, lv, gout=o, ws_bytes=need - 1) == WORKSPACE           # one byte short
    # a level the forward refuses is refused first, whatever the workspace
    assert _call(capi, fwd._level(capi, C=257), ws=None) == UNSUPPORTED


def test_dtgt_on_a_3c_level_is_unsupported_and_the_rest_is_not(capi):
    lv = fwd._level(capi, C=128, K=8, dense=0, N=100)                            # the sparse layout: tgt_has_grad = 1
    assert _query(capi, lv, 1) == 0 and _query(capi, lv, 0) > 0
    assert _call(capi, lv, gout=_gout(capi)) == UNSUPPORTED
    # beyond the resampler gradient's limit B pairs H W C < 2^32 (a dense C-channel level): the same
    big = fwd._level(capi, B=64, H=1024, W=1024, C=128, K=8)
    assert _query(capi, big, 1) == 0 and _query(capi, big, 0) > 0
    assert _call(capi, big, gout=_gout(capi)) == UNSUPPORTED


def _align(n):
    return (n + 255) // 256 * 256


@pytest.mark.parametrize("kw", [dict(C=20, K=5, H=33, W=47), dict(C=128, K=8, B=3), dict(variant=2, C=3, K=0, H=5, W=7),
                                dict(C=128, K=128, pairs=3, H=16, W=24), dict(C=128, K=128, B=32, H=480, W=640),
                                dict(C=16, K=4, pairs=40, H=8, W=8), dict(C=128, K=8, dense=0, N=100)])
def test_workspace_query_is_the_documented_arithmetic(capi, kw):
    """partial rows [B][G][12 pairs + K] with G = ceil(ceil(N / 8) / 64) workgroups of 512 points; the pose
    slots [B][G][16][pairs][12] (doubles) only for pairs > 32; with dtgt the e rows [B pairs][N][C], the projections [B pairs][N][2] and the
    resampler gradient's own workspace for a batch of B pairs; every region rounded up to 256 bytes"""
    lv = fwd._level(capi, **kw)
    B, N, C, K, H, W, pairs = lv.B, lv.N, lv.C, lv.K, lv.H, lv.W, max(lv.pairs, 1)
    G = (((N + 7) // 8) + 63) // 64
    base = _align(B * G * (12 * pairs + K) * 4) + (_align(B * G * 16 * pairs * 12 * 8) if pairs > 32 else 0)
    assert _query(capi, lv, 0) == base
    if lv.tgt_has_grad:
        assert _query(capi, lv, 1) == 0
    else:
        rg = capi.lib().banet_resample_grad_workspace_bytes(B * pairs, N, C, H, W, 1)
        assert rg > 0
        assert _query(capi, lv, 1) == base + _align(B * pairs * N * C * 4) + _align(B * pairs * N * 8) + _align(rg)


def test_invalid_levels_query_zero(capi):
    for name, (kw, _) in fwd.REFUSED.items():
        kw = dict(kw)
        policy = kw.pop("policy", 0)
        lv = fwd._level(capi, **kw)
        lv.policy = policy
        assert _query(capi, lv, 0) == 0 and _query(capi, lv, 1) == 0, name
    assert capi.lib().banet_ba_residual_grad_workspace_bytes(None, 0) == 0


def probe_without_a_device():
    """runs in a child process that sees no device (the pointers are made up): the codes of every call that gets as far as a launch"""
    from banet_amd import _capi as capi
    out = {"valid": [], "valid_subset": [], "refused": {}}
    for kw in fwd.VALID:
        lv = fwd._level(capi, **kw)
        dt = None if lv.tgt_has_grad else 4096
        need = _query(capi, lv, 1 if dt else 0)
        out["valid"].append(_call(capi, lv, gout=_gout(capi, dtgt=dt), ws_bytes=need))      # the exact size is accepted
        lv.flags, lv.policy = capi.DEV_FORCE_STRIP_GATHER, capi.POLICY_BATCH_INVARIANT        # accepted and ignored, as the forward
        out["valid_subset"].append(_call(capi, lv, Wc=4096 if lv.K > 0 else None, gin=_gin(capi, None, 4096, None),
                                         gout=_gout(capi, dsrc=None, dtgt=None, dbasis=None, dWc=None, dR=None), flags=0))
    for name, (kw, _) in fwd.REFUSED.items():
        kw = dict(kw)
        policy = kw.pop("policy", 0)
        lv = fwd._level(capi, **kw)
        lv.policy = policy
        out["refused"][name] = [_call(capi, lv), fwd._call(capi, lv)]
    return out


@pytest.fixture(scope="module")
def probe(capi):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="", BANET_NUM_CUS="256")
    code = ("import sys, json; sys.path[:0] = [%r, %r]; import test_residual_grad_cpu as t; print('PROBE ' + json.dumps(t.probe_without_a_device()))"
            % (ROOT, HERE))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("PROBE ")][-1][len("PROBE "):])


def test_a_level_the_forward_refuses_gets_the_forward_s_code(probe):
    for name, (_, want) in fwd.REFUSED.items():
        got, forward_code = probe["refused"][name]
        assert got == want == forward_code, (name, got, forward_code)


def test_a_valid_level_fails_for_lack_of_a_device_only(probe):
    assert probe["valid"] == [LAUNCH] * len(fwd.VALID), probe["valid"]
    assert probe["valid_subset"] == [LAUNCH] * len(fwd.VALID), probe["valid_subset"]


def test_diff_refuses_a_3c_target_map_that_requires_grad(capi):
    import torch
    from banet_amd import ops
    fake = type("P", (), {})()
    fake.c, fake.K = fwd._level(capi, C=128, K=8, dense=0, N=100), 8
    fake.keep = [torch.zeros(1), torch.zeros(1, requires_grad=True), torch.zeros(1), torch.zeros(1)]
    with pytest.raises(capi.BanetError):
        ops.ba_residual_diff(fake, torch.eye(3)[None], torch.zeros(1, 3, 1), torch.zeros(1, 8, 1))


# ---------------------------------------------------------------------------------------------------------------------
# the torch reference
# ---------------------------------------------------------------------------------------------------------------------
def _scenes():
    """two dense scenes (bundle with a basis, two windows; legacy without, rays not normalised) and one sparse scene on the 3C map:
    (name, variant, a, conv2s, R, T, Wc, numpy maps of tests/residual_ref.py in float64)"""
    import residual_ref as rr
    from oracle import banet_oracle as orc, dense as odense, synth
    out = []
    for name, variant, K, norm, seed in (("dense bundle", "bundle", 4, True, 31), ("dense legacy", "legacy_lm", 0, False, 41)):
        H, W, C, B = 14, 18, 6, 2
        scenes = [synth.make_pair_scene(H, W, C, K, [1], seed + b, normalize_rays=norm, dtype=np.float64) for b in range(B)]
        intr, levels = odense.batch_scene(scenes)
        R = np.stack([synth.rodrigues(np.array([0.02, -0.03, 0.05]) * (b + 1)) for b in range(B)]).reshape(B, 1, 3, 3)
        T = np.array([[0.05, -0.02, 0.04], [-0.3, 0.1, 0.02]]).reshape(B, 1, 3, 1)
        Wc = np.stack([np.asarray(s["W_gt"]) * 0.5 for s in scenes]).reshape(B, K, 1) if K else None
        a, conv2s = rr.dense_inputs(variant, intr, levels[0], np.float64)
        out.append((name, variant, a, conv2s, R, T, Wc, rr.residual_maps(variant, a, conv2s, R, T, Wc, np.float64)))
    rng = np.random.RandomState(5)
    B, N, H, W, C, K = 2, 60, 10, 13, 5, 3
    pts = np.stack([rng.uniform(1.0, W - 2.0, (B, N)), rng.uniform(1.0, H - 2.0, (B, N))], -1)
    fx, fy, ox, oy = np.full((B, N), 0.8 * W), np.full((B, N), 0.8 * W), np.full((B, N), W / 2.0), np.full((B, N), H / 2.0)
    sp = dict(conv1=rng.standard_normal((B, N, C)), conv2=orc.target_map(rng.standard_normal((B, H, W, C)))[:, None],
              p=orc.compute_coordinates(pts, fx, fy, ox, oy, True), fx=fx, fy=fy, ox=ox, oy=oy, D=rng.uniform(2.0, 3.5, (B, N, 1)),
              Bs=rng.standard_normal((B, N, K)) * 0.3)
    Wc = rng.standard_normal((B, K, 1)) * 0.2
    R = np.stack([synth.rodrigues(rng.uniform(-1, 1, 3) * 0.08) for _ in range(B)]).reshape(B, 1, 3, 3)
    T = rng.uniform(-1, 1, (B, 1, 3, 1)) * 0.4
    a, conv2s = rr.sparse_inputs(sp, np.float64)
    out.append(("sparse bundle", "bundle", a, conv2s, R, T, Wc, rr.residual_maps("bundle", a, conv2s, R, T, Wc, np.float64)))
    return out


@pytest.fixture(scope="module")
def scenes():
    return _scenes()


def test_the_torch_forward_equals_the_numpy_reference(scenes):
    import torch
    import residual_grad_ref as rg
    for name, variant, a, conv2s, R, T, Wc, want in scenes:
        with torch.no_grad():
            got = rg.forward(rg.inputs_of(a, conv2s, R, T, Wc, torch.float64))
        mask = got["mask"].numpy()
        assert np.array_equal(mask, want["mask"]) and 0 < mask.sum() < mask.size, name      # some inside, some outside
        for key in ("sq", "ab"):
            np.testing.assert_allclose(got[key].numpy(), want[key], rtol=1e-12, atol=1e-12 * want[key].max(), err_msg="%s %s" % (name, key))
        proj = got["proj"].numpy()
        np.testing.assert_allclose(proj[..., 0][mask], want["px"][mask], rtol=1e-12, err_msg=name)
        np.testing.assert_allclose(proj[..., 1][mask], want["py"][mask], rtol=1e-12, err_msg=name)


def test_the_reference_gradient_against_central_differences(scenes):
    """float64, the dense bundle scene: dL/dT, dL/dWc and dL/d(one source channel) against (L(v + h) - L(v - h)) / 2h, h = 1e-6.
    L is smooth between the floor's and the sign's switches: the points within 1e-4 of one (in pixels / of the largest |d|) get a zero
    upstream gradient, so no evaluation crosses a switch.  Central-difference error: h^2 |L'''| / 6 + 2^-52 |L| / h ~ 1e-9 |L| in
    all, against gradients of the order of |L|: 1e-6 relative to the largest entry is three orders above it."""
    import torch
    import residual_grad_ref as rg
    name, variant, a, conv2s, R, T, Wc, _ = scenes[0]
    rng = np.random.RandomState(3)
    B, pairs, N = len(R), 1, a["conv1"].shape[1]
    with torch.no_grad():
        f = rg.forward(rg.inputs_of(a, conv2s, R, T, Wc, torch.float64))
    proj, d = f["proj"].numpy(), np.abs(f["d"].numpy())
    risky = (np.abs(proj - np.rint(proj)) < 1e-4).any(-1) | (d < 1e-4 * d.max()).any(-1)
    assert risky[f["mask"].numpy()].mean() < 0.1
    keep = (~risky).astype(np.float64)
    gsq, gab = rng.uniform(0.5, 1.5, (B, pairs, N)) * keep, rng.uniform(0.5, 1.5, (B, pairs, N)) * keep
    gproj = rng.standard_normal((B, pairs, N, 2)) * keep[..., None]
    g = rg.gradients(a, conv2s, R, T, Wc, gsq, gab, gproj)

    def L_at(**over):
        t = rg.inputs_of(a, conv2s, over.get("R", R), over.get("T", T), over.get("Wc", Wc), torch.float64)
        if "conv1" in over:
            t["conv1"] = torch.from_numpy(over["conv1"])
        with torch.no_grad():
            return float(rg.loss(t, gsq, gab, gproj)[0])
    h = 1e-6
    checks = []
    for b in range(B):
        for i in range(3):
            Tp, Tm = T.copy(), T.copy()
            Tp[b, 0, i, 0] += h
            Tm[b, 0, i, 0] -= h
            checks.append(("dT", (L_at(T=Tp) - L_at(T=Tm)) / (2 * h), g["dT"][b, 0, i], np.abs(g["dT"]).max()))
        for k in range(Wc.shape[1]):
            Wp, Wm = Wc.copy(), Wc.copy()
            Wp[b, k, 0] += h
            Wm[b, k, 0] -= h
            checks.append(("dWc", (L_at(Wc=Wp) - L_at(Wc=Wm)) / (2 * h), g["dWc"][b, k], np.abs(g["dWc"]).max()))
    inside = np.argwhere(f["mask"].numpy()[:, 0] & ~risky[:, 0])
    for b, n in inside[:: max(1, len(inside) // 6)]:
        c = 2
        Sp, Sm = a["conv1"].copy(), a["conv1"].copy()
        Sp[b, n, c] += h
        Sm[b, n, c] -= h
        checks.append(("dsrc", (L_at(conv1=Sp) - L_at(conv1=Sm)) / (2 * h), g["dsrc"][b, n, c], np.abs(g["dsrc"]).max()))
    assert len(checks) > 12
    for what, fd, an, scale in checks:
        assert scale > 0 and abs(fd - an) <= 1e-6 * scale, (what, fd, an, scale)
