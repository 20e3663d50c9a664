"""CPU-side checks of the dense level preparation (banet_grid_resample_f32 / banet_grid_resample_grad_f32, banet_amd/dense_prep.py,
BundleNet.BundleResizeDense / CameraResizeDense): exports, the struct's layout, argument validation, the candidate ranges of the
adjoint against a brute-forced forward, and the level geometry -- all without a GPU."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ("banet_grid_resample_f32", "banet_grid_resample_grad_f32")
OK, INVALID, WORKSPACE, UNSUPPORTED = 0, -1, -2, -3


@pytest.fixture(scope="module")
def capi():
    sys.path.insert(0, ROOT)
    from banet_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _capi


def test_new_symbols_are_exported_and_bound(capi):
    L = capi.lib()
    for n in NEW:
        assert hasattr(L, n) and n in capi.EXPORTS, n
    assert L.banet_version() == 150


def test_grid_level_layout_matches_the_ctypes_mirror(capi, tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    fields = [n for n, _ in capi.GridLevel._fields_]
    exprs = ["sizeof(banet_grid_level_t)"] + ["offsetof(banet_grid_level_t, %s)" % n for n in fields]
    prog = tmp_path / "l.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "banet_hip.h"\nint main(void){'
                    + "".join('printf("%%zu\\n", %s);' % e for e in exprs) + "return 0;}\n")
    exe = tmp_path / "l"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(capi.GridLevel)] + [getattr(capi.GridLevel, n).offset for n in fields]


def test_c99_unit_calls_the_new_entry_points(capi, tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "g.c"
    src.write_text('#include <stdio.h>\n#include "banet_hip.h"\n'
                   'int main(void){ static float buf[64]; banet_grid_level_t lv[2] = {{4, 4, 1.f, 1.f, 0.f, 0.f, buf}, {2, 2, 2.f, 2.f, 0.f, 0.f, buf}};\n'
                   '  if (banet_grid_resample_f32(0, 1, 4, 4, 1, BANET_RESAMPLE_CLAMP, lv, 2, 0) != BANET_ERR_INVALID_ARG) return 1;\n'
                   '  if (banet_grid_resample_f32(buf, 1, 4, 4, 1, BANET_RESAMPLE_CLAMP, lv, 9, 0) != BANET_ERR_UNSUPPORTED) return 2;\n'
                   '  if (banet_grid_resample_grad_f32(buf, 1, 4, 4, 1, BANET_RESAMPLE_ZERO_PAD, 0, 2, BANET_ADJOINT_OVERWRITE, 0) != BANET_ERR_INVALID_ARG) return 3;\n'
                   '  if (banet_grid_resample_grad_f32(buf, 1, 4, 4, 1, BANET_RESAMPLE_ZERO_PAD, lv, 2, 2, 0) != BANET_ERR_INVALID_ARG) return 4;\n'
                   '  printf("grid c-abi ok\\n"); return 0; }\n')
    libdir = os.path.join(ROOT, "banet_amd", "lib")
    exe = tmp_path / "g"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-lbanet_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    assert subprocess.check_output([str(exe)]).decode().startswith("grid c-abi ok")


def _levels(capi, specs, p):
    tb = (capi.GridLevel * max(len(specs), 1))()
    for e, (Ho, Wo, sx, sy, ox, oy) in zip(tb, specs):
        e.Ho, e.Wo, e.sx, e.sy, e.ox, e.oy, e.out = Ho, Wo, sx, sy, ox, oy, p
    return tb


def test_argument_errors_without_gpu(capi):
    """every check happens before the launch: the stand-in pointer is never dereferenced"""
    L = capi.lib()
    host = ctypes.create_string_buffer(256)
    p = ctypes.c_void_p(ctypes.addressof(host))
    good = [(10, 14, 0.5, 0.5, 0.0, 0.0), (5, 7, 1.0, 1.0, 0.0, 0.0)]

    def fwd(data=p, B=2, H=5, W=7, C=3, mode=1, specs=good, n=None, out=p, tb=True):
        t = _levels(capi, specs, out) if tb else None
        return L.banet_grid_resample_f32(data, B, H, W, C, mode, t, len(specs) if n is None else n, None)

    def bwd(data=p, B=2, H=5, W=7, C=3, mode=1, specs=good, n=None, out=p, tb=True, flags=1):
        t = _levels(capi, specs, out) if tb else None
        return L.banet_grid_resample_grad_f32(data, B, H, W, C, mode, t, len(specs) if n is None else n, flags, None)

    for call in (fwd, bwd):
        assert call(data=None) == INVALID and call(tb=False) == INVALID and call(out=None) == INVALID     # NULL pointers
        assert call(specs=[], n=0) == INVALID                                                              # n_levels 0
        assert call(specs=good * 5, n=9) == UNSUPPORTED                                                    # n_levels 9
        assert call(specs=[(5, 7, 0.2, 0.2, 0.0, 0.0)]) == UNSUPPORTED                                     # step 0.2
        assert call(specs=[(1, 1, 65.0, 65.0, 0.0, 0.0)]) == UNSUPPORTED                                   # step 65
        assert call(specs=[(5, 7, 1.0, 0.2, 0.0, 0.0)]) == UNSUPPORTED and call(specs=[(1, 1, 65.0, 1.0, 0.0, 0.0)]) == UNSUPPORTED
        assert call(specs=[(5, 9, 1.0, 1.0, 0.0, 0.0)]) == UNSUPPORTED                                     # last x = 8 > W = 7
        assert call(specs=[(7, 7, 1.0, 1.0, 0.0, 0.0)]) == UNSUPPORTED                                     # last y = 6 > H = 5
        assert call(specs=[(5, 7, 1.0, 1.0, -1.5, 0.0)]) == UNSUPPORTED                                    # first x = -1.5 < -1
        assert call(C=257) == UNSUPPORTED
        assert call(H=1 << 10, W=1 << 10, C=1 << 10) == UNSUPPORTED                                        # (C first) ...
        assert call(H=1 << 14, W=1 << 14, C=4, specs=[(4, 4, 1.0, 1.0, 0.0, 0.0)]) == UNSUPPORTED          # H W C = 2^30
        assert call(H=1 << 14, W=1 << 14, C=1, specs=[(1 << 15, 1 << 15, 0.5, 0.5, 0.0, 0.0)]) == UNSUPPORTED   # Ho Wo C = 2^30
        for k in ("B", "H", "W", "C"):
            assert call(**{k: 0}) == INVALID and call(**{k: -2}) == INVALID, k
        assert call(mode=2) == INVALID and call(mode=-1) == INVALID
        assert call(specs=[(0, 7, 1.0, 1.0, 0.0, 0.0)]) == INVALID and call(specs=[(5, -1, 1.0, 1.0, 0.0, 0.0)]) == INVALID
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            assert call(specs=[(5, 7, bad, 1.0, 0.0, 0.0)]) == INVALID and call(specs=[(5, 7, 1.0, bad, 0.0, 0.0)]) == INVALID, bad
        for bad in (float("nan"), float("inf"), -float("inf")):
            assert call(specs=[(5, 7, 1.0, 1.0, bad, 0.0)]) == INVALID and call(specs=[(5, 7, 1.0, 1.0, 0.0, bad)]) == INVALID, bad
    assert bwd(flags=2) == INVALID and bwd(flags=1 | 4) == INVALID


# ---- the candidate ranges of the adjoint -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    out = tmp_path_factory.mktemp("grid") / "libgrid_plan_host.so"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(out),
                           os.path.join(ROOT, "tests", "native", "grid_plan_host.cpp")])
    L = ctypes.CDLL(str(out))
    L.banet_test_grid_coord.restype = ctypes.c_float
    L.banet_test_grid_coord.argtypes = [ctypes.c_int, ctypes.c_float, ctypes.c_float]
    L.banet_test_grid_ranges.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.POINTER(ctypes.c_int32),
                                         ctypes.POINTER(ctypes.c_int32)]
    L.banet_test_grid_check_axis.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float]
    return L


def _coords(n, s, o):
    """the documented coordinate: float32 j * s + o, two roundings"""
    return (np.arange(n, dtype=np.float32) * np.float32(s)).astype(np.float32) + np.float32(o)


def _taps(x, W, mode):
    """texels the forward's two taps along one axis touch (brute force, float32), per mode"""
    out = []
    for v in x:
        if mode == 0:                                  # zero padding: sampled iff -1 < x < W, taps floor and floor + 1 inside the map
            if not (v > np.float32(-1.0) and v < np.float32(W)):
                out.append(set())
                continue
            f = int(np.floor(v))
            out.append({t for t in (f, f + 1) if 0 <= t <= W - 1})
        else:                                          # clamp: both taps clamped into the map
            f = int(np.floor(v))
            out.append({min(max(f, 0), W - 1), min(max(f + 1, 0), W - 1)})
    return out


def test_coordinate_is_numpy_float32(plan):
    for s in (0.25, np.float32(1.0 / 3.0), 0.75, 1.5):
        for o in (-1.0, -0.5, 0.0, 0.3):
            want = _coords(50, s, o)
            got = np.array([plan.banet_test_grid_coord(j, float(np.float32(s)), float(np.float32(o))) for j in range(50)], np.float32)
            assert np.array_equal(got, want), (s, o)


def test_candidate_ranges_contain_every_contributor(plan):
    steps = [0.25, float(np.float32(1.0 / 3.0)), 0.5, 0.75, 1.0, 1.5, 2.0, 4.0]
    offsets = [-1.0, -0.5, 0.0, float(np.float32(0.3))]
    swept = 0
    for W in range(1, 10):
        lo, hi = (ctypes.c_int32 * W)(), (ctypes.c_int32 * W)()
        for Wo in range(1, 21):
            for s in steps:
                for o in offsets:
                    x = _coords(Wo, s, o)
                    supported = x[0] >= -1.0 and x[-1] <= W
                    assert (plan.banet_test_grid_check_axis(Wo, W, s, o) == 0) == supported, (W, Wo, s, o)
                    if not supported:
                        continue
                    swept += 1
                    plan.banet_test_grid_ranges(W, Wo, s, o, lo, hi)
                    for mode in (0, 1):
                        taps = _taps(x, W, mode)
                        for X in range(W):
                            for j in range(Wo):
                                if X in taps[j]:
                                    assert lo[X] <= j <= hi[X], (W, Wo, s, o, mode, X, j, lo[X], hi[X])
                    for X in range(W):
                        assert 0 <= lo[X] and hi[X] <= Wo - 1 and hi[X] - lo[X] + 1 <= 2.0 / s + 4.0, (W, Wo, s, o, X, lo[X], hi[X])
    assert swept > 1000


# ---- level geometry ----------------------------------------------------------------------------------------------------------------
def test_grid_levels_reference_geometry(capi):
    from banet_amd import dense_prep
    # bundlenet.py:332-399: levels 2, 3 (scales 2, 1) of a 64 x 80 finest level, depth / basis at 32 x 40
    got = dense_prep.grid_levels(32, 40, [(32, 40), (64, 80)], [2, 1], 2)
    assert got == [(32, 40, 1.0, 1.0, 0.0, 0.0), (64, 80, 0.5, 0.5, 0.0, 0.0)]
    assert dense_prep.is_identity(32, 40, got[0]) and not dense_prep.is_identity(32, 40, got[1])


def test_grid_levels_five_level_pyramid(capi):
    from banet_amd import dense_prep
    shapes = [(30, 40), (60, 80), (120, 160), (240, 320), (480, 640)]
    got = dense_prep.grid_levels(240, 320, shapes, [16, 8, 4, 2, 1], 2)
    assert [g[2] for g in got] == [8.0, 4.0, 2.0, 1.0, 0.5] and [g[3] for g in got] == [8.0, 4.0, 2.0, 1.0, 0.5]
    assert [g[:2] for g in got] == shapes and all(g[4:] == (0.0, 0.0) for g in got)


def test_grid_levels_error_cases(capi):
    from banet_amd import dense_prep
    with pytest.raises(ValueError):
        dense_prep.grid_levels(8, 8, [(8, 8)], [0.25], 2)            # step 1/8
    with pytest.raises(ValueError):
        dense_prep.grid_levels(8, 8, [(1, 1)], [256], 2)             # step 128
    with pytest.raises(ValueError):
        dense_prep.grid_levels(8, 8, [(8, 10)], [2], 2)              # last x = 9 > W
    with pytest.raises(ValueError):
        dense_prep.grid_levels(8, 8, [(20, 16)], [1], 2)             # last y = 9.5 > H
    with pytest.raises(ValueError):
        dense_prep.grid_levels(8, 8, [(8, 8)], [2, 1], 2)            # shapes and scales disagree
    with pytest.raises(ValueError):
        dense_prep.grid_levels(8, 8, [(1, 1)] * 9, [2] * 9, 2)       # nine levels
    with pytest.raises(ValueError):
        dense_prep.grid_levels(8, 8, [], [], 2)
    with pytest.raises(ValueError):
        dense_prep.grid_levels(8, 8, [(8, 8)], [2], 0)
    assert dense_prep.grid_levels(8, 8, [(17, 17)], [1], 2)[0][2] == 0.5   # last coordinate = 8 = W: still supported


def test_dense_drivers_raise_on_cpu_tensors(capi):
    from banet_amd import bundlenet, dense_prep
    net = bundlenet.BundleNet(lambda_weights={str(l): bundlenet.he_normal_lambda_weights(4, l) for l in range(4)})
    layers = [torch.zeros(2, 2 * 2 ** l, 3 * 2 ** l, 4) for l in range(4)]
    intr = torch.ones(2, 4, 1)
    with pytest.raises(capi.BanetError):
        net.BundleResizeDense(intr, layers, torch.zeros(2, 8, 12, 3), torch.ones(2, 8, 12))
    with pytest.raises(capi.BanetError):
        net.CameraResizeDense(intr, layers, torch.ones(2, 8, 12))
    with pytest.raises(capi.BanetError):
        dense_prep.grid_pyramid(torch.zeros(2, 8, 12, 3), [(16, 24, 0.5, 0.5, 0.0, 0.0)])
    with pytest.raises(ValueError):
        net.BundleResizeDense(intr, layers, torch.zeros(2, 8, 12, 3), torch.ones(2, 8, 12), border="mirror")
