"""CPU-side checks of the preparation gradients (banet_resample_grad_f32 / banet_depth_output_grad_f32, torch.ops.banet.resampler /
target_map / depth_output and their *_grad ops, BundleNet(prep_graph=...)): exports, argument validation and shape inference,
all without a GPU."""
import ctypes
import os
import shutil
import subprocess
import sys

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ("banet_resample_grad_workspace_bytes", "banet_resample_grad_f32", "banet_depth_output_grad_workspace_bytes",
       "banet_depth_output_grad_f32")
OK, INVALID, WORKSPACE, UNSUPPORTED = 0, -1, -2, -3


@pytest.fixture(scope="module")
def capi():
    sys.path.insert(0, ROOT)
    from banet_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _capi


class _Ws:
    """a host buffer posing as a 256-byte aligned workspace (validation returns before any launch)"""

    def __init__(self, nbytes):
        self.buf = ctypes.create_string_buffer(nbytes + 512)
        self.addr = (ctypes.addressof(self.buf) + 255) // 256 * 256


def test_new_symbols_are_exported_and_bound(capi):
    L = capi.lib()
    for n in NEW:
        assert hasattr(L, n) and n in capi.EXPORTS, n
    assert L.banet_version() == 150


def test_resample_grad_workspace_query(capi):
    L = capi.lib()
    for mode in (0, 1):
        nb = L.banet_resample_grad_workspace_bytes(2, 4096, 128, 64, 80, mode)
        assert nb > 0 and nb % 256 == 0
        assert L.banet_resample_grad_workspace_bytes(2, 4096, 256, 64, 80, mode) > 0
    assert L.banet_resample_grad_workspace_bytes(2, 4096, 257, 64, 80, 0) == 0               # C > 256
    assert L.banet_resample_grad_workspace_bytes(16, 16, 256, 1024, 1024, 0) == 0            # B H W C >= 2^32
    for bad in ((0, 4, 3, 8, 8, 0), (1, 0, 3, 8, 8, 0), (1, 4, 0, 8, 8, 0), (1, 4, 3, 0, 8, 0), (1, 4, 3, 8, -1, 0),
                (1, 4, 3, 8, 8, 2), (1, 4, 3, 8, 8, -1)):
        assert L.banet_resample_grad_workspace_bytes(*bad) == 0, bad
    assert L.banet_depth_output_grad_workspace_bytes(2, 100, 16) > 0
    for bad in ((0, 100, 16), (2, 0, 16), (2, 100, 0)):
        assert L.banet_depth_output_grad_workspace_bytes(*bad) == 0, bad


def test_resample_grad_argument_errors_without_gpu(capi):
    L = capi.lib()
    B, N, C, H, W = 2, 64, 8, 6, 7
    nb = L.banet_resample_grad_workspace_bytes(B, N, C, H, W, 0)
    ws = _Ws(nb)
    p = ctypes.c_void_p(ws.addr)          # a non-null stand-in pointer: validation never dereferences it
    call = lambda data=p, warp=p, gout=p, ddata=p, dwarp=p, B=B, N=N, C=C, H=H, W=W, mode=0, flags=1, w=p, wb=nb: \
        L.banet_resample_grad_f32(data, warp, gout, ddata, dwarp, B, N, C, H, W, mode, flags, w, wb, None)   # noqa: E731
    assert call(data=None) == INVALID and call(warp=None) == INVALID and call(gout=None) == INVALID
    for k in ("B", "N", "C", "H", "W"):
        assert call(**{k: 0}) == INVALID, k
        assert call(**{k: -3}) == INVALID, k
    assert call(mode=2) == INVALID and call(mode=-1) == INVALID
    assert call(flags=2) == INVALID and call(flags=1 | 16) == INVALID
    assert call(C=257) == UNSUPPORTED
    assert call(w=None) == WORKSPACE
    assert call(wb=nb - 1) == WORKSPACE
    assert call(w=ctypes.c_void_p(ws.addr + 4)) == WORKSPACE


def test_depth_output_grad_argument_errors_without_gpu(capi):
    L = capi.lib()
    B, N, K = 2, 100, 16
    nb = L.banet_depth_output_grad_workspace_bytes(B, N, K)
    ws = _Ws(nb)
    p = ctypes.c_void_p(ws.addr)
    call = lambda basis=p, Wc=p, gout=p, B=B, N=N, K=K, flags=0, w=p, wb=nb: \
        L.banet_depth_output_grad_f32(basis, Wc, gout, p, p, p, B, N, K, flags, w, wb, None)   # noqa: E731
    assert call(basis=None) == INVALID and call(Wc=None) == INVALID and call(gout=None) == INVALID
    for k in ("B", "N", "K"):
        assert call(**{k: 0}) == INVALID, k
    assert call(flags=4) == INVALID
    assert call(w=None) == WORKSPACE and call(wb=nb - 1) == WORKSPACE and call(w=ctypes.c_void_p(ws.addr + 8)) == WORKSPACE


def test_c99_unit_calls_the_new_entry_points(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "g.c"
    src.write_text('#include <stdio.h>\n#include "banet_hip.h"\n'
                   'int main(void){ static char ws[4096]; float* f = (float*)ws;\n'
                   '  size_t nb = banet_resample_grad_workspace_bytes(1, 4, 3, 8, 8, BANET_RESAMPLE_ZERO_PAD);\n'
                   '  if (nb == 0 || banet_resample_grad_workspace_bytes(1, 4, 300, 8, 8, BANET_RESAMPLE_CLAMP) != 0) return 1;\n'
                   '  if (banet_resample_grad_f32(0, f, f, f, f, 1, 4, 3, 8, 8, 0, BANET_ADJOINT_OVERWRITE, ws, nb, 0) != BANET_ERR_INVALID_ARG) return 2;\n'
                   '  if (banet_resample_grad_f32(f, f, f, f, f, 1, 4, 3, 8, 8, 5, 0, ws, nb, 0) != BANET_ERR_INVALID_ARG) return 3;\n'
                   '  if (banet_resample_grad_f32(f, f, f, f, f, 1, 4, 3, 8, 8, 0, 0, 0, nb, 0) != BANET_ERR_WORKSPACE) return 4;\n'
                   '  if (banet_resample_grad_f32(f, f, f, f, f, 1, 4, 300, 8, 8, 0, 0, ws, nb, 0) != BANET_ERR_UNSUPPORTED) return 5;\n'
                   '  if (banet_depth_output_grad_workspace_bytes(1, 4, 0) != 0) return 6;\n'
                   '  if (banet_depth_output_grad_f32(f, f, 0, 0, 0, 0, 1, 4, 2, 0, ws, 4096, 0) != BANET_ERR_INVALID_ARG) return 7;\n'
                   '  if (banet_depth_output_grad_f32(f, f, f, 0, 0, 0, 1, 4, 2, 0, 0, 0, 0) != BANET_ERR_WORKSPACE) return 8;\n'
                   '  printf("prep-grad c-abi ok\\n"); return 0; }\n')
    libdir = os.path.join(ROOT, "banet_amd", "lib")
    exe = tmp_path / "g"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-lbanet_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    assert subprocess.check_output([str(exe)]).decode().startswith("prep-grad c-abi ok")


def test_prep_ops_infer_shapes_on_meta_tensors(capi):
    from banet_amd import prep_grad  # noqa: F401 (registers the ops)
    m = lambda *s: torch.empty(*s, device="meta")   # noqa: E731
    assert tuple(torch.ops.banet.resampler(m(2, 6, 7, 5), m(2, 11, 2), False).shape) == (2, 11, 5)
    dd, dw = torch.ops.banet.resampler_grad(m(2, 6, 7, 5), m(2, 11, 2), m(2, 11, 5), True)
    assert tuple(dd.shape) == (2, 6, 7, 5) and tuple(dw.shape) == (2, 11, 2)
    assert tuple(torch.ops.banet.target_map(m(3, 6, 7, 4)).shape) == (3, 6, 7, 12)
    assert tuple(torch.ops.banet.target_map_grad(m(3, 6, 7, 12)).shape) == (3, 6, 7, 4)
    assert tuple(torch.ops.banet.depth_output(m(2, 6, 7), m(2, 6, 7, 3), m(2, 3, 1)).shape) == (2, 6, 7)
    gi, gb, gw = torch.ops.banet.depth_output_grad(m(2, 6, 7, 3), m(2, 3, 1), m(2, 6, 7))
    assert tuple(gi.shape) == (2, 6, 7) and tuple(gb.shape) == (2, 6, 7, 3) and tuple(gw.shape) == (2, 3, 1)


def test_prep_ops_raise_on_cpu_tensors(capi):
    from banet_amd import prep_grad  # noqa: F401
    with pytest.raises(NotImplementedError):
        torch.ops.banet.resampler(torch.zeros(1, 4, 4, 2), torch.zeros(1, 3, 2), False)
    with pytest.raises(NotImplementedError):
        torch.ops.banet.resampler_grad(torch.zeros(1, 4, 4, 2), torch.zeros(1, 3, 2), torch.zeros(1, 3, 2), False)
    with pytest.raises(NotImplementedError):
        torch.ops.banet.target_map(torch.zeros(1, 4, 4, 2))
    with pytest.raises(NotImplementedError):
        torch.ops.banet.target_map_grad(torch.zeros(1, 4, 4, 6))
    with pytest.raises(NotImplementedError):
        torch.ops.banet.depth_output(torch.zeros(1, 4), torch.zeros(1, 4, 2), torch.zeros(1, 2, 1))
    with pytest.raises(NotImplementedError):
        torch.ops.banet.depth_output_grad(torch.zeros(1, 4, 2), torch.zeros(1, 2, 1), torch.zeros(1, 4))


def test_bundlenet_prep_graph_keyword(capi):
    from banet_amd import bundlenet
    assert bundlenet.BundleNet().prep_graph == "torch"
    assert bundlenet.BundleNet(prep_graph="hip").prep_graph == "hip"
    with pytest.raises(ValueError):
        bundlenet.BundleNet(prep_graph="bogus")
