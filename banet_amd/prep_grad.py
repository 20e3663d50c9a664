"""Differentiable per-level preparation on HIP: the resampler (tf.contrib.resampler / interpolate2d2), the [f | gx | gy]
target map and the output depth init + basis . W (bundlenet.py:320,323-324,343-344,385,397), forward and backward through
libbanet_hip.so.  Registered with the dispatcher as torch.ops.banet.{resampler, target_map, depth_output} and their *_grad
ops -- the counterpart of the gradient TF registers for tf.contrib.resampler.  Device type "cuda" (= HIP) only: a CPU tensor
raises NotImplementedError.  No float atomics in any backward: the gradients are bit-reproducible and run under
torch.use_deterministic_algorithms(True)."""
import ctypes
from typing import Tuple

import torch

from . import _capi as capi
from . import ops

OVERWRITE = 1   # banet_hip.h: BANET_ADJOINT_OVERWRITE


def _resample_shapes(data, warp):
    if data.dim() != 4 or warp.dim() != 3 or warp.shape[0] != data.shape[0] or warp.shape[2] != 2:
        raise capi.BanetError("resampler: expected data [B,H,W,C] and warp [B,N,2]; got %s %s" % (tuple(data.shape), tuple(warp.shape)))
    B, H, W, C = data.shape
    return B, warp.shape[1], C, H, W


def resampler_grad_forward(data, warp, gout, clamp=False, want_data=True, want_warp=True):
    """banet_resample_grad_f32 -> (ddata [B,H,W,C] or None, dwarp [B,N,2] or None), both written (OVERWRITE)."""
    data, warp, gout = capi.f32c(data), capi.f32c(warp), capi.f32c(gout)
    B, N, C, H, W = _resample_shapes(data, warp)
    if tuple(gout.shape) != (B, N, C):
        raise capi.BanetError("resampler_grad: expected gout [B,N,C] = %s, got %s" % ((B, N, C), tuple(gout.shape)))
    L = capi.lib()
    mode = 1 if clamp else 0
    nb = L.banet_resample_grad_workspace_bytes(B, N, C, H, W, mode)
    if nb == 0:
        raise capi.BanetError("resampler_grad: unsupported shape B=%d N=%d C=%d H=%d W=%d" % (B, N, C, H, W))
    ws = capi.workspace(nb, data.device)
    ddata = torch.empty_like(data) if want_data else None
    dwarp = torch.empty((B, N, 2), dtype=torch.float32, device=data.device) if want_warp else None
    capi.check(L.banet_resample_grad_f32(capi.ptr(data), capi.ptr(warp), capi.ptr(gout), capi.ptr(ddata), capi.ptr(dwarp),
                                         B, N, C, H, W, mode, OVERWRITE, ctypes.c_void_p(ws.data_ptr()), ws.numel(), capi.stream()))
    return ddata, dwarp


def target_map_grad_forward(gmap):
    """banet_target_map_adjoint_ex_f32 with OVERWRITE: dimg [B,H,W,C] from the gradient of the [B,H,W,3C] map."""
    gmap = capi.f32c(gmap)
    B, H, W, C3 = gmap.shape
    if C3 % 3:
        raise capi.BanetError("target_map_grad: the last dimension (%d) is not 3C" % C3)
    dimg = torch.empty((B, H, W, C3 // 3), dtype=torch.float32, device=gmap.device)
    capi.check(capi.lib().banet_target_map_adjoint_ex_f32(capi.ptr(gmap), capi.ptr(dimg), B, H, W, C3 // 3, OVERWRITE, capi.stream()))
    return dimg


def _depth_shapes(init, basis, Wc):
    B, K = basis.shape[0], basis.shape[-1]
    N = basis.numel() // (B * K)
    if init.numel() != B * N or Wc.numel() != B * K:
        raise capi.BanetError("depth_output: inconsistent shapes %s %s %s" % (tuple(init.shape), tuple(basis.shape), tuple(Wc.shape)))
    return B, N, K


def depth_output_grad_forward(basis, Wc, gout, want=(True, True, True)):
    """banet_depth_output_grad_f32 -> (dinit shaped like gout, dbasis like basis, dWc like Wc); None where not wanted."""
    basis, Wc, gout = capi.f32c(basis), capi.f32c(Wc), capi.f32c(gout)
    B, N, K = _depth_shapes(gout, basis, Wc)
    L = capi.lib()
    ws = capi.workspace(L.banet_depth_output_grad_workspace_bytes(B, N, K), basis.device)
    dinit = torch.empty_like(gout) if want[0] else None
    dbasis = torch.empty_like(basis) if want[1] else None
    dWc = torch.empty_like(Wc) if want[2] else None
    capi.check(L.banet_depth_output_grad_f32(capi.ptr(basis), capi.ptr(Wc), capi.ptr(gout), capi.ptr(dinit), capi.ptr(dbasis),
                                             capi.ptr(dWc), B, N, K, OVERWRITE, ctypes.c_void_p(ws.data_ptr()), ws.numel(),
                                             capi.stream()))
    return dinit, dbasis, dWc


# --------------------------------------------------------------------------------------
# torch.ops.banet.resampler / resampler_grad
# --------------------------------------------------------------------------------------
@torch.library.custom_op("banet::resampler", mutates_args=(), device_types="cuda")
def _resampler_op(data: torch.Tensor, warp: torch.Tensor, clamp: bool) -> torch.Tensor:
    return ops.resample(data, warp, clamp=clamp)


@_resampler_op.register_fake
def _resampler_fake(data, warp, clamp):
    B, N, C, _, _ = _resample_shapes(data, warp)
    return data.new_empty((B, N, C))


@torch.library.custom_op("banet::resampler_grad", mutates_args=(), device_types="cuda")
def _resampler_grad_op(data: torch.Tensor, warp: torch.Tensor, gout: torch.Tensor, clamp: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    return resampler_grad_forward(data, warp, gout, clamp)


@_resampler_grad_op.register_fake
def _resampler_grad_fake(data, warp, gout, clamp):
    B, N, _, _, _ = _resample_shapes(data, warp)
    return torch.empty_like(data), warp.new_empty((B, N, 2))


def _resampler_setup(ctx, inputs, output):
    data, warp, clamp = inputs
    ctx.save_for_backward(data, warp)
    ctx.clamp = clamp


def _resampler_backward(ctx, gout):
    data, warp = ctx.saved_tensors
    ddata, dwarp = torch.ops.banet.resampler_grad(data, warp, gout.contiguous(), ctx.clamp)
    return ddata.to(data.dtype), dwarp.to(warp.dtype), None


_resampler_op.register_autograd(_resampler_backward, setup_context=_resampler_setup)


# --------------------------------------------------------------------------------------
# torch.ops.banet.target_map / target_map_grad
# --------------------------------------------------------------------------------------
@torch.library.custom_op("banet::target_map", mutates_args=(), device_types="cuda")
def _target_map_op(img: torch.Tensor) -> torch.Tensor:
    return ops.target_map(img)


@_target_map_op.register_fake
def _target_map_fake(img):
    B, H, W, C = img.shape
    return img.new_empty((B, H, W, 3 * C))


@torch.library.custom_op("banet::target_map_grad", mutates_args=(), device_types="cuda")
def _target_map_grad_op(gmap: torch.Tensor) -> torch.Tensor:
    return target_map_grad_forward(gmap)


@_target_map_grad_op.register_fake
def _target_map_grad_fake(gmap):
    B, H, W, C3 = gmap.shape
    return gmap.new_empty((B, H, W, C3 // 3))


def _target_map_setup(ctx, inputs, output):
    ctx.dtype = inputs[0].dtype


def _target_map_backward(ctx, gmap):
    return torch.ops.banet.target_map_grad(gmap.contiguous()).to(ctx.dtype)


_target_map_op.register_autograd(_target_map_backward, setup_context=_target_map_setup)


# --------------------------------------------------------------------------------------
# torch.ops.banet.depth_output / depth_output_grad
# --------------------------------------------------------------------------------------
@torch.library.custom_op("banet::depth_output", mutates_args=(), device_types="cuda")
def _depth_output_op(init: torch.Tensor, basis: torch.Tensor, W: torch.Tensor) -> torch.Tensor:
    _depth_shapes(init, basis, W)
    return ops.depth_output(init, basis.reshape(basis.shape[0], -1, basis.shape[-1]), W).reshape(init.shape)


@_depth_output_op.register_fake
def _depth_output_fake(init, basis, W):
    _depth_shapes(init, basis, W)
    return torch.empty_like(init)


@torch.library.custom_op("banet::depth_output_grad", mutates_args=(), device_types="cuda")
def _depth_output_grad_op(basis: torch.Tensor, W: torch.Tensor, gout: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    return depth_output_grad_forward(basis, W, gout)


@_depth_output_grad_op.register_fake
def _depth_output_grad_fake(basis, W, gout):
    _depth_shapes(gout, basis, W)
    return torch.empty_like(gout), torch.empty_like(basis), torch.empty_like(W)


def _depth_output_setup(ctx, inputs, output):
    init, basis, W = inputs
    ctx.save_for_backward(basis, W)
    ctx.dtypes = (init.dtype, basis.dtype, W.dtype)


def _depth_output_backward(ctx, gout):
    basis, W = ctx.saved_tensors
    grads = torch.ops.banet.depth_output_grad(basis, W, gout.contiguous())
    return tuple(g.to(dt) for g, dt in zip(grads, ctx.dtypes))


_depth_output_op.register_autograd(_depth_output_backward, setup_context=_depth_output_setup)


# --------------------------------------------------------------------------------------
# public wrappers
# --------------------------------------------------------------------------------------
def resampler(data, warp, clamp=False):
    """data [B,H,W,C], warp [B,N,2] (x, y) -> [B,N,C], differentiable w.r.t. both.  clamp=False: tf.contrib.resampler.resampler
    (zero padding); clamp=True: interpolate2d2 (legacy/utils_python.py:177-232)."""
    return torch.ops.banet.resampler(data, warp, bool(clamp))


def target_map(img):
    """[B,H,W,C] -> [B,H,W,3C] = [f | gx | gy] (bundlenet.py:92-100,323-324), differentiable (REFLECT rim -> zero gradient)."""
    return torch.ops.banet.target_map(img)


def depth_output(init, basis, W):
    """init [B,...] + basis [B,...,K] . W [B,K,1] -> shaped like init (bundlenet.py:397), differentiable w.r.t. all three."""
    return torch.ops.banet.depth_output(init, basis, W)
