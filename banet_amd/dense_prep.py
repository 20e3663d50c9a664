"""Dense level preparation: the decoder's depth / basis map at every pyramid level's own resolution.

The dense solver (banet_amd/dense.py) takes `depth [B,H_l,W_l]` and `basis [B,H_l,W_l,K]` per level; the decoder emits one depth
and one basis map at half the finest feature resolution, which the reference resamples at `_points / 2` and reuses at every
level (bundlenet.py:341-344,397).  With every pixel of a level as a point, the sample positions are an affine function of
the pixel index:

    grid_levels    the per-level grids (pure Python, no device)
    grid_pyramid   all levels from one map in one launch (banet_grid_resample_f32), differentiable: the backward is one
                   sort-free gather over the map's texels (banet_grid_resample_grad_f32), bit-reproducible

HIP only: CPU tensors raise BanetError, as everywhere in this package."""
import numpy as np
import torch

from . import _capi as capi

OVERWRITE = 1        # banet_hip.h: BANET_ADJOINT_OVERWRITE
MAX_LEVELS = 8       # grid_plan.hpp: kGridMaxLevels
MIN_STEP, MAX_STEP = 0.25, 64.0


def _coord(j, s, o):
    """the kernels' coordinate: float32 j * s + o, two roundings (grid_plan.hpp: grid_coord)"""
    return np.float32(np.float32(j) * np.float32(s)) + np.float32(o)


def check_grid(H, W, geom):
    """raises ValueError unless the level grid `geom` = (Ho, Wo, sx, sy, ox, oy) over an H x W map is one the kernels take"""
    Ho, Wo, sx, sy, ox, oy = geom
    if Ho < 1 or Wo < 1:
        raise ValueError("grid level: empty grid %dx%d" % (Ho, Wo))
    for n_out, n_in, s, o, axis in ((Wo, W, sx, ox, "x"), (Ho, H, sy, oy, "y")):
        if not (MIN_STEP <= s <= MAX_STEP):
            raise ValueError("grid level: %s step %r outside [1/4, 64]" % (axis, s))
        first, last = float(_coord(0, s, o)), float(_coord(n_out - 1, s, o))
        if first < -1.0 or last > float(n_in):
            raise ValueError("grid level: %s coordinates %g .. %g leave [-1, %d]" % (axis, first, last, n_in))


def grid_levels(H, W, level_shapes, scales, data_scale):
    """Per-level grids (Ho, Wo, sx, sy, ox, oy) for levels of scale `scales[l]` and shape `level_shapes[l]` = (H_l, W_l), sampled
    from an H x W map that lives at scale `data_scale` (scale = finest-level pixels per pixel: 1 for the finest level).  A level
    pixel j lies at finest-level coordinate j s_l, i.e. at map coordinate j s_l / data_scale: step s_l / data_scale, offset 0 --
    the reference's `_points / 2` for its half-resolution depth and basis (bundlenet.py:343-344; data_scale = 2).  Raises
    ValueError when a level's grid leaves what the kernels support (steps in [1/4, 64], coordinates inside [-1, W] x [-1, H],
    at most 8 levels)."""
    if len(level_shapes) != len(scales):
        raise ValueError("grid_levels: %d shapes for %d scales" % (len(level_shapes), len(scales)))
    if not 1 <= len(scales) <= MAX_LEVELS:
        raise ValueError("grid_levels: 1 .. %d levels, got %d" % (MAX_LEVELS, len(scales)))
    if not data_scale > 0:
        raise ValueError("grid_levels: data_scale must be positive")
    out = []
    for (Hl, Wl), s in zip(level_shapes, scales):
        step = float(s) / float(data_scale)
        geom = (int(Hl), int(Wl), step, step, 0.0, 0.0)
        check_grid(H, W, geom)
        out.append(geom)
    return out


def is_identity(H, W, geom):
    return tuple(geom) == (H, W, 1.0, 1.0, 0.0, 0.0)


def _table(geoms, tensors):
    tb = (capi.GridLevel * len(geoms))()
    for e, (Ho, Wo, sx, sy, ox, oy), t in zip(tb, geoms, tensors):
        e.Ho, e.Wo, e.sx, e.sy, e.ox, e.oy = Ho, Wo, sx, sy, ox, oy
        e.out = capi.ptr(t)
    return tb


def grid_resample(data, geoms, clamp=True):
    """banet_grid_resample_f32: data [B,H,W,C] -> one [B,Ho,Wo,C] tensor per grid, one launch"""
    data = capi.f32c(data)
    ptr = capi.ptr(data)
    B, H, W, C = data.shape
    outs = [torch.empty((B, g[0], g[1], C), dtype=torch.float32, device=data.device) for g in geoms]
    capi.check(capi.lib().banet_grid_resample_f32(ptr, B, H, W, C, 1 if clamp else 0, _table(geoms, outs), len(geoms), capi.stream()))
    return outs


def grid_resample_grad(gouts, geoms, shape, clamp=True, out=None, accumulate=False):
    """banet_grid_resample_grad_f32: the levels' gout tensors -> ddata [B,H,W,C], every texel written (OVERWRITE) into a new tensor
    or into `out`; accumulate=True adds to `out` instead"""
    B, H, W, C = shape
    gouts = [capi.f32c(g) for g in gouts]
    for g, geom in zip(gouts, geoms):
        if tuple(g.shape) != (B, geom[0], geom[1], C):
            raise capi.BanetError("grid_resample_grad: expected gout %s, got %s" % ((B, geom[0], geom[1], C), tuple(g.shape)))
    if accumulate and out is None:
        raise capi.BanetError("grid_resample_grad: accumulate needs `out`")
    ddata = torch.empty(shape, dtype=torch.float32, device=gouts[0].device) if out is None else out
    if tuple(ddata.shape) != tuple(shape):
        raise capi.BanetError("grid_resample_grad: expected out %s, got %s" % (tuple(shape), tuple(ddata.shape)))
    capi.check(capi.lib().banet_grid_resample_grad_f32(capi.ptr(ddata), B, H, W, C, 1 if clamp else 0, _table(geoms, gouts), len(geoms),
                                                       0 if accumulate else OVERWRITE, capi.stream()))
    return ddata


class _GridPyramid(torch.autograd.Function):
    """every non-identity level of grid_pyramid: forward = one launch, backward = one launch"""

    @staticmethod
    def forward(ctx, data, clamp, geoms):
        ctx.geoms, ctx.clamp, ctx.shape, ctx.dtype = geoms, clamp, tuple(data.shape), data.dtype
        ctx.set_materialize_grads(False)
        return tuple(grid_resample(data, geoms, clamp))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *gouts):
        live = [(g, geom) for g, geom in zip(gouts, ctx.geoms) if g is not None]
        if not live:
            return None, None, None
        ddata = grid_resample_grad([g for g, _ in live], [geom for _, geom in live], ctx.shape, ctx.clamp)
        return ddata.to(ctx.dtype), None, None


def grid_pyramid(data, levels, clamp=True):
    """data [B,H,W,C] (or [B,H,W]: a depth map, C = 1) -> a list with one [B,Ho,Wo,C] ([B,Ho,Wo]) tensor per level of `levels`
    (grids as grid_levels returns them).  clamp=True: taps clamped into the map (interpolate2d2); False: tf.contrib.resampler's
    zero padding, which halves the last row and column of an upsampled level.  Differentiable in `data`.  A level whose grid
    is the identity (step 1, offset 0, the map's own size) is `data` itself -- no copy, nothing launched; its gradient reaches
    `data` through autograd's own accumulation, every other level's through the one adjoint launch."""
    flat = data.dim() == 3
    d4 = data.unsqueeze(-1) if flat else data
    if d4.dim() != 4:
        raise capi.BanetError("grid_pyramid: expected data [B,H,W,C] or [B,H,W], got %s" % (tuple(data.shape),))
    capi.ptr(capi.f32c(d4))                                   # HIP only: a CPU tensor raises here, before anything else
    B, H, W, C = d4.shape
    levels = [tuple(g) for g in levels]
    for g in levels:
        check_grid(H, W, g)
    work = [g for g in levels if not is_identity(H, W, g)]
    if len(work) > MAX_LEVELS:
        raise ValueError("grid_pyramid: at most %d resampled levels, got %d" % (MAX_LEVELS, len(work)))
    made = iter(_GridPyramid.apply(d4, bool(clamp), tuple(work)) if work else ())
    out = [d4 if is_identity(H, W, g) else next(made) for g in levels]
    return [(data if t is d4 else t.squeeze(-1)) if flat else t for t in out]


__all__ = ["grid_levels", "grid_pyramid", "grid_resample", "grid_resample_grad", "check_grid"]
