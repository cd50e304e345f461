"""Tile rasterizer: front-to-back alpha blending and its gradient (HIP).

Operator interface of the reference rasterizer/function.py:96-161: `rasterize_with_tiles`,
`rasterize`, `RasterOut`.  image / image_weight are (H,W,F) / (H,W); image_weight, visibility and
point_heuristic are non-differentiable (:72); gradients flow to gaussians2d and features.  Two keyword arguments go
beyond the reference: `background` (F,) composites the image on a colour inside the kernel, image = blend + (1 -
image_weight) * background, and receives dL/dbackground; `differentiable_weight=True` lets image_weight take part in
autograd (mask, alpha and sky losses).  Both need use_alpha_blending.  Up to 32 feature channels
run the narrow kernels, 33 to 512 the wide ones (csrc/raster_wide.hip).  float64 splats and features (for gradcheck)
run csrc/raster_f64.hip, up to 32 channels; `rasterize` maps their tiles from a float32 copy.
"""
from __future__ import annotations

from numbers import Integral
from typing import NamedTuple, Optional, Tuple

import torch

from .. import _native as nv
from ..data_types import RasterConfig
from ..mapper.tile_mapper import map_to_tiles

# widest features of gs_raster_fwd / gs_raster_bwd (include/gsplat_hip.h GS_MAX_FEATURES); wider ones, up to
# GS_MAX_WIDE_FEATURES = 512, take gs_raster_fwd_wide / gs_raster_bwd_wide
MAX_FEATURES = 32

RasterOut = NamedTuple('RasterOut', [
    ('image', torch.Tensor),
    ('image_weight', torch.Tensor),
    ('point_heuristic', Optional[torch.Tensor]),
    ('visibility', Optional[torch.Tensor])
])


class _RasterFunction(torch.autograd.Function):
    @staticmethod
    @nv.on_tensor_device
    def forward(ctx, gaussians, features, overlap_to_point, tile_overlap_ranges, image_size, config: RasterConfig,
                background=None, background_offset=0, differentiable_weight=False):
        ctx.dtype = nv.float_dtype(gaussians, features, background, what="rasterize_with_tiles")
        nv.require_device(overlap_to_point, tile_overlap_ranges, dtype=torch.int32, what="rasterize_with_tiles tiles")
        bg = None if background is None else background.contiguous()
        ctx.background, ctx.background_offset, ctx.weight_grad = bg, int(background_offset), bool(differentiable_weight)
        if ctx.dtype == torch.float64:
            return _forward_f64(ctx, gaussians, features, overlap_to_point, tile_overlap_ranges, image_size, config)
        lib = nv.lib()
        dev = features.device
        w, h = int(image_size[0]), int(image_size[1])
        v, F = gaussians.shape[0], features.shape[1]
        g, f = gaussians.contiguous(), features.contiguous()
        o2p, ranges = overlap_to_point.contiguous(), tile_overlap_ranges.contiguous()
        image = torch.empty((h, w, F), dtype=torch.float32, device=dev)
        alpha = torch.empty((h, w), dtype=torch.float32, device=dev)
        # reference function.py:48-59
        heur = (torch.zeros((v, 2), dtype=torch.float32, device=dev) if config.compute_point_heuristic
                else torch.empty((0, 2), dtype=torch.float32, device=dev))
        want_vis = config.compute_visibility or config.compute_point_heuristic
        vis = (torch.zeros((v,), dtype=torch.float32, device=dev) if want_vis
               else torch.empty((0,), dtype=torch.float32, device=dev))
        if F <= MAX_FEATURES:
            nv.check(lib.gs_raster_fwd(v, F, nv.ptr(g), nv.ptr(f), nv.ptr(ranges), nv.ptr(o2p), o2p.shape[0], w, h,
                                       nv.make_config(config), None, None, nv.ptr(image), nv.ptr(alpha),
                                       nv.ptr(vis) if want_vis else None, None, nv.ptr(bg), ctx.background_offset,
                                       nv.stream()), "gs_raster_fwd")
        else:
            nv.check(lib.gs_raster_fwd_wide(v, F, nv.ptr(g), nv.ptr(f), nv.ptr(ranges), nv.ptr(o2p), o2p.shape[0],
                                            w, h, nv.make_config(config), nv.ptr(image), nv.ptr(alpha),
                                            nv.ptr(vis) if want_vis else None, nv.ptr(bg), ctx.background_offset,
                                            nv.stream()), "gs_raster_fwd_wide")
        if not config.compute_visibility:
            vis_out = torch.empty((0,), dtype=torch.float32, device=dev) if not want_vis else vis
        else:
            vis_out = vis
        ctx.image_size, ctx.config = (w, h), config
        ctx.heur = heur
        return _finish_forward(ctx, g, f, o2p, ranges, image, alpha, heur, vis_out)

    @staticmethod
    @nv.on_tensor_device
    def backward(ctx, grad_image, grad_alpha, _gh, _gv):
        if ctx.dtype == torch.float64:
            return _backward_f64(ctx, grad_image, grad_alpha)
        g, f, o2p, ranges, image, alpha = _saved(ctx)
        lib = nv.lib()
        v, F = g.shape[0], f.shape[1]
        w, h = ctx.image_size
        config = ctx.config
        gi = grad_image.contiguous()
        gw = grad_alpha.contiguous() if ctx.weight_grad else None
        nv.require_device(gi, gw, what="rasterize backward")
        tail = (_background_grad(ctx, gi, alpha), None, None)
        if F > MAX_FEATURES:
            grad_g = torch.zeros_like(g)
            grad_f = torch.zeros_like(f)
            heur = ctx.heur if config.compute_point_heuristic else None
            nv.check(lib.gs_raster_bwd_wide(v, F, nv.ptr(g), nv.ptr(f), nv.ptr(ranges), nv.ptr(o2p), o2p.shape[0],
                                            w, h, nv.make_config(config), nv.ptr(image), nv.ptr(gi),
                                            nv.ptr(alpha) if gw is not None else None, nv.ptr(gw), nv.ptr(grad_g),
                                            nv.ptr(grad_f), nv.ptr(heur), nv.stream()), "gs_raster_bwd_wide")
            return (grad_g, grad_f, None, None, None, None, *tail)
        row = lib.gs_grad_row_floats(F)
        rows = torch.zeros((v, row), dtype=torch.float32, device=g.device)
        nv.check(lib.gs_raster_bwd(v, F, nv.ptr(g), nv.ptr(f), nv.ptr(ranges), nv.ptr(o2p), o2p.shape[0], w, h,
                                   nv.make_config(config), None, None, nv.ptr(image), nv.ptr(gi),
                                   nv.ptr(alpha) if gw is not None else None, nv.ptr(gw), nv.ptr(rows), None,
                                   nv.stream()), "gs_raster_bwd")
        grad_g = torch.empty_like(g)
        grad_f = torch.empty_like(f)
        heur = ctx.heur if config.compute_point_heuristic else None
        nv.check(lib.gs_raster_bwd_unpack(v, F, nv.ptr(rows), nv.ptr(grad_g), nv.ptr(grad_f), nv.ptr(heur),
                                          nv.stream()), "gs_raster_bwd_unpack")
        return (grad_g, grad_f, None, None, None, None, *tail)


def _finish_forward(ctx, g, f, o2p, ranges, image, alpha, heur, vis_out):
    """what both precisions save and mark: the weight image stays out of autograd unless differentiable_weight asks for
    it, and is saved only when the backward reads it (its own gradient, or the background's)"""
    if ctx.weight_grad:
        ctx.mark_non_differentiable(vis_out, heur)
    else:
        ctx.mark_non_differentiable(alpha, vis_out, heur)
    ctx.keeps_alpha = ctx.weight_grad or ctx.background is not None
    ctx.save_for_backward(g, f, o2p, ranges, image, *((alpha,) if ctx.keeps_alpha else ()))
    return image, alpha, heur, vis_out


def _saved(ctx):
    saved = ctx.saved_tensors
    return (*saved[:5], saved[5] if ctx.keeps_alpha else None)


def _background_grad(ctx, grad_image, alpha):
    """dL/dbackground_c = sum over the pixels of g_c T, T = 1 - image_weight: torch ops on the stream, no host
    synchronisation (off the default path: None without a background that asks for a gradient)"""
    if ctx.background is None or not ctx.needs_input_grad[6]:
        return None
    return (grad_image[..., ctx.background_offset:] * (1.0 - alpha).unsqueeze(-1)).sum((0, 1))


def _forward_f64(ctx, gaussians, features, overlap_to_point, tile_overlap_ranges, image_size, config):
    """gs_raster_fwd_f64 (csrc/raster_f64.hip): the reference formulas in float64, up to MAX_FEATURES channels.  The
    forward blends each tile's whole list (RasterConfig.forward_cut does not apply)."""
    lib = nv.lib()
    dev = features.device
    w, h = int(image_size[0]), int(image_size[1])
    v, F = gaussians.shape[0], features.shape[1]
    if F > MAX_FEATURES:
        raise NotImplementedError(f"rasterize_with_tiles: float64 features are at most {MAX_FEATURES} wide, got {F}")
    g, f = gaussians.contiguous(), features.contiguous()
    o2p, ranges = overlap_to_point.contiguous(), tile_overlap_ranges.contiguous()
    image = torch.empty((h, w, F), dtype=torch.float64, device=dev)
    alpha = torch.empty((h, w), dtype=torch.float64, device=dev)
    heur = torch.zeros((v if config.compute_point_heuristic else 0, 2), dtype=torch.float64, device=dev)
    want_vis = config.compute_visibility or config.compute_point_heuristic
    vis = torch.zeros((v if want_vis else 0,), dtype=torch.float64, device=dev)
    nbytes = lib.gs_raster_f64_scratch_bytes(v, o2p.shape[0], F)
    scratch = nv.scratch(nbytes, dev)
    nv.check(lib.gs_raster_fwd_f64(v, F, nv.ptr(g), nv.ptr(f), nv.ptr(ranges), nv.ptr(o2p), o2p.shape[0], w, h,
                                   nv.make_config_f64(config), nv.ptr(image), nv.ptr(alpha),
                                   nv.ptr(vis) if want_vis else None, nv.ptr(ctx.background), ctx.background_offset,
                                   nv.ptr(scratch), nbytes, nv.stream()), "gs_raster_fwd_f64")
    vis_out = vis if config.compute_visibility else torch.empty((0,), dtype=torch.float64, device=dev)
    ctx.image_size, ctx.config = (w, h), config
    ctx.heur = heur
    return _finish_forward(ctx, g, f, o2p, ranges, image, alpha, heur, vis_out)


def _backward_f64(ctx, grad_image, grad_alpha):
    """gs_raster_bwd_f64: per-(tile, entry) records summed per splat in list order (bit-reproducible); the point
    heuristics go into the tensor the forward returned, as in float32."""
    g, f, o2p, ranges, image, alpha = _saved(ctx)
    lib = nv.lib()
    v, F = g.shape[0], f.shape[1]
    w, h = ctx.image_size
    config = ctx.config
    gi = grad_image.contiguous()
    gw = grad_alpha.contiguous() if ctx.weight_grad else None
    if nv.float_dtype(gi, gw, what="rasterize backward") != torch.float64:
        raise TypeError("rasterize backward: float64 forward, float32 gradient")
    grad_g = torch.empty_like(g)
    grad_f = torch.empty_like(f)
    nbytes = lib.gs_raster_f64_scratch_bytes(v, o2p.shape[0], F)
    scratch = nv.scratch(nbytes, g.device)
    nv.check(lib.gs_raster_bwd_f64(v, F, nv.ptr(g), nv.ptr(f), nv.ptr(ranges), nv.ptr(o2p), o2p.shape[0], w, h,
                                   nv.make_config_f64(config), nv.ptr(image), nv.ptr(gi),
                                   nv.ptr(alpha) if gw is not None else None, nv.ptr(gw), nv.ptr(grad_g),
                                   nv.ptr(grad_f), nv.ptr(ctx.heur) if config.compute_point_heuristic else None,
                                   nv.ptr(scratch), nbytes, nv.stream()), "gs_raster_bwd_f64")
    return grad_g, grad_f, None, None, None, None, _background_grad(ctx, gi, alpha), None, None


def _validate(gaussians2d, features, overlap_to_point, tile_overlap_ranges, image_size, config):
    for name, t in (("gaussians2d", gaussians2d), ("features", features), ("overlap_to_point", overlap_to_point),
                    ("tile_overlap_ranges", tile_overlap_ranges)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor, got {type(t).__name__}")
    if not (len(image_size) == 2 and all(isinstance(x, Integral) for x in image_size)):
        raise TypeError(f"image_size must be Tuple[Integral, Integral], got {image_size!r}")
    if not isinstance(config, RasterConfig):
        raise TypeError(f"config must be RasterConfig, got {type(config).__name__}")
    assert gaussians2d.ndim == 2 and gaussians2d.shape[1] == 7, f"gaussians2d must be Nx7, got {gaussians2d.shape}"
    assert features.ndim == 2 and features.shape[0] == gaussians2d.shape[0], \
        f"Size mismatch: got {gaussians2d.shape}, {features.shape}"
    ts = config.tile_size
    tiles = (-(-int(image_size[0]) // ts)) * (-(-int(image_size[1]) // ts))
    assert tile_overlap_ranges.ndim == 2 and tile_overlap_ranges.shape == (tiles, 2), \
        f"tile_overlap_ranges must be ({tiles}, 2) for image size {tuple(image_size)}, got {tuple(tile_overlap_ranges.shape)}"


def check_background(background, differentiable_weight, config, features, channels: int, what: str) -> None:
    """the refusals of the two arguments beyond the reference, before anything touches the device: ValueError without
    alpha blending, TypeError for a background that is no tensor or of another dtype or device than the features,
    AssertionError for one that is not (channels,)"""
    if not isinstance(differentiable_weight, bool):
        raise TypeError(f"{what}: differentiable_weight must be bool")
    if background is not None and not isinstance(background, torch.Tensor):
        raise TypeError(f"{what}: background must be a torch.Tensor or None, got {type(background).__name__}")
    if (background is not None or differentiable_weight) and not config.use_alpha_blending:
        raise ValueError(f"{what}: background and differentiable_weight need use_alpha_blending=True (without blending "
                         "nothing is composited and image_weight is a mask)")
    if background is None:
        return
    if background.dtype != features.dtype or background.device != features.device:
        raise TypeError(f"{what}: background is {background.dtype} on {background.device}, the features are "
                        f"{features.dtype} on {features.device}")
    assert tuple(background.shape) == (channels,), \
        f"{what}: background must be ({channels},), one value per output colour channel, got {tuple(background.shape)}"


def rasterize_channels(gaussians2d, features, overlap_to_point, tile_overlap_ranges, image_size, config,
                       background=None, background_offset: int = 0, differentiable_weight: bool = False) -> RasterOut:
    """rasterize_with_tiles whose background covers the channels from `background_offset` on only (a depth render's
    two leading channels carry z and z^2 and composite on 0)"""
    _validate(gaussians2d, features, overlap_to_point, tile_overlap_ranges, image_size, config)
    check_background(background, differentiable_weight, config, features, features.shape[1] - background_offset,
                     "rasterize_with_tiles")
    return RasterOut(*_RasterFunction.apply(gaussians2d, features, overlap_to_point, tile_overlap_ranges, image_size,
                                            config, background, background_offset, differentiable_weight))


def rasterize_with_tiles(gaussians2d: torch.Tensor, features: torch.Tensor, overlap_to_point: torch.Tensor,
                         tile_overlap_ranges: torch.Tensor, image_size: Tuple[Integral, Integral],
                         config: RasterConfig, background: Optional[torch.Tensor] = None,
                         differentiable_weight: bool = False) -> RasterOut:
    """Rasterize an image given 2d gaussians, features and tile overlap information.

    Parameters:
        gaussians2d: (N, 7)  packed gaussians
        features: (N, F)
        tile_overlap_ranges: (TH * TW, 2) maps tile index to a range of overlap indices
        overlap_to_point: (K, ) maps overlap index to point index
        image_size: (width, height)
        config: RasterConfig
        background: optional (F,) colour, same dtype and device as the features (not in the reference; pass by
            keyword): the returned image is blend + (1 - image_weight) * background, composited in the kernel's
            epilogue; it may require grad.  A per-pixel background is composited by the caller in torch, correctly
            once differentiable_weight is set.
        differentiable_weight: image_weight takes part in autograd (not in the reference, where it is marked
            non-differentiable)

    Both need config.use_alpha_blending (ValueError otherwise); a background of another dtype or device than the
    features raises TypeError, one of another shape AssertionError.

    Returns RasterOut(image (H,W,F), image_weight (H,W), point_heuristic (N,2), visibility (N,))
    """
    return rasterize_channels(gaussians2d, features, overlap_to_point, tile_overlap_ranges, image_size, config,
                              background, 0, differentiable_weight)


def rasterize(gaussians2d: torch.Tensor, depth: torch.Tensor, features: torch.Tensor,
              image_size: Tuple[Integral, Integral], config: RasterConfig, use_depth16: bool = False,
              background: Optional[torch.Tensor] = None, differentiable_weight: bool = False) -> RasterOut:
    """Rasterize an image given 2d gaussians, depths (for sorting) and features.  background,
    differentiable_weight: see rasterize_with_tiles."""
    assert gaussians2d.shape[0] == depth.shape[0] == features.shape[0], \
        f"Size mismatch: got {gaussians2d.shape}, {depth.shape}, {features.shape}"
    if isinstance(config, RasterConfig) and isinstance(features, torch.Tensor) and features.ndim == 2:
        # refused before the tile mapper launches anything
        check_background(background, differentiable_weight, config, features, features.shape[1], "rasterize")
    splats = gaussians2d
    if gaussians2d.dtype == torch.float64:  # the mapper is float32-only, as the reference's (tile_mapper.py:12)
        splats, depth = gaussians2d.detach().float(), depth.detach().float()
    overlap_to_point, tile_overlap_ranges = map_to_tiles(
        splats, depth, image_size=image_size, config=config, use_depth16=use_depth16)
    return rasterize_with_tiles(gaussians2d, features, tile_overlap_ranges=tile_overlap_ranges.view(-1, 2),
                                overlap_to_point=overlap_to_point, image_size=image_size, config=config,
                                background=background, differentiable_weight=differentiable_weight)
