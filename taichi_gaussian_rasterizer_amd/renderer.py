"""The 3D renderer entry points and their result record.

`render_gaussians` is what a trainer calls once per view (reference renderer.py:134-171); it runs as the single fused
frame of fused.py, or -- an empty scene, more than 30 feature channels -- as the sequence
project -> features -> `render_projected` (reference renderer.py:183-231) of this file, every stage a HIP operator.
`Rendering` carries the images plus the per-splat by-products a trainer prunes and densifies with (reference
renderer.py:28-131: same field and property names).
"""
from __future__ import annotations

import dataclasses
from collections.abc import Sequence
from functools import cached_property
from numbers import Integral
from typing import Optional, Tuple

import torch

from . import _native as nv
from .data_types import Gaussians3D, RasterConfig
from .mapper.tile_mapper import map_to_tiles
from .perspective.params import CameraParams
from .perspective.projection import project_with_ndc
from .rasterizer.function import check_background, rasterize_channels, rasterize_with_tiles
from .spherical_harmonics import evaluate_sh_at
from .torch_lib.projection import ndc_depth

_NEED_HEURISTIC = "No point heuristic information available (use config.compute_point_heuristic=True)"
_NEED_VISIBILITY = "No visibility information available (use config.compute_visibility=True)"


def unpack(record) -> dict:
    """field name -> value of a dataclass instance (shallow)"""
    return {f.name: getattr(record, f.name) for f in dataclasses.fields(record)}


class _SplatColumns:
    """read-only view of columns [lo, hi) of the packed projected splats (mean 0:2, axis 2:4, sigma 4:6, alpha 6)"""

    def __init__(self, lo: int, hi: Optional[int] = None):
        self.index = lo if hi is None else slice(lo, hi)

    def __get__(self, rendering, owner=None):
        return self if rendering is None else rendering.gaussians2d[:, self.index]


class _HeuristicColumn:
    """one column of point_heuristic; only there when the config asked for it"""

    def __init__(self, column: int):
        self.column = column

    def __get__(self, rendering, owner=None):
        if rendering is None:
            return self
        assert rendering.config.compute_point_heuristic, _NEED_HEURISTIC
        return rendering.point_heuristic[:, self.column]


@dataclasses.dataclass(frozen=True, kw_only=True)
class Rendering:
    """What one view produced.  `depth` / `depth_var` exist with render_depth=True, `median_depth` with
    render_median_depth=True, `point_visibility` / `point_heuristic` with the corresponding RasterConfig switches
    (the heuristic is written by the backward pass)."""
    image: torch.Tensor                              # (H, W, C) blended features
    image_weight: torch.Tensor                       # (H, W) accumulated alpha
    points_in_view: torch.Tensor                     # (V) int64: which Gaussians survived the cull
    point_depth: torch.Tensor                        # (V, 1) camera-space z of those
    point_visibility: Optional[torch.Tensor] = None  # (V) summed blend weight per splat
    point_heuristic: Optional[torch.Tensor] = None   # (V, 2) prune cost, split score
    camera: CameraParams
    config: RasterConfig
    depth: Optional[torch.Tensor] = None             # (H, W)
    depth_var: Optional[torch.Tensor] = None         # (H, W)
    median_depth: Optional[torch.Tensor] = None      # (H, W)
    gaussians2d: torch.Tensor                        # (V, 7) packed projected splats

    # ---- columns of the projected splats, statistics of the backward pass
    point_scale = _SplatColumns(4, 6)
    point_opacity = _SplatColumns(6)
    prune_cost = _HeuristicColumn(0)
    split_score = _HeuristicColumn(1)

    def _to_ndc(self, z: torch.Tensor) -> torch.Tensor:
        return ndc_depth(z, self.camera.near_plane, self.camera.far_plane)

    @cached_property
    def ndc_depth(self) -> torch.Tensor:
        return self._to_ndc(self.depth)

    @cached_property
    def ndc_median_depth(self) -> torch.Tensor:
        return self._to_ndc(self.median_depth)

    @property
    def ndc_point_depth(self) -> torch.Tensor:
        return self._to_ndc(self.point_depth)

    @property
    def gaussian_scale(self) -> torch.Tensor:
        """how many sigmas out a splat still reaches alpha_threshold: the extent the culling uses
        (the original 3DGS takes a constant 3)"""
        return (2.0 * torch.log(self.point_opacity / self.config.alpha_threshold)).sqrt()

    @property
    def point_radii(self) -> torch.Tensor:
        return torch.amax(self.point_scale, dim=1)

    @property
    def _point_visibility(self) -> torch.Tensor:
        assert self.point_visibility is not None, _NEED_VISIBILITY
        return self.point_visibility

    @cached_property
    def visible_mask(self) -> torch.Tensor:
        return self._point_visibility > 0

    @cached_property
    def visible_indices(self) -> torch.Tensor:
        return self.points_in_view[self.visible_mask]

    @cached_property
    def visible(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(indexes into the scene, visibility) of the splats that contributed to some pixel"""
        return self.visible_indices, self._point_visibility[self.visible_mask]

    @property
    def image_size(self) -> Tuple[Integral, Integral]:
        return self.camera.image_size

    @property
    def num_points(self) -> int:
        return int(self.points_in_view.shape[0])

    def detach(self) -> "Rendering":
        cut = {name: (value.detach() if hasattr(value, "detach") else value) for name, value in unpack(self).items()}
        return Rendering(**cut)


def _check_call(gaussians, camera_params, config, flags: dict) -> None:
    for value, kind, name in ((gaussians, Gaussians3D, "gaussians"), (camera_params, CameraParams, "camera_params"),
                              (config, RasterConfig, "config")):
        if not isinstance(value, kind):
            raise TypeError(f"{name} must be {kind.__name__}, got {type(value).__name__}")
    for name, value in flags.items():
        if not isinstance(value, bool):
            raise TypeError(f"{name} must be bool")


def _refuse_float64(gaussians, camera_params) -> None:
    """render_gaussians is float32 only (the float64 operators exist for gradcheck): refuse f64 before any launch.  A
    CPU tensor still raises the device error first."""
    tensors = (*gaussians.shape_tensors(), gaussians.feature, camera_params.T_camera_world, camera_params.projection)
    if any(isinstance(t, torch.Tensor) and t.dtype == torch.float64 for t in tensors):
        nv.require_device(*tensors, dtype=None, what="render_gaussians")
        raise TypeError("render_gaussians: expected float32 tensors, got float64 (float64 runs in project_to_image, "
                        "evaluate_sh_at and rasterize_with_tiles, for gradcheck)")


def _refuse_unfused(gaussians, use_sh: bool, what: str) -> None:
    """a frame the fused node does not cover where only that node will do; tensors that are not float32 on the device
    are refused first, with the error every operator gives them"""
    feature = gaussians.feature
    nv.require_device(*gaussians.shape_tensors(), feature, what=what)
    raise NotImplementedError(
        f"{what}: only the fused frame produces sparse gradients (SH colours, or plain "
        f"features up to 30 channels); got features of shape {tuple(feature.shape)} with use_sh={use_sh}")


def render_gaussians(gaussians: Gaussians3D, camera_params: CameraParams, config: RasterConfig = RasterConfig(),
                     use_sh: bool = False, render_depth: bool = False, use_depth16: bool = False,
                     render_median_depth: bool = False, background: Optional[torch.Tensor] = None,
                     differentiable_weight: bool = False, sparse_grad: bool = False) -> Rendering:
    """Render one view.  `gaussians.feature` holds (N, C) features, or (N, 3, (D+1)^2) SH coefficients with
    use_sh=True.  render_depth adds depth and depth variance images, render_median_depth a second,
    non-blended pass that picks the depth at half opacity, use_depth16 sorts on 16-bit depth codes.

    sparse_grad (not an argument of the reference, like RasterConfig.forward_cut; pass it by keyword): the backward
    leaves `torch.sparse_coo` gradients on position, log_scaling, rotation, alpha_logit and feature -- indices (1, V) =
    `points_in_view` (ascending, distinct), values (V, 3) (V, 3) (V, 4) (V, 1) (V, C[, D]) -- instead of (N, ...) tensors
    that are zero outside the view; the optimizers of `optim` step from them directly.  The camera gradients stay
    dense.  Only frames the fused node covers (SH colours, or plain features up to 30 channels): anything else raises
    NotImplementedError (CPU or non-float32 tensors raise the operators' device or dtype error first); an empty scene
    (N = 0) has no rows and renders as without the switch.  Rendered values are the same either way.

    background, differentiable_weight (not arguments of the reference either; pass them by keyword).  background: a
    (C,) colour, float32 on the device of the features, C the number of colour channels of `image` (the two depth
    channels of render_depth do not count).  The returned image is composited on it inside the rasterizer, image =
    blend + (1 - image_weight) * background; image_weight itself does not change.  It may require grad and then
    receives dL/dbackground.  (A per-pixel background is composited by the caller in torch -- correctly once
    differentiable_weight is set; a learnable cubemap sky looked up by view direction is
    environment.composite_environment.)  differentiable_weight=True: image_weight takes part in autograd, so alpha, mask and
    sky losses reach the Gaussians.  `depth` and `depth_var` of render_depth keep treating the weight in their divisor
    as a constant, and are the same with and without a background; the median-depth pass has no background.  Both
    arguments need config.use_alpha_blending (ValueError); a background of another dtype or device raises TypeError,
    one of another shape AssertionError.  They work with sparse_grad."""
    _check_call(gaussians, camera_params, config, dict(use_sh=use_sh, render_depth=render_depth,
                                                      use_depth16=use_depth16,
                                                      render_median_depth=render_median_depth,
                                                      sparse_grad=sparse_grad,
                                                      differentiable_weight=differentiable_weight))
    _refuse_float64(gaussians, camera_params)
    if background is not None or differentiable_weight:
        feature = gaussians.feature
        check_background(background, differentiable_weight, config, feature,
                         feature.shape[1] if feature.ndim >= 2 else 0, "render_gaussians")
    from .fused import fused_supported, render_fused
    if fused_supported(gaussians, camera_params, use_sh, render_median_depth):
        return render_fused(gaussians, camera_params, config, render_depth, use_depth16,
                            render_median_depth=render_median_depth, sparse_grad=sparse_grad,
                            background=background, differentiable_weight=differentiable_weight)
    if sparse_grad and gaussians.position.shape[0] > 0:
        # an empty scene has no rows to be sparse over and renders as it always did
        _refuse_unfused(gaussians, use_sh, "render_gaussians(sparse_grad=True)")

    splats, depths, visible, sort_depths = project_with_ndc(
        *gaussians.shape_tensors(), camera_params.T_camera_world, camera_params.projection,
        camera_params.image_size, camera_params.depth_range, config)
    if use_sh:  # the view direction is not differentiated through (reference renderer.py:164)
        colours = evaluate_sh_at(gaussians.feature, gaussians.position.detach(), visible,
                                 camera_params.camera_position)
    else:
        colours = gaussians.feature[visible]
        assert colours.dim() == 2, f"Features must be (N, C) if use_sh=False, got {colours.shape}"
    return render_projected(visible, splats, colours, depths, camera_params, config, render_depth=render_depth,
                            use_depth16=use_depth16, render_median_depth=render_median_depth,
                            ndc_depths=sort_depths, background=background,
                            differentiable_weight=differentiable_weight)


class RenderedViews(Sequence):
    """What `render_views` produced: a sequence of the B views' `Rendering`s (len, indexing, iteration; `.renderings`
    is the tuple), plus what the batch has as a whole -- `points_in_view`, the ascending distinct union of the views'
    `points_in_view` (the rows the merged gradient lists), and `point_visibility`, the views' visibility summed in view
    order on those rows (None without config.compute_visibility)."""

    def __init__(self, renderings, points_in_view: torch.Tensor, point_visibility: Optional[torch.Tensor]):
        self.renderings = tuple(renderings)
        self.points_in_view = points_in_view
        self.point_visibility = point_visibility

    def __len__(self) -> int:
        return len(self.renderings)

    def __getitem__(self, index):
        return self.renderings[index]

    @property
    def visible(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(indexes, visibility) of the batch, as `VisibilityAware*.step(*views.visible)` takes them; unlike
        `Rendering.visible` every listed row is kept, as `optim.visible_union` keeps them"""
        assert self.point_visibility is not None, _NEED_VISIBILITY
        return self.points_in_view, self.point_visibility

    @property
    def num_points(self) -> int:
        return int(self.points_in_view.shape[0])


def render_views(gaussians: Gaussians3D, cameras, config: RasterConfig = RasterConfig(), use_sh: bool = False,
                 render_depth: bool = False, use_depth16: bool = False, render_median_depth: bool = False,
                 background: Optional[torch.Tensor] = None, differentiable_weight: bool = False,
                 sparse_grad: bool = True) -> RenderedViews:
    """Render a batch of views of the same Gaussians as ONE autograd node (not a call of the reference).  `cameras`: 1 to
    GS_VIEWS_MAX (16) CameraParams, which may differ in image size.  Every `Rendering` of the result has the fields and
    the values `render_gaussians` gives for that camera; the losses of the views are summed (or given to
    torch.autograd.backward together) and ONE backward leaves one gradient per parameter: the views' row-compact
    gradients merged on the device in view order (gs_views_sum_rows), over the union of the views' visible rows
    (`RenderedViews.points_in_view`) -- nothing goes through autograd's accumulation of sparse gradients, a sort or a
    search.  A view no loss uses costs no backward; the gradient still lists the whole union.

    sparse_grad=True (the default here): the five parameters receive `torch.sparse_coo` gradients, indices (1, U) = the
    union, shared by the five, values (U, ...); the optimizers of `optim` step from them as from a single frame's own
    (`opt.step(*views.visible)`).  sparse_grad=False: dense (N, ...) gradients, zero outside the union.  Camera gradients
    are dense, one per view.  background: (C,) for all views or (B, C), one row per view; it may require grad.  Other
    arguments as `render_gaussians`.

    Only frames the fused node covers (SH colours, or plain features up to 30 channels), whatever sparse_grad is:
    anything else raises NotImplementedError; float64 the TypeError of render_gaussians; an empty or too long `cameras`
    ValueError.  An empty scene (N = 0) renders every view through render_gaussians and has an empty union.  Memory: the
    B frames' workspaces live until the backward, which holds the compact gradient rows of all views (sum of V_b) at
    once."""
    cameras = list(cameras) if isinstance(cameras, (list, tuple)) else cameras
    if not isinstance(cameras, list):
        raise TypeError(f"cameras must be a list or tuple of CameraParams, got {type(cameras).__name__}")
    if not 1 <= len(cameras) <= nv.GS_VIEWS_MAX:
        raise ValueError(f"render_views: {len(cameras)} cameras; a batch has 1 to {nv.GS_VIEWS_MAX} views "
                         "(GS_VIEWS_MAX)")
    for b, cam in enumerate(cameras):
        if not isinstance(cam, CameraParams):
            raise TypeError(f"cameras[{b}] must be CameraParams, got {type(cam).__name__}")
    _check_call(gaussians, cameras[0], config, dict(use_sh=use_sh, render_depth=render_depth, use_depth16=use_depth16,
                                                    render_median_depth=render_median_depth, sparse_grad=sparse_grad,
                                                    differentiable_weight=differentiable_weight))
    for cam in cameras:
        _refuse_float64(gaussians, cam)
    feature = gaussians.feature
    per_view = isinstance(background, torch.Tensor) and background.dim() == 2
    if per_view:
        assert background.shape[0] == len(cameras), \
            f"render_views: a per-view background has one row per camera, got {tuple(background.shape)}"
    if background is not None or differentiable_weight:
        check_background(background[0] if per_view else background, differentiable_weight, config, feature,
                         feature.shape[1] if feature.ndim >= 2 else 0, "render_views")
    if gaussians.position.shape[0] == 0:
        views = [render_gaussians(gaussians, cam, config, use_sh, render_depth, use_depth16, render_median_depth,
                                  background=background[b] if per_view else background,
                                  differentiable_weight=differentiable_weight) for b, cam in enumerate(cameras)]
        nothing = views[0].points_in_view.new_empty((0,))
        return RenderedViews(views, nothing, feature.new_empty((0,)) if config.compute_visibility else None)
    from .fused import fused_supported, render_views_fused
    if not fused_supported(gaussians, cameras[0], use_sh, render_median_depth):
        _refuse_unfused(gaussians, use_sh, "render_views")
    return RenderedViews(*render_views_fused(gaussians, cameras, config, render_depth, use_depth16,
                                             render_median_depth, sparse_grad, background, differentiable_weight))


def compute_depth_variance(depth_depthsq: torch.Tensor, weight: torch.Tensor, eps: float = 1e-6):
    """(…, 2) blended [z, z^2] and the accumulated alpha -> expected depth and its variance"""
    total = weight + eps  # true divisions: bit-identical to the fused frame's gs_depth_split_fwd
    mean = depth_depthsq[..., 0] / total
    return mean, depth_depthsq[..., 1] / total - mean * mean


def render_projected(indexes: torch.Tensor, gaussians2d: torch.Tensor, features: torch.Tensor, depths: torch.Tensor,
                     camera_params: CameraParams, config: RasterConfig, render_depth: bool = False,
                     use_depth16: bool = False, render_median_depth: bool = False, use_ndc_depth: bool = False,
                     ndc_depths: Optional[torch.Tensor] = None, background: Optional[torch.Tensor] = None,
                     differentiable_weight: bool = False) -> Rendering:
    """Tile-map and rasterize splats that are already projected.  `ndc_depths` (the sort depth) comes from the
    projection kernel when the caller has it; otherwise it is derived from `depths` here.  background (C,) over the
    channels of `features`, differentiable_weight: see render_gaussians."""
    size = camera_params.image_size
    if isinstance(features, torch.Tensor) and features.ndim == 2 and isinstance(config, RasterConfig):
        # refused before the tile mapper launches anything
        check_background(background, differentiable_weight, config, features, features.shape[1], "render_projected")
    if ndc_depths is None:
        ndc_depths = ndc_depth(depths.detach(), camera_params.near_plane, camera_params.far_plane)
    channels = features
    raster_config = config
    if render_depth:  # two leading channels carry z and z^2 through the blend
        z = ndc_depths if use_ndc_depth else depths
        channels = torch.cat((z, z * z, features), dim=1)
        if not use_ndc_depth:
            # what the forward's early stop drops is bounded by forward_cut * max|feature|, and z^2 reaches far^2
            # (data_types.RasterConfig.forward_cut; the fused frame applies the same scale)
            raster_config = dataclasses.replace(
                config, forward_cut=config.forward_cut / max(float(camera_params.far_plane) ** 2, 1.0))

    overlap_to_point, tile_ranges = map_to_tiles(gaussians2d, ndc_depths, image_size=size, config=config,
                                                 use_depth16=use_depth16)
    tiles = dict(tile_overlap_ranges=tile_ranges.view(-1, 2), overlap_to_point=overlap_to_point, image_size=size)
    # the background covers the feature channels only: z and z^2 composite on 0
    raster = rasterize_channels(gaussians2d, channels, config=raster_config, background=background,
                                background_offset=channels.shape[1] - features.shape[1],
                                differentiable_weight=differentiable_weight, **tiles)

    median = None
    if render_median_depth:  # first splat that takes a pixel past half opacity, no blending
        pick = dataclasses.replace(config, use_alpha_blending=False, saturate_threshold=0.5)
        median = rasterize_with_tiles(gaussians2d, depths, config=pick, **tiles).image.squeeze(-1)

    image, mean_z, var_z = raster.image, None, None
    if render_depth:
        # the divisor is a constant of the backward, also when image_weight is differentiable
        mean_z, var_z = compute_depth_variance(image[..., :2], raster.image_weight.detach())
        image = image[..., 2:]
    return Rendering(image=image, image_weight=raster.image_weight, depth=mean_z, depth_var=var_z, median_depth=median,
                     camera=camera_params, config=config, points_in_view=indexes, point_depth=depths,
                     gaussians2d=gaussians2d,
                     point_visibility=raster.visibility if config.compute_visibility else None,
                     point_heuristic=raster.point_heuristic if config.compute_point_heuristic else None)


def viewspace_gradient(gaussians2d: torch.Tensor) -> torch.Tensor:
    """length of dL/d(mean) per projected splat, the classic densification signal; needs `gaussians2d.retain_grad()`
    before the backward pass"""
    assert gaussians2d.shape[1] == 7, f"Expected packed 2D gaussians (N, 7), got {gaussians2d.shape}"
    assert gaussians2d.grad is not None, \
        "Expected gradients on gaussians2d, run backward first with gaussians2d.retain_grad()"
    return gaussians2d.grad[:, :2].norm(dim=1)
