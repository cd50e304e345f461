"""Per-image appearance compensation (HIP): a bilateral grid of 3x4 colour transforms sliced at every pixel.

    slice_bilateral_grid(grid, image, guide=None) -> the corrected image, shaped like `image`
    identity_grids(views, L=8, Hg=16, Wg=16)      -> (views, 12, L, Hg, Wg) grids that change nothing
    total_variation(grids)                        -> the smoothness regulariser of the grids

Photos of one scene differ in exposure, white balance and vignetting.  A trainer gives every photo a small grid and
applies it to the render before the loss -- between `Rendering.image` and `losses.photometric_loss` -- so that the
Gaussians do not have to explain brightness changes with geometry.

`image` is (H, W, 3) or (B, H, W, 3), channel-last as `Rendering.image`, read through its strides (`image[..., 2:]`
of a depth render goes in without a copy).  `grid` is (12, L, Hg, Wg) or (B, 12, L, Hg, Wg), the channel-first layout
torch's grid_sample takes, so bilateral-grid checkpoints load as they are; channel 4 r + c is element (r, c) of the
affine matrix.  Any of L, Hg, Wg may be 1: a (12, 1, 1, 1) grid is one exposure / colour matrix per image, the
per-image compensation of the original 3DGS code.  For the pixel at column x, row y:

    luma = 0.299 r + 0.587 g + 0.114 b                 (guide[y, x] when a guide is passed)
    gx = (x + 0.5) / W * (Wg - 1),  gy = (y + 0.5) / H * (Hg - 1),  gz = clamp(luma, 0, 1) * (L - 1)
    A = trilinear interpolation of the 12 channels at (gz, gy, gx)
    out = A[:, :3] @ rgb + A[:, 3]

which is grid_sample(mode="bilinear", padding_mode="border", align_corners=True) at 2 (u, v, luma) - 1 followed by the
affine.  One kernel per direction (csrc/bilagrid.hip) plus the fixed-order sum of the grid gradient.  An identity grid
returns the float32 image bit for bit, so a run that starts at identity starts as a run without correction.  All
outputs of both directions repeat bit for bit.  Gradients flow to the grid, to the image (through the affine and, when
the guide is the image's own luma, through gz) and to an explicit guide; where the luma lies outside (0, 1) the
gradient through gz is zero, as in torch.  float32, or float64 when every tensor is (gradcheck).
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from . import _native as nv
from .losses import _strided, _strided_mask

__all__ = ["slice_bilateral_grid", "identity_grids", "total_variation"]


def _check(what, grid, image, guide):
    """every argument error, cheapest first and all before any launch; returns the dtype"""
    for name, t in (("grid", grid), ("image", image)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{what}: {name} must be a torch.Tensor, got {type(t).__name__}")
    if image.dim() not in (3, 4) or image.shape[-1] != 3:
        raise ValueError(f"{what}: image must be (H, W, 3) or (B, H, W, 3), got {tuple(image.shape)}")
    if grid.dim() != image.dim() + 1 or grid.shape[-4] != 12:
        raise ValueError(f"{what}: grid must be {'(B, 12, L, Hg, Wg)' if image.dim() == 4 else '(12, L, Hg, Wg)'} for "
                         f"an image {tuple(image.shape)}, got {tuple(grid.shape)}")
    if image.dim() == 4 and grid.shape[0] != image.shape[0]:
        raise ValueError(f"{what}: {grid.shape[0]} grids for a batch of {image.shape[0]} images")
    if image.numel() == 0 or grid.numel() == 0:
        raise ValueError(f"{what}: empty image {tuple(image.shape)} or grid {tuple(grid.shape)}")
    if not (image.is_floating_point() and grid.is_floating_point()) or image.dtype != grid.dtype:
        raise TypeError(f"{what}: grid is {grid.dtype}, image {image.dtype}; both float32, or both float64")
    if guide is not None:
        if not isinstance(guide, torch.Tensor):
            raise TypeError(f"{what}: guide must be a torch.Tensor, got {type(guide).__name__}")
        if guide.shape != image.shape[:-1]:
            raise ValueError(f"{what}: guide {tuple(guide.shape)} for an image {tuple(image.shape)}: expected "
                             f"{tuple(image.shape[:-1])}")
        if guide.dtype != image.dtype:
            raise TypeError(f"{what}: guide is {guide.dtype}, image {image.dtype}")
        if guide.device != image.device:
            raise TypeError(f"{what}: guide on {guide.device}, image on {image.device}")
    return nv.float_dtype(grid, image, guide, what=what)


class _Call:
    """one grid / image pair, and its guide if any, prepared for the C-ABI: views, strides, the entry points"""

    def __init__(self, grid, image, guide, dtype):
        self.x, *xs = _strided(image.detach())
        g = grid.detach()
        if g.dim() == 4:
            g = g.unsqueeze(0)
        if not (g[0].is_contiguous() and (g.shape[0] == 1 or g.stride(0) >= g[0].numel())):
            g = g.contiguous()
        self.grid = g
        self.B, self.H, self.W = self.x.shape[:3]
        self.sizes = tuple(g.shape[2:])
        guide_args = (None, 0, 0, 0)
        self.guide = None
        if guide is not None:
            self.guide, *gs = _strided_mask(guide.detach(), dtype)
            if self.B > 1 and gs[0] == 0:  # an expand() over the batch: d_guide has an entry per image
                self.guide = self.guide.contiguous()
                gs = list(self.guide.stride())
            guide_args = (nv.ptr(self.guide), *gs)
        self.dtype = dtype
        self.f64 = dtype == torch.float64
        suffix = "_f64" if self.f64 else ""
        self.fwd_name, self.bwd_name = "gs_bilagrid_slice_fwd" + suffix, "gs_bilagrid_slice_bwd" + suffix
        self.args = (self.B, self.H, self.W, nv.ptr(self.x), *xs, *guide_args, nv.ptr(g), *self.sizes,
                     g.stride(0) if g.shape[0] > 1 else g[0].numel())

    def forward(self):
        out = torch.empty((self.B, self.H, self.W, 3), dtype=self.dtype, device=self.x.device)
        nv.check(getattr(nv.lib(), self.fwd_name)(*self.args, nv.ptr(out), nv.stream()), self.fwd_name)
        return out

    def backward(self, grad_out, want_grid, want_image, want_guide):
        dev = self.x.device
        if nv.float_dtype(grad_out, what=self.bwd_name) != self.dtype:
            raise TypeError(f"{self.bwd_name}: {self.dtype} forward, {grad_out.dtype} gradient")
        grad_out = grad_out.reshape(self.B, self.H, self.W, 3).contiguous()
        d_image = torch.empty_like(grad_out) if want_image else None
        d_guide = torch.empty((self.B, self.H, self.W), dtype=self.dtype, device=dev) if want_guide else None
        d_grid, scratch, nbytes = None, None, 0
        if want_grid:
            d_grid = torch.empty(self.grid.shape, dtype=self.dtype, device=dev)
            lib = nv.lib()
            nbytes = lib.gs_bilagrid_scratch_bytes(self.B, self.H, self.W, *self.sizes, int(self.f64))
            if nbytes < 0:
                nv.check(int(nbytes), "gs_bilagrid_scratch_bytes")
            scratch = nv.scratch(nbytes, dev)
        nv.check(getattr(nv.lib(), self.bwd_name)(*self.args, nv.ptr(grad_out), nv.ptr(d_image), nv.ptr(d_guide),
                                                  nv.ptr(d_grid), nv.ptr(scratch), nbytes, nv.stream()),
                 self.bwd_name)
        return d_grid, d_image, d_guide


class _SliceBilateralGrid(torch.autograd.Function):
    @staticmethod
    @nv.on_tensor_device
    def forward(ctx, image, grid, guide, dtype):
        call = _Call(grid, image, guide, dtype)
        ctx.call, ctx.grid_shape, ctx.image_shape = call, grid.shape, image.shape
        return call.forward().view(image.shape)

    @staticmethod
    @once_differentiable
    @nv.on_tensor_device
    def backward(ctx, grad_out):
        need_image, need_grid, need_guide = ctx.needs_input_grad[:3]
        d_grid, d_image, d_guide = ctx.call.backward(grad_out, need_grid, need_image, need_guide)
        return (d_image.view(ctx.image_shape) if need_image else None,
                d_grid.view(ctx.grid_shape) if need_grid else None,
                d_guide.view(ctx.image_shape[:-1]) if need_guide else None, None)


def slice_bilateral_grid(grid: torch.Tensor, image: torch.Tensor, guide: torch.Tensor | None = None) -> torch.Tensor:
    """`image` corrected by `grid` (module docstring): per pixel, the 3x4 affine interpolated from the grid at the
    pixel's position and luma -- or `guide`, shaped image.shape[:-1], when one is passed -- applied to its colour.
    A view such as `grids[i]` of a (V, 12, L, Hg, Wg) parameter is read in place; indexing it goes through autograd
    as usual.  A (12, 1, 1, 1) grid is the per-image exposure matrix."""
    dtype = _check("slice_bilateral_grid", grid, image, guide)
    return _SliceBilateralGrid.apply(image, grid, guide, dtype)


def identity_grids(views: int, L: int = 8, Hg: int = 16, Wg: int = 16, device=None,
                   dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """(views, 12, L, Hg, Wg) grids whose every node is the identity transform: 1 on channels 0, 5 and 10 (the
    diagonal of the 3x3 part), 0 elsewhere.  `slice_bilateral_grid` returns the image bit for bit under them."""
    for name, v in (("views", views), ("L", L), ("Hg", Hg), ("Wg", Wg)):
        if not isinstance(v, int) or isinstance(v, bool) or v < 1:
            raise ValueError(f"identity_grids: {name} must be a positive int, got {v!r}")
    grids = torch.zeros((views, 12, L, Hg, Wg), dtype=dtype, device=device)
    grids[:, (0, 5, 10)] = 1
    return grids


def total_variation(grids: torch.Tensor) -> torch.Tensor:
    """The mean squared difference between neighbouring nodes along each of the three grid axes (L, Hg, Wg), summed
    over the axes; an axis of one node adds nothing.  Plain torch ops on purpose: the grids are small (about 100 kB
    each) and this is not the hot path."""
    if not isinstance(grids, torch.Tensor) or grids.dim() < 4 or grids.shape[-4] != 12:
        raise ValueError(f"total_variation: expected (..., 12, L, Hg, Wg), got "
                         f"{tuple(grids.shape) if isinstance(grids, torch.Tensor) else type(grids).__name__}")
    total = grids.new_zeros(())
    for axis in (-3, -2, -1):
        if grids.shape[axis] > 1:
            total = total + grids.diff(dim=axis).square().mean()
    return total
