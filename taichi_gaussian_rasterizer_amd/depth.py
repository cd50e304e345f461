"""Losses of a rendered depth against a depth prior, with the prior fitted to the render per image (HIP).

    depth_prior_loss(depth, prior, mask=None, align="affine", inverse=False, return_parts=False)
    pearson_depth_loss(depth, prior, mask=None, inverse=False)
    fit_scale_shift(depth, prior, mask=None, align="affine", inverse=False) -> (scale, shift), (B,) each, detached

`depth` is (H, W) or (B, H, W), `Rendering.depth` of render_gaussians(..., render_depth=True) or a channel slice such as
`image[..., 0]`, read through its batch, row and pixel strides without a copy; `prior` has its shape and dtype: the
inverse depth of a monocular network, known up to scale and shift (align="affine", inverse=True), or metric sensor
depth (align="none").  mask: per-pixel weights w >= 0, bool or the dtype of the depth, (H, W) for every image or
(B, H, W), as losses.photometric_loss takes them.  Gradients flow to `depth` only.  (`Rendering.median_depth` is not
differentiable in the renderer -- it is the depth of one splat per pixel, picked by a threshold -- so a loss on it
trains nothing.)

Per image b, over pixels i with weight w_i (1 without a mask), x_i = depth_i, or 1 / depth_i with inverse=True (the
prior is taken as it is: with inverse=True it is a disparity).  A pixel is SELECTED OUT, not multiplied by 0, when
w_i = 0, when depth_i or prior_i is not finite, or when inverse=True and depth_i <= 0: it adds nothing to any sum even
if it holds NaN or Inf, and its gradient is exactly 0 -- a render is 0 where nothing was drawn and priors have holes.
With W = sum w, pm = sum w p / W, xm = sum w x / W, var = sum w (p - pm)^2, cov = sum w (p - pm)(x - xm):

    align="affine"   s = cov / var, t = xm - s pm: the least-squares map of the prior onto the render, which keeps the
                     scene's units
    align="scale"    s = sum w p x / sum w p^2, t = 0
    align="none"     s = 1, t = 0: a masked L1
    r_i = x_i - s p_i - t,    L_b = sum w_i |r_i| / W,    loss = mean over b of L_b

return_parts: also the detached per-image (L_b, s_b, t_b), (B,) each.  Degenerate cases: W = 0: L_b = 0, zero
gradient, NaN parts; var <= 1e-12 sum w p^2 (affine; a constant prior, a single pixel): s = 0, t = xm; sum w p^2 = 0
(scale): s = 0.  The threshold is compared in float64.

pearson_depth_loss is mean over b of 1 - rho_b, rho = cov / sqrt(var_p var_x) with var_x = sum w (x - xm)^2; rho_b = 0
with zero gradient when W = 0, var_p <= 1e-12 sum w p^2 or var_x <= 1e-12 sum w x^2.

The gradient is exact: the fit is differentiated through, not detached.  s and t are linear in x, so with
A = sum w sgn(r) p and B = sum w sgn(r) (sgn 0 = 0)

    affine   dL_b / dx_k = w_k / W (sgn r_k - B / W - (A - B pm)(p_k - pm) / var)
    scale    dL_b / dx_k = w_k / W (sgn r_k - A p_k / sum w p^2)
    none     dL_b / dx_k = w_k / W sgn r_k
    Pearson  drho / dx_k = w_k ((p_k - pm) / sqrt(var_p var_x) - rho (x_k - xm) / var_x)

(a degenerate fit drops the term that divides by the vanishing sum; inverse multiplies by -1 / depth_k^2).  In affine
mode sum_k g_k = 0 and sum_k g_k p_k = 0: what reaches the Gaussians is the part of w sgn(r) no change of scale or
shift could absorb.

Numerics (csrc/depth_loss.hip): float32 tensors are read as they are and everything else -- the moment sums about a
pivot, s, t, every r_i and its sign, the gradient with its 1 / depth and 1 / depth^2 -- runs in float64; each output
is rounded to float32 once.  The upstream gradient is read on the device and multiplied in before that rounding; the
per-image scalars the backward needs stay on the device in a (B, 18) float64 tensor; nothing is read back.  Every sum
has a fixed order, no atomics: loss and gradient repeat bit for bit.  float64 tensors run the same kernels on double.
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from . import _native as nv
from .losses import _check_mask, _strided, _strided_mask

__all__ = ["depth_prior_loss", "pearson_depth_loss", "fit_scale_shift"]

ALIGN = {"affine": 0, "scale": 1, "none": 2}
KIND_L1, KIND_PEARSON, KIND_FIT = 0, 1, 2
STATS = 18          # float64 per image between forward and backward
WAVE_PIXELS = 256   # pixels of one image a wave sums when the tensors are read pixel by pixel (16-byte reads: 4 or 2 x)
WORKGROUP_WAVES = 4


def _check(what, depth, prior, mask, align, inverse, return_parts=False):
    """every argument error, cheapest first and all before any launch; returns the dtype"""
    for name, t in (("depth", depth), ("prior", prior)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{what}: {name} must be a torch.Tensor, got {type(t).__name__}")
    if depth.shape != prior.shape:
        raise ValueError(f"{what}: depth {tuple(depth.shape)} and prior {tuple(prior.shape)} differ in shape")
    if depth.dim() not in (2, 3):
        raise ValueError(f"{what}: expected (H, W) or (B, H, W), got {tuple(depth.shape)}")
    if depth.numel() == 0:
        raise ValueError(f"{what}: empty image {tuple(depth.shape)}")
    if align not in ALIGN:
        raise ValueError(f"{what}: align {align!r} (\"affine\", \"scale\" or \"none\")")
    for name, v in (("inverse", inverse), ("return_parts", return_parts)):
        if not isinstance(v, bool):
            raise TypeError(f"{what}: {name} must be a bool, got {type(v).__name__}")
    if prior.requires_grad:
        raise ValueError(f"{what}: prior requires grad; gradients flow to depth only (detach the prior)")
    if not (depth.is_floating_point() and prior.is_floating_point()) or depth.dtype != prior.dtype:
        raise TypeError(f"{what}: depth is {depth.dtype}, prior {prior.dtype}; both float32, or both float64")
    if mask is not None:
        _check_mask(what, depth.unsqueeze(-1), mask)
    return nv.float_dtype(depth, prior, what=what)


class _Call:
    """one depth / prior pair, and its mask if any, prepared for the C-ABI"""

    def __init__(self, depth, prior, mask, dtype, kind, align, inverse):
        x, *self.xs = _strided(depth.detach().unsqueeze(-1))
        p, *self.ps = _strided(prior.detach().unsqueeze(-1))
        self.x, self.p = x, p
        self.B, self.H, self.W = x.shape[:3]
        self.dtype, self.modes = dtype, (int(kind), int(ALIGN[align]), int(bool(inverse)))
        self.w, self.w_args = None, (None, 0, 0, 0)
        if mask is not None:
            self.w, *ws = _strided_mask(mask, dtype)
            self.w_args = (nv.ptr(self.w), *ws)
        suffix = "_f64" if dtype == torch.float64 else ""
        self.fwd_name, self.bwd_name = "gs_depth_loss_fwd" + suffix, "gs_depth_loss_bwd" + suffix
        self.stats = None

    def _tensors(self):
        return (self.B, self.H, self.W, nv.ptr(self.x), *self.xs, nv.ptr(self.p), *self.ps, *self.w_args, *self.modes)

    def forward(self):
        lib, dev = nv.lib(), self.x.device
        results = torch.empty(1 + 3 * self.B, dtype=self.dtype, device=dev)
        self.stats = torch.empty(self.B, STATS, dtype=torch.float64, device=dev)
        nbytes = lib.gs_depth_loss_scratch_bytes(self.B, self.H, self.W)
        if nbytes < 0:
            nv.check(int(nbytes), "gs_depth_loss_scratch_bytes")
        scratch = nv.scratch(nbytes, dev)
        nv.check(getattr(lib, self.fwd_name)(*self._tensors(), nv.ptr(results), nv.ptr(self.stats), nv.ptr(scratch),
                                             nbytes, nv.stream()), self.fwd_name)
        return results

    def backward(self, g_loss):
        if nv.float_dtype(g_loss, what=self.bwd_name) != self.dtype:
            raise TypeError(f"{self.bwd_name}: {self.dtype} forward, {g_loss.dtype} gradient")
        d_depth = torch.empty(self.B, self.H, self.W, dtype=self.dtype, device=self.x.device)
        nv.check(getattr(nv.lib(), self.bwd_name)(*self._tensors(), nv.ptr(self.stats), nv.ptr(g_loss),
                                                  nv.ptr(d_depth), nv.stream()), self.bwd_name)
        return d_depth


class _DepthLoss(torch.autograd.Function):
    @staticmethod
    @nv.on_tensor_device
    def forward(ctx, depth, prior, mask, dtype, kind, align, inverse):
        call = _Call(depth, prior, mask, dtype, kind, align, inverse)
        results = call.forward()
        B = call.B
        ctx.call, ctx.depth_shape = call, depth.shape
        loss, parts = results[0], results[1:].view(3, B)
        ctx.mark_non_differentiable(parts)
        return loss, parts

    @staticmethod
    @once_differentiable
    @nv.on_tensor_device
    def backward(ctx, g_loss, _g_parts):
        d = ctx.call.backward(g_loss.contiguous())
        return d.view(ctx.depth_shape), None, None, None, None, None, None


def depth_prior_loss(depth: torch.Tensor, prior: torch.Tensor, mask: torch.Tensor | None = None, align: str = "affine",
                     inverse: bool = False, return_parts: bool = False):
    """mean over the images of sum w |x - s prior - t| / sum w, x = depth or 1 / depth (inverse), (s, t) the weighted
    least-squares fit of the prior to x per image (align: "affine", "scale", "none"), differentiated through.  Pixels
    of weight 0, of non-finite depth or prior and, with inverse, of depth <= 0 are selected out.  return_parts: also
    the detached per-image (L_b, s_b, t_b), NaN for an image without weight.  Module docstring for the rest."""
    dtype = _check("depth_prior_loss", depth, prior, mask, align, inverse, return_parts)
    loss, parts = _DepthLoss.apply(depth, prior, mask, dtype, KIND_L1, align, inverse)
    return (loss, (parts[0], parts[1], parts[2])) if return_parts else loss


def pearson_depth_loss(depth: torch.Tensor, prior: torch.Tensor, mask: torch.Tensor | None = None,
                       inverse: bool = False) -> torch.Tensor:
    """mean over the images of 1 - rho, rho the weighted Pearson correlation of prior and x = depth or 1 / depth
    (inverse) over the selected pixels; rho = 0 with zero gradient for an image without weight or with a constant prior
    or x (module docstring)."""
    dtype = _check("pearson_depth_loss", depth, prior, mask, "affine", inverse)
    return _DepthLoss.apply(depth, prior, mask, dtype, KIND_PEARSON, "affine", inverse)[0]


@nv.on_tensor_device
def _fit(depth, prior, mask, dtype, align, inverse):
    call = _Call(depth, prior, mask, dtype, KIND_FIT, align, inverse)
    parts = call.forward()[1:].view(3, call.B)
    return parts[1], parts[2]


def fit_scale_shift(depth: torch.Tensor, prior: torch.Tensor, mask: torch.Tensor | None = None, align: str = "affine",
                    inverse: bool = False):
    """the per-image (scale, shift) depth_prior_loss fits, (B,) each and detached: prior * scale + shift is the prior
    in the render's units (inverse=True: in its inverse units).  NaN for an image without weight."""
    dtype = _check("fit_scale_shift", depth, prior, mask, align, inverse)
    return _fit(depth, prior, mask, dtype, align, inverse)
