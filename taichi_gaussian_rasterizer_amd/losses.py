"""Photometric training losses on channel-last images (HIP): SSIM and (1 - w) * L1 + w * (1 - SSIM).

    ssim(image, target)              -> mean SSIM (0-dim), or the per-pixel map with reduction="none"
    photometric_loss(image, target)  -> (1 - ssim_weight) * mean|image - target| + ssim_weight * (1 - ssim)

Both take (H, W, C) or (B, H, W, C) tensors as `Rendering.image` is laid out -- no permute to channel-first -- and read
them through their strides, so `image[..., 2:]` of a depth render or a row view goes in without a copy.  One fused
kernel per direction (csrc/loss.hip): 11x11 Gaussian window (any odd size 3..15), zero padding, second moments on
pivot-shifted values, which keeps the float32 map and gradient accurate on smooth, flat and nearly equal images where
the textbook E[x^2] - mu^2 composition cancels.  Loss and gradient repeat bit for bit.  Gradients flow to `image`
only; float32, or float64 when both tensors are (gradcheck).

mask=: per-pixel weights w >= 0 (an object, sky or distractor mask, a confidence, `Rendering.image_weight`), shaped
image.shape[:-1] or (H, W) for every batch entry, bool or the dtype of the image, read through its strides.  Both means
become weighted means in the same two kernels,

    L = sum w |x - y| / (C sum w),    M = sum w ssim_map / (C sum w over the pixels padding counts),

the SSIM map itself is that of the whole images.  A term whose weights sum to zero adds nothing to the loss and zero to
the gradient (its part is NaN), so an all-zero mask gives loss 0 and d_image 0.  The weights must be finite and
non-negative; that is not checked (it would cost a host synchronisation).  No gradient flows to the mask.
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from . import _native as nv

__all__ = ["ssim", "photometric_loss", "gaussian_window"]


def gaussian_window(window_size: int = 11, sigma: float = 1.5) -> torch.Tensor:
    """the float32 1-D window the kernels use (gs_ssim_window), as a CPU tensor"""
    _check_window(window_size, sigma)
    import ctypes
    out = (ctypes.c_float * int(window_size))()
    nv.check(nv.lib().gs_ssim_window(int(window_size), float(sigma), out), "gs_ssim_window")
    return torch.tensor(list(out), dtype=torch.float32)


def _check_window(window_size, sigma) -> None:
    if not isinstance(window_size, int) or isinstance(window_size, bool):
        raise TypeError(f"window_size must be an int, got {type(window_size).__name__}")
    if window_size % 2 == 0 or not 3 <= window_size <= 15:
        raise ValueError(f"window_size {window_size}: an odd size from 3 to 15")
    if not float(sigma) > 0.0:
        raise ValueError(f"sigma {sigma} must be positive")


def _check_mask(what, image, mask) -> None:
    if not isinstance(mask, torch.Tensor):
        raise TypeError(f"{what}: mask must be a torch.Tensor, got {type(mask).__name__}")
    if mask.dtype not in (torch.bool, image.dtype):
        raise TypeError(f"{what}: mask is {mask.dtype}; torch.bool, or {image.dtype} as the image")
    if mask.shape != image.shape[:-1] and not (image.dim() == 4 and mask.shape == image.shape[1:3]):
        raise ValueError(f"{what}: mask {tuple(mask.shape)} for an image {tuple(image.shape)}: expected "
                         f"{tuple(image.shape[:-1])}" + (f" or {tuple(image.shape[1:3])}" if image.dim() == 4 else ""))
    if mask.requires_grad:
        raise ValueError(f"{what}: mask requires grad; gradients flow to image only (detach the mask)")
    if mask.device != image.device:
        raise TypeError(f"{what}: mask on {mask.device}, image on {image.device}")


def _check(what, image, target, window_size, sigma, data_range, padding, mask=None):
    """every argument error, cheapest first and all before any launch; returns (dtype, valid)"""
    for name, t in (("image", image), ("target", target)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{what}: {name} must be a torch.Tensor, got {type(t).__name__}")
    if image.shape != target.shape:
        raise ValueError(f"{what}: image {tuple(image.shape)} and target {tuple(target.shape)} differ in shape")
    if image.dim() not in (3, 4):
        raise ValueError(f"{what}: expected (H, W, C) or (B, H, W, C), got {tuple(image.shape)}")
    if image.numel() == 0:
        raise ValueError(f"{what}: empty image {tuple(image.shape)}")
    _check_window(window_size, sigma)
    if not float(data_range) > 0.0:
        raise ValueError(f"{what}: data_range {data_range} must be positive")
    if padding not in ("same", "valid"):
        raise ValueError(f"{what}: padding {padding!r} (\"same\" or \"valid\")")
    if padding == "valid" and (image.shape[-3] < window_size or image.shape[-2] < window_size):
        raise ValueError(f"{what}: padding=\"valid\" needs an image of at least {window_size} x {window_size}, got "
                         f"{image.shape[-3]} x {image.shape[-2]}")
    if target.requires_grad:
        raise ValueError(f"{what}: target requires grad; gradients flow to image only (detach the target)")
    if not (image.is_floating_point() and target.is_floating_point()) or image.dtype != target.dtype:
        raise TypeError(f"{what}: image is {image.dtype}, target {target.dtype}; both float32, or both float64")
    if mask is not None:
        _check_mask(what, image, mask)
    return nv.float_dtype(image, target, what=what), int(padding == "valid")


def _strided(t: torch.Tensor):
    """(B, H, W, C) view of `t` and its batch / row / pixel strides in elements, copying only what the kernels cannot
    read: channels not contiguous, overlapping or reversed strides"""
    if t.dim() == 3:
        t = t.unsqueeze(0)
    B, H, W, C = t.shape
    sb, sr, sp, sc = t.stride()
    ok = (sc == 1 or C == 1) and sp >= C and sr >= W * sp and (B == 1 or sb >= H * sr)
    if not ok:
        t = t.contiguous()
        sb, sr, sp, _ = t.stride()
    if B == 1:
        sb = H * sr
    return t, sb, sr, sp


def _strided_mask(mask: torch.Tensor, dtype):
    """(H, W) or (B, H, W) weights in `dtype` and their batch / row / pixel strides in elements; batch stride 0 lets
    one (H, W) mask (or an expand() of it) serve every batch entry.  A bool mask is converted with one op; a copy is made
    only of what the kernels cannot read (overlapping rows or batches)"""
    w = mask if mask.dtype == dtype else mask.to(dtype)
    if w.dim() == 2:
        w = w.unsqueeze(0)
    B, H, W = w.shape
    sb, sr, sp = w.stride()
    if not (sp >= 1 and sr >= W * sp and (B == 1 or sb == 0 or sb >= H * sr)):
        w = w.contiguous()
        sb, sr, sp = w.stride()
    if B == 1:
        sb = 0
    return w, sb, sr, sp


class _Call:
    """one image pair, and its mask if any, prepared for the C-ABI: views, strides, the entry points of its dtype"""

    def __init__(self, image, target, dtype, window_size, sigma, valid, mask=None):
        self.x, *self.xs = _strided(image.detach())
        self.y, *self.ys = _strided(target.detach())
        self.shape = tuple(self.x.shape)
        self.dtype, self.ws, self.sigma, self.valid = dtype, int(window_size), float(sigma), int(valid)
        lib = nv.lib()
        stem = "gs_photo_loss_weighted" if mask is not None else "gs_photo_loss"
        suffix = "_f64" if dtype == torch.float64 else ""
        self.fwd_name, self.bwd_name = f"{stem}_fwd{suffix}", f"{stem}_bwd{suffix}"
        self.fwd_fn, self.bwd_fn = getattr(lib, self.fwd_name), getattr(lib, self.bwd_name)
        self.scratch_fn = getattr(lib, f"{stem}_scratch_bytes")
        self.weighted = mask is not None
        self.w_args, self.results = (), None   # the weight and its strides; the forward's results, [3:] = [S, S_v]
        if self.weighted:
            self.w, *ws = _strided_mask(mask, dtype)
            self.w_args = (nv.ptr(self.w), *ws)

    def forward(self, data_range, ssim_weight, want_map, want_saved):
        B, H, W, C = self.shape
        dev = self.x.device
        results = torch.empty(5 if self.weighted else 3, dtype=self.dtype, device=dev)
        ssim_map = torch.empty(self.shape, dtype=self.dtype, device=dev) if want_map else None
        saved = torch.empty((3,) + self.shape, dtype=self.dtype, device=dev) if want_saved else None
        nbytes = self.scratch_fn(B, H, W, C)
        scratch = nv.scratch(nbytes, dev)
        nv.check(self.fwd_fn(B, H, W, C, nv.ptr(self.x), *self.xs, nv.ptr(self.y), *self.ys, *self.w_args, self.ws,
                             self.sigma, float(data_range), float(ssim_weight), self.valid, nv.ptr(ssim_map),
                             nv.ptr(saved), nv.ptr(scratch), nbytes, nv.ptr(results), nv.stream()), self.fwd_name)
        self.results = results
        return results, ssim_map, saved

    def backward(self, saved, upstream, grad, l1_coeff, ssim_coeff):
        B, H, W, C = self.shape
        d_image = torch.empty(self.shape, dtype=self.dtype, device=self.x.device)
        for t in (upstream, grad):
            if t is not None and nv.float_dtype(t, what=self.bwd_name) != self.dtype:
                raise TypeError(f"{self.bwd_name}: {self.dtype} forward, {t.dtype} gradient")
        norm = (nv.ptr(self.results[3:]),) if self.weighted else ()   # read on the device: no copy to the host
        nv.check(self.bwd_fn(B, H, W, C, nv.ptr(self.x), *self.xs, nv.ptr(self.y), *self.ys, *self.w_args, *norm,
                             self.ws, self.sigma, self.valid, nv.ptr(saved), nv.ptr(upstream), nv.ptr(grad),
                             float(l1_coeff), float(ssim_coeff), nv.ptr(d_image), nv.stream()), self.bwd_name)
        return d_image


class _PhotometricLoss(torch.autograd.Function):
    @staticmethod
    @nv.on_tensor_device
    def forward(ctx, image, target, dtype, ssim_weight, window_size, sigma, data_range, valid, mask):
        call = _Call(image, target, dtype, window_size, sigma, valid, mask)
        need = ctx.needs_input_grad[0]
        results, _, saved = call.forward(data_range, ssim_weight, False, need and ssim_weight != 0.0)
        ctx.call, ctx.saved, ctx.ssim_weight, ctx.image_shape = call, saved, float(ssim_weight), image.shape
        loss, l1, ssim_mean = results[0], results[1], results[2]
        ctx.mark_non_differentiable(l1, ssim_mean)
        return loss, l1, ssim_mean

    @staticmethod
    @once_differentiable
    @nv.on_tensor_device
    def backward(ctx, g_loss, _g_l1, _g_ssim):
        w = ctx.ssim_weight
        d = ctx.call.backward(ctx.saved, None, g_loss.contiguous(), 1.0 - w, -w)
        return d.view(ctx.image_shape), None, None, None, None, None, None, None, None


class _SSIM(torch.autograd.Function):
    @staticmethod
    @nv.on_tensor_device
    def forward(ctx, image, target, dtype, window_size, sigma, data_range, valid, want_map, mask):
        call = _Call(image, target, dtype, window_size, sigma, valid, mask)
        results, ssim_map, saved = call.forward(data_range, 1.0, want_map, ctx.needs_input_grad[0])
        ctx.call, ctx.saved, ctx.want_map, ctx.image_shape = call, saved, want_map, image.shape
        return ssim_map.view(image.shape) if want_map else results[2]

    @staticmethod
    @once_differentiable
    @nv.on_tensor_device
    def backward(ctx, g):
        if ctx.want_map:
            d = ctx.call.backward(ctx.saved, g.reshape(ctx.call.shape).contiguous(), None, 0.0, 0.0)
        else:
            d = ctx.call.backward(ctx.saved, None, g.contiguous(), 0.0, 1.0)
        return d.view(ctx.image_shape), None, None, None, None, None, None, None, None


def ssim(image: torch.Tensor, target: torch.Tensor, window_size: int = 11, sigma: float = 1.5,
         data_range: float = 1.0, padding: str = "same", reduction: str = "mean",
         mask: torch.Tensor | None = None) -> torch.Tensor:
    """Structural similarity of two channel-last images.  reduction="mean": the mean over every pixel, channel and
    batch entry (padding="valid": over the pixels whose window lies inside the image); "none": the map, shaped as the
    input (padding does not change it).  mask: per-pixel weights of the mean (module docstring); the map has nothing
    to weight, so reduction="none" refuses one."""
    if reduction not in ("mean", "none"):
        raise ValueError(f"ssim: reduction {reduction!r} (\"mean\" or \"none\")")
    if mask is not None and reduction == "none":
        raise ValueError("ssim: reduction \"none\" returns the map, which a mask does not change; weight it yourself")
    dtype, valid = _check("ssim", image, target, window_size, sigma, data_range, padding, mask)
    return _SSIM.apply(image, target, dtype, window_size, sigma, data_range, valid, reduction == "none", mask)


def photometric_loss(image: torch.Tensor, target: torch.Tensor, ssim_weight: float = 0.2, window_size: int = 11,
                     sigma: float = 1.5, data_range: float = 1.0, padding: str = "same", return_parts: bool = False,
                     mask: torch.Tensor | None = None):
    """(1 - ssim_weight) * mean|image - target| + ssim_weight * (1 - ssim(image, target)), the 3DGS training loss, in
    one kernel per direction.  ssim_weight = 0 skips the SSIM work.  return_parts: also the detached (l1, ssim) means
    of the same pass, for logging (ssim is NaN when it was skipped).  mask: per-pixel weights of both means (module
    docstring); a mean without weight is NaN in the parts and absent from the loss."""
    if not 0.0 <= float(ssim_weight) <= 1.0:
        raise ValueError(f"photometric_loss: ssim_weight {ssim_weight} outside [0, 1]")
    dtype, valid = _check("photometric_loss", image, target, window_size, sigma, data_range, padding, mask)
    loss, l1, ssim_mean = _PhotometricLoss.apply(image, target, dtype, float(ssim_weight), window_size, sigma,
                                                 data_range, valid, mask)
    return (loss, (l1, ssim_mean)) if return_parts else loss
