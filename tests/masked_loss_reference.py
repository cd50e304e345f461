"""The yardstick of the masked-loss tests: the weighted means of |x - y| and of the SSIM map, restated in torch on the
CPU from ssim_reference.ssim_map (which the mask does not change), in the dtype of the inputs.  With w >= 0 per pixel,
S its sum over every pixel and batch entry, S_v its sum over the pixels `padding` counts:

    L = sum w |x - y| / (C S),   M = sum_counted w m / (C S_v),   loss = (1 - lam) L + lam (1 - M)

A term whose weight sum is zero contributes nothing and its part is NaN.  Gradients come from torch autograd.  Shares no
code with taichi_gaussian_rasterizer_amd.losses.  Also the seeded masks of the tests."""
import torch

import ssim_reference as ref


def _weights(x, mask):
    """the mask as (B, H, W, 1) weights in the dtype of x, an (H, W) mask applying to every batch entry"""
    w = mask.to(x.dtype)
    batch = x.shape[0] if x.dim() == 4 else 1
    return w.expand((batch,) + tuple(x.shape[-3:-1])).unsqueeze(-1)


def _batched(t):
    return t if t.dim() == 4 else t.unsqueeze(0)


def parts(x, y, mask, window_size=11, sigma=1.5, data_range=1.0, padding="same"):
    """(L, M, S, S_v); L or M is NaN where its weight sum is zero"""
    w = _weights(x, mask)
    C = x.shape[-1]
    m = _batched(ref.ssim_map(x, y, window_size, sigma, data_range))
    wv = w
    if padding == "valid":
        r = window_size // 2
        m = m[:, r:m.shape[1] - r, r:m.shape[2] - r]
        wv = w[:, r:w.shape[1] - r, r:w.shape[2] - r]
    S, Sv = w.sum(), wv.sum()
    nan = x.sum() * 0.0 + float("nan")   # attached to x, with a zero gradient
    L = (w * (_batched(x) - _batched(y)).abs()).sum() / (C * S) if float(S) > 0 else nan
    M = (wv * m).sum() / (C * Sv) if float(Sv) > 0 else nan
    return L, M, S, Sv


def ssim(x, y, mask, window_size=11, sigma=1.5, data_range=1.0, padding="same"):
    return parts(x, y, mask, window_size, sigma, data_range, padding)[1]


def photometric_loss(x, y, mask, ssim_weight=0.2, window_size=11, sigma=1.5, data_range=1.0, padding="same"):
    L, M, S, Sv = parts(x, y, mask, window_size, sigma, data_range, padding)
    loss = x.sum() * 0.0   # an empty term leaves the loss attached to x with a zero gradient
    if float(S) > 0:
        loss = loss + (1.0 - ssim_weight) * L
    if float(Sv) > 0 and ssim_weight != 0.0:
        loss = loss + ssim_weight * (1.0 - M)
    return loss


def grad_of(fn, x, y, mask, **kw):
    """(value, d value / d x) by torch autograd"""
    x = x.detach().clone().requires_grad_(True)
    value = fn(x, y, mask, **kw)
    (g,) = torch.autograd.grad(value, x)
    return value.detach(), g


# --------------------------------------------------------------------------------------------------- masks
MASKS = ("random", "hole", "one-tile", "single-pixel", "broadcast")


def make_mask(kind, shape, seed=0):
    """float32 weights for an image of `shape` ((H, W, C) or (B, H, W, C)): shaped shape[:-1], or (H, W) for
    "broadcast".  The regions are clipped to the image, so small images get what fits of them."""
    gen = torch.Generator().manual_seed(1000 + seed)
    lead = tuple(shape[:-1])
    H, W = lead[-2:]
    if kind == "random":
        return torch.rand(lead, generator=gen, dtype=torch.float32)
    if kind == "broadcast":
        return torch.rand((H, W), generator=gen, dtype=torch.float32)
    if kind == "hole":      # crosses the tile edge at 16 in both directions
        m = torch.ones(lead, dtype=torch.float32)
        m[..., 10:30, 5:19] = 0.0
        return m
    m = torch.zeros(lead, dtype=torch.float32)
    if kind == "one-tile":
        m[..., 16:32, 0:16] = torch.rand(m[..., 16:32, 0:16].shape, generator=gen, dtype=torch.float32) + 0.25
        return m
    if kind == "single-pixel":
        m[..., min(20, H - 1), min(17, W - 1)] = 1.0
        return m
    raise ValueError(kind)
