"""The yardstick of the loss tests: SSIM and the photometric loss restated from torch.nn.functional.conv2d (grouped, 2-D
window, zero padding), on the CPU, in the dtype of its inputs -- float64 is "truth", float32 is what a user composing
the loss from torch ops has today.  Gradients come from torch autograd.  Shares no code with
taichi_gaussian_rasterizer_amd.losses.

Also the seeded input classes of the accuracy tests.  Inputs are generated in float32 and converted to float64 for
truth, so every version sees the same numbers and sign(x - y) cannot flip in a conversion."""
import math

import torch
import torch.nn.functional as F


def window_1d(window_size=11, sigma=1.5, dtype=torch.float64):
    """g[i] = exp(-(i - (ws - 1) / 2)^2 / (2 sigma^2)), normalised to sum 1 in double, then rounded to `dtype`"""
    g = [math.exp(-((i - (window_size - 1) / 2) ** 2) / (2.0 * sigma * sigma)) for i in range(window_size)]
    total = math.fsum(g)
    return torch.tensor([v / total for v in g], dtype=torch.float64).to(dtype)


def _channel_first(t):
    t = t if t.dim() == 4 else t.unsqueeze(0)
    return t.permute(0, 3, 1, 2)


def ssim_map(x, y, window_size=11, sigma=1.5, data_range=1.0):
    """per-pixel, per-channel SSIM of channel-last x, y ((H, W, C) or (B, H, W, C)), shaped as the input"""
    shape = x.shape
    x, y = _channel_first(x), _channel_first(y)
    C = x.shape[1]
    g = window_1d(window_size, sigma, x.dtype)
    w = torch.outer(g, g).expand(C, 1, window_size, window_size).contiguous()
    pad = window_size // 2

    def blur(t):
        return F.conv2d(t, w, padding=pad, groups=C)

    mu_x, mu_y = blur(x), blur(y)
    var_x = blur(x * x) - mu_x * mu_x
    var_y = blur(y * y) - mu_y * mu_y
    cov = blur(x * y) - mu_x * mu_y
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    m = ((2 * mu_x * mu_y + c1) * (2 * cov + c2)) / ((mu_x * mu_x + mu_y * mu_y + c1) * (var_x + var_y + c2))
    return m.permute(0, 2, 3, 1).reshape(shape)


def ssim(x, y, window_size=11, sigma=1.5, data_range=1.0, padding="same"):
    m = ssim_map(x, y, window_size, sigma, data_range)
    if padding == "valid":
        r = window_size // 2
        m = m[..., r:m.shape[-3] - r, r:m.shape[-2] - r, :]
    return m.mean()


def photometric_loss(x, y, ssim_weight=0.2, window_size=11, sigma=1.5, data_range=1.0, padding="same"):
    l1 = (x - y).abs().mean()
    return (1.0 - ssim_weight) * l1 + ssim_weight * (1.0 - ssim(x, y, window_size, sigma, data_range, padding))


def grad_of(fn, x, y, **kw):
    """(value, d value / d x) by torch autograd"""
    x = x.detach().clone().requires_grad_(True)
    value = fn(x, y, **kw)
    (g,) = torch.autograd.grad(value, x)
    return value.detach(), g


# ------------------------------------------------------------------------------------------------- inputs
CLASSES = ("noise", "smooth", "flat", "near-equal")
SIZES = ((203, 157, 3), (2, 61, 45, 4), (70, 50, 1), (9, 5, 1))


def _pattern(shape):
    """0.5 + 0.4 sin(x / 17 + c) cos(y / 23 - c) per channel c, float32"""
    H, W, C = shape[-3:]
    yy = torch.arange(H, dtype=torch.float32).view(H, 1, 1)
    xx = torch.arange(W, dtype=torch.float32).view(1, W, 1)
    cc = torch.arange(C, dtype=torch.float32).view(1, 1, C)
    p = 0.5 + 0.4 * torch.sin(xx / 17 + cc) * torch.cos(yy / 23 - cc)
    return p.expand(shape).contiguous()


def make_pair(kind, shape, seed=0):
    """(render, target), float32 CPU tensors of `shape`"""
    gen = torch.Generator().manual_seed(seed)
    u = torch.rand(shape, generator=gen, dtype=torch.float32)
    if kind == "noise":
        return u, torch.rand(shape, generator=gen, dtype=torch.float32)
    if kind == "smooth":
        target = _pattern(shape)
        return target + 0.02 * (u - 0.5), target
    if kind == "flat":
        target = torch.full(shape, 0.7, dtype=torch.float32)
        return target + 1e-3 * (u - 0.5), target
    if kind == "near-equal":
        target = _pattern(shape)
        return target + 1e-4 * (u - 0.5), target
    raise ValueError(kind)


def normwise(error, truth):
    """max |error| over max |truth|"""
    return float(error.abs().max()) / max(float(truth.abs().max()), 1e-300)
