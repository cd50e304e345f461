"""Yardstick of appearance.slice_bilateral_grid: torch's grid_sample followed by the affine, meant for CPU tensors in
float64 (it runs on any device and dtype: the float32 composition on the device is the same function), and an explicit
per-pixel loop of the formula that the yardstick is checked against."""
import torch
import torch.nn.functional as F

LUMA = (0.299, 0.587, 0.114)


def luma_of(image):
    return (image * image.new_tensor(LUMA)).sum(-1)


def slice_reference(grid, image, guide=None):
    """grid (12, L, Hg, Wg) or (B, 12, L, Hg, Wg); image (H, W, 3) or (B, H, W, 3); guide shaped image.shape[:-1]"""
    batched = image.dim() == 4
    x, g = (image, grid) if batched else (image[None], grid[None])
    B, H, W, _ = x.shape
    z = luma_of(x) if guide is None else (guide if batched else guide[None])
    u = ((torch.arange(W, dtype=x.dtype, device=x.device) + 0.5) / W).expand(B, H, W)
    v = ((torch.arange(H, dtype=x.dtype, device=x.device) + 0.5) / H).view(1, H, 1).expand(B, H, W)
    coords = torch.stack([u, v, z], dim=-1) * 2 - 1
    A = F.grid_sample(g, coords[:, None], mode="bilinear", padding_mode="border", align_corners=True)  # (B, 12, 1, H, W)
    A = A[:, :, 0].permute(0, 2, 3, 1).reshape(B, H, W, 3, 4)
    out = (A[..., :3] @ x[..., None])[..., 0] + A[..., 3]
    return out if batched else out[0]


def slice_loop(grid, image, guide=None):
    """the formula of the module docstring, pixel by pixel, for one (H, W, 3) image and one (12, L, Hg, Wg) grid"""
    _, L, Hg, Wg = grid.shape
    H, W, _ = image.shape

    def cell(coord, size):
        c = 0 if size == 1 else min(int(torch.floor(coord.detach())), size - 2)
        return c, min(c + 1, size - 1), coord - c

    def lerp(a, b, f):
        return a + (b - a) * f

    rows = []
    for y in range(H):
        row = []
        for x in range(W):
            rgb = image[y, x]
            luma = (rgb * rgb.new_tensor(LUMA)).sum() if guide is None else guide[y, x]
            gx = torch.tensor((x + 0.5) / W * (Wg - 1), dtype=image.dtype)
            gy = torch.tensor((y + 0.5) / H * (Hg - 1), dtype=image.dtype)
            gz = luma.clamp(0, 1) * (L - 1)
            (x0, x1, fx), (y0, y1, fy), (z0, z1, fz) = cell(gx, Wg), cell(gy, Hg), cell(gz, L)
            planes = []
            for zz in (z0, z1):
                top = lerp(grid[:, zz, y0, x0], grid[:, zz, y0, x1], fx)
                bot = lerp(grid[:, zz, y1, x0], grid[:, zz, y1, x1], fx)
                planes.append(lerp(top, bot, fy))
            A = lerp(planes[0], planes[1], fz).view(3, 4)
            row.append(A[:, :3] @ rgb + A[:, 3])
        rows.append(torch.stack(row))
    return torch.stack(rows)


def grads_of(fn, grid, image, guide=None, upstream=None):
    """value and the gradients for grid, image and guide (None without one) of sum(fn(...) * upstream)"""
    leaves = [t.detach().clone().requires_grad_(True) for t in (grid, image)]
    gd = None if guide is None else guide.detach().clone().requires_grad_(True)
    out = fn(leaves[0], leaves[1], gd)
    (out * (torch.ones_like(out) if upstream is None else upstream)).sum().backward()
    return out.detach(), leaves[0].grad, leaves[1].grad, None if gd is None else gd.grad


def smooth_pixels(image, guide, L, margin=1e-4):
    """bool image.shape[:-1]: the pixels where d_image and d_guide are continuous -- the float64 luma (or guide) at least
    `margin` from 0 and 1 and, inside [0, 1], luma * (L - 1) at least `margin` from an integer (no cell boundary
    without a second level)"""
    z = (luma_of(image.double()) if guide is None else guide.double())
    keep = ((z - 0).abs() >= margin) & ((z - 1).abs() >= margin)
    if L > 1:
        gz = z * (L - 1)
        keep &= ((gz - gz.round()).abs() >= margin) | (z < 0) | (z > 1)
    return keep


def random_case(shape, grid_sizes, seed=0, batch=None, dtype=torch.float64, spread=0.3):
    """image and guide uniform in [-0.2, 1.2], a grid of identity plus uniform noise, an upstream gradient"""
    gen = torch.Generator().manual_seed(seed)
    lead = () if batch is None else (batch,)
    image = torch.rand(*lead, *shape, 3, generator=gen, dtype=torch.float64) * 1.4 - 0.2
    guide = torch.rand(*lead, *shape, generator=gen, dtype=torch.float64) * 1.4 - 0.2
    grid = torch.zeros(*lead, 12, *grid_sizes, dtype=torch.float64)
    grid[..., (0, 5, 10), :, :, :] = 1
    grid = grid + spread * (torch.rand(grid.shape, generator=gen, dtype=torch.float64) - 0.5)
    upstream = torch.rand(*lead, *shape, 3, generator=gen, dtype=torch.float64) - 0.5
    return tuple(t.to(dtype) for t in (grid, image, guide, upstream))
