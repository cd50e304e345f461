"""appearance.slice_bilateral_grid on the GPU against tests/bilagrid_reference.py (grid_sample + affine, CPU float64).

Float64: value, d_grid, d_image, d_guide at rtol 1e-10 / atol 1e-12 (the same float64 arithmetic in another order).
d_image and d_guide are discontinuous where gz crosses a cell boundary or the luma crosses 0 or 1; the pixels whose
float64 luma * (L - 1) lies within 1e-4 of an integer or whose luma lies within 1e-4 of 0 or 1 are left out of those two
comparisons (bilagrid_reference.smooth_pixels), at most 1 % of the pixels.  Float32: against the float64 yardstick on
the same float32 inputs, each output within 4 times the error the float32 torch composition makes on the device (floor
1e-6 of the output's largest magnitude); the same pixels are left out of d_image and d_guide, since 1e-4 is far above
what float32 rounding moves gz by.  Shapes: every tile edge the host can choose -- 8 (small images), 16 (512 x 512),
32 (1024 x 1024), and 4, 2, 1 where a grid is finer than the image (5 x 6 under 16 x 16 nodes).

`python tests/test_bilagrid_gpu.py [PATH]` writes the float32 errors of both paths (profiles/bilagrid/accuracy.txt)."""
import math
import os
import sys

import pytest
import torch
from torch.autograd import gradcheck

import bilagrid_reference as ref
import ssim_reference
import taichi_gaussian_rasterizer_amd as gs
from taichi_gaussian_rasterizer_amd import RasterConfig, appearance, losses, scenes
from taichi_gaussian_rasterizer_amd.appearance import slice_bilateral_grid

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IMAGES = ((1, 1), (5, 6), (37, 53), (64, 130))
GRIDS = ((1, 1, 1), (2, 1, 7), (4, 3, 5), (8, 16, 16))
LARGE = (((512, 512), (8, 16, 16)), ((1024, 1024), (4, 3, 5)))  # 16 x 16 and 32 x 32 pixel tiles
F64 = dict(rtol=1e-10, atol=1e-12)
NAMES = ("value", "d_grid", "d_image", "d_guide")


def _hip(grid, image, guide, upstream, fn=slice_bilateral_grid):
    """value and gradients of `fn` on the device for CPU tensors, back on the CPU in double"""
    out = ref.grads_of(fn, grid.to(DEV), image.to(DEV), None if guide is None else guide.to(DEV), upstream.to(DEV))
    return [None if t is None else t.cpu().double() for t in out]


def _yardstick(grid, image, guide, upstream):
    return ref.grads_of(ref.slice_reference, grid.double(), image.double(), None if guide is None else guide.double(),
                        upstream.double())


_CASES = {}


def _case(shape, sizes, batch=None, with_guide=False):
    """one seeded float64 case and its yardstick, computed once and shared"""
    key = (shape, sizes, batch, with_guide)
    if key not in _CASES:
        grid, image, guide, upstream = ref.random_case(shape, sizes, seed=0, batch=batch)
        guide = guide if with_guide else None
        keep = ref.smooth_pixels(image, guide, sizes[0])
        _CASES[key] = (grid, image, guide, upstream, keep, _yardstick(grid, image, guide, upstream))
    return _CASES[key]


def _left_out_share(keep):
    share = 1.0 - float(keep.double().mean())
    assert share <= 0.01, f"{share:.2%} of the pixels left out"
    return share


def _compare_f64(got, want, keep):
    for name, a, b in zip(NAMES, got, want):
        if b is None:
            assert a is None
            continue
        if name in ("d_image", "d_guide"):
            a, b = a[keep], b[keep]
        assert torch.allclose(a, b, **F64), f"{name}: max |difference| {float((a - b).abs().max()):.3e}"


@pytest.mark.parametrize("sizes", GRIDS)
@pytest.mark.parametrize("shape", IMAGES)
def test_float64_against_the_yardstick(shape, sizes):
    for with_guide in (False, True):
        grid, image, guide, upstream, keep, want = _case(shape, sizes, None, with_guide)
        _left_out_share(keep)
        _compare_f64(_hip(grid, image, guide, upstream), want, keep)


@pytest.mark.parametrize("shape,sizes", LARGE)
def test_float64_on_the_larger_pixel_tiles(shape, sizes):
    grid, image, guide, upstream, keep, want = _case(shape, sizes, None, shape[0] == 1024)
    _left_out_share(keep)
    _compare_f64(_hip(grid, image, guide, upstream), want, keep)


def test_float64_batch_of_two_with_two_grids():
    for with_guide in (False, True):
        grid, image, guide, upstream, keep, want = _case((37, 53), (4, 3, 5), 2, with_guide)
        assert not torch.equal(grid[0], grid[1])
        _compare_f64(_hip(grid, image, guide, upstream), want, keep)
        # and each entry alone gives the same bits as its place in the batch
        both = _hip(grid, image, guide, upstream)
        for i in range(2):
            one = _hip(grid[i], image[i], None if guide is None else guide[i], upstream[i])
            for a, b in zip(one, both):
                assert (a is None and b is None) or torch.equal(a, b[i])


# ------------------------------------------------------------------------------------------------- float32
def _float32_errors(shape, sizes, with_guide, batch=None):
    """per output: (error of the HIP operator, error of the float32 torch composition on the device, magnitude), all
    against the float64 yardstick on the same float32 inputs"""
    grid, image, guide, upstream = (t.float() for t in ref.random_case(shape, sizes, seed=0, batch=batch))
    guide = guide if with_guide else None
    keep = ref.smooth_pixels(image, guide, sizes[0])
    _left_out_share(keep)
    want = _yardstick(grid, image, guide, upstream)
    ours = _hip(grid, image, guide, upstream)
    theirs = _hip(grid, image, guide, upstream, fn=ref.slice_reference)
    rows = {}
    for name, a, t, w in zip(NAMES, ours, theirs, want):
        if w is None:
            continue
        if name in ("d_image", "d_guide"):
            a, t, w = a[keep], t[keep], w[keep]
        rows[name] = (float((a - w).abs().max()), float((t - w).abs().max()), float(w.abs().max()))
    return rows


def _assert_float32(rows, what):
    for name, (ours, theirs, scale) in rows.items():
        bound = max(4.0 * theirs, 1e-6 * scale)
        print(f"{what} {name}: HIP {ours:.3e}, torch float32 {theirs:.3e}, bound {bound:.3e}, magnitude {scale:.3e}")
        assert ours <= bound, f"{what} {name}: {ours:.3e} > {bound:.3e} (torch float32: {theirs:.3e})"


@pytest.mark.parametrize("sizes", GRIDS)
@pytest.mark.parametrize("shape", IMAGES)
def test_float32_within_four_times_the_torch_compositions_error(shape, sizes):
    for with_guide in (False, True):
        _assert_float32(_float32_errors(shape, sizes, with_guide), f"{shape} {sizes} guide={with_guide}")


@pytest.mark.parametrize("shape,sizes", LARGE)
def test_float32_on_the_larger_pixel_tiles(shape, sizes):
    _assert_float32(_float32_errors(shape, sizes, shape[0] == 1024), f"{shape} {sizes}")


def test_float32_batch_of_two():
    _assert_float32(_float32_errors((37, 53), (8, 16, 16), False, batch=2), "batch of two")


# ------------------------------------------------------------------------------------------- exact properties
@pytest.mark.parametrize("shape", [(37, 53), (64, 130), (512, 512)])
def test_identity_grid_returns_the_image_bit_for_bit(shape):
    _, image, guide, _ = ref.random_case(shape, (1, 1, 1), seed=3, dtype=torch.float32)
    assert float(image.min()) < 0 and float(image.max()) > 1
    image, guide = image.to(DEV), guide.to(DEV)
    for sizes in ((8, 16, 16), (1, 1, 1), (4, 3, 5)):
        grid = appearance.identity_grids(1, *sizes, device=DEV)[0]
        assert torch.equal(slice_bilateral_grid(grid, image), image)
        assert torch.equal(slice_bilateral_grid(grid, image, guide), image)


@pytest.mark.parametrize("shape,sizes", [((37, 53), (8, 16, 16)), ((64, 130), (4, 3, 5)), ((512, 512), (8, 16, 16))])
def test_two_runs_give_identical_bits(shape, sizes):
    for with_guide in (False, True):
        grid, image, guide, upstream = (t.to(DEV) for t in ref.random_case(shape, sizes, seed=4, dtype=torch.float32))
        runs = [ref.grads_of(slice_bilateral_grid, grid, image, guide if with_guide else None, upstream)
                for _ in range(2)]
        for a, b in zip(*runs):
            assert (a is None and b is None) or torch.equal(a, b)


def _gradcheck_inputs(with_guide):
    """a 5 x 6 image under a (3, 2, 2) grid whose guide (or luma) keeps 0.05 away from 0, 0.5 and 1, where
    gz = 2 * guide crosses a cell boundary or the clamp"""
    gen = torch.Generator().manual_seed(5)

    def good(z):
        return (z > 0.05) & (z < 0.95) & ((z - 0.5).abs() > 0.025)

    cand = torch.rand(4000, 3, generator=gen, dtype=torch.float64)
    image = cand[good(ref.luma_of(cand))][:30].reshape(5, 6, 3)
    z = torch.rand(4000, generator=gen, dtype=torch.float64)
    guide = z[good(z)][:30].reshape(5, 6) if with_guide else None
    grid = torch.rand(12, 3, 2, 2, generator=gen, dtype=torch.float64)
    return grid, image, guide


@pytest.mark.parametrize("with_guide", [False, True])
def test_gradcheck_float64(with_guide):
    grid, image, guide = _gradcheck_inputs(with_guide)
    z = ref.luma_of(image) if guide is None else guide
    assert float((2 * z - (2 * z).round()).abs().min()) >= 0.05 and 0.05 <= float(z.min()) and float(z.max()) <= 0.95
    inputs = [t.to(DEV).requires_grad_(True) for t in (grid, image)]
    if with_guide:
        inputs.append(guide.to(DEV).requires_grad_(True))
    assert gradcheck(slice_bilateral_grid, inputs, eps=1e-6, check_grad_dtypes=True, check_undefined_grad=True)


def test_channel_slice_of_a_wider_render_needs_no_copy():
    grid, image, _, upstream = (t.to(DEV) for t in ref.random_case((37, 53), (4, 3, 5), seed=6, dtype=torch.float32))
    wide = torch.rand(37, 53, 5, device=DEV)
    wide[..., 2:] = image
    a = ref.grads_of(slice_bilateral_grid, grid, image, None, upstream)
    w = wide.clone().requires_grad_(True)
    g = grid.clone().requires_grad_(True)
    out = slice_bilateral_grid(g, w[..., 2:])
    (out * upstream).sum().backward()
    assert torch.equal(out.detach(), a[0]) and torch.equal(g.grad, a[1]) and torch.equal(w.grad[..., 2:], a[2])
    assert not w.grad[..., :2].any()


def test_a_view_of_a_stack_of_grids_gives_the_bits_of_its_clone():
    _, image, _, upstream = (t.to(DEV) for t in ref.random_case((37, 53), (4, 3, 5), seed=7, dtype=torch.float32))
    grids = (appearance.identity_grids(3, 4, 3, 5) + 0.2 * torch.rand(3, 12, 4, 3, 5)).to(DEV).requires_grad_(True)
    out = slice_bilateral_grid(grids[1], image)
    (out * upstream).sum().backward()
    want = ref.grads_of(slice_bilateral_grid, grids[1].detach().clone(), image, None, upstream)
    assert torch.equal(out.detach(), want[0]) and torch.equal(grids.grad[1], want[1])
    assert not grids.grad[0].any() and not grids.grad[2].any()


def test_clamped_guide_gets_no_gradient():
    grid, image, guide, upstream = (t.to(DEV) for t in ref.random_case((37, 53), (8, 16, 16), seed=8, dtype=torch.float32))
    guide[0, 0], guide[3, 7], guide[36, 52] = -0.1, 1.3, 0.4
    _, _, _, d_guide = ref.grads_of(slice_bilateral_grid, grid, image, guide, upstream)
    outside = (guide < 0) | (guide > 1)
    assert int(outside.sum()) > 100 and not d_guide[outside].any()
    assert bool((d_guide[~outside] != 0).all()) and float(d_guide[36, 52]) != 0.0
    # the image's own luma: a clamped pixel keeps the gradient through the affine only
    _, _, d_image, _ = ref.grads_of(slice_bilateral_grid, grid, image, None, upstream)
    _, _, d_affine, _ = ref.grads_of(slice_bilateral_grid, grid, image, ref.luma_of(image).detach(), upstream)
    luma = ref.luma_of(image)
    clamped = (luma < -1e-3) | (luma > 1 + 1e-3)  # clearly: both lumas round to the same side, and gz is 0 or L - 1
    assert int(clamped.sum()) > 10 and torch.equal(d_image[clamped], d_affine[clamped])
    assert not torch.allclose(d_image[~clamped], d_affine[~clamped], rtol=1e-3, atol=1e-5)


# ------------------------------------------------------------------------------------------ behind the renderer
def test_behind_the_renderer():
    """render -> slice_bilateral_grid -> photometric_loss: the gradients on feature, alpha_logit and the grid against
    the same chain with the float32 torch composition, both measured against a render whose backward is seeded with
    the float64 d_image of the composition and the loss on the CPU"""
    size, n = (64, 48), 800
    g, camera = scenes.benchmark_scene(n, size, sh_degree=3, seed=0)
    cam, cfg = camera.to(device=DEV), RasterConfig()
    gen = torch.Generator().manual_seed(9)
    target = torch.rand(size[1], size[0], 3, generator=gen)
    grid = appearance.identity_grids(1, 4, 3, 5)[0] + 0.1 * (torch.rand(12, 4, 3, 5, generator=gen) - 0.5)

    def chain(fn):
        gd = g.to(DEV).requires_grad_(True)
        gr = grid.to(DEV).requires_grad_(True)
        image = gs.render_gaussians(gd, cam, cfg, use_sh=True).image
        losses.photometric_loss(fn(gr, image), target.to(DEV)).backward()
        return image.detach(), gd.feature.grad.cpu().double(), gd.alpha_logit.grad.cpu().double(), gr.grad.cpu().double()

    image, *ours = chain(slice_bilateral_grid)
    _, *theirs = chain(ref.slice_reference)
    x = image.cpu().double().requires_grad_(True)
    gr64 = grid.double().requires_grad_(True)
    ssim_reference.photometric_loss(ref.slice_reference(gr64, x), target.double()).backward()
    gd = g.to(DEV).requires_grad_(True)
    (gs.render_gaussians(gd, cam, cfg, use_sh=True).image * x.grad.float().to(DEV)).sum().backward()
    want = [gd.feature.grad.cpu().double(), gd.alpha_logit.grad.cpu().double(), gr64.grad]
    rows = {name: (float((a - w).abs().max()), float((t - w).abs().max()), float(w.abs().max()))
            for name, a, t, w in zip(("d_feature", "d_alpha_logit", "d_grid"), ours, theirs, want)}
    assert all(scale > 0 for _, _, scale in rows.values())
    _assert_float32(rows, "behind the renderer")


def test_fit_of_a_vignette_and_a_tint():
    """a (4, 4, 4) grid from identity under Adam on the L1 mean: the loss falls below a tenth of its first value (the
    yardstick alone goes from 0.075 to 0.0026 on the CPU)"""
    H, W = 48, 64
    image = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(1))
    u = ((torch.arange(W) + 0.5) / W).view(1, W, 1)
    v = ((torch.arange(H) + 0.5) / H).view(H, 1, 1)
    target = (image * (0.7 + 0.5 * u) + 0.1 * v).clamp(0, 1.5).to(DEV)
    image = image.to(DEV)
    grid = appearance.identity_grids(1, 4, 4, 4, device=DEV)[0].requires_grad_(True)
    optimizer = torch.optim.Adam([grid], lr=2e-2)
    history = []
    for _ in range(200):
        optimizer.zero_grad()
        loss = (slice_bilateral_grid(grid, image) - target).abs().mean()
        loss.backward()
        optimizer.step()
        history.append(loss.detach())
    first, last = float(history[0]), float(history[-1])
    print(f"fit: L1 {first:.4f} -> {last:.4f}")
    assert math.isfinite(last) and last < 0.1 * first, (first, last)


# ----------------------------------------------------------------------------------------------- the record
def write_accuracy(path):
    lines = ["float32 accuracy of appearance.slice_bilateral_grid on the MI355X (tests/test_bilagrid_gpu.py)",
             "max |error| against the float64 yardstick (grid_sample + affine on the CPU) on the same float32 inputs:",
             "the HIP operator, the float32 torch composition on the device, and the largest magnitude of the output.",
             "The test's bound is 4 x the composition's error (floor 1e-6 of the magnitude).", "",
             f"{'image':>12} {'grid':>12} {'guide':>6} {'output':>8} {'HIP':>10} {'torch f32':>10} {'magnitude':>10} "
             f"{'HIP/torch':>9}"]
    cases = [(shape, sizes) for shape in IMAGES for sizes in GRIDS] + list(LARGE)
    for shape, sizes in cases:
        for with_guide in (False, True):
            for name, (ours, theirs, scale) in _float32_errors(shape, sizes, with_guide).items():
                ratio = ours / theirs if theirs > 0 else float("nan")
                lines.append(f"{'x'.join(map(str, shape)):>12} {'x'.join(map(str, sizes)):>12} {str(with_guide):>6} "
                             f"{name:>8} {ours:10.3e} {theirs:10.3e} {scale:10.3e} {ratio:9.2f}")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    write_accuracy(sys.argv[1] if len(sys.argv) > 1 else os.path.join(root, "profiles", "bilagrid", "accuracy.txt"))
