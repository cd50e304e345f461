"""losses.ssim / losses.photometric_loss on the GPU against tests/ssim_reference.py: the float32 accuracy bars per input
class (fractions of the float32 conv2d restatement's own error against float64 truth), float64 at the project's bar
and under gradcheck, strides and shapes, determinism, the loss behind the renderer, and the benchmark.

Measured on the MI355X, HIP error over the float32 restatement's error, worst of the four sizes (table in DESIGN.md
section 4): noise 0.45 (map), 0.51 (gradient of ssim), 1.0 (scalars); smooth 0.026 / 0.014; flat 0.015 / 1.9e-3;
near-equal 8.1e-3 / 2.1e-4; the scalars and the gradient of the loss at most 0.22 on those three classes."""
import math

import numpy as np
import pytest
import torch
from torch.autograd import gradcheck

import parity_util as pu
import ssim_reference as ref
import taichi_gaussian_rasterizer_amd as gs
from taichi_gaussian_rasterizer_amd import RasterConfig, losses, scenes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRADCHECK = dict(eps=1e-6, check_grad_dtypes=True, check_undefined_grad=True)
F64_BAR = dict(rtol=1e-5, atol=1e-8)


def _hip_quantities(x, y, **kw):
    """map, ssim, loss, d ssim / dx, d loss / dx of the HIP operators for CPU tensors x, y, back on the CPU in double"""
    xd, yd = x.to(DEV), y.to(DEV)
    m = losses.ssim(xd, yd, reduction="none", **kw)
    xs = xd.clone().requires_grad_(True)
    s = losses.ssim(xs, yd, **kw)
    s.backward()
    xl = xd.clone().requires_grad_(True)
    l = losses.photometric_loss(xl, yd, **kw)
    l.backward()
    return [t.detach().cpu().double() for t in (m, s, l, xs.grad, xl.grad)]


def _ref_quantities(x, y, **kw):
    kw_map = {k: v for k, v in kw.items() if k != "padding"}
    m = ref.ssim_map(x, y, **kw_map)
    s, gs_ = ref.grad_of(ref.ssim, x, y, **kw)
    l, gl = ref.grad_of(ref.photometric_loss, x, y, **kw)
    return [t.detach().double() for t in (m, s, l, gs_, gl)]


NAMES = ("map", "ssim", "loss", "grad ssim", "grad loss")


def _errors(got, truth):
    """max abs error for the map, abs error for the scalars, normwise error for the gradients"""
    return [float((got[0] - truth[0]).abs().max()), float((got[1] - truth[1]).abs()), float((got[2] - truth[2]).abs()),
            ref.normwise(got[3] - truth[3], truth[3]), ref.normwise(got[4] - truth[4], truth[4])]


@pytest.mark.parametrize("shape", ref.SIZES, ids=["x".join(map(str, s)) for s in ref.SIZES])
@pytest.mark.parametrize("kind", ref.CLASSES)
def test_float32_accuracy(kind, shape):
    """noise: every quantity within 2x the float32 restatement's error; smooth / flat / near-equal: map and gradient
    of ssim within 1/10 of it, the scalars and the gradient of the photometric loss no worse than it."""
    x, y = ref.make_pair(kind, shape)
    truth = _ref_quantities(x.double(), y.double())
    e32 = _errors(_ref_quantities(x, y), truth)
    hip = _errors(_hip_quantities(x, y), truth)
    for name, a, b in zip(NAMES, hip, e32):
        print(f"{kind} {shape} {name}: hip {a:.3e}  float32 restatement {b:.3e}  ratio {a / b if b else math.inf:.3g}")
    for name, a, b in zip(NAMES, hip, e32):
        if kind == "noise":
            assert a <= 2 * b, f"{name}: {a:.3e} > 2 x {b:.3e}"
        elif name in ("map", "grad ssim"):
            assert a <= b / 10, f"{name}: {a:.3e} > {b:.3e} / 10"
        else:
            assert a <= b, f"{name}: {a:.3e} > {b:.3e}"


def test_ssim_of_an_image_with_itself_is_one():
    for kind in ("noise", "smooth"):
        x, _ = ref.make_pair(kind, (70, 50, 3))
        m = losses.ssim(x.to(DEV), x.to(DEV).clone(), reduction="none")
        assert float((m - 1).abs().max()) <= 16 * 2.0 ** -23


# ------------------------------------------------------------------------------------------------- float64
@pytest.mark.parametrize("shape", ref.SIZES, ids=["x".join(map(str, s)) for s in ref.SIZES])
@pytest.mark.parametrize("kind", ["noise", "near-equal"])
def test_float64_matches_truth(kind, shape):
    x, y = (t.double() for t in ref.make_pair(kind, shape))
    truth, hip = _ref_quantities(x, y), _hip_quantities(x, y)
    for name, a, b in zip(NAMES, hip, truth):
        assert a.dtype == torch.float64
        assert torch.allclose(a, b, **F64_BAR), f"{name}: {float((a - b).abs().max()):.3e}"


def _gradcheck_pair(shape, seed):
    """float64 inputs on the GPU with |x - y| >= 1e-3, so the L1 kink is not inside the finite-difference step"""
    x, y = (t.double() for t in ref.make_pair("noise", shape, seed=seed))
    x = torch.where((x - y).abs() < 1e-3, y + 1e-2, x)
    return x.to(DEV).requires_grad_(True), y.to(DEV)


@pytest.mark.parametrize("padding", ["same", "valid"])
@pytest.mark.parametrize("reduction", ["mean", "none"])
def test_gradcheck_ssim(reduction, padding):
    x, y = _gradcheck_pair((13, 18, 2), seed=1)
    assert gradcheck(lambda t: losses.ssim(t, y, padding=padding, reduction=reduction), (x,), **GRADCHECK)


def test_gradcheck_ssim_small_window_batch_and_tile_edges():
    x, y = _gradcheck_pair((2, 19, 7, 3), seed=2)   # two tile rows, three channels (two float64 channel groups)
    assert gradcheck(lambda t: losses.ssim(t, y, window_size=5, sigma=1.0), (x,), **GRADCHECK)


@pytest.mark.parametrize("padding", ["same", "valid"])
def test_gradcheck_photometric_loss(padding):
    x, y = _gradcheck_pair((12, 17, 3), seed=3)
    assert gradcheck(lambda t: losses.photometric_loss(t, y, padding=padding), (x,), **GRADCHECK)
    assert gradcheck(lambda t: losses.photometric_loss(t, y, ssim_weight=0.0), (x,), **GRADCHECK)


# --------------------------------------------------------------------------------------- strides and shapes
def _loss_and_grad(fn, x, y, **kw):
    x = x.detach().requires_grad_(True)
    v = fn(x, y, **kw)
    (g,) = torch.autograd.grad(v.sum(), x)
    return v.detach(), g


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_strided_views_match_their_contiguous_copies_bit_for_bit(dtype):
    gen = torch.Generator().manual_seed(5)
    wide = torch.rand(45, 37, 5, generator=gen, dtype=dtype).to(DEV)      # a depth render: image[..., 2:]
    big = torch.rand(64, 80, 3, generator=gen, dtype=dtype).to(DEV)       # a crop: rows and columns of a larger image
    target = torch.rand(64, 80, 5, generator=gen, dtype=dtype).to(DEV)
    views = [(wide[..., 2:], target[:45, :37, :3]), (big[5:45, 7:60], target[5:45, 7:60, 1:4]),
             (big[None, 3:50, :64], target[None, 3:50, :64, 2:])]
    for xv, yv in views:
        assert not xv.is_contiguous() and not yv.is_contiguous()
        assert losses._strided(xv)[0].data_ptr() == xv.data_ptr(), "the view must go in without a copy"
        xc, yc = xv.contiguous(), yv.contiguous()
        for fn, kw in ((losses.photometric_loss, {}), (losses.ssim, {}), (losses.ssim, dict(reduction="none"))):
            v1, g1 = _loss_and_grad(fn, xv, yv, **kw)
            v2, g2 = _loss_and_grad(fn, xc, yc, **kw)
            assert torch.equal(v1, v2) and torch.equal(g1, g2), (fn.__name__, kw)
    # anything the kernels cannot read is copied, not refused: a channel-first tensor seen channel-last
    xt = torch.rand(3, 30, 40, generator=gen, dtype=dtype).to(DEV).permute(1, 2, 0)
    yt = torch.rand(30, 40, 3, generator=gen, dtype=dtype).to(DEV)
    v1, g1 = _loss_and_grad(losses.photometric_loss, xt, yt)
    v2, g2 = _loss_and_grad(losses.photometric_loss, xt.contiguous(), yt)
    assert torch.equal(v1, v2) and torch.equal(g1, g2)


def test_batch_is_the_mean_of_the_single_calls():
    x, y = (t.to(DEV) for t in ref.make_pair("noise", (3, 61, 45, 4), seed=7))
    for fn in (losses.ssim, losses.photometric_loss):
        whole, gw = _loss_and_grad(fn, x, y)
        parts = [_loss_and_grad(fn, x[b], y[b]) for b in range(3)]
        mean = sum(float(v) for v, _ in parts) / 3
        # every value is a double sum rounded once to float32: half an ulp each, and the division by three
        assert abs(float(whole) - mean) <= 2 * 2.0 ** -23 * abs(mean)
        for b in range(3):   # the same sums with the upstream constant rounded at a third of its size
            assert float((gw[b] * 3 - parts[b][1]).abs().max()) <= 1e-6 * float(parts[b][1].abs().max())
        assert torch.equal(losses.ssim(x, y, reduction="none")[1], losses.ssim(x[1], y[1], reduction="none"))


@pytest.mark.parametrize("kw", [dict(padding="valid"), dict(window_size=3, sigma=0.8), dict(window_size=7),
                                dict(window_size=15, sigma=2.5), dict(window_size=15, sigma=2.5, padding="valid"),
                                dict(data_range=2.0)], ids=str)
def test_padding_windows_and_range(kw):
    """float64 at the float64 bar; float32 on the noise class at the noise bar of the accuracy test (2x the float32
    restatement's error; scalars also pass within one float32 ulp of truth, the rounding of the result itself)"""
    x, y = ref.make_pair("noise", (47, 53, 3), seed=11)
    truth = _ref_quantities(x.double(), y.double(), **kw)
    for name, a, b in zip(NAMES, _hip_quantities(x.double(), y.double(), **kw), truth):
        assert torch.allclose(a, b, **F64_BAR), f"float64 {name}: {float((a - b).abs().max()):.3e}"
    e32 = _errors(_ref_quantities(x, y, **kw), truth)
    hip = _errors(_hip_quantities(x, y, **kw), truth)
    for name, a, b, t in zip(NAMES, hip, e32, truth):
        floor = 2.0 ** -23 * float(t.abs().max()) if t.dim() == 0 else 0.0
        print(f"{kw} {name}: hip {a:.3e}  float32 restatement {b:.3e}")
        assert a <= max(2 * b, floor), f"{name}: {a:.3e} > 2 x {b:.3e}"


def test_map_with_a_random_upstream_gradient():
    x, y = ref.make_pair("noise", (61, 45, 4), seed=13)
    up = torch.rand(61, 45, 4, generator=torch.Generator().manual_seed(14)) - 0.3
    xt = x.double().requires_grad_(True)
    (truth,) = torch.autograd.grad((ref.ssim_map(xt, y.double()) * up.double()).sum(), xt)
    x32 = x.clone().requires_grad_(True)
    (g32,) = torch.autograd.grad((ref.ssim_map(x32, y) * up).sum(), x32)
    for dtype in (torch.float64, torch.float32):
        xd = x.to(DEV, dtype).requires_grad_(True)
        (g,) = torch.autograd.grad((losses.ssim(xd, y.to(DEV, dtype), reduction="none") * up.to(DEV, dtype)).sum(), xd)
        g = g.cpu().double()
        if dtype == torch.float64:
            assert torch.allclose(g, truth, **F64_BAR)
        else:
            a, b = ref.normwise(g - truth, truth), ref.normwise(g32.double() - truth, truth)
            print(f"upstream map: hip {a:.3e}  float32 restatement {b:.3e}")
            assert a <= 2 * b


def test_no_grad_and_parts():
    x, y = (t.to(DEV) for t in ref.make_pair("smooth", (40, 50, 3)))
    loss, (l1, ssim_mean) = losses.photometric_loss(x.clone().requires_grad_(True), y, return_parts=True)
    assert loss.requires_grad and not l1.requires_grad and not ssim_mean.requires_grad
    assert torch.equal(ssim_mean, losses.ssim(x, y)) and float(l1) == pytest.approx(float((x - y).abs().mean()), rel=1e-6)
    assert float(loss) == pytest.approx(0.8 * float(l1) + 0.2 * (1 - float(ssim_mean)), rel=1e-6)
    with torch.no_grad():
        assert torch.equal(losses.photometric_loss(x.clone().requires_grad_(True), y), loss.detach())
    l0, (l1_0, s0) = losses.photometric_loss(x, y, ssim_weight=0.0, return_parts=True)
    assert torch.equal(l0, l1_0) and torch.equal(l1_0, l1) and math.isnan(float(s0))
    xg = x.clone().requires_grad_(True)
    losses.photometric_loss(xg, y, ssim_weight=0.0).backward()
    assert torch.equal(xg.grad, torch.sign(x - y) / x.numel())


# --------------------------------------------------------------------------------------------- determinism
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_two_calls_are_bit_identical(dtype):
    x, y = (t.to(DEV, dtype) for t in ref.make_pair("noise", (203, 157, 3), seed=21))
    runs = []
    for _ in range(2):
        v, g = _loss_and_grad(losses.photometric_loss, x, y)
        s, gs_ = _loss_and_grad(losses.ssim, x, y)
        runs.append((v, g, s, gs_, losses.ssim(x, y, reduction="none")))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------- through the renderer
def test_loss_behind_the_renderer():
    """photometric_loss(render).backward() gives the parameter gradients of a render whose backward is seeded with the
    restatement's float64 d_image of the same image, at the bar smoke() uses"""
    size, n = (128, 96), 3000
    g, camera = scenes.benchmark_scene(n, size, sh_degree=3, seed=0)
    cfg = RasterConfig()
    target = torch.rand(size[1], size[0], 3, generator=torch.Generator().manual_seed(1))
    cam = camera.to(device=DEV)

    gd = g.to(DEV).requires_grad_(True)
    r = gs.render_gaussians(gd, cam, cfg, use_sh=True)
    losses.photometric_loss(r.image, target.to(DEV)).backward()

    _, d_image = ref.grad_of(ref.photometric_loss, r.image.detach().cpu().double(), target.double())
    gd2 = g.to(DEV).requires_grad_(True)
    r2 = gs.render_gaussians(gd2, cam, cfg, use_sh=True)
    (r2.image * d_image.float().to(DEV)).sum().backward()
    torch.cuda.synchronize()
    for name in ("position", "log_scaling", "rotation", "alpha_logit", "feature"):
        a, b = getattr(gd, name).grad, getattr(gd2, name).grad
        assert a is not None and float(b.abs().max()) > 0
        pu.assert_grad_close(a, pu.to_np(b), f"d_{name} through photometric_loss", tol=2e-3)


def test_loss_takes_the_depth_renders_channel_slice():
    size, n = (96, 64), 1500
    g, camera = scenes.benchmark_scene(n, size, sh_degree=3, seed=2)
    gd = g.to(DEV).requires_grad_(True)
    r = gs.render_gaussians(gd, camera.to(device=DEV), RasterConfig(), use_sh=True, render_depth=True)
    target = torch.rand(size[1], size[0], r.image.shape[-1], generator=torch.Generator().manual_seed(3)).to(DEV)
    loss = losses.photometric_loss(r.image, target)
    loss.backward()
    assert math.isfinite(float(loss)) and float(gd.feature.grad.abs().max()) > 0


# ------------------------------------------------------------------------------------------------ benchmark
def test_bench_loss():
    from taichi_gaussian_rasterizer_amd.benchmarks import bench_loss
    results = bench_loss.bench_loss(bench_loss.parse_args(["--image_size", "320,200", "--iters", "5"]))
    names = ["fused forward", "fused forward+backward", "torch forward+backward", "l1 only"]
    assert set(names) <= set(results), results
    assert all(math.isfinite(v) and v > 0 for v in results.values()), results
    record = bench_loss.compare(bench_loss.parse_args(["--image_size", "320,200"]), warmup=2, iters=5, rounds=2)
    assert record["fused_ms"] > 0 and record["torch_ms"] > 0 and len(record["fused_ms_rounds"]) == 2
