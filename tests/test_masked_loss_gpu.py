"""losses.photometric_loss / losses.ssim with mask= on the GPU against tests/masked_loss_reference.py: float64 at the
project's bar and under gradcheck, the float32 accuracy bars of test_losses_gpu.py on masked inputs, the identities
that hold bit for bit, the support of the gradient, empty terms, and the masked loss behind the renderer.

Shapes: (2, 37, 21, 5) is 3 x 2 pixel tiles with partial edge tiles, two float32 / three float64 channel groups and a
batch; (9, 5, 1) is smaller than the window; (40, 33, 3) has room for "valid" padding.  Masks that do not fit a shape are
clipped to it (masked_loss_reference.make_mask).

Measured on the MI355X, HIP error over the float32 restatement's error on the same masked input, worst over the
shapes and masks of test_float32_accuracy (table in DESIGN.md, "Masked loss"): noise 0.53 (gradient of ssim), 0.54
(gradient of the loss), scalars at the one-ulp floor; smooth 0.021 / 0.021; flat 2.5e-3 / 2.7e-3; near-equal 1.9e-4 /
3.0e-4; the scalars at most 0.11 on those three classes."""
import functools
import math

import pytest
import torch
from torch.autograd import gradcheck

import masked_loss_reference as mref
import parity_util as pu
import ssim_reference as ref
import taichi_gaussian_rasterizer_amd as gs
from taichi_gaussian_rasterizer_amd import RasterConfig, losses, scenes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRADCHECK = dict(eps=1e-6, check_grad_dtypes=True, check_undefined_grad=True)   # as test_losses_gpu.GRADCHECK
F64_BAR = dict(rtol=1e-5, atol=1e-8)                                            # as test_losses_gpu.F64_BAR
SHAPES = ((2, 37, 21, 5), (9, 5, 1), (40, 33, 3))
IDS = ["x".join(map(str, s)) for s in SHAPES]
NAMES = ("ssim", "loss", "grad ssim", "grad loss")


def _hip(x, y, mask, dtype=None, **kw):
    """M, loss, d M / dx, d loss / dx of the HIP operators for CPU tensors, back on the CPU in double"""
    dtype = dtype or x.dtype
    xd, yd = x.to(DEV, dtype), y.to(DEV, dtype)
    md = mask.to(DEV) if mask.dtype == torch.bool else mask.to(DEV, dtype)
    xs = xd.clone().requires_grad_(True)
    s = losses.ssim(xs, yd, mask=md, **kw)
    s.backward()
    xl = xd.clone().requires_grad_(True)
    l = losses.photometric_loss(xl, yd, mask=md, **kw)
    l.backward()
    return [t.detach().cpu().double() for t in (s, l, xs.grad, xl.grad)]


def _kw_key(kw):
    return tuple(sorted(kw.items()))


@functools.lru_cache(maxsize=None)
def _yardstick(kind, shape, mask_kind, dtype, kw_key):
    """the restatement's M, loss and both gradients in `dtype` (computed once per case, shared by the tests)"""
    kw = dict(kw_key)
    x, y = (t.to(dtype) for t in ref.make_pair(kind, shape))
    mask = mref.make_mask(mask_kind, shape)
    s, gs_ = mref.grad_of(mref.ssim, x, y, mask, **kw)
    l, gl = mref.grad_of(mref.photometric_loss, x, y, mask, **kw)
    return tuple(t.detach().double() for t in (s, l, gs_, gl))


def _settings(shape):
    """both paddings, windows 11 and 5, where the image has room for them"""
    for padding in ("same", "valid"):
        for ws, sigma in ((11, 1.5), (5, 1.5)):
            if padding == "same" or (shape[-3] >= ws and shape[-2] >= ws):
                yield dict(padding=padding, window_size=ws, sigma=sigma)


# ------------------------------------------------------------------------------------------------- float64
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
@pytest.mark.parametrize("mask_kind", mref.MASKS)
def test_float64_matches_the_yardstick(mask_kind, shape):
    mask = mref.make_mask(mask_kind, shape)
    settings = list(_settings(shape))
    assert dict(padding="same", window_size=11, sigma=1.5) in settings
    assert shape != (40, 33, 3) or dict(padding="valid", window_size=5, sigma=1.5) in settings
    for kind in ("noise", "near-equal"):
        x, y = (t.double() for t in ref.make_pair(kind, shape))
        for kw in settings:
            truth = _yardstick(kind, shape, mask_kind, torch.float64, _kw_key(kw))
            for name, a, b in zip(NAMES, _hip(x, y, mask, **kw), truth):
                assert a.dtype == torch.float64
                # equal_nan: a mask clipped to nothing, or with no counted pixel, has NaN parts in both
                assert torch.allclose(a, b, equal_nan=True, **F64_BAR), \
                    f"{kind} {kw} {name}: {float((a - b).abs().max()):.3e}"


def _gradcheck_case(shape, seed, mask_kind):
    """float64 inputs on the GPU with |x - y| >= 1e-3, so the L1 kink is not inside the finite-difference step"""
    x, y = (t.double() for t in ref.make_pair("noise", shape, seed=seed))
    x = torch.where((x - y).abs() < 1e-3, y + 1e-2, x)
    return x.to(DEV).requires_grad_(True), y.to(DEV), mref.make_mask(mask_kind, shape).double().to(DEV)


@pytest.mark.parametrize("padding", ["same", "valid"])
@pytest.mark.parametrize("mask_kind", ["random", "hole"])
@pytest.mark.parametrize("shape,window", [((13, 18, 2), dict()), ((2, 19, 7, 3), dict(window_size=5, sigma=1.0))],
                         ids=["13x18x2", "2x19x7x3"])
def test_gradcheck(shape, window, mask_kind, padding):
    x, y, m = _gradcheck_case(shape, 1, mask_kind)
    assert float(m.min()) == 0.0 or mask_kind == "random"
    assert gradcheck(lambda t: losses.ssim(t, y, padding=padding, mask=m, **window), (x,), **GRADCHECK)
    assert gradcheck(lambda t: losses.photometric_loss(t, y, padding=padding, mask=m, **window), (x,), **GRADCHECK)
    assert gradcheck(lambda t: losses.photometric_loss(t, y, ssim_weight=0.0, padding=padding, mask=m, **window), (x,),
                     **GRADCHECK)


# ------------------------------------------------------------------------------------------------- float32
def _errors(got, truth):
    """abs error for the scalars, normwise error for the gradients"""
    return [float((got[0] - truth[0]).abs()), float((got[1] - truth[1]).abs()),
            ref.normwise(got[2] - truth[2], truth[2]), ref.normwise(got[3] - truth[3], truth[3])]


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2]], ids=[IDS[0], IDS[2]])
@pytest.mark.parametrize("mask_kind", ["random", "hole"])
@pytest.mark.parametrize("kind", ref.CLASSES)
def test_float32_accuracy(kind, mask_kind, shape):
    """The rule of test_losses_gpu.test_float32_accuracy on masked inputs.  noise: every quantity within 2x the
    float32 restatement's error; smooth / flat / near-equal: the gradient of ssim within 1/10 of it, the scalars and
    the gradient of the loss no worse than it.  A scalar is rounded to float32 and cannot beat one ulp of the true
    value, 2^-23 |truth|, so that is its floor."""
    x, y = ref.make_pair(kind, shape)
    mask = mref.make_mask(mask_kind, shape)
    truth = _yardstick(kind, shape, mask_kind, torch.float64, ())
    e32 = _errors(_yardstick(kind, shape, mask_kind, torch.float32, ()), truth)
    hip = _errors(_hip(x, y, mask), truth)
    for name, a, b in zip(NAMES, hip, e32):
        print(f"{kind} {mask_kind} {shape} {name}: hip {a:.3e}  float32 restatement {b:.3e}  "
              f"ratio {a / b if b else math.inf:.3g}")
    for name, a, b, t in zip(NAMES, hip, e32, truth):
        floor = 2.0 ** -23 * float(t.abs()) if t.dim() == 0 else 0.0
        if kind == "noise":
            assert a <= max(2 * b, floor), f"{name}: {a:.3e} > 2 x {b:.3e}"
        elif name == "grad ssim":
            assert a <= b / 10, f"{name}: {a:.3e} > {b:.3e} / 10"
        else:
            assert a <= max(b, floor), f"{name}: {a:.3e} > {b:.3e}"


# -------------------------------------------------------------------------------------- exact identities
def _all(x, y, mask, **kw):
    """loss, both parts, d loss / dx, M and d M / dx of one masked (or mask=None) call, on the GPU"""
    xl = x.detach().clone().requires_grad_(True)
    loss, (l1, m) = losses.photometric_loss(xl, y, return_parts=True, mask=mask, **kw)
    loss.backward()
    xs = x.detach().clone().requires_grad_(True)
    s = losses.ssim(xs, y, mask=mask, **kw)
    s.backward()
    return [loss.detach(), l1, m, xl.grad, s.detach(), xs.grad]


def _same_bits(a, b):
    return all(torch.equal(p, q) or (p.dim() == 0 and bool(p.isnan()) and bool(q.isnan())) for p, q in zip(a, b))


@pytest.mark.parametrize("kw", [dict(), dict(padding="valid"), dict(window_size=5, padding="valid"),
                                dict(ssim_weight=0.0)], ids=str)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_identities_hold_bit_for_bit(dtype, kw):
    shape = SHAPES[0]
    B, H, W, _ = shape
    x, y = (t.to(DEV, dtype) for t in ref.make_pair("noise", shape, seed=5))

    def run(mask):
        if "ssim_weight" not in kw:
            return _all(x, y, mask, **kw)
        xl = x.detach().clone().requires_grad_(True)
        loss, (l1, m) = losses.photometric_loss(xl, y, return_parts=True, mask=mask, **kw)
        loss.backward()
        return [loss.detach(), l1, m, xl.grad]

    # ones: multiplying by 1 is exact and S summed in double is the pixel count
    assert _same_bits(run(torch.ones(B, H, W, dtype=dtype, device=DEV)), run(None))
    assert _same_bits(run(torch.ones(H, W, dtype=dtype, device=DEV)), run(None))
    assert _same_bits(run(torch.ones(B, H, W, dtype=torch.bool, device=DEV)), run(None))
    for mask_kind in ("random", "hole", "one-tile"):
        m = mref.make_mask(mask_kind, shape).to(DEV, dtype)
        base = run(m)
        assert all(bool(t.isfinite().all()) for t in base[:2] + base[3:])
        assert _same_bits(run(m), base), "two calls"
        assert _same_bits(run(2 * m), base) and _same_bits(run(0.25 * m), base), "a power of two"
        wide = torch.rand(B, H, W + 9, generator=torch.Generator().manual_seed(6)).to(DEV, dtype)
        big = torch.rand(B, H + 4, W + 9, 2, generator=torch.Generator().manual_seed(7)).to(DEV, dtype)
        wide[:, :, 3:3 + W] = m
        big[:, 2:2 + H, 3:3 + W, 1] = m
        for view in (wide[:, :, 3:3 + W], big[:, 2:2 + H, 3:3 + W, 1]):
            assert not view.is_contiguous() and torch.equal(view, m)
            assert losses._strided_mask(view, dtype)[0].data_ptr() == view.data_ptr(), "the view goes in without a copy"
            assert _same_bits(run(view), base), "a column, row and pixel-strided view of a larger buffer"
        if mask_kind != "random":
            assert _same_bits(run(m != 0), run((m != 0).to(dtype))), "a bool mask and its 0 / 1 copy"
    m2 = mref.make_mask("broadcast", shape).to(DEV, dtype)
    assert m2.shape == (H, W)
    assert _same_bits(run(m2), run(m2.expand(B, H, W)))
    assert _same_bits(run(m2), run(m2.expand(B, H, W).contiguous()))
    assert _same_bits(run(m2 > 0.5), run((m2 > 0.5).to(dtype)))


# ------------------------------------------------------------------------------------ support of the gradient
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_support_of_the_gradient(dtype):
    shape = SHAPES[2]
    H, W, C = shape
    x, y = (t.to(DEV, dtype) for t in ref.make_pair("noise", shape, seed=8))

    def grad(mask, **kw):
        xl = x.detach().clone().requires_grad_(True)
        loss, parts = losses.photometric_loss(xl, y, return_parts=True, mask=mask, **kw)
        loss.backward()
        return loss.detach(), parts, xl.grad

    # L1 alone: the gradient lives where the mask does
    for mask_kind in ("random", "hole", "one-tile", "single-pixel"):
        m = mref.make_mask(mask_kind, shape).to(DEV, dtype)
        _, _, g = grad(m, ssim_weight=0.0)
        assert not g[m == 0].any() and bool((g[m != 0] != 0).all())
        expect = (torch.sign(x - y) * m[..., None]).double() / (C * m.double().sum())
        assert torch.allclose(g.double(), expect, rtol=1e-6, atol=0)
    # one weighted pixel, default window: its 11 x 11 block and nothing else
    m = mref.make_mask("single-pixel", shape).to(DEV, dtype)
    loss, (l1, ssim_mean), g = grad(m)
    block = torch.zeros(H, W, dtype=torch.bool, device=DEV)
    block[15:26, 12:23] = True
    assert not g[~block].any() and bool((g[block] != 0).all())
    assert float(l1) == pytest.approx(float((x - y).abs()[20, 17].mean()), rel=1e-6)
    full_map = losses.ssim(x, y, reduction="none")
    assert float(ssim_mean) == pytest.approx(float(full_map[20, 17].double().mean()), rel=1e-6)
    # no weight at all: nothing to average, nothing to learn from
    for zero in (torch.zeros(H, W, dtype=dtype, device=DEV), torch.zeros(H, W, dtype=torch.bool, device=DEV)):
        for kw in (dict(), dict(padding="valid"), dict(ssim_weight=0.0)):
            loss, (l1, ssim_mean), g = grad(zero, **kw)
            assert float(loss) == 0.0 and not g.any() and bool(g.isfinite().all())
            assert math.isnan(float(l1)) and math.isnan(float(ssim_mean))
        assert math.isnan(float(losses.ssim(x, y, mask=zero)))
    # "valid" and weight on the border only: no counted pixel has weight, so the L1 term alone is left
    border = torch.ones(H, W, dtype=dtype, device=DEV)
    border[5:H - 5, 5:W - 5] = 0
    loss, (l1, ssim_mean), g = grad(border, padding="valid")
    loss_l1, (l1_only, _), g_l1 = grad(border, padding="valid", ssim_weight=0.0)
    assert math.isnan(float(ssim_mean)) and torch.equal(l1, l1_only) and math.isfinite(float(loss))
    assert float(loss) == pytest.approx(0.8 * float(l1), rel=1e-6)
    assert torch.allclose(g, 0.8 * g_l1, rtol=1e-6, atol=0) and not g[border == 0].any()


def test_batch_entries_share_one_normaliser():
    """S runs over the whole batch: the batched loss is the S-weighted mean of the single-image losses"""
    shape = SHAPES[0]
    x, y = (t.to(DEV).double() for t in ref.make_pair("noise", shape, seed=9))
    m = mref.make_mask("random", shape).to(DEV).double()
    _, (l1, s) = losses.photometric_loss(x, y, return_parts=True, mask=m)
    singles = [losses.photometric_loss(x[b], y[b], return_parts=True, mask=m[b])[1] for b in range(2)]
    S = [float(m[b].sum()) for b in range(2)]
    assert float(l1) == pytest.approx(sum(S[b] * float(singles[b][0]) for b in range(2)) / sum(S), rel=1e-12)
    assert float(s) == pytest.approx(sum(S[b] * float(singles[b][1]) for b in range(2)) / sum(S), rel=1e-12)


# ------------------------------------------------------------------------------------- through the renderer
def test_masked_loss_behind_the_renderer():
    """photometric_loss(render, mask=).backward(), behind a render with a background and a differentiable weight,
    gives the parameter gradients of a render whose backward is seeded with the yardstick's float64 d_image of the
    same image and mask, at the bar of test_losses_gpu.test_loss_behind_the_renderer"""
    size, n = (128, 96), 3000
    g, camera = scenes.benchmark_scene(n, size, sh_degree=3, seed=0)
    cfg = RasterConfig()
    gen = torch.Generator().manual_seed(1)
    target = torch.rand(size[1], size[0], 3, generator=gen)
    background = torch.rand(3, generator=gen).to(DEV)
    mask = mref.make_mask("hole", (size[1], size[0], 3))
    cam = camera.to(device=DEV)

    gd = g.to(DEV).requires_grad_(True)
    r = gs.render_gaussians(gd, cam, cfg, use_sh=True, background=background, differentiable_weight=True)
    assert r.image_weight.shape == mask.shape
    losses.photometric_loss(r.image, target.to(DEV), mask=mask.to(DEV)).backward()

    _, d_image = mref.grad_of(mref.photometric_loss, r.image.detach().cpu().double(), target.double(), mask)
    assert bool(d_image[10:30, 5:19].any())   # the windows reach into the hole: SSIM sees every pixel
    gd2 = g.to(DEV).requires_grad_(True)
    r2 = gs.render_gaussians(gd2, cam, cfg, use_sh=True, background=background, differentiable_weight=True)
    (r2.image * d_image.float().to(DEV)).sum().backward()
    torch.cuda.synchronize()
    for name in ("position", "log_scaling", "rotation", "alpha_logit", "feature"):
        a, b = getattr(gd, name).grad, getattr(gd2, name).grad
        assert a is not None and float(b.abs().max()) > 0
        pu.assert_grad_close(a, pu.to_np(b), f"d_{name} through the masked photometric_loss", tol=2e-3)
