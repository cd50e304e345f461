"""environment.composite_environment on the GPU against tests/envmap_reference.py (index gathers in torch, CPU float64).

Float64: value, d_env and d_image_weight at rtol 1e-10 / atol 1e-12 (the same float64 arithmetic in another order).
The output is discontinuous across a face edge; the pixels whose two largest |d_i| differ by less than 1e-4 of the
largest (envmap_reference.kept_pixels) are left out of the value and d_image_weight, at most 1 % of the pixels (0.04 %
at the most here), and carry a zero upstream gradient and a weight of one, so that d_env compares in full.  Float32:
against the float64 yardstick on the same float32 inputs, each output within 4 times the error the float32 torch
composition makes on the device (floor 1e-6 of the output's largest magnitude).

Shapes: the cameras of envmap_reference x map edges 1, 2, 7, 64 x 1, 3, 4 channels; 512 x 512 over an edge of 256; and
the host's choice of kernel for the map's gradient (csrc/envmap.hip env_plan: from the side s = 2 max(W, H) / R + 1 of
the box a texel would have under a 90-degree field of view), the smallest shapes on each side of each threshold under a
64 x 64 image: one lane per texel below s^2 = 256 (R = 9) and one wave from there (R = 8); one slice of a wave's box
while s^2 / 256 < 2 (R = 6), two from there (R = 5); one wave per texel below s^2 = 1024 (R = 5), four from there
(R = 4); one slice of four waves' box while s^2 / 1024 < 2 (R = 3), more from there (R = 2).

`python tests/test_envmap_gpu.py [PATH]` writes the float32 errors of both paths (profiles/envmap/accuracy.txt)."""
import math
import os
import sys

import pytest
import torch
from torch.autograd import gradcheck

import envmap_reference as ref
import ssim_reference
import taichi_gaussian_rasterizer_amd as gs
from taichi_gaussian_rasterizer_amd import RasterConfig, losses, scenes
from taichi_gaussian_rasterizer_amd.environment import (composite_environment, constant_environment,
                                                        sample_environment)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EDGES = (1, 2, 7, 64)
CHANNELS = (1, 3, 4)
THRESHOLD_EDGES = (2, 3, 4, 5, 6, 8, 9)
F64 = dict(rtol=1e-10, atol=1e-12)
NAMES = ("value", "d_env", "d_image_weight")


def _extra_camera(name, dtype):
    if name == "large":
        return ref.make_camera((512, 512), (300.0, 310.0, 256.3, 255.1), ref.rotation((1, 2, 3), 0.9), dtype=dtype)
    if name == "switch":  # a 64 x 64 image: the host's thresholds sit at small map edges
        return ref.make_camera((64, 64), (40.0, 42.0, 31.3, 32.9), ref.rotation((2, -1, 1), 0.7), dtype=dtype)
    return ref.camera(name, dtype)


_CASES = {}


def _case(name, R, C, dtype=torch.float64):
    """one seeded case (camera, env, image, weight, upstream, kept pixels) and its float64 yardstick, computed once"""
    key = (name, R, C, dtype)
    if key not in _CASES:
        cam = _extra_camera(name, dtype)
        W, H = cam.image_size
        gen = torch.Generator().manual_seed(0)
        env = torch.rand(6, R, R, C, generator=gen, dtype=torch.float64).to(dtype)
        image = torch.rand(H, W, C, generator=gen, dtype=torch.float64).to(dtype)
        weight = torch.rand(H, W, generator=gen, dtype=torch.float64).to(dtype)
        upstream = (torch.rand(H, W, C, generator=gen, dtype=torch.float64) - 0.5).to(dtype)
        keep = ref.kept_pixels(cam)
        share = 1.0 - float(keep.double().mean())
        assert share <= 0.01, f"{share:.2%} of the pixels left out"
        weight[~keep] = 1.0
        upstream[~keep] = 0.0
        cam64 = _extra_camera(name, torch.float64)
        if dtype != torch.float64:  # the float64 yardstick on the same float32 inputs, the camera's included
            cam64 = ref.make_camera(cam.image_size, cam.projection.double(), cam.T_camera_world.double()[:3, :3],
                                    cam.T_camera_world.double()[:3, 3])
        want = ref.grads_of(ref.composite_reference, env.double(), image.double(), weight.double(), cam64,
                            upstream.double())
        _CASES[key] = (cam, env, image, weight, upstream, keep, want)
    return _CASES[key]


def _on_device(fn, cam, env, image, weight, upstream):
    out = ref.grads_of(fn, env.to(DEV), None if image is None else image.to(DEV),
                       None if weight is None else weight.to(DEV), cam.to(device=DEV), upstream.to(DEV))
    return [None if t is None else t.cpu().double() for t in out]


def _masked(name, t, keep):
    return t if name == "d_env" else t[keep]


def _compare_f64(name, R, C):
    cam, env, image, weight, upstream, keep, want = _case(name, R, C)
    got = _on_device(composite_environment, cam, env, image, weight, upstream)
    for what, a, b in zip(NAMES, got, want):
        a, b = _masked(what, a, keep), _masked(what, b, keep)
        assert torch.allclose(a, b, **F64), f"{name} R={R} C={C} {what}: max |difference| {float((a - b).abs().max()):.3e}"


@pytest.mark.parametrize("R", EDGES)
@pytest.mark.parametrize("name", ref.CAMERAS)
def test_float64_against_the_yardstick(name, R):
    for C in CHANNELS:
        _compare_f64(name, R, C)


def test_float64_on_the_larger_image():
    _compare_f64("large", 256, 3)


@pytest.mark.parametrize("R", THRESHOLD_EDGES)
def test_float64_on_each_side_of_the_hosts_thresholds(R):
    """module docstring: under 64 x 64, R = 9 | 8 (lane | wave), 6 | 5 (one slice | two), 5 | 4 (one wave | four),
    3 | 2 (one slice of four waves | four)"""
    q = gs._native.lib().gs_envmap_scratch_bytes
    assert (q(64, 64, 3, 6, 1) == 0) and (q(64, 64, 3, 5, 1) == 6 * 25 * 2 * 3 * 8) and q(64, 64, 3, 4, 1) == 0 \
        and q(64, 64, 3, 3, 1) == 0 and q(64, 64, 3, 2, 1) == 6 * 4 * 4 * 3 * 8
    _compare_f64("switch", R, 3)


def test_float64_sky_alone():
    cam, env, _, _, upstream, keep, _ = _case("wide", 7, 3)
    want = ref.grads_of(ref.composite_reference, env, None, None, cam, upstream)
    got = _on_device(composite_environment, cam, env, None, None, upstream)
    assert got[2] is None and want[2] is None
    assert torch.allclose(got[0][keep], want[0][keep], **F64) and torch.allclose(got[1], want[1], **F64)
    assert torch.equal(sample_environment(env.to(DEV), cam.to(device=DEV)).cpu(), got[0])


# ------------------------------------------------------------------------------------------------- float32
def _float32_errors(name, R, C):
    """per output: (error of the HIP operator, error of the float32 torch composition on the device, magnitude), all
    against the float64 yardstick on the same float32 inputs"""
    cam, env, image, weight, upstream, keep, want = _case(name, R, C, torch.float32)
    ours = _on_device(composite_environment, cam, env, image, weight, upstream)
    theirs = _on_device(ref.composite_reference, cam, env, image, weight, upstream)
    rows = {}
    for what, a, t, w in zip(NAMES, ours, theirs, want):
        a, t, w = _masked(what, a, keep), _masked(what, t, keep), _masked(what, w, keep)
        rows[what] = (float((a - w).abs().max()), float((t - w).abs().max()), float(w.abs().max()))
    return rows


def _assert_float32(rows, what):
    for name, (ours, theirs, scale) in rows.items():
        bound = max(4.0 * theirs, 1e-6 * scale)
        print(f"{what} {name}: HIP {ours:.3e}, torch float32 {theirs:.3e}, bound {bound:.3e}, magnitude {scale:.3e}")
        assert ours <= bound, f"{what} {name}: {ours:.3e} > {bound:.3e} (torch float32: {theirs:.3e})"


@pytest.mark.parametrize("R", EDGES)
@pytest.mark.parametrize("name", ref.CAMERAS)
def test_float32_within_four_times_the_torch_compositions_error(name, R):
    for C in CHANNELS:
        _assert_float32(_float32_errors(name, R, C), f"{name} R={R} C={C}")


def test_float32_on_the_larger_image():
    _assert_float32(_float32_errors("large", 256, 3), "large R=256")


@pytest.mark.parametrize("R", THRESHOLD_EDGES)
def test_float32_on_each_side_of_the_hosts_thresholds(R):
    _assert_float32(_float32_errors("switch", R, 3), f"switch R={R}")


# ------------------------------------------------------------------------------------------- exact properties
def _device_case(name, R, C=3):
    cam, env, image, weight, upstream, _, _ = _case(name, R, C, torch.float32)
    return cam.to(device=DEV), env.to(DEV), image.to(DEV), weight.to(DEV), upstream.to(DEV)


@pytest.mark.parametrize("name,R", [("seam", 7), ("corner", 2), ("tele", 64)])
def test_full_weight_returns_the_image_and_no_map_gradient(name, R):
    cam, env, image, _, upstream = _device_case(name, R)
    out, d_env, _ = ref.grads_of(composite_environment, env, image, torch.ones_like(image[..., 0]), cam, upstream)
    assert torch.equal(out, image)
    assert not d_env.any() and not torch.signbit(d_env).any()


@pytest.mark.parametrize("name,R", [("seam", 7), ("corner", 2), ("wide", 64), ("one", 1)])
def test_constant_map_returns_the_constant(name, R):
    cam = _extra_camera(name, torch.float32).to(device=DEV)
    colour = torch.tensor([0.1, 0.7, 1.0 / 3.0], device=DEV)
    sky = sample_environment(constant_environment(colour, R, device=DEV), cam)
    assert sky.shape == (cam.image_size[1], cam.image_size[0], 3) and bool((sky == colour).all())


def test_translation_changes_no_bit():
    _, env, image, weight, upstream = _device_case("seam", 7)
    runs = [ref.grads_of(composite_environment, env, image, weight, ref.camera("seam", torch.float32, t).to(device=DEV),
                         upstream) for t in (ref.TRANSLATION, (-40.0, 3.0, 1e3))]
    for a, b in zip(*runs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("name,R", [("corner", 2), ("seam", 7), ("tele", 64), ("switch", 5), ("large", 256)])
def test_two_runs_give_identical_bits(name, R):
    cam, env, image, weight, upstream = _device_case(name, R)
    runs = [ref.grads_of(composite_environment, env, image, weight, cam, upstream) for _ in range(2)]
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_strided_views_give_the_bits_of_their_clones():
    cam, env, image, weight, upstream = _device_case("seam", 7)
    H, W, _ = image.shape
    wide = torch.rand(H, W, 5, device=DEV)
    wide[..., 2:] = image
    pair = torch.rand(H, W, 2, device=DEV)
    pair[..., 1] = weight
    want = ref.grads_of(composite_environment, env, image, weight, cam, upstream)
    e = env.clone().requires_grad_(True)
    x, p = wide.clone().requires_grad_(True), pair.clone().requires_grad_(True)
    out = composite_environment(e, x[..., 2:], p[..., 1], cam)
    (out * upstream).sum().backward()
    assert torch.equal(out.detach(), want[0]) and torch.equal(e.grad, want[1]) and torch.equal(p.grad[..., 1], want[2])
    assert torch.equal(x.grad[..., 2:], upstream) and not x.grad[..., :2].any() and not p.grad[..., 0].any()


def test_texels_no_pixel_looks_at_hold_positive_zero():
    cam, env, image, weight, upstream = _device_case("tele", 64)
    _, d_env, _ = ref.grads_of(composite_environment, env, image, weight, cam, upstream)
    face, v, u = ref.lookup(ref.view_directions(ref.camera("tele")), 64)
    looked = torch.zeros(6, 64, 64, dtype=torch.bool)
    for dj in (0, 1):
        for di in (0, 1):
            looked[face, (v.floor().long() + dj).clamp(max=63), (u.floor().long() + di).clamp(max=63)] = True
    assert 0 < int(looked.sum()) < 0.05 * looked.numel()
    unseen = d_env.cpu()[~looked]
    assert not unseen.any() and not torch.signbit(unseen).any()
    assert bool(d_env.any())


@pytest.mark.parametrize("name,R", [("seam", 7), ("corner", 2), ("wide", 64), ("large", 256)])
def test_map_gradient_sums_to_the_weighted_upstream_gradient(name, R):
    """bilinear weights sum to one: d_env summed over texels = sum over pixels of (1 - w) grad_out, per channel"""
    cam, env, image, weight, upstream, _, _ = _case(name, R, 3)
    _, d_env, _ = _on_device(composite_environment, cam, env, image, weight, upstream)
    want = ((1 - weight)[..., None] * upstream).sum((0, 1))
    scale = float(((1 - weight)[..., None] * upstream).abs().sum())
    assert float((d_env.sum((0, 1, 2)) - want).abs().max()) <= 1e-13 * scale


def test_gradcheck_float64():
    cam, env, image, weight, _, keep, _ = _case("seam", 7, 3)
    assert bool(keep.all())
    inputs = [env.to(DEV).requires_grad_(True), weight.to(DEV).requires_grad_(True)]
    c, x = cam.to(device=DEV), image.to(DEV)
    assert gradcheck(lambda e, w: composite_environment(e, x, w, c), inputs, eps=1e-6, check_grad_dtypes=True,
                     check_undefined_grad=True)


def test_only_the_gradients_asked_for():
    cam, env, image, weight, upstream = _device_case("seam", 7)
    e = env.clone().requires_grad_(True)
    (composite_environment(e, image, weight, cam) * upstream).sum().backward()
    w = weight.clone().requires_grad_(True)
    (composite_environment(env, image, w, cam) * upstream).sum().backward()
    want = ref.grads_of(composite_environment, env, image, weight, cam, upstream)
    assert torch.equal(e.grad, want[1]) and torch.equal(w.grad, want[2])
    x = image.clone().requires_grad_(True)
    (composite_environment(env, x, weight, cam) * upstream).sum().backward()
    assert torch.equal(x.grad, upstream)
    c = cam.requires_grad_(True)
    (composite_environment(e, image, weight, c) * upstream).sum().backward()
    assert c.projection.grad is None and c.T_camera_world.grad is None
    c.requires_grad_(False)


# ------------------------------------------------------------------------------------------ behind the renderer
PARAMS = ("position", "log_scaling", "rotation", "alpha_logit", "feature")


def _dense(t, idx=None):
    t = t.to_dense() if t.is_sparse else t
    return t.cpu().double()


@pytest.mark.parametrize("sparse", [False, True])
def test_behind_the_renderer(sparse):
    """render(differentiable_weight) -> composite_environment -> photometric_loss: value and the gradients on the map
    and the five Gaussian parameters against the same chain with the float32 torch composition, both measured against
    a render whose backward is seeded with the float64 d_image and d_image_weight of the composition and the loss on
    the CPU"""
    size, n = (64, 48), 800
    g, camera = scenes.benchmark_scene(n, size, sh_degree=3, seed=0)
    cam, cfg = camera.to(device=DEV), RasterConfig()
    gen = torch.Generator().manual_seed(9)
    target = torch.rand(size[1], size[0], 3, generator=gen)
    env = torch.rand(6, 16, 16, 3, generator=gen)

    def render(gd):
        return gs.render_gaussians(gd, cam, cfg, use_sh=True, differentiable_weight=True, sparse_grad=sparse)

    def chain(fn):
        gd = g.to(DEV).requires_grad_(True)
        e = env.to(DEV).requires_grad_(True)
        r = render(gd)
        loss = losses.photometric_loss(fn(e, r.image, r.image_weight, cam), target.to(DEV))
        loss.backward()
        return (r, float(loss.detach())), [e.grad.cpu().double()] + [_dense(getattr(gd, k).grad) for k in PARAMS]

    (r, loss_ours), ours = chain(composite_environment)
    (_, loss_theirs), theirs = chain(ref.composite_reference)
    x = r.image.detach().cpu().double().requires_grad_(True)
    w = r.image_weight.detach().cpu().double().requires_grad_(True)
    e64 = env.double().requires_grad_(True)
    cam64 = ref.make_camera(size, camera.projection.double(), camera.T_camera_world.double()[:3, :3],
                            camera.T_camera_world.double()[:3, 3])
    loss64 = ssim_reference.photometric_loss(ref.composite_reference(e64, x, w, cam64), target.double())
    loss64.backward()
    truth = float(loss64.detach())
    gd = g.to(DEV).requires_grad_(True)
    r2 = render(gd)
    ((r2.image * x.grad.float().to(DEV)).sum() + (r2.image_weight * w.grad.float().to(DEV)).sum()).backward()
    want = [e64.grad] + [_dense(getattr(gd, k).grad) for k in PARAMS]
    rows = {"loss": (abs(loss_ours - truth), abs(loss_theirs - truth), abs(truth))}
    rows.update({name: (float((a - t0).abs().max()), float((t - t0).abs().max()), float(t0.abs().max()))
                 for name, a, t, t0 in zip(("d_env",) + PARAMS, ours, theirs, want)})
    assert all(scale > 0 for _, _, scale in rows.values())
    assert float(want[1 + PARAMS.index("alpha_logit")].abs().max()) > 0 and bool(ours[1 + PARAMS.index("alpha_logit")].any())
    _assert_float32(rows, f"behind the renderer (sparse_grad={sparse})")


def test_views_of_two_sizes_leave_one_summed_map_gradient():
    n = 800
    g, camera_a = scenes.benchmark_scene(n, (64, 48), sh_degree=3, seed=0)
    _, camera_b = scenes.benchmark_scene(n, (40, 56), sh_degree=3, seed=0)
    cams = [camera_a.to(device=DEV), camera_b.to(device=DEV)]
    gen = torch.Generator().manual_seed(10)
    env = torch.rand(6, 16, 16, 3, generator=gen).to(DEV)
    targets = [torch.rand(c.image_size[1], c.image_size[0], 3, generator=gen).to(DEV) for c in cams]

    def losses_of(views, e):
        return [losses.photometric_loss(composite_environment(e, r.image, r.image_weight, c), t)
                for r, c, t in zip(views, cams, targets)]

    e = env.clone().requires_grad_(True)
    gd = g.to(DEV).requires_grad_(True)
    views = gs.render_views(gd, cams, RasterConfig(), use_sh=True, differentiable_weight=True)
    sum(losses_of(views, e)).backward()
    singles = []
    for k in range(2):
        ek = env.clone().requires_grad_(True)
        gk = g.to(DEV).requires_grad_(True)
        r = gs.render_gaussians(gk, cams[k], RasterConfig(), use_sh=True, differentiable_weight=True)
        losses.photometric_loss(composite_environment(ek, r.image, r.image_weight, cams[k]), targets[k]).backward()
        singles.append(ek.grad)
    assert bool(singles[0].any()) and bool(singles[1].any())
    assert torch.equal(e.grad, singles[0] + singles[1])
    assert gd.alpha_logit.grad is not None and bool(_dense(gd.alpha_logit.grad).any())


def test_fit_of_a_sky_behind_fixed_gaussians():
    """Adam on a zero map of edge 16 against a frame rendered over a known map: the loss falls from one window of five
    steps to the next, and the looked-at texels come as close to the known map as the torch composition brings them in
    the same number of steps"""
    size, n, steps = (64, 48), 800, 40
    g, camera = scenes.benchmark_scene(n, size, sh_degree=3, seed=0)
    cam = camera.to(device=DEV)
    known = torch.rand(6, 16, 16, 3, generator=torch.Generator().manual_seed(11)).to(DEV)
    with torch.no_grad():
        r = gs.render_gaussians(g.to(DEV), cam, RasterConfig(), use_sh=True)
        image, weight = r.image.clone(), r.image_weight.clone()
        target = composite_environment(known, image, weight, cam)

    def fit(fn):
        env = torch.zeros_like(known).requires_grad_(True)
        optimizer = torch.optim.Adam([env], lr=5e-2)
        history = []
        for _ in range(steps):
            optimizer.zero_grad()
            loss = (fn(env, image, weight, cam) - target).square().mean()
            loss.backward()
            optimizer.step()
            history.append(loss.detach())
        return env.detach(), [float(v) for v in history], env.grad != 0

    ours, history, looked = fit(composite_environment)
    theirs, history_torch, looked_torch = fit(ref.composite_reference)
    windows = [sum(history[k:k + 5]) for k in range(0, steps, 5)]
    print(f"fit: loss {history[0]:.3e} -> {history[-1]:.3e} (torch {history_torch[-1]:.3e})")
    assert all(b < a for a, b in zip(windows, windows[1:])), windows
    assert torch.equal(looked, looked_torch) and 0 < int(looked.sum()) < looked.numel()
    err = float((ours - known)[looked].abs().mean())
    err_torch = float((theirs - known)[looked].abs().mean())
    start = float(known[looked].abs().mean())
    print(f"fit: mean |map - known| on the looked-at texels {start:.3e} -> {err:.3e} (torch {err_torch:.3e})")
    assert err_torch < start and err <= 1.01 * err_torch + 1e-6  # the same trajectory up to float32 rounding
    assert not ours[~looked].any()


# ----------------------------------------------------------------------------------------------- the record
def write_accuracy(path):
    lines = ["float32 accuracy of environment.composite_environment on the MI355X (tests/test_envmap_gpu.py)",
             "max |error| against the float64 yardstick (index gathers in torch on the CPU) on the same float32 inputs:",
             "the HIP operator, the float32 torch composition on the device, and the largest magnitude of the output.",
             "The test's bound is 4 x the composition's error (floor 1e-6 of the magnitude).", "",
             f"{'camera':>8} {'R':>4} {'C':>2} {'output':>15} {'HIP':>10} {'torch f32':>10} {'magnitude':>10} "
             f"{'HIP/torch':>9}"]
    cases = [(name, R, C) for name in ref.CAMERAS for R in EDGES for C in CHANNELS]
    cases += [("large", 256, 3)] + [("switch", R, 3) for R in THRESHOLD_EDGES]
    worst = 0.0
    for name, R, C in cases:
        for what, (ours, theirs, scale) in _float32_errors(name, R, C).items():
            ratio = ours / theirs if theirs > 0 else float("nan")
            if ours > 1e-6 * scale and theirs > 0:
                worst = max(worst, ratio)
            lines.append(f"{name:>8} {R:4d} {C:2d} {what:>15} {ours:10.3e} {theirs:10.3e} {scale:10.3e} {ratio:9.2f}")
    lines += ["", f"largest HIP / torch ratio among the errors above the floor: {worst:.2f}"]
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    write_accuracy(sys.argv[1] if len(sys.argv) > 1 else os.path.join(root, "profiles", "envmap", "accuracy.txt"))
