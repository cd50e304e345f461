"""Background colour and differentiable image_weight (`background=`, `differentiable_weight=` of rasterize*,
render_projected and render_gaussians), composited and differentiated inside the HIP rasterizer.

With T = 1 - image_weight the transmittance a pixel's walk ends with:  image_c = sum_i w_i f_ic + T bg_c, and both new
gradient terms enter the backward through the pixel's initial remaining colour only (dT/dalpha_i = -T / (1 - alpha_i)).

Reference: the CPU oracle, unchanged, through one construction -- the weight image IS a blended feature channel whose
feature is 1 everywhere, and a background is what remains of the image: feed `rasterize_backward` the features with a
ones column appended, the image [blended + T bg, W] and the gradient [G, G_W].  (Against autograd through
tests/dense_renderer.py that construction is exact to 5e-16 in f64.)  Bars: parity_util's, unchanged.
"""
import numpy as np
import pytest
import torch
from torch.autograd import gradcheck

import parity_util as pu
import taichi_gaussian_rasterizer_amd as gs
from oracle import oracle as orc
from taichi_gaussian_rasterizer_amd import RasterConfig, scenes
from taichi_gaussian_rasterizer_amd import _native as nv
from taichi_gaussian_rasterizer_amd.misc.renderer2d import project_gaussians2d
from taichi_gaussian_rasterizer_amd.perspective import projection as hip_proj
from taichi_gaussian_rasterizer_amd.renderer import render_projected

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
GRADCHECK = dict(eps=1e-6, check_grad_dtypes=True, check_undefined_grad=True)  # test_float64_gpu.GRADCHECK


def dev(x, dtype=None):
    return torch.as_tensor(np.asarray(x) if not isinstance(x, torch.Tensor) else x).to(device=DEV, dtype=dtype)


def _split(g2d):
    """(mean, axis, sigma, alpha) leaves of a packed (N, 7) tensor"""
    return [g2d[:, a:b].detach().clone().requires_grad_(True) for a, b in ((0, 2), (2, 4), (4, 6), (6, 7))]


def _raster_fn(o2p, ranges, size, cfg):
    def fn(mean, axis, sigma, alpha, colours, background):
        out = gs.rasterize_with_tiles(torch.cat((mean, axis, sigma, alpha), 1), colours, o2p, ranges, size, cfg,
                                      background=background, differentiable_weight=True)
        return out.image, out.image_weight
    return fn


# ------------------------------------------------------------------------------------------ 1. f64 gradcheck
@pytest.mark.parametrize("antialias", [False, True])
@pytest.mark.parametrize("seed", range(6))
def test_gradcheck_reference_scene(seed, antialias):
    """the reference's scene (8x8, one tile of 8, n < 50): (mean, axis, sigma, alpha, colours, background) ->
    (image, image_weight), saturate_threshold = 1 so that the function gradcheck differences is the one differentiated"""
    torch.manual_seed(seed)
    n = torch.randint(1, 50, (1,)).item()
    channels = torch.randint(1, 4, (1,)).item()
    size = (8, 8)
    g = scenes.random_2d_gaussians(n, size, num_channels=channels, scale_factor=1.0, alpha_range=(0.2, 0.8))
    g2d = project_gaussians2d(g).to(DEV, F64)
    colours = g.feature.to(DEV, F64).requires_grad_(True)
    bg = torch.rand(channels, dtype=F64).to(DEV).requires_grad_(True)
    cfg = RasterConfig(tile_size=8, pixel_stride=(1, 1), antialias=antialias, saturate_threshold=1.0)
    o2p = torch.arange(n, dtype=torch.int32, device=DEV)
    ranges = torch.tensor([[0, n]], dtype=torch.int32, device=DEV)
    assert gradcheck(_raster_fn(o2p, ranges, size, cfg), (*_split(g2d), colours, bg), **GRADCHECK)


@pytest.mark.parametrize("seed,tile,size,n", [(0, 8, (37, 21), 14), (2, 32, (45, 21), 12)])
def test_gradcheck_across_tiles(seed, tile, size, n):
    """lists from the float32 mapper, image sizes that are no tile multiples, splats in several lists, visibility and
    heuristics on"""
    torch.manual_seed(seed)
    g = scenes.random_2d_gaussians(n, size, num_channels=2, scale_factor=1.5, alpha_range=(0.2, 0.8))
    g2d = project_gaussians2d(g).to(DEV, F64)
    depth = g.z_depth.clamp(0, 1).to(DEV, torch.float32)
    cfg = RasterConfig(tile_size=tile, saturate_threshold=1.0, compute_visibility=True, compute_point_heuristic=True)
    o2p, ranges = gs.map_to_tiles(g2d.float(), depth, size, cfg)
    ranges = ranges.view(-1, 2)
    assert int((torch.bincount(o2p.long(), minlength=n) >= 2).sum()) >= 2, "scene must put splats in several lists"
    colours = g.feature.to(DEV, F64).requires_grad_(True)
    bg = torch.rand(2, dtype=F64).to(DEV).requires_grad_(True)
    assert gradcheck(_raster_fn(o2p, ranges, size, cfg), (*_split(g2d), colours, bg), **GRADCHECK)


# --------------------------------------------------------------------------------------- 2. f64 bit equality
def test_f64_zero_background_is_the_plain_call_bit_for_bit():
    """background = zeros and a constant weight change nothing: image and every gradient equal with ==  (the f64
    kernels are deterministic)"""
    size, n = (45, 21), 60
    torch.manual_seed(3)
    g = scenes.random_2d_gaussians(n, size, num_channels=3, scale_factor=1.0, alpha_range=(0.2, 0.8))
    g2d = project_gaussians2d(g).to(DEV, F64)
    depth = g.z_depth.clamp(0, 1).to(DEV, torch.float32)
    cfg = RasterConfig(tile_size=16, compute_point_heuristic=True)
    o2p, ranges = gs.map_to_tiles(g2d.float(), depth, size, cfg)
    ranges = ranges.view(-1, 2)
    G = torch.rand(size[1], size[0], 3, dtype=F64, generator=torch.Generator().manual_seed(4)).to(DEV)
    results = []
    for kw in (dict(), dict(background=torch.zeros(3, dtype=F64, device=DEV), differentiable_weight=False)):
        a, f = g2d.clone().requires_grad_(True), g.feature.to(DEV, F64).requires_grad_(True)
        out = gs.rasterize_with_tiles(a, f, o2p, ranges, size, cfg, **kw)
        (out.image * G).sum().backward()
        results.append((out.image.detach(), out.image_weight, a.grad, f.grad, out.point_heuristic))
    for x, y in zip(*results):
        assert torch.equal(x, y)


# ------------------------------------------------------------------- 3. f32 narrow and wide kernels vs oracle
def oracle_with_weight(g2d, feat, o2p, ranges, size, ocfg, bg, G, GW, dtype=np.float32, hip_image=None,
                       hip_weight=None):
    """the construction of the module docstring.  hip_image / hip_weight: the backward consumes the forward's own images,
    so the f32 oracle gets the HIP ones and only the backward kernel is measured.  Returns (composited image, weight,
    grad_gaussians2d, grad_features, grad_background, heuristics)"""
    g, f = pu.to_np(g2d).astype(dtype), pu.to_np(feat).astype(dtype)
    bg, G, GW = (pu.to_np(t).astype(dtype) for t in (bg, G, GW))
    blended, weight, _ = orc.rasterize_with_tiles(g, f, o2p, ranges, size, ocfg)
    T = 1 - weight
    comp = blended + T[..., None] * bg
    f1 = np.concatenate([f, np.ones((f.shape[0], 1), dtype)], 1)
    img1 = np.concatenate([comp if hip_image is None else pu.to_np(hip_image).astype(dtype),
                           (weight if hip_weight is None else pu.to_np(hip_weight).astype(dtype))[..., None]], -1)
    gg, gf1, heur = orc.rasterize_backward(g, f1, o2p, ranges, size, img1, np.concatenate([G, GW[..., None]], -1), ocfg)
    return comp, weight, gg, gf1[:, :-1], (G * T[..., None]).sum((0, 1)), heur


def _check_against_oracle(seed, n, size, tile, F, cfg_kw=None, scale_factor=0.5, flip_bar=pu.FLIP_MARGIN,
                          min_T=1e-3):
    g2d, depth, feat = pu.make_2d_scene(seed, n, size, channels=F, scale_factor=scale_factor, alpha_range=(0.2, 0.8))
    cfg = RasterConfig(tile_size=tile, **(cfg_kw or {}))
    ocfg = orc.OracleConfig.of(cfg)
    o2p, ranges = orc.map_to_tiles(g2d, depth, size, ocfg)
    gen = torch.Generator().manual_seed(1000 + seed)
    bg = torch.rand(F, generator=gen)
    G = torch.rand(size[1], size[0], F, generator=gen)
    GW = torch.rand(size[1], size[0], generator=gen) * 2 - 1  # mixed sign
    g_t, f_t, bg_t = dev(g2d).requires_grad_(True), dev(feat).requires_grad_(True), dev(bg).requires_grad_(True)
    out = gs.rasterize_with_tiles(g_t, f_t, dev(o2p), dev(ranges.reshape(-1, 2)), size, cfg, background=bg_t,
                                  differentiable_weight=True)
    ((out.image * dev(G)).sum() + (out.image_weight * dev(GW)).sum()).backward()
    comp, weight, gg, gf, gbg, heur = oracle_with_weight(g2d, feat, o2p, ranges, size, ocfg, bg, G, GW,
                                                        hip_image=out.image, hip_weight=out.image_weight)
    _, _, gg64, gf64, gbg64, _ = oracle_with_weight(g2d, feat, o2p, ranges, size, ocfg, bg, G, GW, dtype=np.float64)
    if min_T is not None:
        # neither saturation nor forward_cut is active: the dense renderer and the oracle agree exactly here
        assert float((1 - weight).min()) > min_T
    proof = pu.flip_proof(g2d, feat, o2p, ranges, size, ocfg, bar=flip_bar)
    # a flipped splat moves the composited channel by thr T |f_c - bg_c| <= thr T max(|f_c|, 1) for bg in [0, 1]
    pu.assert_pixels_close(out.image, comp, "composited image", flips=proof)
    pu.assert_pixels_close(out.image_weight, weight, "weight", flips=proof.weight())
    assert torch.isfinite(g_t.grad).all() and torch.isfinite(f_t.grad).all() and torch.isfinite(bg_t.grad).all()
    pu.assert_grad_close_vs_truth(g_t.grad, gg, gg64, "grad_gaussians2d")
    pu.assert_grad_close_vs_truth(f_t.grad, gf, gf64, "grad_features")
    pu.assert_grad_close_vs_truth(bg_t.grad, gbg, gbg64, "grad_background")
    if cfg.compute_point_heuristic:
        pu.assert_grad_close(out.point_heuristic, heur, "point_heuristic", tol=1e-3)  # test_gpu_parity's bar for them


SIZES = [(0, 120, (45, 21), 16), (1, 80, (37, 21), 8), (2, 300, (64, 48), 16)]


@pytest.mark.parametrize("F", [1, 3, 5, 8, 32, 40])
@pytest.mark.parametrize("seed,n,size,tile", SIZES)
def test_raster_with_background_and_weight_gradient(seed, n, size, tile, F):
    """every narrow feature-width instantiation (3, 5, 8, 32) and the wide kernels (F = 40)"""
    _check_against_oracle(seed, n, size, tile, F)


@pytest.mark.parametrize("nb", [1, 2, 4])
@pytest.mark.parametrize("seed,n,size,tile", SIZES)
def test_raster_wave_regions(nb, seed, n, size, tile, monkeypatch):
    monkeypatch.setitem(nv.TUNING, "wave_sub_blocks", int(nb))
    _check_against_oracle(seed, n, size, tile, 3)


@pytest.mark.parametrize("F", [3, 40])
@pytest.mark.parametrize("seed,n,size,tile", SIZES)
def test_raster_heuristics(seed, n, size, tile, F):
    """the densification statistics are sums of functions of the corrected dL/dalpha and dL/dmean"""
    _check_against_oracle(seed, n, size, tile, F, dict(compute_point_heuristic=True))


@pytest.mark.parametrize("F", [3, 40])
@pytest.mark.parametrize("seed,n,size,tile", SIZES)
def test_raster_antialias(seed, n, size, tile, F):
    _check_against_oracle(seed, n, size, tile, F, dict(antialias=True, blur_cov=0.0, compute_point_heuristic=True),
                          flip_bar=pu.AA_FLIP_MARGIN)


# ------------------------------------------------------------------------------------------- 4. crowded case
@pytest.mark.parametrize("F", [3, 40])
def test_raster_crowded(F):
    """scale_factor 2, 600 splats on 45x21: saturated pixels (the backward stops at saturate_threshold, the forward at
    forward_cut), compared with the f32 oracle and with the f64 oracle as the yardstick; everything finite"""
    _check_against_oracle(7, 600, (45, 21), 16, F, scale_factor=2.0, min_T=None)


# -------------------------------------------------------------------------- 5. render_gaussians, fused frame
def _plain_scene(n, size, seed, scale_factor=1.5):
    torch.manual_seed(seed)
    camera = scenes.benchmark_camera(size)
    g = scenes.random_3d_gaussians(n, camera, scale_factor=scale_factor, margin=0.1)
    assert g.feature.shape == (n, 3)
    return g, camera.to(device=DEV)


def _upstream(size, seed):
    gen = torch.Generator().manual_seed(seed)
    return (dev(torch.rand(size[1], size[0], 3, generator=gen)),
            dev(torch.rand(size[1], size[0], generator=gen) * 2 - 1), dev(torch.rand(3, generator=gen)))


@pytest.mark.parametrize("size,n", [((64, 48), 500), ((100, 70), 2000)])
def test_fused_weight_gradient_against_a_ones_channel(size, n, frame_path):
    """plain features, C = 3.  Reference: the existing path with a ones column appended (four channels, the fourth IS the
    weight), loss sum(G img[..., :3]) + sum(G_W img[..., 3]) -- kernels that are already oracle-verified.  Then the same
    with a background: image(bg) - image(0) == (1 - image_weight) * bg."""
    g, cam = _plain_scene(n, size, seed=n)
    G, GW, bg = _upstream(size, 11)
    cfg = RasterConfig()
    ones = torch.ones(n, 1)
    ref = g.replace(feature=torch.cat((g.feature, ones), 1)).to(DEV).requires_grad_(True)
    r_ref = gs.render_gaussians(ref, cam, cfg)
    ((r_ref.image[..., :3] * G).sum() + (r_ref.image[..., 3] * GW).sum()).backward()
    a = g.to(DEV).requires_grad_(True)
    r = gs.render_gaussians(a, cam, cfg, differentiable_weight=True)
    assert r.image_weight.requires_grad
    ((r.image * G).sum() + (r.image_weight * GW).sum()).backward()
    assert torch.equal(r.image, r_ref.image[..., :3]) and torch.equal(r.image_weight, r_ref.image_weight)
    for k, t in a.items():
        expect = getattr(ref, k).grad
        pu.assert_grad_close(t.grad, expect[:, :3] if k == "feature" else expect, f"grad {k}", tol=pu.GRAD_TOL)
    # ... with a background
    b = g.to(DEV).requires_grad_(True)
    bg_t = bg.clone().requires_grad_(True)
    rb = gs.render_gaussians(b, cam, cfg, background=bg_t, differentiable_weight=True)
    assert torch.equal(rb.image_weight, r.image_weight)
    T = 1 - r.image_weight.detach()
    assert torch.allclose(rb.image.detach() - r.image.detach(), T.unsqueeze(-1) * bg, rtol=0, atol=pu.ATOL)
    ((rb.image * G).sum() + (rb.image_weight * GW).sum()).backward()
    # d/dalpha of T bg . G is the weight gradient -(bg . G): the ones-channel reference with G_W - bg . G
    ref2 = g.replace(feature=torch.cat((g.feature, ones), 1)).to(DEV).requires_grad_(True)
    r2 = gs.render_gaussians(ref2, cam, cfg)
    ((r2.image[..., :3] * G).sum() + (r2.image[..., 3] * (GW - (G * bg).sum(-1))).sum()).backward()
    for k, t in b.items():
        expect = getattr(ref2, k).grad
        pu.assert_grad_close(t.grad, expect[:, :3] if k == "feature" else expect, f"grad {k} with background",
                             tol=pu.GRAD_TOL)
    pu.assert_grad_close(bg_t.grad, (G * T.unsqueeze(-1)).sum((0, 1)), "grad background", tol=pu.GRAD_TOL)


def _frame_counts(rendering):
    """the eight counters of the frame's workspace (fused._forward_call): [7] = tiles split into four workgroups"""
    node = rendering.image.grad_fn
    layout = node.meta["frame"][1]
    return node.saved_tensors[7].view(torch.int32)[layout.counts // 4:layout.counts // 4 + 8].tolist()


@pytest.mark.parametrize("degree,size,n,crowded", [(0, (64, 48), 500, False), (3, (100, 70), 2000, False),
                                                   (3, (100, 70), 2000, True)])
def test_fused_sh_frame_against_composed_operators(degree, size, n, crowded, frame_path, monkeypatch):
    """SH colours: the fused frame against project_with_ndc -> evaluate_sh_at -> render_projected (rasterize with the
    two arguments).  Images bit-equal, gradients at GRAD_TOL, the camera's included.  crowded: 16x16 wave regions forced
    on the benchmark scene (scale_factor 2), where the mapper marks heavy tiles (counts[7] > 0) that the frame gives four
    8x8 workgroups each -- the composed operators split nothing, so pixels agree as in
    test_gpu_parity.test_fused_frame_splits_heavy_tiles (the saturation cut of an 8x8 quadrant may fall at another
    splat than the region's: 2e-6)."""
    cfg = RasterConfig()
    g, camera = scenes.benchmark_scene(n, size, sh_degree=degree, seed=degree, scale_factor=2.0 if crowded else 1.0)
    G, GW, bg = _upstream(size, 12)
    outs = []
    for fused in (False, True):
        cam = camera.to(device=DEV)
        cam.T_camera_world.requires_grad_(True)
        cam.projection.requires_grad_(True)
        a = g.to(DEV).requires_grad_(True)
        bg_t = bg.clone().requires_grad_(True)
        if fused:
            if crowded:
                monkeypatch.setitem(nv.TUNING, "wave_sub_blocks", 4)
            r = gs.render_gaussians(a, cam, cfg, use_sh=True, background=bg_t, differentiable_weight=True)
            if crowded:
                assert _frame_counts(r)[7] > 0, "the scene must have heavy tiles"
        else:
            g2d, depths, idx, ndc = hip_proj.project_with_ndc(*a.shape_tensors(), cam.T_camera_world, cam.projection,
                                                              cam.image_size, cam.depth_range, cfg)
            colours = gs.evaluate_sh_at(a.feature, a.position.detach(), idx, cam.camera_position)
            r = render_projected(idx, g2d, colours, depths, cam, cfg, ndc_depths=ndc, background=bg_t,
                                 differentiable_weight=True)
        ((r.image * G).sum() + (r.image_weight * GW).sum()).backward()
        outs.append((r.image.detach().clone(), r.image_weight.detach().clone(),
                     {k: t.grad.clone() for k, t in a.items()}, cam.T_camera_world.grad.clone(),
                     cam.projection.grad.clone(), bg_t.grad.clone()))
    composed, frame = outs
    if crowded:
        assert torch.allclose(frame[0], composed[0], rtol=0, atol=2e-6)
        assert torch.allclose(frame[1], composed[1], rtol=0, atol=2e-6)
    else:
        assert torch.equal(frame[0], composed[0]) and torch.equal(frame[1], composed[1])
    tol = pu.GRAD_TOL
    for k in frame[2]:
        pu.assert_grad_close(frame[2][k], composed[2][k], f"grad {k}", tol=tol)
    pu.assert_grad_close(frame[3], composed[3], "grad T_camera_world", tol=tol)
    pu.assert_grad_close(frame[4], composed[4], "grad projection", tol=tol)
    pu.assert_grad_close(frame[5], composed[5], "grad background", tol=tol)


def test_fused_depth_render_composites_the_colour_channels_only(frame_path):
    """render_depth: the blended image has 2 + C channels and the background applies to channels 2... only -- depth and
    depth_var are bit-identical with and without it, and keep treating the weight in their divisor as a constant"""
    size, n = (64, 48), 800
    g, cam = _plain_scene(n, size, seed=5)
    G, GW, bg = _upstream(size, 13)
    cfg = RasterConfig()
    a = g.to(DEV).requires_grad_(True)
    plain = gs.render_gaussians(a, cam, cfg, render_depth=True)
    (plain.depth.sum() + 0.1 * plain.depth_var.sum()).backward()
    b = g.to(DEV).requires_grad_(True)
    r = gs.render_gaussians(b, cam, cfg, render_depth=True, background=bg, differentiable_weight=True)
    assert torch.equal(r.depth, plain.depth) and torch.equal(r.depth_var, plain.depth_var)
    assert torch.equal(r.image_weight, plain.image_weight)
    T = 1 - plain.image_weight
    assert torch.allclose(r.image - plain.image, T.unsqueeze(-1) * bg, rtol=0, atol=pu.ATOL)
    (r.depth.sum() + 0.1 * r.depth_var.sum()).backward()
    for k, t in b.items():  # the divisor is a constant: the same gradients as without the switch
        pu.assert_grad_close(t.grad, getattr(a, k).grad, f"grad {k} of depth, depth_var", tol=pu.GRAD_TOL)
    # and the composed operators agree with the frame on image + weight gradients of a depth render
    c = g.to(DEV).requires_grad_(True)
    rc = gs.render_gaussians(c, cam, cfg, render_depth=True, background=bg, differentiable_weight=True)
    ((rc.image * G).sum() + (rc.image_weight * GW).sum() + rc.depth.sum()).backward()
    d = g.to(DEV).requires_grad_(True)
    g2d, depths, idx, ndc = hip_proj.project_with_ndc(*d.shape_tensors(), cam.T_camera_world, cam.projection,
                                                      cam.image_size, cam.depth_range, cfg)
    rd = render_projected(idx, g2d, d.feature[idx], depths, cam, cfg, render_depth=True, ndc_depths=ndc,
                          background=bg, differentiable_weight=True)
    assert torch.equal(rd.image, rc.image) and torch.equal(rd.depth, rc.depth)
    ((rd.image * G).sum() + (rd.image_weight * GW).sum() + rd.depth.sum()).backward()
    for k, t in c.items():
        pu.assert_grad_close(t.grad, getattr(d, k).grad, f"grad {k}: frame vs composed depth render", tol=pu.GRAD_TOL)


def test_fused_sparse_gradients(frame_path):
    """sparse_grad=True: the sparse values are the dense rows"""
    size, n = (100, 70), 1500
    g, camera = scenes.benchmark_scene(n, size, sh_degree=2, seed=9, scale_factor=1.0)
    cam = camera.to(device=DEV)
    G, GW, bg = _upstream(size, 14)
    grads = []
    for sparse in (False, True):
        a = g.to(DEV).requires_grad_(True)
        bg_t = bg.clone().requires_grad_(True)
        r = gs.render_gaussians(a, cam, RasterConfig(), use_sh=True, background=bg_t, differentiable_weight=True,
                                sparse_grad=sparse)
        ((r.image * G).sum() + (r.image_weight * GW).sum()).backward()
        grads.append(({k: t.grad for k, t in a.items()}, bg_t.grad, r.points_in_view))
    (dense, bg_dense, idx), (sparse, bg_sparse, _) = grads
    assert 0 < idx.shape[0] < n
    for k, t in sparse.items():
        assert t.is_sparse and torch.equal(t._indices()[0], idx)
        pu.assert_grad_close(t._values(), dense[k][idx], f"sparse grad {k}", tol=pu.GRAD_TOL)
    pu.assert_grad_close(bg_sparse, bg_dense, "grad background", tol=pu.GRAD_TOL)


# ------------------------------------------------------------------------------------------- 6. empty frames
@pytest.mark.parametrize("case", ["no_gaussians", "all_culled", "no_overlaps"])
def test_empty_frames(case, frame_path):
    """image == background, weight == 0, dL/dbackground = sum of the upstream gradient: N = 0 (composed operators), all
    Gaussians behind the camera (V = 0) and projected splats below the alpha threshold (K = 0)"""
    size = (40, 24)
    g, camera = scenes.benchmark_scene(50, size, sh_degree=1, seed=1)
    cam = camera.to(device=DEV)
    if case == "no_gaussians":
        g = g[:0]
    elif case == "all_culled":
        g = g.replace(position=g.position * torch.tensor([1.0, 1.0, -1.0]))
    else:
        g = g.replace(alpha_logit=torch.full_like(g.alpha_logit, -12.0))
    G, GW, bg = _upstream(size, 15)
    a = g.to(DEV).requires_grad_(True)
    bg_t = bg.clone().requires_grad_(True)
    r = gs.render_gaussians(a, cam, RasterConfig(), use_sh=True, background=bg_t, differentiable_weight=True)
    if case != "no_overlaps":
        assert r.points_in_view.shape[0] == 0
    assert torch.equal(r.image.detach(), bg.expand(size[1], size[0], 3))
    assert float(r.image_weight.detach().abs().max()) == 0.0
    ((r.image * G).sum() + (r.image_weight * GW).sum()).backward()
    assert torch.allclose(bg_t.grad, G.sum((0, 1)), rtol=1e-6, atol=0)
    for k, t in a.items():
        assert t.grad is None or float(t.grad.abs().max() if t.grad.numel() else 0.0) == 0.0


def test_empty_tile_lists_raster_every_kernel():
    """rasterize_with_tiles with K = 0 (five splats, listed by no tile): narrow, wide and float64 kernels fill the image
    with the background, and the splats get zero gradients"""
    size, tile = (21, 13), 8
    tiles = (-(-size[0] // tile)) * (-(-size[1] // tile))
    o2p = torch.zeros((0,), dtype=torch.int32, device=DEV)
    ranges = torch.zeros((tiles, 2), dtype=torch.int32, device=DEV)
    for F, dt in ((3, torch.float32), (40, torch.float32), (3, F64)):
        bg = torch.rand(F, dtype=dt).to(DEV).requires_grad_(True)
        G = torch.rand(size[1], size[0], F, dtype=dt).to(DEV)
        g2d, _, feat = pu.make_2d_scene(0, 5, size, channels=F)
        g_t, f_t = dev(g2d, dt).requires_grad_(True), dev(feat, dt).requires_grad_(True)
        out = gs.rasterize_with_tiles(g_t, f_t, o2p, ranges, size, RasterConfig(tile_size=tile), background=bg,
                                      differentiable_weight=True)
        assert torch.equal(out.image.detach(), bg.detach().expand(size[1], size[0], F))
        assert float(out.image_weight.detach().abs().max()) == 0.0
        ((out.image * G).sum() + out.image_weight.sum()).backward()
        assert torch.allclose(bg.grad, G.sum((0, 1)), rtol=1e-6 if dt == torch.float32 else 1e-14, atol=0)
        assert float(g_t.grad.abs().max()) == 0.0 and float(f_t.grad.abs().max()) == 0.0


def test_refusals_on_device_tensors():
    size = (16, 16)
    g2d, depth, feat = pu.make_2d_scene(0, 10, size)
    args = (dev(g2d), dev(depth), dev(feat), size)
    pick = RasterConfig(use_alpha_blending=False, saturate_threshold=0.5)
    with pytest.raises(ValueError, match="use_alpha_blending"):
        gs.rasterize(*args, pick, background=torch.zeros(3, device=DEV))
    with pytest.raises(ValueError, match="use_alpha_blending"):
        gs.rasterize(*args, pick, differentiable_weight=True)
    with pytest.raises(TypeError):
        gs.rasterize(*args, RasterConfig(), background=torch.zeros(3, device=DEV, dtype=F64))
    with pytest.raises(TypeError):
        gs.rasterize(*args, RasterConfig(), background=torch.zeros(3))
    with pytest.raises(AssertionError, match="background"):
        gs.rasterize(*args, RasterConfig(), background=torch.zeros(4, device=DEV))
    # the median-depth pass of render_gaussians stays as it is, without a background
    g, camera = scenes.benchmark_scene(300, (64, 48), sh_degree=1, seed=2)
    cam = camera.to(device=DEV)
    bg = torch.rand(3, device=DEV)
    m0 = gs.render_gaussians(g.to(DEV), cam, RasterConfig(), use_sh=True, render_median_depth=True)
    m1 = gs.render_gaussians(g.to(DEV), cam, RasterConfig(), use_sh=True, render_median_depth=True, background=bg,
                             differentiable_weight=True)
    assert torch.equal(m0.median_depth, m1.median_depth)
