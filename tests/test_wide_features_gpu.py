"""Feature widths 33..512 (gs_raster_fwd_wide / gs_raster_bwd_wide, csrc/raster_wide.hip) against the CPU oracle, which
takes any width (oracle/gsplat_oracle.cpp), at the bars of the narrow rasterizer's tests in test_gpu_parity.py."""
import dataclasses

import numpy as np
import pytest
import torch

import parity_util as pu
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

import taichi_gaussian_rasterizer_amd as gs  # noqa: E402
from taichi_gaussian_rasterizer_amd import RasterConfig, scenes  # noqa: E402

DEV = "cuda:0"


def dev(x):
    t = torch.as_tensor(np.ascontiguousarray(x)) if not isinstance(x, torch.Tensor) else x
    return t.to(DEV).contiguous()


def raster_case(seed, n, size, F, cfg, scale_factor=1.0, alpha_range=(0.2, 0.8)):
    g2d, depth, feat = pu.make_2d_scene(seed, n, size, channels=F, scale_factor=scale_factor, alpha_range=alpha_range)
    ocfg = orc.OracleConfig.of(cfg)
    o2p, ranges = orc.map_to_tiles(g2d, depth, size, ocfg)
    g_t, f_t = dev(g2d).requires_grad_(True), dev(feat).requires_grad_(True)
    out = gs.rasterize_with_tiles(g_t, f_t, dev(o2p), dev(ranges.reshape(-1, 2)), size, cfg)
    return g2d, feat, o2p, ranges, ocfg, g_t, f_t, out


def check_backward(g2d, feat, o2p, ranges, size, ocfg, g_t, f_t, out, seed):
    F = feat.shape[1]
    gi = torch.rand(size[1], size[0], F, generator=torch.Generator().manual_seed(100 + seed))
    (out.image * dev(gi)).sum().backward()
    gg, gf, heur = orc.rasterize_backward(g2d, feat, o2p, ranges, size, pu.to_np(out.image), gi.numpy(), ocfg)
    _, gg64, gf64 = pu.raster_truth(g2d, feat, o2p, ranges, size, ocfg, gi)
    pu.assert_grad_close_vs_truth(g_t.grad, gg, gg64, "grad_gaussians2d")
    pu.assert_grad_close_vs_truth(f_t.grad, gf, gf64, "grad_features")
    return gi, heur


@pytest.mark.parametrize("seed,n,size,tile,F", [(1, 1500, (100, 70), 16, 33), (2, 1500, (90, 53), 8, 64),
                                                (3, 1200, (130, 75), 32, 100), (4, 700, (72, 40), 16, 256)])
def test_wide_raster_forward_backward(seed, n, size, tile, F):
    """image, weight and both gradients; image sizes that are not tile multiples, tiles with several staging batches"""
    cfg = RasterConfig(tile_size=tile)
    g2d, feat, o2p, ranges, ocfg, g_t, f_t, out = raster_case(seed, n, size, F, cfg)
    assert int((ranges[..., 1] - ranges[..., 0]).max()) > 64
    image_ref, alpha_ref, _ = orc.rasterize_with_tiles(g2d, feat, o2p, ranges, size, ocfg)
    assert tuple(out.image.shape) == (size[1], size[0], F)
    proof = pu.flip_proof(g2d, feat, o2p, ranges, size, ocfg)
    pu.assert_pixels_close(out.image, image_ref, "image", flips=proof)
    pu.assert_pixels_close(out.image_weight, alpha_ref, "alpha", flips=proof.weight())
    check_backward(g2d, feat, o2p, ranges, size, ocfg, g_t, f_t, out, seed)


def test_wide_point_heuristic_and_visibility():
    """the heuristics square and take |.| of dL/dalpha, which sums over ALL channels: rasterizing 32-channel slices
    and adding their heuristics does not give them (checked below), the wide backward does"""
    size, n, F = (120, 80), 1500, 64
    cfg = RasterConfig(compute_visibility=True, compute_point_heuristic=True)
    g2d, feat, o2p, ranges, ocfg, g_t, f_t, out = raster_case(5, n, size, F, cfg, alpha_range=(0.2, 1.0))
    _, _, vis_ref = orc.rasterize_with_tiles(g2d, feat, o2p, ranges, size, ocfg)
    pu.assert_grad_close(out.visibility, vis_ref, "visibility", tol=1e-5)
    gi, heur_ref = check_backward(g2d, feat, o2p, ranges, size, ocfg, g_t, f_t, out, 5)
    pu.assert_grad_close(out.point_heuristic, heur_ref, "point_heuristic", tol=1e-3)
    # the slicing workaround is measurably wrong on the same scene
    sliced = torch.zeros_like(out.point_heuristic)
    for c0 in range(0, F, 32):
        part = gs.rasterize_with_tiles(g_t.detach(), f_t.detach()[:, c0:c0 + 32].contiguous().requires_grad_(True),
                                       dev(o2p), dev(ranges.reshape(-1, 2)), size, cfg)
        (part.image * dev(gi[..., c0:c0 + 32])).sum().backward()
        sliced += part.point_heuristic
    err = float((sliced - dev(heur_ref)).abs().max()) / float(np.abs(heur_ref).max())
    assert err > 1e-2


def test_wide_antialias():
    size, n, F = (96, 72), 2500, 48
    cfg = RasterConfig(antialias=True, blur_cov=0.0)
    g2d, feat, o2p, ranges, ocfg, g_t, f_t, out = raster_case(6, n, size, F, cfg, scale_factor=1.5)
    image_ref, alpha_ref, _ = orc.rasterize_with_tiles(g2d, feat, o2p, ranges, size, ocfg)
    proof = pu.flip_proof(g2d, feat, o2p, ranges, size, ocfg, bar=pu.AA_FLIP_MARGIN)
    pu.assert_pixels_close(out.image, image_ref, "antialias image", flips=proof)
    pu.assert_pixels_close(out.image_weight, alpha_ref, "antialias weight", flips=proof.weight())
    check_backward(g2d, feat, o2p, ranges, size, ocfg, g_t, f_t, out, 6)


def test_wide_forward_cut_zero():
    size, n, F = (80, 64), 3000, 40
    cfg = RasterConfig(forward_cut=0.0)
    g2d, feat, o2p, ranges, ocfg, g_t, f_t, out = raster_case(7, n, size, F, cfg, scale_factor=2.0)
    image_ref, alpha_ref, _ = orc.rasterize_with_tiles(g2d, feat, o2p, ranges, size, ocfg)
    proof = pu.flip_proof(g2d, feat, o2p, ranges, size, ocfg)
    pu.assert_pixels_close(out.image, image_ref, "image", flips=proof)
    pu.assert_pixels_close(out.image_weight, alpha_ref, "alpha", flips=proof.weight())
    check_backward(g2d, feat, o2p, ranges, size, ocfg, g_t, f_t, out, 7)


def test_wide_without_alpha_blending():
    """quantile mode (forward.py:109-114): the pixel takes the features of the first splat past the level; there is
    no backward (reference tests/test_rasterizer.py:92-101)"""
    size, n, F = (96, 64), 800, 40
    cfg = RasterConfig(use_alpha_blending=False, saturate_threshold=0.5)
    g2d, feat, o2p, ranges, ocfg, g_t, f_t, out = raster_case(8, n, size, F, cfg, scale_factor=0.6,
                                                              alpha_range=(0.3, 0.9))
    image_ref, alpha_ref, _ = orc.rasterize_with_tiles(g2d, feat, o2p, ranges, size, ocfg)
    proof = pu.flip_proof(g2d, feat, o2p, ranges, size, ocfg)
    pu.assert_pixels_close(out.image, image_ref, "quantile image", flips=proof, bound=False)
    assert (pu.to_np(out.image_weight) == alpha_ref).mean() > 0.999
    with pytest.raises(NotImplementedError):
        out.image.sum().backward()


def test_wide_empty():
    cfg = RasterConfig()
    size, F = (40, 30), 64
    ranges = torch.zeros((6, 2), dtype=torch.int32, device=DEV)
    f0 = torch.zeros((0, F), device=DEV, requires_grad=True)
    out = gs.rasterize_with_tiles(torch.zeros((0, 7), device=DEV), f0, torch.zeros((0,), dtype=torch.int32, device=DEV),
                                  ranges, size, cfg)
    assert tuple(out.image.shape) == (30, 40, F) and float(out.image.abs().sum()) == 0.0
    assert float(out.image_weight.abs().sum()) == 0.0
    out.image.sum().backward()
    assert tuple(f0.grad.shape) == (0, F)
    # Gaussians but empty tile lists
    g2d, _, feat = pu.make_2d_scene(9, 50, size, channels=F)
    g_t, f_t = dev(g2d).requires_grad_(True), dev(feat).requires_grad_(True)
    out = gs.rasterize_with_tiles(g_t, f_t, torch.zeros((0,), dtype=torch.int32, device=DEV), ranges, size, cfg)
    assert float(out.image.abs().sum()) == 0.0 and float(out.image_weight.abs().sum()) == 0.0
    out.image.sum().backward()
    assert float(g_t.grad.abs().sum()) == 0.0 and float(f_t.grad.abs().sum()) == 0.0


def test_wide_render_gaussians_depth_median_statistics():
    """render_gaussians with (N, 64) features takes the composed operators (the fused frame stops at 30 channels):
    the raster stage with depth channels (66 wide), the median-depth pass, visibility and heuristics against the
    oracle fed the same projected splats; the gradient reaches Gaussians3D.feature"""
    size, n, F = (128, 96), 3000, 64
    torch.manual_seed(10)
    camera = scenes.benchmark_camera(size)
    g = scenes.random_3d_gaussians(n, camera, scale_factor=1.5, margin=0.1)
    g = type(g)(position=g.position, log_scaling=g.log_scaling, rotation=g.rotation, alpha_logit=g.alpha_logit,
                feature=torch.rand(n, F, generator=torch.Generator().manual_seed(11)))
    cfg = RasterConfig(compute_visibility=True, compute_point_heuristic=True)
    gd = g.to(DEV).requires_grad_(True)
    r = gs.render_gaussians(gd, camera.to(device=DEV), cfg, use_sh=False, render_depth=True,
                            render_median_depth=True)
    assert tuple(r.image.shape) == (size[1], size[0], F)
    ocfg = orc.OracleConfig.of(cfg)
    p_np, d_np, idx = pu.to_np(r.gaussians2d), pu.to_np(r.point_depth), pu.to_np(r.points_in_view)
    o2p, ranges = orc.map_to_tiles(p_np, orc.ndc_depth(d_np, camera.near_plane, camera.far_plane), size, ocfg)
    feats = np.concatenate([d_np, d_np ** 2, g.feature.numpy()[idx]], 1).astype(np.float32)
    image_ref, alpha_ref, vis_ref = orc.rasterize_with_tiles(p_np, feats, o2p, ranges, size, ocfg)
    proof = pu.flip_proof(p_np, feats, o2p, ranges, size, ocfg)
    pu.assert_pixels_close(r.image, image_ref[..., 2:], "image", flips=proof.channels(slice(2, None)))
    pu.assert_pixels_close(r.image_weight, alpha_ref, "weight", flips=proof.weight())
    w = alpha_ref + np.float32(1e-6)
    pu.assert_pixels_close(r.depth, image_ref[..., 0] / w, "depth", atol=1e-3, rtol=1e-3, flips=proof.weight(),
                           bound=False)
    pu.assert_grad_close(r.point_visibility, vis_ref, "visibility", tol=1e-5)
    mcfg = orc.OracleConfig.of(dataclasses.replace(cfg, use_alpha_blending=False, saturate_threshold=0.5))
    med_ref, _, _ = orc.rasterize_with_tiles(p_np, d_np, o2p, ranges, size, mcfg)
    pu.assert_pixels_close(r.median_depth, med_ref[..., 0], "median depth", atol=1e-4, rtol=1e-4,
                           flips=proof.weight(), bound=False)
    gi = torch.rand(size[1], size[0], F, generator=torch.Generator().manual_seed(12))
    (r.image * dev(gi)).sum().backward()
    g_img = np.zeros_like(image_ref)
    g_img[..., 2:] = gi.numpy()
    hip_img = np.concatenate([image_ref[..., :2], pu.to_np(r.image)], -1).astype(np.float32)
    _, gf, heur_ref = orc.rasterize_backward(p_np, feats, o2p, ranges, size, hip_img, g_img, ocfg)
    dfeat = np.zeros((n, F), np.float32)
    dfeat[idx] = gf[:, 2:]
    pu.assert_grad_close(gd.feature.grad, dfeat, "d feature", tol=1e-3)
    pu.assert_grad_close(r.point_heuristic, heur_ref, "point_heuristic", tol=1e-3)
    assert bool(torch.isfinite(gd.position.grad).all()) and float(gd.position.grad.abs().sum()) > 0


def test_wider_than_supported_is_refused():
    g2d, depth, feat = pu.make_2d_scene(13, 20, (32, 32), channels=513)
    with pytest.raises(NotImplementedError):
        gs.rasterize(dev(g2d), dev(depth), dev(feat), (32, 32), RasterConfig())
