"""float64 projection, SH and rasterizer on the GPU (csrc/*_f64.hip): the reference's own f64 golden bar, gradcheck of
each operator, parity with the f64 oracle, the visibility identity and bit reproducibility."""
import dataclasses

import numpy as np
import pytest
import torch
from torch.autograd import gradcheck

import config_cases as cc
import parity_util as pu
import taichi_gaussian_rasterizer_amd as gs
from golden_util import projection_cases, sh_cases
from oracle import oracle as orc
from taichi_gaussian_rasterizer_amd import RasterConfig, scenes
from taichi_gaussian_rasterizer_amd.misc.renderer2d import project_gaussians2d
from taichi_gaussian_rasterizer_amd.perspective import projection as hip_proj

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
GRADCHECK = dict(eps=1e-6, check_grad_dtypes=True, check_undefined_grad=True)


def dev64(x):
    return torch.as_tensor(x).to(device=DEV, dtype=F64)


# ------------------------------------------------------------------------------------------ golden vectors
PROJ = [c for c in projection_cases() if c[1] == np.float64]
SHC = [c for c in sh_cases() if c[1] == np.float64]


@pytest.mark.parametrize("name,dt,ins,exp,meta", PROJ, ids=[c[0] for c in PROJ])
def test_projection_golden_f64(name, dt, ins, exp, meta):
    """the reference's f64 bar (torch.allclose defaults) on points, depth and all six gradients"""
    keys = ["position", "log_scaling", "rotation", "alpha_logit", "T_camera_world", "projection"]
    t = [dev64(ins[k]).requires_grad_(True) for k in keys]
    points, depth, idx = hip_proj.apply(*t, meta["image_size"], meta["depth_range"], blur_cov=meta["blur_cov"])
    assert points.dtype == F64 and depth.dtype == F64 and idx.dtype == torch.int64
    assert idx.shape == exp["indexes"].shape and (pu.to_np(idx) == exp["indexes"]).all(), "visible index mismatch"
    if idx.shape[0] == 0:
        return
    assert np.allclose(pu.to_np(points), exp["points"], rtol=1e-5, atol=1e-8)
    assert np.allclose(pu.to_np(depth), exp["depth"], rtol=1e-5, atol=1e-8)
    (points.mean() + depth.mean()).backward()
    for tensor, k in zip(t, keys):
        assert tensor.grad.dtype == F64
        assert np.allclose(pu.to_np(tensor.grad), exp[f"grad_{k}"], rtol=1e-5, atol=1e-8), f"grad {k}"


@pytest.mark.parametrize("name,dt,ins,indexes,exp", SHC, ids=[c[0] for c in SHC])
def test_sh_golden_f64(name, dt, ins, indexes, exp):
    params, points, cam = (dev64(ins[k]).requires_grad_(True) for k in ("params", "points", "camera_pos"))
    out = gs.evaluate_sh_at(params, points, torch.as_tensor(indexes).to(DEV), cam)
    assert out.dtype == F64
    assert np.allclose(pu.to_np(out), exp["out"], rtol=1e-5, atol=1e-8)
    out.mean().backward()
    for t, k in ((params, "grad_params"), (points, "grad_points"), (cam, "grad_camera_pos")):
        assert np.allclose(pu.to_np(t.grad), exp[k], rtol=1e-5, atol=1e-8), k


# ------------------------------------------------------------------------------------------------ gradcheck
def _split(g2d):
    """(mean, axis, sigma, alpha) leaves of a packed (N, 7) tensor"""
    return [g2d[:, a:b].detach().clone().requires_grad_(True) for a, b in ((0, 2), (2, 4), (4, 6), (6, 7))]


def _raster_fn(o2p, ranges, size, cfg):
    def fn(mean, axis, sigma, alpha, colours):
        return gs.rasterize_with_tiles(torch.cat((mean, axis, sigma, alpha), 1), colours, o2p, ranges, size,
                                       cfg).image
    return fn


@pytest.mark.parametrize("antialias", [False, True])
@pytest.mark.parametrize("seed", range(20))
def test_raster_gradcheck_reference_scene(seed, antialias):
    """the reference's scene (tests/test_rasterizer.py:30-90): 8x8 image, one tile, n < 50, C < 4, alpha in
    (0.2, 0.8), one list [[0, n]], identity overlap_to_point"""
    torch.manual_seed(seed)
    n = torch.randint(1, 50, (1,)).item()
    channels = torch.randint(1, 4, (1,)).item()
    size = (8, 8)
    g = scenes.random_2d_gaussians(n, size, num_channels=channels, scale_factor=1.0, alpha_range=(0.2, 0.8))
    g2d = project_gaussians2d(g).to(DEV, F64)
    colours = g.feature.to(DEV, F64).requires_grad_(True)
    cfg = RasterConfig(tile_size=8, pixel_stride=(1, 1), antialias=antialias)
    o2p = torch.arange(n, dtype=torch.int32, device=DEV)
    ranges = torch.tensor([[0, n]], dtype=torch.int32, device=DEV)
    assert gradcheck(_raster_fn(o2p, ranges, size, cfg), (*_split(g2d), colours), **GRADCHECK)


OTHER_SETTINGS = dict(tile_size=8, pixel_stride=(1, 1), alpha_threshold=1e-3, clamp_max_alpha=0.7, saturate_threshold=1.0)


def _reference_scene_at_other_settings(alpha_range):
    """test_raster_gradcheck_reference_scene's scene (seed 0) with the threshold, the clamp and the saturation level
    away from their defaults; also returns how far the clamp moves the image (against 0.99)"""
    torch.manual_seed(0)
    n = torch.randint(1, 50, (1,)).item()
    channels = torch.randint(1, 4, (1,)).item()
    size = (8, 8)
    g = scenes.random_2d_gaussians(n, size, num_channels=channels, scale_factor=1.0, alpha_range=alpha_range)
    g2d = project_gaussians2d(g).to(DEV, F64)
    colours = g.feature.to(DEV, F64).requires_grad_(True)
    cfg = RasterConfig(**OTHER_SETTINGS)
    o2p = torch.arange(n, dtype=torch.int32, device=DEV)
    ranges = torch.tensor([[0, n]], dtype=torch.int32, device=DEV)
    with torch.no_grad():
        free = gs.rasterize_with_tiles(g2d, colours, o2p, ranges, size, dataclasses.replace(cfg, clamp_max_alpha=0.99))
        held = gs.rasterize_with_tiles(g2d, colours, o2p, ranges, size, cfg)
        low = gs.rasterize_with_tiles(g2d, colours, o2p, ranges, size,
                                      dataclasses.replace(cfg, alpha_threshold=1.0 / 255.0))
    assert float((low.image - held.image).abs().max()) > 1e-4, "the threshold must decide some pixel"
    return g2d, colours, o2p, ranges, size, cfg, float((free.image - held.image).abs().max())


def test_raster_gradcheck_reference_scene_at_other_settings():
    """every input, opacities in (0.2, 0.65): below the clamp of 0.7 the backward is the derivative of the forward.
    At saturate_threshold = 1 the backward never stops a pixel, so the analytic gradient is that of the whole blend.
    The clamp never holds here (asserted), so this gradcheck constrains alpha_threshold and saturate_threshold only and
    would pass with the clamp fixed at 0.99; the clamp is covered by the next test and by
    test_raster_matches_f64_oracle[seed6] and [seed8]."""
    g2d, colours, o2p, ranges, size, cfg, clamp_effect = _reference_scene_at_other_settings((0.2, 0.65))
    assert clamp_effect == 0.0
    assert gradcheck(_raster_fn(o2p, ranges, size, cfg), (*_split(g2d), colours), **GRADCHECK)


def test_raster_gradcheck_colours_where_the_clamp_holds():
    """opacities in (0.2, 0.8) as in the reference's scene: one splat is held at 0.7 on the pixels at its centre.  There
    the reference's backward hands the splat's own geometry the gradient of the UNCLAMPED alpha (backward.py:166-169
    tests and differentiates the raw alpha, then clamps; the oracle and the kernels follow it), so the gradient is not
    the derivative of the forward for that splat's row and a gradcheck over the geometry cannot pass: the float64 oracle
    itself is 1.5e-2 off its own central differences in that one row, 3e-10 in every other and in every row at 0.99.
    Those rows are held to the oracle by test_raster_matches_f64_oracle[seed6] and [seed8]; what is exact through the
    clamp is the gradient of the colours, and it is checked here."""
    g2d, colours, o2p, ranges, size, cfg, clamp_effect = _reference_scene_at_other_settings((0.2, 0.8))
    assert clamp_effect > 1e-3, "the clamp must hold some pixel"
    mean, axis, sigma, alpha = (t.detach() for t in _split(g2d))
    fn = _raster_fn(o2p, ranges, size, cfg)
    assert gradcheck(lambda c: fn(mean, axis, sigma, alpha, c), (colours,), **GRADCHECK)


@pytest.mark.parametrize("seed,tile,size,n", [(0, 8, (37, 21), 14), (1, 16, (40, 23), 14), (2, 32, (45, 21), 12)])
def test_raster_gradcheck_across_tiles(seed, tile, size, n):
    """lists from the float32 mapper, held fixed; image sizes that are not tile multiples; splats in several lists so
    that the per-splat sum of (tile, entry) records runs; visibility and heuristics on"""
    torch.manual_seed(seed)
    g = scenes.random_2d_gaussians(n, size, num_channels=2, scale_factor=1.5, alpha_range=(0.2, 0.8))
    g2d = project_gaussians2d(g).to(DEV, F64)
    depth = g.z_depth.clamp(0, 1).to(DEV, torch.float32)
    cfg = RasterConfig(tile_size=tile, saturate_threshold=1.0, compute_visibility=True, compute_point_heuristic=True)
    o2p, ranges = gs.map_to_tiles(g2d.float(), depth, size, cfg)
    ranges = ranges.view(-1, 2)
    per_splat = torch.bincount(o2p.long(), minlength=n)
    assert int((per_splat >= 2).sum()) >= 2, "scene must put splats in several lists"
    colours = g.feature.to(DEV, F64).requires_grad_(True)
    assert gradcheck(_raster_fn(o2p, ranges, size, cfg), (*_split(g2d), colours), **GRADCHECK)


@pytest.mark.parametrize("seed", range(3))
def test_projection_gradcheck(seed):
    torch.manual_seed(seed)
    camera = scenes.random_camera()
    g = scenes.random_3d_gaussians(16, camera, scale_factor=0.5).to(dtype=F64)
    camera = camera.to(dtype=F64)
    inputs = [t.to(DEV).detach().requires_grad_(True) for t in (*g.shape_tensors(), camera.T_camera_world,
                                                                  camera.projection)]
    _, _, idx = hip_proj.apply(*inputs, camera.image_size, camera.depth_range)
    assert idx.shape[0] >= 8

    def fn(*t):
        points, depth, _ = hip_proj.apply(*t, camera.image_size, camera.depth_range)
        return points, depth
    assert gradcheck(fn, inputs, **GRADCHECK)


def clamp_and_cull_scene():
    """Six hand-placed Gaussians, image 40x24, for the branches the f32 and f64 adjoint share: camera at the origin
    looking down +z, fx = fy = 30, principal point (20, 12), so that u = 20 + 30 x / z and v = 12 + 30 y / z; the
    clamp bounds are x in [-6, 44.85], y in [-3.6, 26.45].  Rows: 0, 4, 5 ordinary; 1 a large splat with u = -10 (left
    of the bound by 4 px, still reaching the image); 3 a large splat with v = 35 (below the lower bound by 8.55 px);
    2 a small splat at u = 140, culled.  Returns (the six projection inputs in float64, image size, depth range)."""
    position = torch.tensor([[0.0, 0.0, 3.0], [-3.0, 0.2, 3.0], [8.0, 0.3, 2.0], [0.5, 2.3, 3.0], [0.4, -0.3, 2.5],
                             [-0.6, 0.5, 4.0]], dtype=F64)
    log_scaling = torch.tensor([[-1.6, -1.2, -2.0], [0.5, 0.2, 0.35], [-3.0, -3.2, -2.8], [0.1, 0.3, -0.2],
                                [-1.0, -2.0, -1.5], [-0.7, -1.4, -1.1]], dtype=F64)
    rotation = torch.tensor([[0.1, 0.2, 0.3, 0.9], [0.5, -0.3, 0.2, 0.7], [0.0, 0.0, 0.0, 1.0], [-0.4, 0.1, 0.6, 0.5],
                             [0.3, 0.3, -0.2, 1.1], [-0.2, 0.7, 0.1, 0.6]], dtype=F64)
    alpha_logit = torch.tensor([[0.5], [1.0], [0.0], [0.8], [-0.5], [1.5]], dtype=F64)
    T_camera_world = torch.eye(4, dtype=F64)
    projection = torch.tensor([30.0, 30.0, 20.0, 12.0], dtype=F64)
    return (position, log_scaling, rotation, alpha_logit, T_camera_world, projection), (40, 24), (0.1, 100.0)


def test_projection_gradcheck_clamp_and_cull():
    """gradcheck through the clamp's zero-gradient branch and past a culled row"""
    inputs, size, depth_range = clamp_and_cull_scene()
    margin = 0.15  # the default clamp_margin of apply()
    ref_points, _, ref_idx = orc.project(*(t.numpy() for t in inputs), size, depth_range)
    u, v = ref_points[:, 0], ref_points[:, 1]
    lo_x, hi_x, lo_y, hi_y = -size[0] * margin, (size[0] - 1) * (1 + margin), -size[1] * margin, \
        (size[1] - 1) * (1 + margin)
    assert (u < lo_x).any(), "scene must hold a visible Gaussian left of the clamp margin"
    culled = np.setdiff1d(np.arange(6), ref_idx)
    assert culled.size >= 1, "scene must hold a culled Gaussian"
    away = 1e-3 * size[0]  # the clamp is not differentiable at its bounds
    assert min(np.abs(u - lo_x).min(), np.abs(u - hi_x).min(), np.abs(v - lo_y).min(), np.abs(v - hi_y).min()) >= away
    leaves = [t.to(DEV).requires_grad_(True) for t in inputs]
    points, depth, idx = hip_proj.apply(*leaves, size, depth_range)
    assert (pu.to_np(idx) == ref_idx).all()
    (points.sum() + depth.sum()).backward()
    for t in leaves[:4]:
        assert float(t.grad[culled].abs().sum()) == 0.0 and float(t.grad.abs().sum()) > 0.0

    def fn(*t):
        points, depth, _ = hip_proj.apply(*t, size, depth_range)
        return points, depth
    assert gradcheck(fn, [t.detach().requires_grad_(True) for t in leaves], **GRADCHECK)


def test_projection_gradcheck_without_margin_and_with_a_wide_blur():
    """clamp_margin = 0: every mean outside the image takes the clamp's zero-gradient branch (rows 1 and 3 here);
    blur_cov = 1 dominates the covariance of the small splats"""
    inputs, size, depth_range = clamp_and_cull_scene()
    kw = dict(blur_cov=1.0, clamp_margin=0.0)
    ref_points, _, ref_idx = orc.project(*(t.numpy() for t in inputs), size, depth_range, **kw)
    u, v = ref_points[:, 0], ref_points[:, 1]
    outside = (u < 0) | (u > size[0] - 1) | (v < 0) | (v > size[1] - 1)
    assert int(outside.sum()) >= 2 and int((~outside).sum()) >= 3
    away = 1e-3 * size[0]
    assert min(np.abs(u).min(), np.abs(u - (size[0] - 1)).min(), np.abs(v).min(), np.abs(v - (size[1] - 1)).min()) >= away
    leaves = [t.to(DEV).requires_grad_(True) for t in inputs]
    points, depth, idx = hip_proj.apply(*leaves, size, depth_range, **kw)
    assert (pu.to_np(idx) == ref_idx).all()
    assert np.allclose(pu.to_np(points), ref_points, rtol=1e-9, atol=1e-12)
    default_points, _, _ = hip_proj.apply(*leaves, size, depth_range)
    assert float((points[:, 4:6] - default_points[:, 4:6]).abs().min()) > 1e-3, "every sigma must move"

    def fn(*t):
        points, depth, _ = hip_proj.apply(*t, size, depth_range, **kw)
        return points, depth
    assert gradcheck(fn, [t.detach().requires_grad_(True) for t in leaves], **GRADCHECK)


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_sh_gradcheck_repeated_indexes(degree):
    torch.manual_seed(degree)
    n, C = 6, 3
    params = (0.2 * torch.randn(n, C, (degree + 1) ** 2, dtype=F64)).to(DEV).requires_grad_(True)
    points = torch.randn(n, 3, dtype=F64).to(DEV).requires_grad_(True)
    cam = torch.randn(3, dtype=F64).to(DEV).requires_grad_(True)
    indexes = torch.tensor([0, 3, 3, 5, 1, 3, 0, 2], device=DEV)
    assert gradcheck(lambda p, x, c: gs.evaluate_sh_at(p, x, indexes, c), (params, points, cam), **GRADCHECK)


# ------------------------------------------------------------------------------------- parity with the oracle
def _scene(seed, n, size, channels=3, scale_factor=0.5, alpha_range=(0.2, 0.8)):
    torch.manual_seed(seed)
    g = scenes.random_2d_gaussians(n, size, num_channels=channels, scale_factor=scale_factor, alpha_range=alpha_range)
    return project_gaussians2d(g).to(DEV, F64), g.z_depth.clamp(0, 1).to(DEV, torch.float32), g.feature.to(DEV, F64)


PARITY = [
    dict(seed=0, n=2000, size=(160, 120), cfg=dict(tile_size=16)),
    dict(seed=1, n=800, size=(100, 72), channels=32, cfg=dict(tile_size=8)),
    dict(seed=2, n=1500, size=(150, 90), cfg=dict(tile_size=16, antialias=True)),
    dict(seed=3, n=1500, size=(130, 100), cfg=dict(tile_size=32, compute_visibility=True,
                                                   compute_point_heuristic=True)),
    dict(seed=4, n=1500, size=(120, 80), cfg=dict(tile_size=16, use_alpha_blending=False, saturate_threshold=0.5)),
    # thresholds, clamps and levels away from the defaults (config_cases.CONFIGS), opacities up to 1
    dict(seed=5, n=1200, size=(130, 75), alpha_range=(0.05, 1.0), cfg=dict(tile_size=16, **cc.CONFIGS["thr_small"])),
    dict(seed=6, n=1200, size=(101, 67), alpha_range=(0.05, 1.0), cfg=dict(tile_size=8, **cc.CONFIGS["clamp_half"])),
    dict(seed=7, n=1200, size=(130, 75), alpha_range=(0.05, 1.0), scale_factor=0.8,
         cfg=dict(tile_size=32, **cc.CONFIGS["sat_half"])),
    dict(seed=8, n=1200, size=(101, 67), alpha_range=(0.05, 1.0), scale_factor=0.8,
         cfg=dict(tile_size=16, compute_point_heuristic=True, **cc.CONFIGS["mixed"])),
    dict(seed=9, n=1200, size=(130, 75), alpha_range=(0.05, 1.0), cfg=dict(tile_size=16, **cc.CONFIGS["aa_mixed"])),
]


@pytest.mark.parametrize("case", PARITY, ids=[f"seed{c['seed']}" for c in PARITY])
def test_raster_matches_f64_oracle(case):
    """the bars the oracle meets against the dense f64 renderer (tests/test_oracle_raster.py:36-45)"""
    g2d, depth, feat = _scene(case["seed"], case["n"], case["size"], channels=case.get("channels", 3),
                              scale_factor=case.get("scale_factor", 0.5), alpha_range=case.get("alpha_range", (0.2, 0.8)))
    size = case["size"]
    cfg = RasterConfig(**case["cfg"])
    o2p, ranges = gs.map_to_tiles(g2d.float(), depth, size, cfg)
    ranges = ranges.view(-1, 2)
    gd, fd = g2d.clone().requires_grad_(True), feat.clone().requires_grad_(True)
    out = gs.rasterize_with_tiles(gd, fd, o2p, ranges, size, cfg)
    image, alpha, vis = orc.rasterize_with_tiles(pu.to_np(g2d), pu.to_np(feat), pu.to_np(o2p), pu.to_np(ranges), size,
                                                 cfg)
    assert out.image.dtype == F64 and out.image_weight.dtype == F64
    assert np.allclose(pu.to_np(out.image), image, rtol=1e-9, atol=1e-10)
    assert np.allclose(pu.to_np(out.image_weight), alpha, rtol=1e-9, atol=1e-10)
    if cfg.compute_visibility:
        assert np.allclose(pu.to_np(out.visibility), vis, rtol=1e-6, atol=1e-9)
    if not cfg.use_alpha_blending:
        return
    gi = torch.rand(out.image.shape, dtype=F64, generator=torch.Generator().manual_seed(case["seed"]))
    (out.image * gi.to(DEV)).sum().backward()
    gg, gf, heur = orc.rasterize_backward(pu.to_np(g2d), pu.to_np(feat), pu.to_np(o2p), pu.to_np(ranges), size, image,
                                          gi.numpy(), cfg)
    assert np.allclose(pu.to_np(gd.grad), gg, rtol=1e-6, atol=1e-9)
    assert np.allclose(pu.to_np(fd.grad), gf, rtol=1e-6, atol=1e-9)
    if cfg.compute_point_heuristic:
        assert np.allclose(pu.to_np(out.point_heuristic), heur, rtol=1e-6, atol=1e-9)


@pytest.mark.parametrize("seed", range(2))
def test_visibility_identity_f64(seed):
    """reference tests/test_visibility.py:34-64: visibility == d(sum image) / d feature[:, 0], through `rasterize`
    with float64 splats and float32 depth (tiles mapped from a float32 copy)"""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1000, 4000))
    size = (320, 200)
    torch.manual_seed(seed)
    g = scenes.random_2d_gaussians(n, size, scale_factor=0.2, alpha_range=(0.2, 1.0))
    g2d = project_gaussians2d(g).to(DEV, F64)
    depth = g.z_depth.clamp(0, 1).to(DEV, torch.float32)
    feat = g.feature.to(DEV, F64).requires_grad_(True)
    cfg = RasterConfig(compute_visibility=True, compute_point_heuristic=True)
    out = gs.rasterize(g2d, depth, feat, size, cfg)
    out.image.sum().backward()
    assert out.visibility.dtype == F64 and out.point_heuristic.shape == (n, 2)
    assert np.allclose(pu.to_np(feat.grad[:, 0]), pu.to_np(out.visibility), rtol=1e-5, atol=1e-4 * 3)
    assert bool((out.point_heuristic >= 0).all())


def test_results_are_bit_reproducible():
    """a crowded scene (many staging batches per tile): visibility and every gradient repeat bit for bit"""
    g2d, depth, feat = _scene(7, 5000, (320, 200), scale_factor=1.5)
    size = (320, 200)
    cfg = RasterConfig(compute_visibility=True, compute_point_heuristic=True)
    o2p, ranges = gs.map_to_tiles(g2d.float(), depth, size, cfg)
    ranges = ranges.view(-1, 2)
    assert int((ranges[:, 1] - ranges[:, 0]).max()) > 3 * 32
    gi = torch.rand((size[1], size[0], 3), dtype=F64, generator=torch.Generator().manual_seed(0)).to(DEV)
    runs = []
    for _ in range(2):
        gd, fd = g2d.clone().requires_grad_(True), feat.clone().requires_grad_(True)
        out = gs.rasterize_with_tiles(gd, fd, o2p, ranges, size, cfg)
        (out.image * gi).sum().backward()
        runs.append((out.image, out.visibility, gd.grad, fd.grad, out.point_heuristic))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    # SH with repeated indexes: every entry of a Gaussian is summed in list order
    params = 0.2 * torch.randn(300, 3, 16, dtype=F64, device=DEV)
    points = torch.randn(300, 3, dtype=F64, device=DEV)
    idx = torch.randint(0, 300, (5000,), device=DEV)
    cam = torch.tensor([0.1, 0.2, -3.0], dtype=F64, device=DEV)
    runs = []
    for _ in range(2):
        leaves = [t.clone().requires_grad_(True) for t in (params, points, cam)]
        (gs.evaluate_sh_at(leaves[0], leaves[1], idx, leaves[2]) * gi.view(-1)[:15000].view(5000, 3)).sum().backward()
        runs.append([t.grad for t in leaves])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------- refusals
def test_f64_refusals_and_empty_inputs():
    cfg = RasterConfig()
    size = (40, 30)
    ranges = torch.zeros((6, 2), dtype=torch.int32, device=DEV)
    o2p = torch.zeros((0,), dtype=torch.int32, device=DEV)
    with pytest.raises(TypeError, match="float32"):
        gs.rasterize_with_tiles(torch.rand(4, 7, device=DEV, dtype=F64), torch.rand(4, 3, device=DEV), o2p,
                                ranges, size, cfg)
    with pytest.raises(TypeError, match="float64"):
        gs.evaluate_sh_at(torch.rand(4, 3, 4, device=DEV, dtype=F64), torch.rand(4, 3, device=DEV, dtype=F64),
                          torch.arange(4, device=DEV), torch.zeros(3, device=DEV))
    camera = scenes.random_camera()
    g = scenes.random_3d_gaussians(10, camera).to(dtype=F64)
    with pytest.raises(TypeError, match="float64"):
        hip_proj.apply(*(t.to(DEV) for t in g.shape_tensors()), camera.T_camera_world.to(DEV),
                       camera.projection.to(DEV, F64), camera.image_size, camera.depth_range)
    with pytest.raises(NotImplementedError, match="32"):
        gs.rasterize_with_tiles(torch.rand(4, 7, device=DEV, dtype=F64), torch.rand(4, 33, device=DEV, dtype=F64),
                                o2p, ranges, size, cfg)
    with pytest.raises(RuntimeError, match="HIP device"):
        gs.rasterize_with_tiles(torch.rand(4, 7, dtype=F64), torch.rand(4, 3, dtype=F64), o2p.cpu(), ranges.cpu(),
                                size, cfg)
    g2d, depth, feat = _scene(0, 200, (64, 48))
    qcfg = RasterConfig(use_alpha_blending=False)
    o2p2, ranges2 = gs.map_to_tiles(g2d.float(), depth, (64, 48), qcfg)
    out = gs.rasterize_with_tiles(g2d, feat.requires_grad_(True), o2p2, ranges2.view(-1, 2), (64, 48), qcfg)
    with pytest.raises(NotImplementedError):
        out.image.sum().backward()
    empty = gs.rasterize_with_tiles(torch.zeros((0, 7), device=DEV, dtype=F64), torch.zeros((0, 3), device=DEV,
                                                                                             dtype=F64),
                                    o2p, ranges, size, RasterConfig(compute_visibility=True))
    assert empty.image.shape == (30, 40, 3) and empty.image.dtype == F64 and float(empty.image.abs().sum()) == 0.0
    assert float(empty.image_weight.abs().sum()) == 0.0 and empty.visibility.shape == (0,)
