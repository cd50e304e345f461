"""The HIP kernels against the oracle with alpha_threshold, clamp_max_alpha, saturate_threshold, clamp_margin and
blur_cov away from their defaults, and the fused frame at tile sizes 8 and 32 (config_cases.py holds the settings and
the scenes, test_config_sweep_cpu.py the conditions on them).  The bodies are those of the default-setting tests in
test_gpu_parity.py, test_wide_features_gpu.py, test_sparse_grad_gpu.py and test_background_gpu.py, at their tolerances;
the flip bar alone is scaled to the threshold (config_cases.flip_bar)."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

import config_cases as cc
import parity_util as pu
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

import taichi_gaussian_rasterizer_amd as gs  # noqa: E402
from taichi_gaussian_rasterizer_amd import RasterConfig, _native as nv  # noqa: E402
from taichi_gaussian_rasterizer_amd.perspective import projection as hip_proj  # noqa: E402

DEV = "cuda:0"
SIZE = cc.SIZE_2D


def dev(x):
    t = torch.as_tensor(np.ascontiguousarray(x)) if not isinstance(x, torch.Tensor) else x
    return t.to(DEV).contiguous()


# ------------------------------------------------------------------------------------------------ rasterizer
def check_raster(cfg, channels=3, lists_cfg=None):
    """test_gpu_parity.test_raster_forward_backward on the 2D scene: image and weight against the f32 oracle with a
    flip proof, both gradients against the f32 oracle fed the HIP image with the f64 oracle as yardstick; with the
    heuristics on, visibility and point_heuristic too.  Returns (output, gradient of the splats)."""
    g2d, _, feat = cc.scene_2d(channels)
    ref = cc.oracle_2d(cfg, channels, lists_cfg)
    o2p, ranges, ocfg, proof = ref["o2p"], ref["ranges"], ref["ocfg"], ref["proof"]
    g_t, f_t = dev(g2d).requires_grad_(True), dev(feat).requires_grad_(True)
    out = gs.rasterize_with_tiles(g_t, f_t, dev(o2p), dev(ranges.reshape(-1, 2)), SIZE, cfg)
    assert tuple(out.image.shape) == (SIZE[1], SIZE[0], channels)
    gi = cc.grad_image_2d(channels)
    (out.image * dev(gi)).sum().backward()
    gg, gf, heur_ref = orc.rasterize_backward(g2d, feat, o2p, ranges, SIZE, pu.to_np(out.image), gi, ocfg)
    _, gg64, gf64 = cc.truth_2d(cfg, channels, lists_cfg)
    print(f"image err {np.abs(pu.to_np(out.image) - ref['image']).max():.2e}; grad_gaussians2d vs f32 "
          f"{np.abs(pu.to_np(g_t.grad) - gg).max() / np.abs(gg64).max():.2e} vs f64 "
          f"{np.abs(pu.to_np(g_t.grad) - gg64).max() / np.abs(gg64).max():.2e} (oracle "
          f"{np.abs(gg - gg64).max() / np.abs(gg64).max():.2e}); grad_features vs f32 "
          f"{np.abs(pu.to_np(f_t.grad) - gf).max() / np.abs(gf64).max():.2e}")
    rep = pu.assert_pixels_close(out.image, ref["image"], "image", flips=proof)
    if rep["outlier_pixels"]:
        print(f"flip outliers: {rep}")
    pu.assert_pixels_close(out.image_weight, ref["weight"], "alpha", flips=proof.weight())
    pu.assert_grad_close_vs_truth(g_t.grad, gg, gg64, "grad_gaussians2d")
    pu.assert_grad_close_vs_truth(f_t.grad, gf, gf64, "grad_features")
    if cfg.compute_point_heuristic:
        pu.assert_grad_close(out.point_heuristic, heur_ref, "point_heuristic", tol=1e-3)
        pu.assert_grad_close(out.visibility, ref["visibility"], "visibility", tol=1e-5)
    return out, g_t.grad


def heuristics(on):
    return dict(compute_point_heuristic=True, compute_visibility=True) if on else {}


# sat_one also with forward_cut = 0: the backward then walks past nothing the forward left out
SWEEP = [(cid, {}) for cid in cc.CONFIGS] + [("sat_one", dict(forward_cut=0.0))]
SWEEP_IDS = [cid + ("-cut0" if extra else "") for cid, extra in SWEEP]


@pytest.mark.parametrize("heur", [False, True], ids=["lean", "heur"])
@pytest.mark.parametrize("tile", cc.TILES)
@pytest.mark.parametrize("cid,extra", SWEEP, ids=SWEEP_IDS)
def test_raster_sweep(cid, extra, tile, heur):
    """gs_raster_fwd / gs_raster_bwd: lean (modes 0), with statistics (1) and general (2, aa_mixed)"""
    cfg = cc.raster_config(cid, tile, **extra, **heuristics(heur))
    out, grad = check_raster(cfg)
    if cid == "clamp_below_thr":
        # the forward tests the CLAMPED alpha against the threshold, the backward the raw one (the reference's asymmetry)
        assert float(out.image.abs().max()) == 0.0 and float(out.image_weight.abs().max()) == 0.0
        assert float(grad.abs().max()) > 0.0


@pytest.mark.parametrize("tile", [8, 16])
@pytest.mark.parametrize("cid,extra", SWEEP, ids=SWEEP_IDS)
def test_wide_raster_sweep(cid, extra, tile):
    """gs_raster_fwd_wide / gs_raster_bwd_wide at 40 channels, statistics on"""
    cfg = cc.raster_config(cid, tile, **extra, **heuristics(True))
    out, grad = check_raster(cfg, channels=40)
    if cid == "clamp_below_thr":
        assert float(out.image.abs().max()) == 0.0 and float(out.image_weight.abs().max()) == 0.0
        assert float(grad.abs().max()) > 0.0


@pytest.mark.parametrize("nb", [1, 2, 4])
@pytest.mark.parametrize("cid", ["mixed", "aa_mixed", "sat_half"])
def test_raster_wave_region_variants_sweep(cid, nb, monkeypatch):
    """16x16, 16x8 and 8x8 wave regions forced (test_gpu_parity.test_raster_wave_region_variants): the backward stops
    per sub-block on the saturation level, the sub-block cull takes its radius from the threshold"""
    monkeypatch.setitem(nv.TUNING, "wave_sub_blocks", int(nb))
    check_raster(cc.raster_config(cid, 16, **heuristics(nb == 2)))


@pytest.mark.parametrize("channels", [3, 40], ids=["narrow", "wide"])
@pytest.mark.parametrize("heur", [False, True], ids=["lean", "heur"])
def test_raster_lists_built_for_a_lower_threshold(heur, channels):
    """lists from the mapper at 1/255, rasterized at 0.3: most listed splats have an opacity below the threshold, so the
    staging's `opacity > thr` shortcut around the sub-block mask is not taken and the mask's radius log2(opacity / thr)
    has no real value"""
    lists_cfg = RasterConfig(tile_size=16)
    cfg = cc.raster_config("thr_big", 16, **heuristics(heur))
    g2d, _, _ = cc.scene_2d(channels)
    listed = np.unique(cc.oracle_2d(cfg, channels, lists_cfg)["o2p"])
    assert int((g2d[listed, 6] <= cfg.alpha_threshold).sum()) >= 100
    _, grad = check_raster(cfg, channels, lists_cfg)
    below = dev(g2d[:, 6] <= cfg.alpha_threshold)
    assert float(grad[below].abs().max()) == 0.0


@pytest.mark.parametrize("antialias", [False, True], ids=["plain", "antialias"])
@pytest.mark.parametrize("cmax", [0.5, 0.99])
@pytest.mark.parametrize("thr", [1e-3, 1.0 / 255.0])
@pytest.mark.parametrize("level", [0.25, 0.5, 0.9])
def test_quantile_pass_sweep(level, thr, cmax, antialias):
    """use_alpha_blending = False: the pixel takes the features of the splat at which the weight crosses the level
    (test_gpu_parity.test_quantile_mode_median_depth)"""
    g2d, depth, _ = cc.scene_2d()
    cfg = RasterConfig(use_alpha_blending=False, saturate_threshold=level, alpha_threshold=thr, clamp_max_alpha=cmax,
                       **(dict(antialias=True, blur_cov=0.0) if antialias else {}))
    ocfg = orc.OracleConfig.of(cfg)
    o2p, ranges = orc.map_to_tiles(g2d, depth, SIZE, ocfg)
    image_ref, alpha_ref, _ = orc.rasterize_with_tiles(g2d, depth, o2p, ranges, SIZE, ocfg)
    other, _, _ = orc.rasterize_with_tiles(g2d, depth, o2p, ranges, SIZE,
                                           dataclasses.replace(ocfg, saturate_threshold=0.5 if level != 0.5 else 0.6))
    assert float((other != image_ref).mean()) > 0.05, "the level must decide which splat a pixel takes"
    out = gs.rasterize_with_tiles(dev(g2d), dev(depth), dev(o2p), dev(ranges.reshape(-1, 2)), SIZE, cfg)
    # a flipped alpha decision moves the crossing to another splat: the pixel then takes that splat's depth
    proof = pu.flip_proof(g2d, depth, o2p, ranges, SIZE, ocfg, bar=cc.raster_bar(cfg, g2d))
    pu.assert_pixels_close(out.image, image_ref, "quantile", flips=proof, bound=False)
    assert (pu.to_np(out.image_weight) == alpha_ref).mean() > 0.999


# ------------------------------------------------------------------------------------------------ projection
PROJ_KEYS = ("position", "log_scaling", "rotation", "alpha_logit", "T", "proj")


def hip_project(kw, upstream=None):
    """project_with_ndc on the projection scene; with upstream (gp (400, 7), gd (400,)) rows also the six gradients"""
    cfg = RasterConfig(**kw)
    t = [dev(a).requires_grad_(upstream is not None) for a in cc.projection_scene()]
    p, d, i, ndc = hip_proj.project_with_ndc(*t, cc.PROJ_SIZE, cc.PROJ_DEPTH_RANGE, cfg)
    if upstream is not None:
        gp, gd = upstream
        idx = pu.to_np(i)
        ((p * dev(gp[idx])).sum() + (d.reshape(-1) * dev(gd[idx])).sum()).backward()
    return p, d, i, [x.grad for x in t]


def proj_upstream():
    rng = np.random.default_rng(1)
    return rng.random((400, 7)).astype(np.float32), rng.random(400).astype(np.float32)


@pytest.mark.parametrize("pid", list(cc.PROJ_CASES))
def test_projection_sweep(pid):
    """gs_project_fwd / gs_project_bwd: the cull's extent sqrt(2 ln(alpha / thr)), the blur on the covariance and the
    clamp of the mean in the affine Jacobian, forward and adjoint (test_gpu_parity.test_projection_vs_oracle)"""
    kw = cc.PROJ_CASES[pid]
    args = [a.numpy() for a in cc.projection_scene()]
    p_ref, d_ref, i_ref = orc.project(*args, cc.PROJ_SIZE, cc.PROJ_DEPTH_RANGE, **kw)
    gp, gd = proj_upstream()
    p, d, i, grads = hip_project(kw, (gp, gd))
    assert i.shape[0] == i_ref.shape[0] and (pu.to_np(i) == i_ref).all(), "visible sets differ"
    pu.assert_grad_close(pu.cov_form(p), pu.cov_form(p_ref), "points (cov form)", tol=1e-3)
    assert np.allclose(pu.to_np(d), d_ref, rtol=1e-5)
    bkw = dict(blur_cov=kw["blur_cov"], clamp_margin=kw["clamp_margin"])
    truth = orc.project_backward(*(a.astype(np.float64) for a in args), cc.PROJ_SIZE, i_ref,
                                 gp[i_ref].astype(np.float64), gd[i_ref].astype(np.float64), **bkw)
    cpu32 = orc.project_backward(*args, cc.PROJ_SIZE, i_ref, gp[i_ref], gd[i_ref], **bkw)
    for grad, tr, c32, k in zip(grads, truth, cpu32, PROJ_KEYS):
        s = max(float(np.abs(tr).max()), 1e-30)
        cpu_err = float(np.abs(c32 - tr).max()) / s
        hip_err = float(np.abs(pu.to_np(grad) - tr).max()) / s
        print(f"{pid} d_{k}: HIP {hip_err:.2e}, CPU f32 {cpu_err:.2e}")
        assert hip_err <= 4 * cpu_err + 2e-4, f"d_{k}: HIP f32 error {hip_err:.2e} vs CPU f32 error {cpu_err:.2e}"


def test_projection_clamp_shows_in_the_position_gradient():
    """the means between the margins are clamped at 0.0 and free at 1.0: their d_position rows must differ, as in the
    oracle (test_config_sweep_cpu.py) -- a margin the kernel does not read would give the same rows twice"""
    rows = {}
    for m in (0.0, 1.0):
        _, _, i, grads = hip_project(dict(cc.PROJ_DEFAULT, clamp_margin=m), proj_upstream())
        rows[m] = (pu.to_np(i), pu.to_np(grads[0]))
    both = np.intersect1d(rows[0.0][0], rows[1.0][0])
    differ = int((np.abs(rows[0.0][1][both] - rows[1.0][1][both]).max(1) > 0).sum())
    assert differ >= 40


def test_project_bwd_rows_matches_dense_rows_at_other_settings():
    """gs_project_bwd_rows (row-compact) against gs_project_bwd, bit for bit, with the margin, the blur and the threshold
    away from their defaults (test_sparse_grad_gpu.test_project_bwd_rows_matches_dense_rows)"""
    cfg = RasterConfig(**cc.PROJ_COMBINED)
    t = [dev(a) for a in cc.projection_scene()]
    N, size, ROW = 400, cc.PROJ_SIZE, 16
    with torch.no_grad():
        _, _, indexes, _ = hip_proj.project_with_ndc(*t, size, cc.PROJ_DEPTH_RANGE, cfg)
    indexes = indexes.contiguous()
    V = int(indexes.shape[0])
    assert 0 < V < N
    slot_of = torch.full((N,), -1, dtype=torch.int32, device=DEV)
    slot_of[indexes] = torch.arange(V, dtype=torch.int32, device=DEV)
    rows = torch.randn(V, ROW, generator=torch.Generator().manual_seed(5)).to(DEV)
    lib, c = nv.lib(), nv.make_config(cfg)
    shape_tensors, T, proj = t[:4], t[4].contiguous(), t[5].contiguous()

    def off(x, floats):
        return ctypes.c_void_p(x.data_ptr() + 4 * floats)

    tails = ((3,), (3,), (4,), (1,))
    dense = [torch.full((N, *s), 7.0, device=DEV) for s in tails]
    compact = [torch.full((V, *s), 7.0, device=DEV) for s in tails]
    nv.check(lib.gs_project_bwd(N, V, *map(nv.ptr, shape_tensors), nv.ptr(T), nv.ptr(proj), size[0], size[1], c,
                                nv.ptr(slot_of), nv.ptr(rows), ROW, off(rows, 7), off(rows, 8), ROW,
                                *map(nv.ptr, dense), None, None, None, 0, nv.stream()), "gs_project_bwd")
    nv.check(lib.gs_project_bwd_rows(N, V, *map(nv.ptr, shape_tensors), nv.ptr(T), nv.ptr(proj), size[0], size[1], c,
                                     nv.ptr(indexes), nv.ptr(rows), ROW, off(rows, 7), off(rows, 8), ROW,
                                     *map(nv.ptr, compact), None, None, None, 0, nv.stream()), "gs_project_bwd_rows")
    torch.cuda.synchronize()
    culled = slot_of < 0
    for name, d, r in zip(PROJ_KEYS, dense, compact):
        assert torch.equal(r, d[indexes]), f"{name}: compact rows differ from the dense kernel's"
        assert float(d[culled].abs().max()) == 0.0 and float(r.abs().max()) > 0.0
    # and the dense rows are the oracle's at these settings (the default margin would free rows the clamp holds)
    args = [a.numpy() for a in cc.projection_scene()]
    args64 = [a.astype(np.float64) for a in args]
    r_np = pu.to_np(rows)
    _, d_ref, i_ref = orc.project(*args, size, cc.PROJ_DEPTH_RANGE, **cc.PROJ_COMBINED)
    assert (pu.to_np(indexes) == i_ref).all()
    gd = r_np[:, 7] + 2.0 * d_ref[:, 0] * r_np[:, 8]   # the frame's z and z^2 columns
    bkw = dict(blur_cov=cfg.blur_cov, clamp_margin=cfg.clamp_margin)
    truth = orc.project_backward(*args64, size, i_ref, r_np[:, :7].astype(np.float64), gd.astype(np.float64), **bkw)
    cpu32 = orc.project_backward(*args, size, i_ref, np.ascontiguousarray(r_np[:, :7]), gd, **bkw)
    for name, d, tr, c32 in zip(PROJ_KEYS, dense, truth, cpu32):
        s = max(float(np.abs(tr).max()), 1e-30)
        cpu_err = float(np.abs(c32 - tr).max()) / s
        hip_err = float(np.abs(pu.to_np(d).reshape(tr.shape) - tr).max()) / s
        assert hip_err <= 4 * cpu_err + 2e-4, f"d_{name}: HIP f32 error {hip_err:.2e} vs CPU f32 error {cpu_err:.2e}"


# ------------------------------------------------------------------------------------------------ fused frame
PARAMS = ("position", "log_scaling", "rotation", "alpha_logit", "feature")


def frame_upstream():
    s = cc.FRAME_SCENE
    return torch.rand(s["size"][1], s["size"][0], 3, generator=torch.Generator().manual_seed(s["seed"] + 7))


_E2E_REF = {}


def e2e_reference(fid, render_depth):
    """the f32 and f64 oracle pipelines of a frame, computed once for both frame paths"""
    key = (fid, render_depth)
    if key not in _E2E_REF:
        g, camera = cc.frame_scene()
        cfg = cc.frame_config(fid)
        gi = frame_upstream()
        ref = pu.oracle_render(g, camera, cfg, use_sh=True, render_depth=render_depth, grads=dict(image=gi.numpy()))
        ref64 = pu.oracle_render(g, camera, cfg, use_sh=True, render_depth=render_depth,
                                 grads=dict(image=gi.numpy().astype(np.float64)), dtype=np.float64, flips=False)
        _E2E_REF[key] = (ref, ref64)
    return _E2E_REF[key]


@pytest.mark.parametrize("render_depth", [False, True], ids=["colour", "depth"])
@pytest.mark.parametrize("fid", list(cc.FRAMES))
def test_frame_end_to_end_sweep(fid, render_depth, frame_path):
    """test_gpu_parity.test_render_gaussians_end_to_end_vs_oracle: gs_frame_fwd / gs_frame_bwd (and the staged path) at
    tile sizes 8, 16 and 32 with every scalar away from its default, against the whole oracle pipeline"""
    g, camera = cc.frame_scene()
    n = cc.FRAME_SCENE["n"]
    cfg = cc.frame_config(fid)
    gi = frame_upstream()
    ref, ref64 = e2e_reference(fid, render_depth)
    assert (ref["indexes"] == ref64["indexes"]).all()
    gd = g.to(DEV).requires_grad_(True)
    r = gs.render_gaussians(gd, camera.to(device=DEV), cfg, use_sh=True, render_depth=render_depth)
    assert (pu.to_np(r.points_in_view) == ref["indexes"]).all()
    flips = cc.frame_flip_proof(fid, ref, ref64, cfg)
    rep = pu.assert_pixels_close(r.image, ref["image"], "image", atol=1e-3, rtol=1e-3, flips=flips)
    print(f"{fid} image: {rep}")
    rep_w = pu.assert_pixels_close(r.image_weight, ref["alpha"], "image_weight", atol=1e-3, rtol=1e-3,
                                   flips=flips.weight())
    # the escape is for a handful of pixels (the oracles themselves part at one, in frame_b), never for a region
    assert rep["outlier_pixels"] <= cc.MAX_E2E_OUTLIERS and rep_w["outlier_pixels"] <= cc.MAX_E2E_OUTLIERS
    (r.image * dev(gi)).sum().backward()
    relgap = np.full(n, np.inf)
    relgap[ref["indexes"]] = pu.relative_eigen_gap(ref["points"])
    for name in PARAMS:
        rep = pu.assert_rows_close_e2e(getattr(gd, name).grad, ref[f"d_{name}"], ref64[f"d_{name}"], relgap,
                                       f"grad {name}")
        print(f"{fid} {name}: {rep}")


def test_frame_plain_features_background_and_weight_gradient():
    """use_sh=False with six channels, a background and differentiable_weight under frame_b's settings: the frame's
    in-kernel background and weight gradient against rasterize_with_tiles on the oracle's lists with a ones channel
    appended (the seventh channel IS the weight), as test_background_gpu.test_fused_weight_gradient_against_a_ones_channel"""
    g, camera = cc.frame_scene()
    n, size = cc.FRAME_SCENE["n"], cc.FRAME_SCENE["size"]
    cfg = cc.frame_config("frame_b")
    gen = torch.Generator().manual_seed(8)
    g = g.replace(feature=torch.rand(n, 6, generator=gen))
    G = dev(torch.rand(size[1], size[0], 6, generator=gen))
    GW = dev(torch.rand(size[1], size[0], generator=gen) * 2 - 1)
    bg = dev(torch.rand(6, generator=gen))
    a = g.to(DEV).requires_grad_(True)
    bg_t = bg.clone().requires_grad_(True)
    r = gs.render_gaussians(a, camera.to(device=DEV), cfg, use_sh=False, background=bg_t, differentiable_weight=True)
    r.gaussians2d.retain_grad()
    ((r.image * G).sum() + (r.image_weight * GW).sum()).backward()
    # the reference: the rasterizer alone on the frame's splats, lists from the oracle's mapper
    p_np, d_np, idx = pu.to_np(r.gaussians2d), pu.to_np(r.point_depth), pu.to_np(r.points_in_view)
    ocfg = orc.OracleConfig.of(cfg)
    o2p, ranges = orc.map_to_tiles(p_np, orc.ndc_depth(d_np, camera.near_plane, camera.far_plane), size, ocfg)
    g_ref = dev(p_np).requires_grad_(True)
    f_ref = torch.cat((dev(g.feature)[dev(idx)], torch.ones(idx.shape[0], 1, device=DEV)), 1).requires_grad_(True)
    out = gs.rasterize_with_tiles(g_ref, f_ref, dev(o2p), dev(ranges.reshape(-1, 2)), size, cfg)
    T = 1 - out.image_weight.detach()
    assert torch.equal(r.image_weight, out.image_weight)
    assert torch.allclose(r.image_weight, out.image[..., 6].detach(), rtol=0, atol=pu.ATOL)
    assert torch.allclose(r.image.detach(), out.image[..., :6].detach() + T.unsqueeze(-1) * bg, rtol=0, atol=pu.ATOL)
    # d/dalpha of T bg . G is the weight gradient -(bg . G)
    ((out.image[..., :6] * G).sum() + (out.image[..., 6] * (GW - (G * bg).sum(-1))).sum()).backward()
    pu.assert_grad_close(r.gaussians2d.grad, g_ref.grad, "grad gaussians2d", tol=pu.GRAD_TOL)
    pu.assert_grad_close(a.feature.grad[dev(idx)], f_ref.grad[:, :6], "grad feature", tol=pu.GRAD_TOL)
    pu.assert_grad_close(bg_t.grad, (G * T.unsqueeze(-1)).sum((0, 1)), "grad background", tol=pu.GRAD_TOL)
    outside = torch.ones(n, dtype=torch.bool, device=DEV)
    outside[dev(idx)] = False
    assert float(a.feature.grad[outside].abs().sum()) == 0.0


def test_frame_median_depth_takes_every_other_field(frame_path):
    """render_median_depth under frame_a: the second, non-blending pass runs at saturate_threshold = 0.5 with the
    frame's own tile size, threshold and clamp (test_gpu_parity.test_render_gaussians_plain_features_median_depth_...)"""
    g, camera = cc.frame_scene()
    size = cc.FRAME_SCENE["size"]
    cfg = cc.frame_config("frame_a")
    r = gs.render_gaussians(g.to(DEV), camera.to(device=DEV), cfg, use_sh=True, render_depth=True,
                            render_median_depth=True)
    p_np, d_np = pu.to_np(r.gaussians2d), pu.to_np(r.point_depth)
    ocfg = orc.OracleConfig.of(cfg)
    o2p, ranges = orc.map_to_tiles(p_np, orc.ndc_depth(d_np, camera.near_plane, camera.far_plane), size, ocfg)
    mcfg = orc.OracleConfig.of(dataclasses.replace(cfg, use_alpha_blending=False, saturate_threshold=0.5))
    med_ref, _, _ = orc.rasterize_with_tiles(p_np, d_np, o2p, ranges, size, mcfg)
    # (the clamp of 0.8 moves no median of this scene, whose opacities end at 0.9: test_quantile_pass_sweep has it)
    other, _, _ = orc.rasterize_with_tiles(p_np, d_np, o2p, ranges, size,
                                           dataclasses.replace(mcfg, alpha_threshold=1.0 / 255.0))
    assert float((other != med_ref).mean()) > 0.01, "the threshold must decide the median of some pixels"
    proof = pu.flip_proof(p_np, d_np, o2p, ranges, size, ocfg, bar=cc.raster_bar(cfg, p_np))
    assert r.median_depth.shape == (size[1], size[0])
    pu.assert_pixels_close(r.median_depth, med_ref[..., 0], "median depth", atol=1e-4, rtol=1e-4, flips=proof.weight(),
                           bound=False)
