"""The conditions test_config_sweep_gpu.py rests on, checked with the oracle alone (no GPU): every setting of
config_cases.CONFIGS changes what the oracle computes by far more than the tolerances, the float32 oracle is itself
inside those tolerances against the float64 one, and so few pixels sit at the alpha threshold that the flip escape of
assert_pixels_close cannot hide a wrong kernel.  Run with -s to see the figures per setting."""
import dataclasses

import numpy as np
import pytest

import config_cases as cc
import parity_util as pu
from oracle import oracle as orc

MAX_FLIP_FRACTION = 0.002  # of the pixels: a condition on the inputs (change the seed, not the cap)


def normwise(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(float(np.abs(b).max()), 1e-20))


def oracle_grads(cfg):
    g2d, _, feat = cc.scene_2d()
    ref = cc.oracle_2d(cfg)
    gg, gf, _ = orc.rasterize_backward(g2d, feat, ref["o2p"], ref["ranges"], cc.SIZE_2D, ref["image"],
                                       cc.grad_image_2d(), ref["ocfg"])
    return gg, gf


def test_scene_is_the_stated_one():
    g2d, depth, feat = cc.scene_2d()
    assert g2d.shape == (600, 7) and depth.shape == (600, 1) and feat.shape == (600, 3)
    assert 0.05 < g2d[:, 6].min() < 0.06 and 0.999 < g2d[:, 6].max() < 1.0
    assert all(cc.SIZE_2D[0] % t and cc.SIZE_2D[1] % t for t in cc.TILES)


@pytest.mark.parametrize("tile", cc.TILES)
@pytest.mark.parametrize("cid", list(cc.CONFIGS))
def test_setting_matters_and_oracle_is_inside_the_tolerances(cid, tile):
    cfg = cc.raster_config(cid, tile)
    g2d, _, feat = cc.scene_2d()
    ref = cc.oracle_2d(cfg)
    gg, gf = oracle_grads(cfg)
    figures = [f"{cid} tile {tile}: K = {ref['o2p'].shape[0]}"]

    # 1. the setting does something
    if cid in cc.SAT_IDS:
        # (sat_one is not here: no pixel of the scene reaches a weight of 0.9999, so the oracle computes the same at
        # 1.0 -- what it probes is the kernels' own `Tr > 1 - saturate_threshold` with a right-hand side of zero)
        base, _ = oracle_grads(dataclasses.replace(cfg, saturate_threshold=0.9999))
        moved = normwise(gg, base)
        above = float((ref["weight"] >= cfg.saturate_threshold).mean())
        figures.append(f"gradient moves by {moved:.3e} against 0.9999; {above:.1%} of pixels at or above the level")
        assert moved > 100 * pu.GRAD_TOL
    if "clamp_max_alpha" in cc.CONFIGS[cid]:
        base = cc.oracle_2d(dataclasses.replace(cfg, clamp_max_alpha=0.99))
        moved = float(np.abs(ref["image"] - base["image"]).max())
        figures.append(f"image moves by {moved:.3e} against clamp 0.99")
        if cid == "clamp_high":
            # 0.999 against 0.99 cannot move a pixel by 1000 x ATOL = 0.02: alpha changes by at most 0.009 and the
            # features are in [0, 1].  What the setting is for is the backward's 1 / (1 - alpha), on the few pixels where
            # an opacity above 0.99 meets a splat's centre: an order of magnitude over the tolerances either way
            base_gg, _ = oracle_grads(dataclasses.replace(cfg, clamp_max_alpha=0.99))
            moved_gg = normwise(gg, base_gg)
            figures.append(f"gradient moves by {moved_gg:.3e}")
            assert moved > 10 * pu.ATOL and moved_gg > 5 * pu.GRAD_TOL
        else:
            assert moved > 1000 * pu.ATOL
    if cid in cc.THR_IDS:
        base = cc.oracle_2d(dataclasses.replace(cfg, alpha_threshold=1.0 / 255.0))
        figures.append(f"K = {base['o2p'].shape[0]} at 1/255")
        assert ref["o2p"].shape[0] != base["o2p"].shape[0]
    if cid == "clamp_below_thr":
        assert float(np.abs(ref["image"]).max()) == 0.0 and float(np.abs(ref["weight"]).max()) == 0.0
        assert float(np.abs(gg).max()) > 0.0
    if cid == "sat_one":
        assert float(ref["weight"].max()) < 0.9999

    # 2. the reference alone is inside the tolerances of the GPU tests
    image64, gg64, gf64 = cc.truth_2d(cfg)
    weight64 = orc.rasterize_with_tiles(g2d.astype(np.float64), feat.astype(np.float64), ref["o2p"], ref["ranges"],
                                        cc.SIZE_2D, ref["ocfg"])[1]
    pu.assert_pixels_close(ref["image"], image64, "f32 oracle image vs f64")
    pu.assert_pixels_close(ref["weight"], weight64, "f32 oracle weight vs f64")
    # the f64 backward reads its own image; the f32 one its own: the difference is the whole f32 path
    pu.assert_grad_close(gg, gg64, "f32 oracle grad_gaussians2d vs f64")
    pu.assert_grad_close(gf, gf64, "f32 oracle grad_features vs f64")
    figures.append(f"f32 vs f64: image {np.abs(ref['image'] - image64).max():.2e}, gradients {normwise(gg, gg64):.2e} "
                   f"{normwise(gf, gf64):.2e}")

    # 3. the flip escape cannot hide a failure
    proof = ref["proof"]
    could_flip = int((proof.margin <= proof.bar).sum())
    figures.append(f"{could_flip} of {proof.margin.size} pixels within the bar {proof.bar:.2e}")
    print("; ".join(figures))
    assert could_flip <= MAX_FLIP_FRACTION * proof.margin.size


def test_flip_bar_scales_with_the_exponent():
    """the stated bars hold at the defaults and never shrink; a lower threshold lengthens them in proportion"""
    assert cc.flip_bar(pu.FLIP_MARGIN, 0.99, 1.0 / 255.0) == pytest.approx(pu.FLIP_MARGIN, rel=1e-3)
    assert cc.flip_bar(pu.FLIP_MARGIN, 0.9, 0.3) == pu.FLIP_MARGIN
    assert cc.flip_bar(pu.FLIP_MARGIN, 4.0, 1e-4) == cc.flip_bar(pu.FLIP_MARGIN, 1.0, 1e-4)
    assert cc.flip_bar(pu.AA_FLIP_MARGIN, 1.0, 1e-4) == pytest.approx(pu.AA_FLIP_MARGIN * np.log(1e4) / 5.54)


# ------------------------------------------------------------------------------------------------ the frame scene
@pytest.mark.parametrize("fid", list(cc.FRAMES))
def test_frame_scene_visible_lists_agree_in_both_precisions(fid):
    g, camera = cc.frame_scene()
    cfg = cc.frame_config(fid)
    r32 = pu.oracle_render(g, camera, cfg, use_sh=True, flips=False)
    r64 = pu.oracle_render(g, camera, cfg, use_sh=True, flips=False, dtype=np.float64)
    assert (r32["indexes"] == r64["indexes"]).all()
    V, n = r32["indexes"].shape[0], cc.FRAME_SCENE["n"]
    assert 0.95 * n < V <= n
    W, H = cc.FRAME_SCENE["size"]
    m = cfg.clamp_margin
    u, v = r32["points"][:, 0], r32["points"][:, 1]
    clamped = int(((u < -W * m) | (u > (W - 1) * (1 + m)) | (v < -H * m) | (v > (H - 1) * (1 + m))).sum())
    print(f"{fid}: V = {V}, clamp_margin {m}: {clamped} clamped means")
    if m == 0.0:
        assert clamped > 0
    else:
        # the scene's means stay within 0.05 of the size of the image: nothing is clamped at 0.15 or 0.5, so in the
        # fused frame only frame_a exercises clamp_margin (0.5 and 1.0 are told apart from 0.15 in the projection
        # sweep, on config_cases.projection_scene)
        assert clamped == 0


@pytest.mark.parametrize("fid", list(cc.FRAMES))
def test_frame_scene_f32_oracle_is_inside_the_end_to_end_tolerances(fid):
    """the f32 oracle pipeline against the f64 one at the bar test_config_sweep_gpu.py applies to the HIP pipeline, and
    how many pixels that bar could excuse at all.  Where the two oracles part by more than the tolerance (one pixel, in
    frame_b) the pixel's margin is the figure behind parity_util.E2E_AXIS_FLIP_MARGIN, and only the splats with an
    ill-conditioned axis get that bar (config_cases.frame_flip_proof)."""
    g, camera = cc.frame_scene()
    cfg = cc.frame_config(fid)
    r32 = pu.oracle_render(g, camera, cfg, use_sh=True)
    r64 = pu.oracle_render(g, camera, cfg, use_sh=True, flips=False, dtype=np.float64)
    flips = cc.frame_flip_proof(fid, r32, r64, cfg)
    assert flips.bar == cc.flip_bar(pu.E2E_FLIP_MARGIN, r32["points"][:, 6].max(), cfg.alpha_threshold)
    could_flip = float((flips.margin <= flips.bar).mean())
    stated = float((r32["flips"].margin <= flips.bar).mean())
    rep = pu.assert_pixels_close(r32["image"], r64["image"], "f32 oracle image", atol=1e-3, rtol=1e-3, flips=flips)
    rep_w = pu.assert_pixels_close(r32["alpha"], r64["alpha"], "f32 oracle weight", atol=1e-3, rtol=1e-3,
                                   flips=flips.weight())
    print(f"{fid}: {could_flip:.4f} of the pixels within the bar ({stated:.4f} at the stated bar alone); f32 oracle "
          f"pipeline vs f64: {rep}")
    assert could_flip <= cc.MAX_E2E_COULD_FLIP and could_flip - stated <= 0.002
    assert rep["outlier_pixels"] <= 1 and rep_w["outlier_pixels"] <= 1
    if fid not in cc.AXIS_EXCEPTION_FRAMES:
        assert rep["outlier_pixels"] == 0 and (flips.margin == r32["flips"].margin).all()
    elif rep["outlier_pixels"]:
        wide = cc.flip_bar(pu.E2E_AXIS_FLIP_MARGIN, r32["points"][:, 6].max(), cfg.alpha_threshold)
        measured = rep["max_margin_of_outliers"] * wide / flips.bar   # the ill splats' margins are stored rescaled
        assert measured * 3 <= wide, "the bar keeps about 4x over what was measured"


# ------------------------------------------------------------------------------------------------ the projection scene
@pytest.mark.parametrize("pid", list(cc.PROJ_CASES))
def test_projection_scene_holds_clamped_and_culled_rows(pid):
    kw = cc.PROJ_CASES[pid]
    args = [t.numpy() for t in cc.projection_scene()]
    n = args[0].shape[0]
    assert n == 400
    p32, _, i32 = orc.project(*args, cc.PROJ_SIZE, cc.PROJ_DEPTH_RANGE, **kw)
    _, _, i64 = orc.project(*(a.astype(np.float64) for a in args), cc.PROJ_SIZE, cc.PROJ_DEPTH_RANGE, **kw)
    assert i32.shape == i64.shape and (i32 == i64).all(), "the visible set must not hang on rounding"
    assert 10 <= n - i32.shape[0], "culled rows"
    beyond = cc.clamped_rows(p32, i32, kw["clamp_margin"], n)
    counts = [int(cc.clamped_rows(p32, i32, m, n).sum()) for m in cc.PROJ_MARGINS]
    print(f"{pid}: {i32.shape[0]} visible; clamped at margins {cc.PROJ_MARGINS}: {counts}")
    assert int(beyond.sum()) >= 40, "visible means outside the image by more than margin x size"
    assert counts[0] - counts[1] >= 40 and counts[1] - counts[2] >= 40, "visible means between the margins"


def test_projection_clamp_shows_in_the_oracle_position_gradient():
    args = [t.numpy().astype(np.float64) for t in cc.projection_scene()]
    rows = {}
    for m in (0.0, 1.0):
        kw = dict(cc.PROJ_DEFAULT, clamp_margin=m)
        p, d, idx = orc.project(*args, cc.PROJ_SIZE, cc.PROJ_DEPTH_RANGE, **kw)
        gen = np.random.default_rng(1)
        gp = gen.random((400, 7))
        dpos = orc.project_backward(*args, cc.PROJ_SIZE, idx, gp[idx], np.zeros(idx.shape[0]),
                                    blur_cov=kw["blur_cov"], clamp_margin=m)[0]
        rows[m] = (idx, dpos)
    both = np.intersect1d(rows[0.0][0], rows[1.0][0])
    differ = int((np.abs(rows[0.0][1][both] - rows[1.0][1][both]).max(1) > 0).sum())
    assert differ >= 40
