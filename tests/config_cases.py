"""RasterConfig settings away from the defaults, and the scenes they run on: shared by test_config_sweep_cpu.py (the
conditions on the inputs, oracle only) and test_config_sweep_gpu.py (the HIP kernels against the oracle).  Every kernel
receives alpha_threshold, clamp_max_alpha, saturate_threshold, clamp_margin and blur_cov as scalars; a constant that
happens to equal a default, or a reformulation valid only near one, passes every test that builds RasterConfig()."""
import functools
import math

import numpy as np

import parity_util as pu

# id -> RasterConfig keyword arguments, and what the setting reaches
CONFIGS = {
    "thr_small": dict(alpha_threshold=1e-4),  # long tails: r2 = log2(opacity / thr) ~ 13, about 1.3x the overlaps
    "thr_mid": dict(alpha_threshold=0.05),  # the cull radius shrinks to ln(20 opacity): lists a third shorter
    "thr_big": dict(alpha_threshold=0.3),  # most opacities of the scene are below the threshold
    "clamp_half": dict(clamp_max_alpha=0.5),  # the clamp bites on most central pixels
    "clamp_high": dict(clamp_max_alpha=0.999),  # 1 / (1 - alpha) up to 1000 in the backward
    "clamp_below_thr": dict(clamp_max_alpha=0.002),  # forward blends nothing; backward (raw-alpha test) still writes
    "sat_half": dict(saturate_threshold=0.5),  # the backward stops most pixels inside their lists
    "sat_090": dict(saturate_threshold=0.9),  # ... a quarter of them
    "sat_one": dict(saturate_threshold=1.0),  # tsat = 0: the backward walks past where the forward stopped
    "mixed": dict(alpha_threshold=1e-4, clamp_max_alpha=0.6, saturate_threshold=0.95),  # all three at once
    "aa_mixed": dict(antialias=True, blur_cov=0.0, alpha_threshold=1e-3, clamp_max_alpha=0.7),  # the general kernels
}
THR_IDS = ("thr_small", "thr_mid", "thr_big")
CLAMP_IDS = ("clamp_half", "clamp_high", "clamp_below_thr")  # what their clamp does is measured against 0.99
SAT_IDS = ("sat_half", "sat_090", "mixed")  # what their level does is measured against 0.9999
TILES = (8, 16, 32)

# the fused frame: RasterConfig keyword arguments per frame, every scalar away from its default, tiles 8 / 32 / 16
FRAMES = {
    "frame_a": dict(tile_size=8, alpha_threshold=1e-3, clamp_max_alpha=0.8, saturate_threshold=0.99, clamp_margin=0.0,
                    blur_cov=0.1),
    "frame_b": dict(tile_size=32, alpha_threshold=0.02, clamp_max_alpha=0.95, saturate_threshold=0.9, clamp_margin=0.5,
                    blur_cov=1.0),
    "frame_c": dict(tile_size=16, compute_point_heuristic=True, **CONFIGS["mixed"]),
}
FRAME_SCENE = dict(n=3000, size=(129, 65), sh_degree=2, seed=3)

SIZE_2D = (90, 61)  # no multiple of 8, 16 or 32


def raster_config(cid, tile=16, **extra):
    from taichi_gaussian_rasterizer_amd import RasterConfig
    return RasterConfig(tile_size=tile, **{**CONFIGS[cid], **extra})


@functools.lru_cache(maxsize=None)
def scene_2d(channels=3):
    """(gaussians2d (600, 7), depth (600, 1), features (600, channels)) as float32 numpy, read only: opacities from
    0.053 to 0.9996 on a 90 x 61 image"""
    g2d, depth, feat = pu.make_2d_scene(5, 600, SIZE_2D, channels=channels, scale_factor=0.8, alpha_range=(0.05, 1.0))
    out = tuple(np.ascontiguousarray(pu.to_np(t), dtype=np.float32) for t in (g2d, depth, feat))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def grad_image_2d(channels=3):
    """the upstream gradient of the 2D scene: signed, so that what a pixel's splats receive does not cancel to the
    same sign everywhere -- with a positive one (torch.rand) `mixed`'s level of 0.95 moves the geometry gradient by
    0.9 % only, with this one by 2.3 % (test_config_sweep_cpu.py asserts more than 100 x GRAD_TOL = 2 %)"""
    import torch
    gi = torch.randn(SIZE_2D[1], SIZE_2D[0], channels, generator=torch.Generator().manual_seed(3)).numpy()
    gi.setflags(write=False)
    return gi


@functools.lru_cache(maxsize=None)
def oracle_2d(cfg, channels=3, lists_cfg=None):
    """the float32 oracle's lists, image, weight and visibility for the 2D scene under `cfg`, with the flip proof at
    the scaled bar; computed once per config and shared.  lists_cfg: the config the tile lists are built with, when it
    is not the one that rasterizes (rasterize_with_tiles takes the caller's lists)"""
    from oracle import oracle as orc
    g2d, depth, feat = scene_2d(channels)
    ocfg = orc.OracleConfig.of(cfg)
    o2p, ranges = orc.map_to_tiles(g2d, depth, SIZE_2D, orc.OracleConfig.of(lists_cfg or cfg))
    image, weight, vis = orc.rasterize_with_tiles(g2d, feat, o2p, ranges, SIZE_2D, ocfg)
    proof = pu.flip_proof(g2d, feat, o2p, ranges, SIZE_2D, ocfg, bar=raster_bar(cfg, g2d))
    return dict(ocfg=ocfg, o2p=o2p, ranges=ranges, image=image, weight=weight, visibility=vis, proof=proof)


@functools.lru_cache(maxsize=None)
def truth_2d(cfg, channels=3, lists_cfg=None):
    """(image, grad_gaussians2d, grad_features) of the float64 oracle on the float32 oracle's lists"""
    g2d, _, feat = scene_2d(channels)
    ref = oracle_2d(cfg, channels, lists_cfg)
    return pu.raster_truth(g2d, feat, ref["o2p"], ref["ranges"], SIZE_2D, ref["ocfg"], grad_image_2d(channels))


def frame_scene():
    from taichi_gaussian_rasterizer_amd import scenes
    s = FRAME_SCENE
    return scenes.benchmark_scene(s["n"], s["size"], sh_degree=s["sh_degree"], seed=s["seed"])


def frame_config(fid, **extra):
    from taichi_gaussian_rasterizer_amd import RasterConfig
    return RasterConfig(**{**FRAMES[fid], **extra})


# ------------------------------------------------------------------------------------------------ projection
# one-at-a-time sweeps of the projection's three scalars plus one case with all three away from their defaults
PROJ_DEFAULT = dict(clamp_margin=0.15, blur_cov=0.3, alpha_threshold=1.0 / 255.0)
PROJ_COMBINED = dict(clamp_margin=0.0, blur_cov=1.0, alpha_threshold=0.1)
PROJ_CASES = {
    "default": PROJ_DEFAULT,
    "margin_0": dict(PROJ_DEFAULT, clamp_margin=0.0),
    "margin_1": dict(PROJ_DEFAULT, clamp_margin=1.0),
    "blur_0": dict(PROJ_DEFAULT, blur_cov=0.0),
    "blur_1": dict(PROJ_DEFAULT, blur_cov=1.0),
    "thr_1e-4": dict(PROJ_DEFAULT, alpha_threshold=1e-4),
    "thr_0.1": dict(PROJ_DEFAULT, alpha_threshold=0.1),
    "combined": PROJ_COMBINED,
}
PROJ_SIZE = (160, 96)
PROJ_DEPTH_RANGE = (0.1, 100.0)
PROJ_MARGINS = (0.0, 0.15, 1.0)


@functools.lru_cache(maxsize=None)
def projection_scene():
    """400 Gaussians for a camera at the origin looking down +z (fx = fy = 120, principal point (80, 48), image
    160 x 96), modelled on test_float64_gpu.clamp_and_cull_scene.  Returns the six projection inputs as float32 torch
    tensors.  Rows:
      0..179    ordinary, means inside the image, every sixth with an opacity around the thresholds tested;
      180..219  means outside by 0.1 .. 0.6 of the size, sigma ~ 0.05 of the width: in view or not with the threshold;
      220..279  large, means outside by 1.05 .. 1.3 of the size: beyond every margin tested, extent reaching in;
      280..339  large, means outside by 0.2 .. 0.9 of the size: between the margins 0.15 and 1.0;
      340..399  large, means outside by 0.02 .. 0.13 of the size: between the margins 0.0 and 0.15."""
    import torch
    rng = np.random.default_rng(7)
    W, H = PROJ_SIZE
    f, cx, cy = 120.0, W / 2.0, H / 2.0

    def outside(count, lo, hi):
        """means outside the image by lo .. hi of its size, on a random side, in x (even rows) or in y (odd rows)"""
        frac = rng.uniform(lo, hi, count)
        side = rng.integers(0, 2, count)
        u, v = rng.uniform(0, W, count), rng.uniform(0, H, count)
        in_x = np.arange(count) % 2 == 0
        u = np.where(in_x, np.where(side == 0, -frac * W, (W - 1) + frac * W), u)
        v = np.where(~in_x, np.where(side == 0, -frac * H, (H - 1) + frac * H), v)
        return np.stack([u, v], 1)

    uv = np.concatenate([rng.uniform(0, 1, (180, 2)) * [W, H], outside(40, 0.1, 0.6), outside(60, 1.05, 1.3),
                         outside(60, 0.2, 0.9), outside(60, 0.02, 0.13)])
    n = uv.shape[0]
    z = rng.uniform(2.0, 8.0, n)
    position = np.stack([(uv[:, 0] - cx) * z / f, (uv[:, 1] - cy) * z / f, z], 1)
    scale = rng.uniform(0.02, 0.15, (n, 3)) * z[:, None]
    scale[180:220] = (0.05 * W / f) * rng.uniform(0.8, 1.2, (40, 3)) * z[180:220, None]
    reach = np.concatenate([np.full(60, 1.0), np.full(60, 0.7), np.full(60, 0.15)])  # sigma, in image widths
    scale[220:] = (reach * W / f)[:, None] * rng.uniform(0.8, 1.2, (180, 3)) * z[220:, None]
    rotation = rng.standard_normal((n, 4))
    opacity = rng.uniform(0.3, 0.95, n)
    opacity[:180:6] = rng.uniform(0.002, 0.2, 30)  # some below the thresholds tested
    tensors = (position, np.log(scale), rotation, np.log(opacity / (1 - opacity))[:, None], np.eye(4),
               np.array([f, f, cx, cy]))
    return tuple(torch.as_tensor(np.ascontiguousarray(t), dtype=torch.float32) for t in tensors)


def clamped_rows(points, indexes, margin, n):
    """bool (n,): visible rows whose projected mean the affine Jacobian clamps at `margin`"""
    W, H = PROJ_SIZE
    u, v = points[:, 0], points[:, 1]
    out = np.zeros(n, bool)
    out[indexes] = (u < -W * margin) | (u > (W - 1) * (1 + margin)) | (v < -H * margin) | (v > (H - 1) * (1 + margin))
    return out


# parity_util's flip bars are stated at the default threshold: two f32 evaluations of alpha = opacity * exp(-q) land on
# different sides of `alpha > thr` when |alpha - thr| / thr is within the rounding of the exponent q, which carries ~4
# roundings RELATIVE to its size -- and at a threshold pixel q = ln(opacity / thr), at most ln(opacity_max / thr):
# ln(0.99 * 255) = 5.54 at the defaults (parity_util.FLIP_MARGIN's comment).  A lower threshold lengthens the exponent
# and the bar in proportion; a higher one never shortens the bar below its stated value.  Opacities above 1 reach the
# blend clamped, and what they add to q beyond ln(1 / thr) is not claimed.
DEFAULT_EXPONENT = 5.54


def flip_bar(base, opacity_max, alpha_threshold):
    """`base` (pu.FLIP_MARGIN, pu.AA_FLIP_MARGIN or pu.E2E_FLIP_MARGIN) scaled to the exponent ln(opacity_max / thr)"""
    return base * max(1.0, math.log(min(float(opacity_max), 1.0) / float(alpha_threshold)) / DEFAULT_EXPONENT)


# End to end, the f32 and f64 oracles part at one pixel of frame_b beyond the stated bar, through the AXIS of one splat
# (parity_util.E2E_AXIS_FLIP_MARGIN).  The wider bar is confined to the splats whose axis the two oracles themselves
# place more than AXIS_ILL apart (3 or 4 of the 3000): a rotation by d moves ln alpha at a splat's rim by about
# 2 ln(opacity / thr) * (sigma1^2 - sigma2^2) / (2 sigma1 sigma2) * d, which for d below 1e-3 and the anisotropies at
# which the axis is ill-conditioned (<= 0.1) stays below 1e-3, inside E2E_FLIP_MARGIN.  Every other splat keeps the
# stated bar, and the number of pixels that take the escape at all is capped (the oracles show 1, in frame_b).
AXIS_ILL = 1e-3
AXIS_EXCEPTION_FRAMES = ("frame_b",)
MAX_E2E_OUTLIERS = 4
MAX_E2E_COULD_FLIP = 0.13   # of the pixels within the bar, oracle alone: 9 % (frame_a, frame_b), 12 % (frame_c)


def frame_flip_proof(fid, ref, ref64, cfg):
    """the end-to-end flip proof of a frame of FRAMES from its f32 and f64 oracle renders: E2E_FLIP_MARGIN scaled to
    the threshold; in AXIS_EXCEPTION_FRAMES, E2E_AXIS_FLIP_MARGIN for the splats with an ill-conditioned axis only"""
    from oracle import oracle as orc
    points = ref["points"]
    bar = flip_bar(pu.E2E_FLIP_MARGIN, points[:, 6].max(), cfg.alpha_threshold)
    base = ref["flips"]
    if fid not in AXIS_EXCEPTION_FRAMES:
        return pu.FlipProof(base.margin, base.thr, base.feat_max, bar)
    p64 = ref64["points"]
    ill = np.abs(points[:, 2].astype(np.float64) * p64[:, 3] - points[:, 3].astype(np.float64) * p64[:, 2]) > AXIS_ILL
    assert 0 < int(ill.sum()) <= 8, "the exception is for a handful of splats"
    wide = flip_bar(pu.E2E_AXIS_FLIP_MARGIN, points[:, 6].max(), cfg.alpha_threshold)
    ocfg, size = orc.OracleConfig.of(cfg), FRAME_SCENE["size"]
    well, badly = points.copy(), points.copy()
    well[ill, 6] = 0.0      # a splat without opacity is at margin 1
    badly[~ill, 6] = 0.0
    m_well = orc.raster_flip_margin(well, ref["o2p"], ref["ranges"], size, ocfg)
    m_ill = orc.raster_flip_margin(badly, ref["o2p"], ref["ranges"], size, ocfg)
    return pu.FlipProof(np.minimum(m_well, m_ill * np.float32(bar / wide)), base.thr, base.feat_max, bar)


def raster_bar(cfg, g2d):
    """the rasterizer bar for a config and the splats it blends"""
    base = pu.AA_FLIP_MARGIN if cfg.antialias else pu.FLIP_MARGIN
    return flip_bar(base, np.max(pu.to_np(g2d)[:, 6]), cfg.alpha_threshold)
