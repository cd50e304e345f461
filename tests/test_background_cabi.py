"""Background colour and differentiable weight image: one entry point per operation takes them (the twins that once
carried them are gone from the header, the binding and the library), refuses bad arguments on the host before any
launch, and the Python operators refuse theirs before they look at the device (no GPU needed)."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import taichi_gaussian_rasterizer_amd as gs
from taichi_gaussian_rasterizer_amd import RasterConfig, _native, scenes
from taichi_gaussian_rasterizer_amd.misc import renderer2d
from taichi_gaussian_rasterizer_amd.renderer import render_projected

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gsplat_hip.h")
FAKE = ctypes.c_void_p(256)  # never dereferenced: every call below is refused before a launch
# the consolidated surface: entry point -> number of arguments
SURFACE = {"gs_raster_fwd": 19, "gs_raster_bwd": 19, "gs_raster_fwd_wide": 16, "gs_raster_bwd_wide": 18,
           "gs_raster_fwd_f64": 18, "gs_raster_bwd_f64": 20, "gs_frame_fwd": 17, "gs_frame_bwd": 31,
           "gs_frame_bwd_rows": 31}
# the ten twins it replaced (suffixes kept apart from the names, so that a search of the tree for a twin finds none)
BG, PART = "bg", "part"
REMOVED = [f"{name}_{BG}" for name in SURFACE if name != "gs_frame_bwd"] + [f"gs_frame_bwd_{PART}",
                                                                             f"gs_frame_bwd_{PART}_{BG}"]


def test_entry_points_are_declared_exported_and_bound():
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    _native.build()
    handle = ctypes.CDLL(_native.LIB_PATH)
    assert len(REMOVED) == 10
    for name in REMOVED:
        assert name not in raw, f"{name} is still in the header"
        assert name not in _native.SIGNATURES and not hasattr(handle, name)
    for name, count in SURFACE.items():
        declared = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert declared, f"{name} is not declared"
        assert len(declared.group(1).split(",")) == count
        assert len(_native.SIGNATURES[name][1]) == count and hasattr(handle, name)
    assert _native.SIGNATURES["gs_frame_bwd"] == _native.SIGNATURES["gs_frame_bwd_rows"]
    assert _native.lib().gs_version() >= 7
    # the pinned structs did not grow
    assert ctypes.sizeof(_native.GsRasterConfig) == 60 and ctypes.sizeof(_native.GsFrame) == 168
    assert ctypes.sizeof(_native.GsFrameBwdPart) == 48


def cfg(blend=1, **kw):
    return _native.GsRasterConfig(tile_size=16, alpha_threshold=1 / 255., saturate_threshold=0.9999,
                                  clamp_max_alpha=0.99, use_alpha_blending=blend, **kw)


def cfg64(blend=1):
    return _native.GsRasterConfigF64(tile_size=16, alpha_threshold=1 / 255., saturate_threshold=0.9999,
                                     clamp_max_alpha=0.99, use_alpha_blending=blend)


def test_host_side_refusals_of_the_raster_entry_points():
    lib = _native.lib()

    def fwd(c, bg=FAKE, off=0, F=3):
        return lib.gs_raster_fwd(10, F, FAKE, FAKE, FAKE, FAKE, 10, 64, 48, c, None, None, FAKE, FAKE, None, None, bg,
                                 off, None)

    def fwd_wide(c, bg=FAKE, off=0, F=64):
        return lib.gs_raster_fwd_wide(10, F, FAKE, FAKE, FAKE, FAKE, 10, 64, 48, c, FAKE, FAKE, None, bg, off, None)

    def fwd_f64(c, bg=FAKE, off=0, F=3):
        return lib.gs_raster_fwd_f64(10, F, FAKE, FAKE, FAKE, FAKE, 10, 64, 48, c, FAKE, FAKE, None, bg, off, FAKE,
                                     1 << 40, None)

    for call, blend_off in ((fwd, cfg(0)), (fwd_wide, cfg(0)), (fwd_f64, cfg64(0))):
        assert call(blend_off) == -2 and b"use_alpha_blending" in lib.gs_last_error()
    for call, c, F in ((fwd, cfg(), 3), (fwd_wide, cfg(), 64), (fwd_f64, cfg64(), 3)):
        assert call(c, off=F) == -1 and b"background_offset" in lib.gs_last_error()
        assert call(c, off=-1) == -1
    # grad_weight without the forward's alpha image
    assert lib.gs_raster_bwd(10, 3, FAKE, FAKE, FAKE, FAKE, 10, 64, 48, cfg(), None, None, FAKE, FAKE, None, FAKE,
                             FAKE, None, None) == -1 and b"alpha" in lib.gs_last_error()
    assert lib.gs_raster_bwd_wide(10, 64, FAKE, FAKE, FAKE, FAKE, 10, 64, 48, cfg(), FAKE, FAKE, None, FAKE, FAKE,
                                  FAKE, None, None) == -1 and b"alpha" in lib.gs_last_error()
    assert lib.gs_raster_bwd_f64(10, 3, FAKE, FAKE, FAKE, FAKE, 10, 64, 48, cfg64(), FAKE, FAKE, None, FAKE, FAKE,
                                 FAKE, None, FAKE, 1 << 40, None) == -1 and b"alpha" in lib.gs_last_error()
    # no gradient without alpha blending, with or without a weight gradient
    assert lib.gs_raster_bwd(10, 3, FAKE, FAKE, FAKE, FAKE, 10, 64, 48, cfg(0), None, None, FAKE, FAKE, FAKE, FAKE,
                             FAKE, None, None) == -2


def _frame(**kw):
    f = _native.GsFrame()
    f.n, f.channels, f.sh_degree, f.width, f.height = 100, 3, -1, 64, 48
    f.near_plane, f.far_plane, f.k_capacity = 0.1, 100.0, 65536
    f.cfg = cfg(kw.pop("blend", 1))
    for k, v in kw.items():
        setattr(f, k, v)
    return f


def test_host_side_refusals_of_the_frame_entry_points():
    lib = _native.lib()
    frame = _frame(blend=0)
    rc = lib.gs_frame_fwd(ctypes.byref(frame), *[FAKE] * 7, FAKE, 1 << 40, FAKE, 1 << 40, None, None, None, FAKE, None)
    assert rc == -2 and b"use_alpha_blending" in lib.gs_last_error()

    def bwd(fn, frame, grad_image, grad_weight):
        return fn(ctypes.byref(frame), *[FAKE] * 7, FAKE, 1 << 40, FAKE, 1 << 40, 10, 10, grad_image, None, None,
                  grad_weight, None, None, *[FAKE] * 5, None, None, None, None, None, None)

    for fn in (lib.gs_frame_bwd, lib.gs_frame_bwd_rows):
        assert bwd(fn, _frame(blend=0), FAKE, FAKE) == -2 and b"use_alpha_blending" in lib.gs_last_error()
        assert bwd(fn, _frame(), None, FAKE) == -1 and b"grad_image" in lib.gs_last_error()


def test_python_refusals_come_before_the_device_check():
    """CPU tensors throughout: a refusal of the new arguments is raised where the operators would otherwise raise their
    'HIP device only' RuntimeError"""
    size = (16, 16)
    torch.manual_seed(0)
    g2 = scenes.random_2d_gaussians(10, size, num_channels=3)
    g2d = renderer2d.project_gaussians2d(g2).float()
    depth, feat = g2.z_depth.clamp(0, 1).float(), g2.feature.float()
    o2p = torch.zeros((0,), dtype=torch.int32)
    ranges = torch.zeros((1, 2), dtype=torch.int32)
    pick = RasterConfig(use_alpha_blending=False, saturate_threshold=0.5)
    bg = torch.zeros(3)
    calls = {
        "rasterize_with_tiles": lambda cfg, **kw: gs.rasterize_with_tiles(g2d, feat, o2p, ranges, size, cfg, **kw),
        "rasterize": lambda cfg, **kw: gs.rasterize(g2d, depth, feat, size, cfg, **kw),
        "renderer2d": lambda cfg, **kw: renderer2d.render_gaussians(g2, size, cfg, **kw),
    }
    g3, cam = scenes.benchmark_scene(16, (32, 32), sh_degree=0, seed=0)
    plain = g3.replace(feature=torch.rand(16, 3))
    calls["render_gaussians"] = lambda cfg, **kw: gs.render_gaussians(plain, cam, cfg, **kw)
    calls["render_gaussians_sh"] = lambda cfg, **kw: gs.render_gaussians(g3, cam, cfg, use_sh=True, **kw)
    calls["render_projected"] = lambda cfg, **kw: render_projected(torch.arange(10), g2d, feat, depth.view(-1, 1), cam,
                                                                   cfg, **kw)
    for name, call in calls.items():
        with pytest.raises(ValueError, match="use_alpha_blending"):
            call(pick, background=bg)
        with pytest.raises(ValueError, match="use_alpha_blending"):
            call(pick, differentiable_weight=True)
        with pytest.raises(TypeError):
            call(RasterConfig(), background=bg.double())
        with pytest.raises(TypeError):
            call(RasterConfig(), background=[0.0, 0.0, 0.0])
        with pytest.raises(AssertionError, match="background"):
            call(RasterConfig(), background=torch.zeros(4))
        with pytest.raises(AssertionError, match="background"):
            call(RasterConfig(), background=torch.zeros(1, 1, 3))
        with pytest.raises(TypeError, match="differentiable_weight must be bool"):
            call(RasterConfig(), differentiable_weight=1)
        # well-formed arguments get as far as the device check
        with pytest.raises(RuntimeError, match="HIP device"):
            call(RasterConfig(), background=bg, differentiable_weight=True)


def test_signatures_default_to_the_behaviour_before():
    for fn in (gs.render_gaussians, render_projected, gs.rasterize, gs.rasterize_with_tiles, renderer2d.render_gaussians):
        p = inspect.signature(fn).parameters
        assert p["background"].default is None and p["differentiable_weight"].default is False
    from taichi_gaussian_rasterizer_amd import parallel
    sharded = inspect.signature(parallel.render_gaussians_sharded).parameters
    assert "background" not in sharded and "differentiable_weight" not in sharded


def test_a_sharded_frame_refuses_both_arguments():
    from taichi_gaussian_rasterizer_amd import fused, parallel
    g, cam = scenes.benchmark_scene(16, (32, 32), sh_degree=0, seed=0)
    shard = parallel.RowShard(0, 1, 1, 1, 0, 16, 32)
    for kw in (dict(background=torch.zeros(3)), dict(differentiable_weight=True)):
        with pytest.raises(NotImplementedError, match="sharded"):
            fused.render_fused(g, cam, RasterConfig(), False, False, shard=shard, **kw)
