"""gs_raster_fwd_wide / gs_raster_bwd_wide (feature widths up to GS_MAX_WIDE_FEATURES): declared, exported, bound, and
validated on the host before any launch (no GPU needed)."""
import ctypes
import os
import re

from taichi_gaussian_rasterizer_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gsplat_hip.h")
FAKE = ctypes.c_void_p(256)  # never dereferenced: every call below is refused before a launch


def test_wide_entry_points_are_declared_exported_and_bound():
    text = open(HEADER).read()
    assert re.search(r"#define GS_MAX_WIDE_FEATURES 512\b", text)
    for name in ("gs_raster_fwd_wide", "gs_raster_bwd_wide"):
        assert re.search(r"\b" + name + r"\s*\(", text)
        assert name in _native.SIGNATURES
    _native.build()
    handle = ctypes.CDLL(_native.LIB_PATH)
    assert hasattr(handle, "gs_raster_fwd_wide") and hasattr(handle, "gs_raster_bwd_wide")
    assert _native.lib().gs_version() >= 5


def cfg(**kw):
    return _native.GsRasterConfig(tile_size=kw.pop("tile_size", 16), alpha_threshold=1 / 255.,
                                  saturate_threshold=0.9999, clamp_max_alpha=0.99, use_alpha_blending=1, **kw)


def fwd(F, c, image=FAKE, alpha=FAKE, ranges=FAKE, k=10):
    return _native.lib().gs_raster_fwd_wide(10, F, FAKE, FAKE, ranges, FAKE, k, 64, 48, c, image, alpha, None, None, 0,
                                            None)


def bwd(F, c, grad_points=FAKE, grad_features=FAKE, image=FAKE, heur=None, v=10, k=10):
    return _native.lib().gs_raster_bwd_wide(v, F, FAKE, FAKE, FAKE, FAKE, k, 64, 48, c, image, FAKE, None, None,
                                            grad_points, grad_features, heur, None)


def test_wide_validation():
    lib = _native.lib()
    assert fwd(513, cfg()) == -2 and b"feature width" in lib.gs_last_error()
    assert fwd(0, cfg()) == -2
    assert bwd(513, cfg()) == -2 and b"feature width" in lib.gs_last_error()
    assert fwd(64, cfg(tile_size=12)) == -2 and b"tile_size" in lib.gs_last_error()
    assert bwd(64, cfg(tile_size=64)) == -2
    blend_off = cfg()
    blend_off.use_alpha_blending = 0
    assert bwd(64, blend_off) == -2 and b"alpha blending" in lib.gs_last_error()
    assert fwd(64, cfg(), image=None) == -1 and b"NULL" in lib.gs_last_error()
    assert fwd(64, cfg(), alpha=None) == -1
    assert fwd(64, cfg(), ranges=None) == -1
    assert fwd(100, cfg(compute_visibility=1)) == -1 and b"visibility" in lib.gs_last_error()
    assert bwd(64, cfg(), grad_points=None) == -1 and b"NULL" in lib.gs_last_error()
    assert bwd(64, cfg(), grad_features=None) == -1
    assert bwd(64, cfg(), image=None) == -1
    assert bwd(64, cfg(compute_point_heuristic=1)) == -1 and b"point_heuristic" in lib.gs_last_error()
    # nothing to add: a no-op, whatever the gradient buffers
    assert bwd(64, cfg(), grad_points=None, grad_features=None, v=0, k=0) == 0


def test_narrow_entry_points_keep_their_limit():
    lib = _native.lib()
    c = cfg()
    assert lib.gs_raster_fwd(0, 33, None, None, None, None, 0, 16, 16, c, None, None, None, None, None, None, None, 0,
                             None) == -2
    assert lib.gs_raster_bwd(0, 33, None, None, None, None, 0, 16, 16, c, None, None, None, None, None, None, None, None,
                             None) == -2
