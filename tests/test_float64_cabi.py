"""The float64 entry points (include/gsplat_hip.h, csrc/*_f64.hip) are declared, exported and bound, and validate their
arguments on the host before any launch (no GPU needed)."""
import ctypes
import os
import re

import pytest

from taichi_gaussian_rasterizer_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gsplat_hip.h")
F64 = ("gs_project_f64_scratch_bytes", "gs_project_fwd_f64", "gs_project_bwd_f64_scratch_bytes", "gs_project_bwd_f64",
       "gs_sh_fwd_f64", "gs_sh_bwd_f64_scratch_bytes", "gs_sh_bwd_f64", "gs_raster_f64_scratch_bytes",
       "gs_raster_fwd_f64", "gs_raster_bwd_f64")


def test_f64_entry_points_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    _native.build()
    handle = ctypes.CDLL(_native.LIB_PATH)
    for name in F64:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert hasattr(handle, name), name
        assert name in _native.SIGNATURES
    assert "GsRasterConfigF64" in text


def _cfg(**kw):
    c = dict(tile_size=16, antialias=0, use_alpha_blending=1, compute_point_heuristic=0, compute_visibility=0,
             clamp_margin=0.15, blur_cov=0.3, clamp_max_alpha=0.99, alpha_threshold=1 / 255., saturate_threshold=0.9999)
    c.update(kw)
    return _native.GsRasterConfigF64(**c)


def test_f64_config_keeps_double_thresholds():
    from taichi_gaussian_rasterizer_amd import RasterConfig
    c = _native.make_config_f64(RasterConfig(compute_point_heuristic=True))
    assert c.clamp_max_alpha == 0.99 and c.alpha_threshold == 1.0 / 255.0 and c.saturate_threshold == 0.9999
    assert c.compute_visibility == 1 and c.tile_size == 16


def test_f64_raster_validation_on_the_host():
    lib = _native.lib()
    fake = ctypes.c_void_p(16)  # never dereferenced: every call below fails validation first
    big = 1 << 20
    rc = lib.gs_raster_fwd_f64(0, 3, None, None, fake, None, 0, 16, 16, _cfg(tile_size=12), fake, fake, None, None, 0,
                               fake, big, None)
    assert rc == -2 and b"tile_size" in lib.gs_last_error()
    with pytest.raises(NotImplementedError):
        _native.check(rc, "gs_raster_fwd_f64")
    rc = lib.gs_raster_fwd_f64(0, 33, None, None, fake, None, 0, 16, 16, _cfg(), fake, fake, None, None, 0, fake, big,
                               None)
    assert rc == -2 and b"feature width" in lib.gs_last_error()
    rc = lib.gs_raster_bwd_f64(0, 33, None, None, fake, None, 0, 16, 16, _cfg(), fake, fake, None, None, None, None,
                               None, fake, big, None)
    assert rc == -2 and b"feature width" in lib.gs_last_error()
    rc = lib.gs_raster_fwd_f64(4, 3, None, None, fake, None, 4, 16, 16, _cfg(), fake, fake, None, None, 0, fake, big,
                               None)
    assert rc == -1 and b"NULL" in lib.gs_last_error()
    with pytest.raises(ValueError):
        _native.check(rc, "gs_raster_fwd_f64")
    rc = lib.gs_raster_fwd_f64(0, 3, None, None, fake, None, 0, 16, 16, _cfg(), fake, fake, None, None, 0, fake, 0,
                               None)
    assert rc == -4 and b"scratch" in lib.gs_last_error()
    rc = lib.gs_raster_bwd_f64(0, 3, None, None, fake, None, 0, 16, 16, _cfg(use_alpha_blending=0), fake, fake, None,
                               None, None, None, None, fake, big, None)
    assert rc == -2 and b"use_alpha_blending" in lib.gs_last_error()
    assert lib.gs_raster_f64_scratch_bytes(100, 1000, 3) >= 1000 * 12 * 8


def test_f64_projection_and_sh_validation_on_the_host():
    lib = _native.lib()
    fake = ctypes.c_void_p(16)
    rc = lib.gs_project_fwd_f64(8, None, None, None, None, fake, fake, 64, 64, 0.1, 100.0, _cfg(), None, None, None,
                                None, None, fake, fake, 1 << 20, None)
    assert rc == -1 and b"NULL gaussian tensor" in lib.gs_last_error()
    rc = lib.gs_project_fwd_f64(0, None, None, None, None, None, None, 64, 64, 0.1, 100.0, _cfg(), None, None, None,
                                None, None, fake, None, 0, None)
    assert rc == -1 and b"NULL camera" in lib.gs_last_error()
    rc = lib.gs_project_bwd_f64(8, None, None, None, None, fake, fake, 64, 64, None, None, None, None, None, None,
                                None, None, None, None, None, 0, None)
    assert rc == -1 and b"config is NULL" in lib.gs_last_error()
    rc = lib.gs_sh_fwd_f64(4, 3, 4, fake, fake, fake, fake, fake, None)
    assert rc == -2 and b"degree" in lib.gs_last_error()
    rc = lib.gs_sh_fwd_f64(4, 9, 1, fake, fake, fake, fake, fake, None)
    assert rc == -2 and b"channels" in lib.gs_last_error()
    rc = lib.gs_sh_fwd_f64(4, 3, 1, None, fake, fake, fake, fake, None)
    assert rc == -1 and b"NULL" in lib.gs_last_error()
    rc = lib.gs_sh_bwd_f64(4, 4, 3, 1, fake, fake, fake, fake, fake, fake, None, None, fake, 0, None)
    assert rc == -4 and b"scratch" in lib.gs_last_error()
