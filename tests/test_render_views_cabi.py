"""A batch of views as one node, the part that needs no GPU: gs_views_union and gs_views_sum_rows validate their
arguments on the host before any launch, an empty call is a no-op, and render_views / RenderedViews are public and refuse
bad arguments before anything is launched."""
import ctypes
import os

import pytest
import torch

import taichi_gaussian_rasterizer_amd as gs
from taichi_gaussian_rasterizer_amd import RasterConfig, _native, scenes

P = ctypes.c_void_p(16)  # a non-NULL pointer that is never dereferenced: every call below stops at a host-side check
VIEWS_MAX = 16


def _err(lib):
    return lib.gs_last_error()


def _tables(*entries):
    """host array of GsViewRows from (slot_of, values, count, stride)"""
    table = (_native.GsViewRows * max(len(entries), 1))()
    for k, entry in enumerate(entries):
        table[k] = _native.GsViewRows(*entry)
    return table


def test_views_union_validates_on_the_host():
    lib = _native.lib()
    n = 100_000
    need = lib.gs_views_union_scratch_bytes(n)
    two = (ctypes.c_void_p * 2)(16, 16)

    def call(n_, views=2, tables=two, union=P, union_count=P, scratch=P, scratch_bytes=need):
        return lib.gs_views_union(n_, views, tables, union, union_count, scratch, scratch_bytes, None)

    assert call(n, tables=None) == -1 and b"NULL buffer" in _err(lib)
    assert call(n, union=None) == -1 and b"NULL buffer" in _err(lib)
    assert call(n, union_count=None) == -1 and b"NULL buffer" in _err(lib)
    assert call(n, tables=(ctypes.c_void_p * 2)(16, None)) == -1 and b"NULL buffer" in _err(lib)
    assert call(-1) == -1 and b"rows" in _err(lib)
    for views in (-1, VIEWS_MAX + 1):
        assert call(n, views=views) == -1 and b"views" in _err(lib), views
    assert call(0, views=VIEWS_MAX + 1) == -1  # the range holds for an empty call too
    assert call(n, scratch_bytes=need - 1) == -4 and b"scratch" in _err(lib)
    assert call(n, scratch=None) == -4 and b"scratch" in _err(lib)
    assert call(n, scratch=ctypes.c_void_p(8)) == -1 and b"aligned" in _err(lib)
    # empty calls
    assert call(0, tables=None, union=None, union_count=None, scratch=None, scratch_bytes=0) == 0
    assert call(n, views=0, tables=None, union=None, union_count=None, scratch=None, scratch_bytes=0) == 0
    for size in (1, 31, 32, 33, 1000, n, 32768, 32769, 4_000_000):
        assert lib.gs_views_union_scratch_bytes(size) == lib.gs_rows_union_scratch_bytes(size) >= (size + 7) // 8
    assert lib.gs_views_union_scratch_bytes(0) == 0


def test_views_sum_rows_validates_on_the_host():
    lib = _native.lib()
    good = _tables((16, 16, 10, 3), (16, 16, 0, 3))

    def call(rows, indexes=P, views=2, tables=good, dims=3, out=P):
        return lib.gs_views_sum_rows(rows, indexes, views, tables, dims, out, None)

    assert call(10, indexes=None) == -1 and b"NULL buffer" in _err(lib)
    assert call(10, out=None) == -1 and b"NULL buffer" in _err(lib)
    assert call(10, tables=None) == -1 and b"NULL buffer" in _err(lib)
    assert call(10, tables=_tables((None, 16, 10, 3))) == -1 and b"NULL buffer" in _err(lib)
    assert call(10, tables=_tables((16, None, 10, 3))) == -1 and b"NULL buffer" in _err(lib)
    assert call(10, tables=_tables((16, 16, 10, 3), (16, 16, -1, 3))) == -1 and b"value rows" in _err(lib)
    assert call(10, tables=_tables((16, 16, 10, 2))) == -1 and b"stride" in _err(lib)
    assert call(-1) == -1 and b"rows" in _err(lib)
    for dims in (0, -3):
        assert call(10, dims=dims) == -1 and b"dims" in _err(lib), dims
    for views in (-1, VIEWS_MAX + 1):
        assert call(10, views=views) == -1 and b"views" in _err(lib), views
    assert call(0, dims=0) == -1              # the ranges hold for an empty call too
    assert call(0, views=VIEWS_MAX + 1) == -1
    assert call(0, indexes=None, tables=None, out=None) == 0
    assert call(0, views=VIEWS_MAX) == 0


def test_names_are_public_and_the_limit_is_in_the_header():
    for name in ("render_views", "RenderedViews"):
        assert name in gs.__all__ and callable(getattr(gs, name)), name
    assert _native.GS_VIEWS_MAX == VIEWS_MAX
    for name in ("gs_views_union_scratch_bytes", "gs_views_union", "gs_views_sum_rows"):
        assert name in _native.SIGNATURES, name
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "gsplat_hip.h")).read()
    assert f"#define GS_VIEWS_MAX {VIEWS_MAX}\n" in header
    assert ctypes.sizeof(_native.GsViewRows) == 32  # two pointers, int64_t, int32_t and its padding


def test_rendered_views_is_a_sequence_with_the_union():
    from taichi_gaussian_rasterizer_amd import optim
    rows, vis = torch.tensor([1, 4, 7]), torch.tensor([0.5, 0.0, 2.0])
    views = gs.RenderedViews(["a", "b"], rows, vis)
    assert len(views) == 2 and views[1] == "b" and list(views) == ["a", "b"] and views.renderings == ("a", "b")
    assert views.points_in_view is rows and views.point_visibility is vis and views.num_points == 3
    assert views.visible[0] is rows and views.visible[1] is vis  # every listed row, zero visibility included
    same = optim.visible_union(views)  # the stored pair: no launch, so it works on CPU tensors
    assert same[0] is rows and same[1] is vis
    with pytest.raises(AssertionError, match="compute_visibility"):
        gs.RenderedViews(["a"], rows, None).visible


def test_render_views_refuses_bad_arguments_before_any_launch():
    n, size = 50, (32, 24)
    g, cam = scenes.benchmark_scene(n, size, sh_degree=1)
    with pytest.raises(ValueError, match=str(VIEWS_MAX)):
        gs.render_views(g, [], use_sh=True)
    with pytest.raises(ValueError, match=str(VIEWS_MAX)):
        gs.render_views(g, [cam] * (VIEWS_MAX + 1), use_sh=True)
    with pytest.raises(TypeError, match=r"cameras\[1\]"):
        gs.render_views(g, [cam, "camera"], use_sh=True)
    with pytest.raises(TypeError, match="cameras"):
        gs.render_views(g, cam, use_sh=True)
    with pytest.raises(TypeError, match="config"):
        gs.render_views(g, [cam], config=None, use_sh=True)
    with pytest.raises(TypeError, match="sparse_grad"):
        gs.render_views(g, [cam], use_sh=True, sparse_grad=1)
    with pytest.raises(ValueError, match="use_alpha_blending"):
        gs.render_views(g, [cam], RasterConfig(use_alpha_blending=False), use_sh=True, differentiable_weight=True)
    with pytest.raises(AssertionError, match="one row per camera"):
        gs.render_views(g, [cam, cam], use_sh=True, background=torch.zeros(3, 3))
    with pytest.raises(AssertionError, match="background"):
        gs.render_views(g, [cam, cam], use_sh=True, background=torch.zeros(2, 4))
    # tensors that are not on the HIP device, float64 ones too, and features the fused frame does not cover: what
    # render_gaussians raises for the same call
    wide = g.replace(feature=torch.rand(n, 31))
    for gaussians, kw in ((g, dict(use_sh=True)), (g.to(dtype=torch.float64), dict(use_sh=True)),
                          (wide, dict(use_sh=False))):
        with pytest.raises((RuntimeError, TypeError, NotImplementedError)) as single:
            gs.render_gaussians(gaussians, cam, sparse_grad=True, **kw)
        for sparse in (True, False):
            with pytest.raises(type(single.value)):
                gs.render_views(gaussians, [cam, cam], sparse_grad=sparse, **kw)
