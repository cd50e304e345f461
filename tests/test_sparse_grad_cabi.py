"""Sparse visible-row gradients, the part that needs no GPU: the row-compact entry points (gs_project_bwd_rows,
gs_sh_bwd_rows, gs_feature_gather_bwd_rows, gs_frame_bwd_rows, gs_optim_grad_rows, gs_optim_step_rows) validate their
arguments on the host before any launch, an empty call is a no-op, and the public switch is type-checked."""
import ctypes

import pytest
import torch

from taichi_gaussian_rasterizer_amd import _native

P = ctypes.c_void_p(16)  # a non-NULL pointer that is never dereferenced: every call below stops at a host-side check


def _cfg():
    return _native.GsRasterConfig(tile_size=16, alpha_threshold=1 / 255., forward_cut=2.0 ** -20)


def _err(lib):
    return lib.gs_last_error()


def test_project_bwd_rows_validates_on_the_host():
    lib = _native.lib()
    cfg = _cfg()

    def call(n, v, indexes=P, outs=(P, P, P, P), cam=(None, None), scratch=(None, 0), params=(P, P, P, P)):
        return lib.gs_project_bwd_rows(n, v, *params, P, P, 64, 64, cfg, indexes, P, 7, None, None, 1, *outs, *cam,
                                       *scratch, None)

    assert call(10, 11) == -1 and b"visible rows" in _err(lib)           # v > n
    assert call(10, -1) == -1 and b"visible rows" in _err(lib)
    assert call(10, 5, indexes=None) == -1 and b"NULL buffer" in _err(lib)
    assert call(10, 5, outs=(P, P, None, P)) == -1 and b"NULL buffer" in _err(lib)
    assert call(10, 5, params=(None, P, P, P)) == -1 and b"NULL" in _err(lib)
    # camera gradients need the per-block partials
    assert call(10, 5, cam=(P, None)) == -4 and b"scratch" in _err(lib)
    assert call(10, 5, cam=(P, P), scratch=(P, 63)) == -4
    bad = _native.GsRasterConfig(tile_size=7, alpha_threshold=1 / 255.)
    assert lib.gs_project_bwd_rows(10, 5, P, P, P, P, P, P, 64, 64, bad, P, P, 7, None, None, 1, P, P, P, P, None,
                                   None, None, 0, None) == -2 and b"tile_size" in _err(lib)
    # nothing visible: a no-op, whatever the output pointers
    assert call(10, 0, indexes=None, outs=(None, None, None, None)) == 0
    assert call(0, 0, indexes=None, outs=(None, None, None, None), params=(None, None, None, None)) == 0
    assert lib.gs_project_bwd_rows_scratch_bytes(1000) >= 4 * 64
    assert lib.gs_project_bwd_rows_scratch_bytes(1000) == lib.gs_project_bwd_scratch_bytes(1000)


def test_sh_bwd_rows_validates_on_the_host():
    lib = _native.lib()

    def call(n, v, channels=3, degree=3, bufs=(P, P, P, P, P), d_params=P):
        params, positions, indexes, cam, gout = bufs
        return lib.gs_sh_bwd_rows(n, v, channels, degree, params, positions, indexes, cam, gout, 16, None, 0, d_params,
                                  None, None, None)

    assert call(10, 5, degree=4) == -2 and b"degree" in _err(lib)
    assert call(10, 5, degree=-1) == -2 and b"degree" in _err(lib)
    assert call(10, 5, channels=0) == -2 and b"channels" in _err(lib)
    assert call(10, 5, channels=9) == -2 and b"channels" in _err(lib)
    assert call(10, 11) == -1 and b"visible rows" in _err(lib)
    assert call(10, 5, bufs=(P, P, None, P, P)) == -1 and b"NULL buffer" in _err(lib)
    assert call(10, 5, d_params=None) == -1 and b"NULL buffer" in _err(lib)
    assert call(10, 0, bufs=(None,) * 5, d_params=None) == 0


def test_feature_gather_bwd_rows_validates_on_the_host():
    lib = _native.lib()
    assert lib.gs_feature_gather_bwd_rows(10, 0, P, 16, P, None) == -1 and b"channels" in _err(lib)
    assert lib.gs_feature_gather_bwd_rows(-1, 3, P, 16, P, None) == -1 and b"rows" in _err(lib)
    assert lib.gs_feature_gather_bwd_rows(10, 3, None, 16, P, None) == -1 and b"NULL buffer" in _err(lib)
    assert lib.gs_feature_gather_bwd_rows(10, 3, P, 16, None, None) == -1 and b"NULL buffer" in _err(lib)
    assert lib.gs_feature_gather_bwd_rows(0, 3, None, 16, None, None) == 0


def test_optim_rows_entry_points_validate_on_the_host():
    lib = _native.lib()

    def step(rows, grad=P, grad_count=10, grad_rows=P, dims=3, indexes=P, param=P):
        return lib.gs_optim_step_rows(0, 0, rows, dims, indexes, P, P, P, P, grad, grad_count, grad_rows, 1e-3, 0.9,
                                      0.999, 1e-16, 1, None, None, param, None, None, None)

    assert step(10, dims=0) == -1 and b"dims" in _err(lib)
    assert step(10, grad_rows=None, grad_count=9) == -1 and b"no grad_rows" in _err(lib)   # row i needs >= rows rows
    assert step(10, indexes=None) == -1 and b"NULL buffer" in _err(lib)
    assert step(10, grad=None) == -1 and b"NULL buffer" in _err(lib)
    assert step(10, param=None) == -1 and b"NULL buffer" in _err(lib)      # neither lr_step nor param
    assert step(0, grad=None, grad_count=0, grad_rows=None, indexes=None, param=None) == 0
    assert lib.gs_optim_grad_rows(10, None, 5, P, P, None) == -1 and b"NULL buffer" in _err(lib)
    assert lib.gs_optim_grad_rows(10, P, 5, None, P, None) == -1 and b"NULL buffer" in _err(lib)
    assert lib.gs_optim_grad_rows(10, P, -1, P, P, None) == -1
    assert lib.gs_optim_grad_rows(0, None, 5, None, None, None) == 0


def test_frame_bwd_rows_refuses_shards_and_row_ranges():
    """gs_frame_bwd_rows takes gs_frame_bwd's arguments; a sharded frame and a row sub-range are refused as
    unsupported, before the buffers are looked at"""
    lib = _native.lib()

    def frame(**kw):
        f = _native.GsFrame(n=1000, channels=3, sh_degree=3, width=100, height=70, near_plane=0.1, far_plane=100.0,
                            k_capacity=5000, cfg=_cfg())
        for k, v in kw.items():
            setattr(f, k, v)
        return f

    R, C, END = _native.GS_BWD_RASTER, _native.GS_BWD_COLOURS, _native.GS_BWD_STAGES

    def bwd(fr, first=R, end=END, rows=(0, 1000), part=True):
        p = _native.GsFrameBwdPart(first_stage=first, end_stage=end, row_begin=rows[0], row_end=rows[1])
        return lib.gs_frame_bwd_rows(ctypes.byref(fr), *([None] * 7), None, 0, None, 0, 0, 0, *([None] * 14), None,
                                     ctypes.byref(p) if part else None, None)

    plain = frame()
    sharded = frame(has_shard=1, shard=_native.GsRowShard(1, 3, 5, 1, 0))
    assert bwd(sharded, R, C) == -2 and b"sharded" in _err(lib)
    assert bwd(sharded, C, END) == -2 and b"sharded" in _err(lib)
    for rows in ((0, 999), (1, 1000), (200, 400)):
        assert bwd(plain, rows=rows) == -2 and b"sub-range" in _err(lib), rows
    assert bwd(plain, rows=(0, 1001)) == -1 and b"rows" in _err(lib)
    assert bwd(plain, R, R) == -1 and b"stages" in _err(lib)
    assert bwd(frame(sh_degree=4)) == -2
    # well-formed calls -- one call, or stage by stage -- get as far as the buffer checks
    assert bwd(plain) == -4 and b"workspace" in _err(lib)
    assert bwd(plain, part=False) == -4
    assert bwd(plain, R, C) == -4 and bwd(plain, C, END) == -4


def test_sparse_grad_switch_is_type_checked():
    """render_gaussians(sparse_grad=...) must be a bool, like the other switches; checked before anything else"""
    import inspect

    import taichi_gaussian_rasterizer_amd as gs
    from taichi_gaussian_rasterizer_amd import RasterConfig, scenes
    g, cam = scenes.benchmark_scene(16, (32, 32), sh_degree=0, seed=0)
    with pytest.raises(TypeError, match="sparse_grad must be bool"):
        gs.render_gaussians(g, cam, RasterConfig(), use_sh=True, sparse_grad=1)
    sig = inspect.signature(gs.render_gaussians)
    assert list(sig.parameters)[-1] == "sparse_grad" and sig.parameters["sparse_grad"].default is False


def test_frame_sparse_gradient_is_recognised_by_its_index_storage():
    """fused.is_frame_sparse_grad: the index list registered by a frame is recognised through the gradient autograd
    stores (same storage, is_coalesced dropped); a gradient with other indices, or the sum of two, is not"""
    from taichi_gaussian_rasterizer_amd import fused
    idx = torch.tensor([[1, 3, 4]])
    fused._register_sparse_indexes(idx)
    p = torch.zeros(6, 2, requires_grad=True)

    class Rows(torch.autograd.Function):
        @staticmethod
        def forward(ctx, t):
            return t.sum()

        @staticmethod
        def backward(ctx, g):
            return torch.sparse_coo_tensor(idx, torch.ones(3, 2), (6, 2), is_coalesced=True)

    Rows.apply(p).backward()
    assert p.grad.is_sparse and fused.is_frame_sparse_grad(p.grad)
    foreign = torch.sparse_coo_tensor(torch.tensor([[4, 1, 1]]), torch.ones(3, 2), (6, 2))
    assert not fused.is_frame_sparse_grad(foreign)
    assert not fused.is_frame_sparse_grad(torch.sparse_coo_tensor(idx[:, :2], torch.ones(2, 2), (6, 2)))  # a prefix
    Rows.apply(p).backward()  # accumulated over two backward passes: autograd's own index storage
    assert p.grad.is_sparse and not fused.is_frame_sparse_grad(p.grad)
    assert torch.equal(p.grad.to_dense()[[1, 3, 4]], torch.full((3, 2), 2.0))
    del idx, p, Rows
