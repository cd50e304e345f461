"""The 3D smoothing filter of Mip-Splatting, on the device: a model that survives a change of sampling rate.

    table = pack_cameras(train_cameras)                      # once per camera set
    f = filter_3d(gaussians.position, table)                 # every K iterations, and after densify / relocate / grow
    rendering = render_gaussians(smooth_gaussians(gaussians, f), camera, sparse_grad=True)

Every Gaussian is low-passed with an isotropic Gaussian whose size comes from the highest rate focal / depth at which
any training camera samples it (`sampling_rate`, gs_mip_sampling_rate: one lane per point over the packed camera table,
exact and reproducible bit for bit), and its opacity is rescaled so that it keeps its mass (`smooth3d`):

    scale' = sqrt(scale^2 + f^2),   opacity' = opacity * sqrt(det S / det S')

in the (log_scaling, alpha_logit) parametrisation `Gaussians3D` stores, as one autograd Function whose backward keeps the
row-compact gradients of a `sparse_grad=True` frame row-compact.  `RasterConfig.antialias` is the screen-space half of
the same cure.  The filter size is a constant of the graph: a trainer recomputes it with `filter_3d` after `densify` /
`relocate` / `grow` (the positions and the rows have changed), and between those calls carries the table through a
densification plan with `move_rows({"filter3d": f}, plan)`.  The `.detach()`ed result of `smooth_gaussians` is what an
export writes for viewers that render at other resolutions.  Everything here runs on a HIP device only."""
from __future__ import annotations

import math
from typing import Sequence, Tuple, Union

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _native as nv
from .data_types import Gaussians3D
from .fused import is_frame_sparse_grad
from .perspective.params import CameraParams

Cameras = Union[torch.Tensor, Sequence[CameraParams]]


def pack_cameras(cameras: Sequence[CameraParams], margin: float = 0.15) -> torch.Tensor:
    """The (C, 24) float32 table `sampling_rate` reads (include/gsplat_hip.h, gs_mip_sampling_rate), on the cameras'
    device: rows 0-2 of T_camera_world, fx fy cx cy, the bounds -m W, (1 + m) W, -m H, (1 + m) H of the image widened
    by `margin` (products of float32 values, rounded once), near, far, max(fx, fy), 0.  Built on the host, once per
    camera set: the cameras' tensors are read back here."""
    what = "pack_cameras"
    cameras = list(cameras)
    if not all(isinstance(c, CameraParams) for c in cameras):
        raise TypeError(f"{what}: expected a sequence of CameraParams")
    if len(cameras) > nv.GS_MIP_CAMERAS_MAX:
        raise ValueError(f"{what}: {len(cameras)} cameras (at most {nv.GS_MIP_CAMERAS_MAX})")
    if not (isinstance(margin, (int, float)) and math.isfinite(margin) and margin >= 0):
        raise ValueError(f"{what}: margin {margin!r} must be a finite number >= 0")
    table = np.zeros((len(cameras), nv.GS_MIP_CAMERA_FLOATS), dtype=np.float32)
    m, one = np.float32(margin), np.float32(1)
    for row, cam in zip(table, cameras):
        row[0:12] = cam.T_camera_world.detach().to("cpu", torch.float32).numpy()[:3].reshape(12)
        row[12:16] = cam.projection.detach().to("cpu", torch.float32).numpy()
        w, h = np.float32(cam.image_size[0]), np.float32(cam.image_size[1])
        row[16:20] = (-m * w, (one + m) * w, -m * h, (one + m) * h)
        row[20], row[21] = cam.near_plane, cam.far_plane
        row[22] = max(row[12], row[13])
    device = cameras[0].projection.device if cameras else torch.device("cpu")
    return torch.from_numpy(table).to(device)


def _camera_table(cameras: Cameras, what: str) -> torch.Tensor:
    if isinstance(cameras, torch.Tensor):
        if cameras.dtype != torch.float32:
            raise TypeError(f"{what}: a packed camera table must be float32, got {cameras.dtype}")
        if cameras.dim() != 2 or cameras.shape[1] != nv.GS_MIP_CAMERA_FLOATS:
            raise ValueError(f"{what}: a packed camera table has shape (C, {nv.GS_MIP_CAMERA_FLOATS}), got "
                             f"{tuple(cameras.shape)}")
        if cameras.shape[0] > nv.GS_MIP_CAMERAS_MAX:
            raise ValueError(f"{what}: {cameras.shape[0]} cameras (at most {nv.GS_MIP_CAMERAS_MAX})")
        return cameras
    if isinstance(cameras, CameraParams) or not hasattr(cameras, "__iter__"):
        raise TypeError(f"{what}: cameras must be a sequence of CameraParams or a table from pack_cameras, got "
                        f"{type(cameras).__name__}")
    return pack_cameras(cameras)


def sampling_rate(positions: torch.Tensor, cameras: Cameras) -> Tuple[torch.Tensor, torch.Tensor]:
    """positions (N, 3) float32; cameras: a list of CameraParams or the table of `pack_cameras` ->
    (rate (N,) float32, seen (N,) int32): the largest focal / depth over the cameras whose frustum (widened by the
    table's margin, clipped at near and far) holds the point, 0 where there is none, and how many do.  This is the
    paper's definition, per camera with its own focal length: mixed focal lengths and image pyramids are handled.
    Exact (every float32 operation fixed, module docstring of csrc/mip.hip): the result equals a numpy restatement bit
    for bit.  No gradient and no host synchronisation."""
    what = "sampling_rate"
    if not isinstance(positions, torch.Tensor):
        raise TypeError(f"{what}: positions must be a torch.Tensor, got {type(positions).__name__}")
    if positions.dtype != torch.float32:
        raise TypeError(f"{what}: positions must be float32, got {positions.dtype}")
    if positions.dim() != 2 or positions.shape[1] != 3:
        raise ValueError(f"{what}: positions has shape {tuple(positions.shape)}, expected (N, 3)")
    n = int(positions.shape[0])
    if n >= 2 ** 31:
        raise ValueError(f"{what}: {n} points (must stay below 2^31)")
    table = _camera_table(cameras, what)
    if table.shape[0] == 0:  # no camera names a device
        table = table.to(positions.device)
    nv.require_device(positions, table, what=what)
    device = positions.device
    with torch.cuda.device(device):
        rate = torch.empty((n,), dtype=torch.float32, device=device)
        seen = torch.empty((n,), dtype=torch.int32, device=device)
        nv.check(nv.lib().gs_mip_sampling_rate(n, nv.ptr(positions.detach().contiguous()), int(table.shape[0]),
                                               nv.ptr(table.contiguous()), nv.ptr(rate), nv.ptr(seen), nv.stream()),
                 "gs_mip_sampling_rate")
    return rate, seen


def filter_3d(positions: torch.Tensor, cameras: Cameras, variance: float = 0.2) -> torch.Tensor:
    """The filter size of every Gaussian, (N,) float32: sqrt(variance) / rate for the rows some camera sees; rows no
    camera sees take the largest filter among the seen rows (as the original code does); all zeros when no row is seen.
    Plain torch on top of `sampling_rate`, off the hot path, without a host read.

    The result is tied to the rows and positions it was computed from: recompute it after `densify`, `relocate` and
    `grow` (and every few hundred iterations, as the positions move); between those calls a densification plan carries
    it along like any per-row table, `move_rows({"filter3d": f}, plan)["filter3d"]`."""
    if not (isinstance(variance, (int, float)) and math.isfinite(variance) and variance >= 0):
        raise ValueError(f"filter_3d: variance {variance!r} must be a finite number >= 0")
    rate, seen = sampling_rate(positions, cameras)
    if rate.numel() == 0:
        return rate
    visible = seen > 0
    size = torch.where(visible, math.sqrt(variance) / rate, torch.zeros_like(rate))
    return torch.where(visible, size, size.max())


# ------------------------------------------------------------------------------------------------------ smoothing
def _sparse_rows(grad):
    """the index tensor of a gradient the row kernel takes (sparse over rows only, indices ascending and distinct), or
    None"""
    if grad.layout != torch.sparse_coo or grad.sparse_dim() != 1:
        return None
    if not (grad.is_coalesced() or is_frame_sparse_grad(grad)):
        return None
    return grad._indices()


def _same_indexes(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.stride() == b.stride()


class _Smooth3D(torch.autograd.Function):
    @staticmethod
    @nv.on_tensor_device
    def forward(ctx, log_scaling, alpha_logit, filter3d, dtype):
        l, a, f = (t.detach().contiguous() for t in (log_scaling, alpha_logit, filter3d))
        ctx.set_materialize_grads(False)
        ctx.rows, ctx.dtype, ctx.shapes = (l, a, f), dtype, (log_scaling.shape, alpha_logit.shape)
        out_l, out_a = torch.empty_like(l), torch.empty_like(a)
        name = "gs_smooth3d_fwd" + ("_f64" if dtype == torch.float64 else "")
        nv.check(getattr(nv.lib(), name)(int(l.shape[0]), nv.ptr(l), nv.ptr(a), nv.ptr(f), nv.ptr(out_l), nv.ptr(out_a),
                                         nv.stream()), name)
        return out_l, out_a

    @staticmethod
    @once_differentiable
    @nv.on_tensor_device
    def backward(ctx, grad_l, grad_a):
        if grad_l is None and grad_a is None:
            return None, None, None, None
        (l, a, f), dtype, (shape_l, shape_a) = ctx.rows, ctx.dtype, ctx.shapes
        n, device, lib = int(l.shape[0]), l.device, nv.lib()
        grads = [g for g in (grad_l, grad_a) if g is not None]
        for g in grads:
            if g.dtype != dtype:
                raise TypeError(f"smooth3d: {dtype} forward, {g.dtype} gradient")
        idx = None
        if dtype == torch.float32 and all(g.layout == torch.sparse_coo for g in grads):
            lists = [_sparse_rows(g) for g in grads]
            if all(i is not None for i in lists) and (len(lists) == 1 or _same_indexes(lists[0], lists[1])):
                idx = lists[0]
        if idx is not None:  # row-compact in, row-compact out, over the index tensor that came in
            v = int(idx.shape[1])
            vl = grad_l._values().reshape(v, 3).contiguous() if grad_l is not None else None
            va = grad_a._values().reshape(v).contiguous() if grad_a is not None else None
            d_l = torch.empty((v, 3), dtype=dtype, device=device)
            d_a = torch.empty((v,) + tuple(shape_a[1:]), dtype=dtype, device=device)
            nv.check(lib.gs_smooth3d_bwd_rows(n, v, nv.ptr(idx), nv.ptr(l), nv.ptr(a), nv.ptr(f), nv.ptr(vl), nv.ptr(va),
                                              nv.ptr(d_l), nv.ptr(d_a), nv.stream()), "gs_smooth3d_bwd_rows")
            d_l = torch.sparse_coo_tensor(idx, d_l, shape_l, is_coalesced=True)
            d_a = torch.sparse_coo_tensor(idx, d_a, shape_a, is_coalesced=True)
        else:
            gl, ga = (None if g is None else (g.to_dense() if g.layout != torch.strided else g).contiguous()
                      for g in (grad_l, grad_a))
            d_l, d_a = torch.empty_like(l), torch.empty_like(a)
            name = "gs_smooth3d_bwd" + ("_f64" if dtype == torch.float64 else "")
            nv.check(getattr(lib, name)(n, nv.ptr(l), nv.ptr(a), nv.ptr(f), nv.ptr(gl), nv.ptr(ga), nv.ptr(d_l),
                                        nv.ptr(d_a), nv.stream()), name)
        need_l, need_a = ctx.needs_input_grad[:2]
        return d_l if need_l else None, d_a if need_a else None, None, None


def smooth3d(log_scaling: torch.Tensor, alpha_logit: torch.Tensor,
             filter3d: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """log_scaling (N, 3), alpha_logit (N, 1) or (N,), filter3d (N,) or (N, 1), >= 0 -> (log_scaling', alpha_logit'):
        log_scaling' = log(exp(2 log_scaling) + filter3d^2) / 2
        alpha_logit' = logit(sigmoid(alpha_logit) * sqrt(det S / det S'))
    one autograd Function on gs_smooth3d_fwd / _bwd / _bwd_rows, in forms that stay finite and accurate for
    |log_scaling|, |alpha_logit| <= 40 and filters from 0 to 1e6.  Rows with filter3d == 0 come back bit for bit, values
    and gradients.  float32, or float64 when all three tensors are float64 (for gradcheck); the filter is a constant and
    must not require grad.  Nothing but the inputs is kept for the backward.

    Backward.  Dense gradients go through the dense kernel.  The row-compact gradients of one `sparse_grad=True` frame
    (`render_gaussians`, or `render_views` for a batch: one merged gradient over the union of the views' rows) stay
    row-compact: sparse_dim 1, coalesced or recognised by `fused.is_frame_sparse_grad`, and when both outputs have a
    gradient, over one index tensor.  The returned gradients are sparse over that same index tensor, so all five
    parameters of the Gaussians still share one registered index list and the optimizers take their binary-search path;
    nothing of size N is written.  Any other sparse gradient -- the uncoalesced sum autograd forms when several frames
    read one smoothed set, or two different index lists -- is made dense and goes through the dense kernel: batches
    should go through `render_views`."""
    what = "smooth3d"
    for name, t in (("log_scaling", log_scaling), ("alpha_logit", alpha_logit), ("filter3d", filter3d)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{what}: {name} must be a torch.Tensor, got {type(t).__name__}")
        if not t.is_floating_point():
            raise TypeError(f"{what}: {name} must be float32 or float64, got {t.dtype}")
    if log_scaling.dim() != 2 or log_scaling.shape[1] != 3:
        raise ValueError(f"{what}: log_scaling has shape {tuple(log_scaling.shape)}, expected (N, 3)")
    n = int(log_scaling.shape[0])
    for name, t in (("alpha_logit", alpha_logit), ("filter3d", filter3d)):
        if tuple(t.shape) not in ((n,), (n, 1)):
            raise ValueError(f"{what}: {name} has shape {tuple(t.shape)}, expected ({n},) or ({n}, 1)")
    if n >= 2 ** 31:
        raise ValueError(f"{what}: {n} rows (must stay below 2^31)")
    if filter3d.requires_grad:
        raise ValueError(f"{what}: filter3d requires grad; the filter size is a constant (detach it)")
    dtype = nv.float_dtype(log_scaling, alpha_logit, filter3d, what=what)
    return _Smooth3D.apply(log_scaling, alpha_logit, filter3d, dtype)


def smooth_gaussians(gaussians: Gaussians3D, filter3d: torch.Tensor) -> Gaussians3D:
    """`gaussians` with log_scaling and alpha_logit put through `smooth3d`; the other fields are the same tensors.
    Render the result; optimise the original.  `smooth_gaussians(g, f).detach()` is what an export writes."""
    if not isinstance(gaussians, Gaussians3D):
        raise TypeError(f"smooth_gaussians: expected a Gaussians3D, got {type(gaussians).__name__}")
    log_scaling, alpha_logit = smooth3d(gaussians.log_scaling, gaussians.alpha_logit, filter3d)
    return gaussians.replace(log_scaling=log_scaling, alpha_logit=alpha_logit)


__all__ = ["filter_3d", "pack_cameras", "sampling_rate", "smooth3d", "smooth_gaussians"]
