"""Nearest neighbours of a point cloud on the device, and the first Gaussians3D of a training run built from one.

    dist2, index = knn(points, k=3)                    # exact: (N,k) squared distances, ascending, and their rows
    gaussians = gaussians_from_points(points, colors, sh_degree=3)

`knn` is gs_knn3d (include/gsplat_hip.h, "Nearest neighbours"): exact, ties to the smaller index, the point itself
excluded by index, `+inf` / `-1` where a point has fewer than k neighbours or a non-finite coordinate.  The squared
distance is the float32 value of `(dx * dx + dy * dy) + dz * dz` in exactly this order, so a float32 reimplementation
reproduces it bit for bit.  `gaussians_from_points` is the initialisation every 3DGS trainer starts from: isotropic
scales from the distance to the nearest neighbours, identity rotations, one opacity, colours as features or as the DC
term of spherical harmonics.  Everything here runs on a HIP device only.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

from . import _native as nv
from .data_types import Gaussians3D

SH_C0 = 0.2820948  # the DC basis function, as scenes.benchmark_scene and evaluate_sh_at use it


def _check_points(points, what: str) -> int:
    if not isinstance(points, torch.Tensor):
        raise TypeError(f"{what}: points must be a torch.Tensor, got {type(points).__name__}")
    if points.dtype != torch.float32:
        raise TypeError(f"{what}: points must be float32, got {points.dtype}")
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"{what}: points has shape {tuple(points.shape)}, expected (N, 3)")
    if points.shape[0] >= 2 ** 31:
        raise ValueError(f"{what}: {points.shape[0]} points (must stay below 2^31)")
    return int(points.shape[0])


def _check_k(k, what: str) -> int:
    if not 1 <= int(k) <= nv.GS_KNN_MAX:
        raise ValueError(f"{what}: k {k} not in [1, {nv.GS_KNN_MAX}]")
    return int(k)


def knn(points: torch.Tensor, k: int = 3, return_index: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """points (N,3) float32 on the device -> (dist2 (N,k) float32, index (N,k) int64, or None with return_index=False).
    Row i: the k points j != i with the smallest (dist2, j), ascending.  A strided view is made contiguous.  No
    gradient flows through it.  No host synchronisation."""
    what = "knn"
    n = _check_points(points, what)
    k = _check_k(k, what)
    nv.require_device(points, what=what)
    device = points.device
    with torch.no_grad(), torch.cuda.device(device):
        points = points.detach().contiguous()
        dist2 = torch.empty((n, k), dtype=torch.float32, device=device)
        index = torch.empty((n, k), dtype=torch.int32, device=device) if return_index else None
        if n > 0:
            lib = nv.lib()
            need = lib.gs_knn3d_scratch_bytes(n)
            scratch = nv.scratch(need, device)
            nv.check(lib.gs_knn3d(n, nv.ptr(points), k, nv.ptr(dist2), nv.ptr(index), nv.ptr(scratch), need,
                                  nv.stream()), "gs_knn3d")
        return dist2, (index.long() if return_index else None)


def neighbour_scale(dist2: torch.Tensor, scale_factor: float = 1.0, min_scale: float = 1e-7,
                    max_scale: float = math.inf) -> torch.Tensor:
    """(N,k) squared neighbour distances -> (N,) clamp(scale_factor * sqrt(mean of the finite ones), min_scale,
    max_scale); a row without a finite entry takes min_scale.  Plain torch, one pass."""
    finite = torch.isfinite(dist2)
    count = finite.sum(dim=1)
    mean = torch.where(finite, dist2, torch.zeros_like(dist2)).sum(dim=1) / count.clamp(min=1).to(dist2.dtype)
    scale = torch.where(count > 0, scale_factor * torch.sqrt(mean), torch.full_like(mean, min_scale))
    return scale.clamp(min=min_scale, max=max_scale)


def gaussians_from_points(points: torch.Tensor, colors: Optional[torch.Tensor] = None, *,
                          sh_degree: Optional[int] = None, k: int = 3, initial_alpha: float = 0.1,
                          scale_factor: float = 1.0, min_scale: float = 1e-7,
                          max_scale: float = math.inf) -> Gaussians3D:
    """A Gaussians3D from a point cloud (SfM points, lidar, a depth back-projection), on the points' device.

    position = points; log_scaling = log(neighbour_scale(knn(points, k))) in all three columns; rotation = identity
    (xyzw: 0, 0, 0, 1); alpha_logit = logit(initial_alpha).  feature: `colors` (N,C) as it is with sh_degree=None;
    with sh_degree = D (colors (N,3) in 0..1) an (N, 3, (D+1)^2) table whose DC term is (rgb - 0.5) / 0.2820948 and
    whose higher terms are zero.  colors=None is mid-grey (0.5; three channels)."""
    what = "gaussians_from_points"
    n = _check_points(points, what)
    k = _check_k(k, what)
    if not 0.0 < float(initial_alpha) < 1.0:
        raise ValueError(f"{what}: initial_alpha {initial_alpha} must lie in (0, 1)")
    if not float(scale_factor) > 0.0:
        raise ValueError(f"{what}: scale_factor {scale_factor} must be positive")
    if not 0.0 < float(min_scale) <= float(max_scale):
        raise ValueError(f"{what}: need 0 < min_scale <= max_scale, got {min_scale} and {max_scale}")
    if sh_degree is not None and not 0 <= int(sh_degree) <= 3:
        raise ValueError(f"{what}: sh_degree {sh_degree} not in [0, 3]")
    if colors is not None:
        if not isinstance(colors, torch.Tensor) or colors.dtype != torch.float32:
            got = colors.dtype if isinstance(colors, torch.Tensor) else type(colors).__name__
            raise TypeError(f"{what}: colors must be a float32 torch.Tensor, got {got}")
        if colors.dim() != 2 or colors.shape[0] != n or colors.shape[1] < 1:
            raise ValueError(f"{what}: colors has shape {tuple(colors.shape)}, expected ({n}, C)")
        if sh_degree is not None and colors.shape[1] != 3:
            raise ValueError(f"{what}: spherical harmonics need colors of shape ({n}, 3), got {tuple(colors.shape)}")
        if colors.device != points.device:
            raise ValueError(f"{what}: colors on {colors.device}, points on {points.device}")
    nv.require_device(points, colors, what=what)
    device = points.device
    with torch.no_grad():
        points = points.detach().contiguous()
        dist2, _ = knn(points, k, return_index=False)
        scale = neighbour_scale(dist2, float(scale_factor), float(min_scale), float(max_scale))
        log_scaling = torch.log(scale).unsqueeze(1).repeat(1, 3)
        rotation = torch.zeros((n, 4), dtype=torch.float32, device=device)
        rotation[:, 3] = 1.0
        alpha_logit = torch.full((n, 1), math.log(initial_alpha / (1.0 - initial_alpha)), dtype=torch.float32,
                                 device=device)
        rgb = torch.full((n, 3), 0.5, dtype=torch.float32, device=device) if colors is None else colors.detach()
        if sh_degree is None:
            feature = rgb.contiguous().clone()
        else:
            feature = torch.zeros((n, 3, (int(sh_degree) + 1) ** 2), dtype=torch.float32, device=device)
            feature[:, :, 0] = (rgb - 0.5) / SH_C0
    return Gaussians3D(position=points.clone(), log_scaling=log_scaling, rotation=rotation, alpha_logit=alpha_logit,
                       feature=feature, batch_size=(n,))


__all__ = ["knn", "neighbour_scale", "gaussians_from_points"]
