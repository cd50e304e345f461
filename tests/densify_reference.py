"""Torch restatement of densification, the reference the HIP path (taichi_gaussian_rasterizer_amd.densify) is held
against: masks -> the `nonzero` order of the plan, `params[keep]` + `append_tensors` for the tables (the unchanged
ParameterClass methods), and the 3D split evaluated in float64.  Runs on whatever device its inputs live on."""
import math

import numpy as np
import torch

from taichi_gaussian_rasterizer_amd.optim.parameter_class import TensorTable


def classes(n, prune=None, split=None, clone=None, device=None):
    """(keep, clone, split) bool masks after precedence: prune over split over clone"""
    none = torch.zeros(n, dtype=torch.bool, device=device)
    p = none if prune is None else prune
    s = (none if split is None else split) & ~p
    c = (none if clone is None else clone) & ~p & ~s
    return ~(p | s), c, s


def reference_plan(n, prune=None, split=None, clone=None, children=2, device=None):
    """(src_of int64 (rows,), [kept, clones, split_parents, rows])"""
    keep, c, s = classes(n, prune, split, clone, device)
    kept_rows = keep.nonzero().flatten()
    clone_rows = c.nonzero().flatten()
    child_rows = s.nonzero().flatten().repeat_interleave(children)
    src_of = torch.cat([kept_rows, clone_rows, child_rows])
    return src_of, [int(kept_rows.numel()), int(clone_rows.numel()), int(s.sum()), int(src_of.numel())]


def log_shrink32(shrink):
    return float(np.float32(math.log(shrink)))


def quat_to_mat64(q):
    """rotation matrices (M, 3, 3) float64 of quaternions xyzw, normalised here"""
    q = q.double()
    q = q / q.norm(dim=1, keepdim=True)
    x, y, z, w = q.unbind(1)
    rows = [1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * w * z, 2 * x * z + 2 * w * y,
            2 * x * y + 2 * w * z, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * w * x,
            2 * x * z - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x * x - 2 * y * y]
    return torch.stack(rows, dim=1).view(-1, 3, 3)


def reference_split(position, log_scaling, rotation, parent_of, noise, shrink):
    """children of rows parent_of (M,) with noise (M, 3), from the float32 inputs:
    position in float64 (M, 3), its error scale |p_i| + ||exp(ls) * noise||_2 (M, 3), log_scaling float32 (M, 3)"""
    parent_of = parent_of.long()
    p = position[parent_of].double()
    offset = log_scaling[parent_of].double().exp() * noise.double()
    child = p + torch.einsum("mij,mj->mi", quat_to_mat64(rotation[parent_of]), offset)
    scale = p.abs() + offset.norm(dim=1, keepdim=True)
    child_ls = log_scaling[parent_of] - torch.tensor(log_shrink32(shrink), dtype=torch.float32,
                                                     device=log_scaling.device)
    return child, scale, child_ls


SPLIT_BOUND = 32 * 2.0 ** -24  # |err_i| <= SPLIT_BOUND * (|p_i| + ||exp(ls) * noise||_2)


def reference_densify(params, prune, split, clone, children, noise, shrink, state, child_position=None):
    """The composition densify replaces: `params[keep]`, then `append_tensors` of the clones and the children, whose
    optimizer state starts at zero (state="zero", append_tensors' default) or is the parent's (state="parent").
    Returns (ParameterClass, float64 child positions, their error scale).  child_position: float32 (M, 3) to use for the
    children in the tables instead of the rounded float64 ones."""
    n = int(params.batch_size[0])
    device = params.position.device
    keep, c, s = classes(n, prune, split, clone, device)
    new_src = torch.cat([c.nonzero().flatten(), s.nonzero().flatten().repeat_interleave(children)])
    clones = int(c.sum())
    tensors = params.tensors.detach()
    new = {name: t[new_src].clone() for name, t in tensors.items()}
    child64 = scale = None
    if new_src.numel() > clones:
        child64, scale, child_ls = reference_split(tensors["position"], tensors["log_scaling"], tensors["rotation"],
                                                   new_src[clones:], noise, shrink)
        new["position"][clones:] = child64.float() if child_position is None else child_position
        new["log_scaling"][clones:] = child_ls
    new_state = None
    if state == "parent":
        new_state = {name: TensorTable({k: v[new_src] for k, v in table.items()})
                     for name, table in params.tensor_state.items()}
    return params[keep].append_tensors(new, new_state), child64, scale


def bits(t):
    """the tensor's bits as integers, so that NaNs compare equal to themselves and -0.0 differs from 0.0"""
    t = t.detach().contiguous()
    if t.dtype == torch.bool:
        return t.to(torch.uint8)
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))
